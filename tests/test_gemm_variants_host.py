"""CPU: the case table of tests/test_16_gemm_exact_gpu.py names real kernels, and all of them.

The rows of that table claim which gemm_f32_kernel / gemm_bf16_kernel instantiation they reach.  The set of claimed
<BM, BN, WM, WN, TA, TB, FAST> must EQUAL the set of instantiations in the gfx950 code object of the built library (read from the
mangled symbol names, tools/isa_scan.py): a kernel variant that is compiled in and has no row fails here, so a new tile shape
cannot be added untested, and a row that names a kernel that does not exist fails too.  What the library's queries can confirm
of every row -- K slices, BM, _supported -- is checked as well: host arithmetic, so the table can be debugged without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import isa_scan  # noqa: E402
import test_16_gemm_exact_gpu as exact  # noqa: E402

LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")


@pytest.fixture(scope="module")
def built():
    """(family, BM, BN, WM, WN, TA, TB, FAST) of every GEMM kernel in the built library"""
    if not isa_scan.tools_present():
        pytest.skip("no ROCm LLVM tools on this machine")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    symbols = isa_scan.kernel_symbols(LIB)
    assert len(symbols) > 100, "symbol listing looks empty"
    return sorted((fam,) + inst[:7] for fam in ("f32", "bf16")
                  for inst in isa_scan.template_instances(symbols, "gemm_%s_kernel" % fam))


def test_mangled_template_arguments_are_read():
    sym = "_ZN8cloudaae15gemm_f32_kernelILi128ELi128ELi2ELi2ELb0ELb1ELb1ELi16EEEviiiPKfiS2_iPfiS2_iiiiNS_4FoldES4_Pdx"
    assert isa_scan.template_instances([sym, "_ZN8cloudaae9bn_kernelEv"], "gemm_f32_kernel") == [(128, 128, 2, 2, False, True, True, 16)]
    assert isa_scan.template_instances([sym], "gemm_bf16_kernel") == []


def test_table_claims_exactly_the_kernels_that_were_built(built):
    # two families x six tile shapes x four transposes x (predicate-free, predicated)
    assert len(built) == 96 and len(set(b[:3] for b in built)) == 12, built
    claimed = exact.kernel_variants()
    untested = [b for b in built if b not in claimed]
    unknown = [c for c in claimed if c not in built]
    assert not untested, "kernel variants in the library that no row of CASES reaches: %r" % untested
    assert not unknown, "rows of CASES claim kernel variants the library does not hold: %r" % unknown


def test_removing_the_rows_of_a_variant_is_noticed(built):
    """the comparison above fails when a variant loses its rows (here: every row of one variant is dropped in turn for a few)"""
    claimed = exact.kernel_variants()
    for victim in (claimed[0], claimed[len(claimed) // 2], claimed[-1]):
        fam, BM, BN, _, _, ta, tb, fast = victim
        rest = [c for c in exact.CASES if (c.fam, c.BM, c.BN, bool(c.ta), bool(c.tb), c.fast) != (fam, BM, BN, ta, tb, fast)]
        assert len(rest) < len(exact.CASES) and victim not in exact.kernel_variants(rest) and victim in built


def test_no_row_was_dropped():
    """several rows may reach one kernel variant (each for another reason), which the set comparison above cannot tell apart:
    the row counts are pinned, so dropping a row is a visible edit here as well"""
    ids = [c.id for c in exact.CASES + exact.OTHER]
    assert len(ids) == len(set(ids))
    assert (len(exact.CASES), len(exact.OTHER), sum(len(g) for g in exact.GROUPS.values())) == (502, 24, 12)


@pytest.fixture(scope="module")
def host():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib


@pytest.mark.parametrize("case", exact.CASES + exact.OTHER, ids=[c.id for c in exact.CASES + exact.OTHER])
def test_row_claims_hold(host, case):
    try:
        exact.check_claims(case, host.lib()._cdll, host.set_knob)
    finally:
        host.set_knob("CLOUDAAE_DETERMINISTIC", None)
    assert 2 * case.K * exact.amplitude(case.K) ** 2 + 2 * exact.amplitude(case.K) < 2 ** 24
