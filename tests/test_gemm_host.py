"""CPU: the host half of the fp32 / bf16 GEMM families (csrc/gemm.h) and of the bf16-storage products (gemm_b16.hip).

The cut every query reports -- K slices, ordered workspace, column-statistics parts, the shapes cloudaae_gemm_b16 serves --
is pinned by tests/golden/gemm_plans.npz over a grid of shapes that reaches every plan rule, with and without the
CLOUDAAE_DETERMINISTIC knob; bad arguments are refused in validation, before any HIP runtime call.

A pull request that changes a plan on purpose rewrites the fixture:  python tests/test_gemm_host.py --regenerate"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plans.npz")

MS = [1, 31, 32, 33, 64, 96, 128, 160, 320, 1024, 4096, 32768]
NS = [1, 24, 64, 96, 128, 160, 320, 1024, 12288]
KS = [1, 16, 63, 64, 128, 256, 512, 1024, 32768, 131072]
B16_PAIRS = [(0, 0), (0, 1), (1, 0)]       # the (trans_a, trans_b) pairs cloudaae_gemm_b16 serves


def _cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib, _lib.lib()._cdll


@pytest.fixture(scope="module")
def cdll():
    return _cdll()[1]


def _queries(c):
    """name -> function (M, N, K) of every plan query"""
    q = {}
    for fam in ("f32", "bf16"):
        for what in ("splits", "ordered_workspace", "colstats_parts"):
            q["%s_%s" % (fam, what)] = getattr(c, "cloudaae_gemm_%s_%s" % (fam, what))
    for ta, tb in B16_PAIRS:
        q["b16_supported_%d%d" % (ta, tb)] = (lambda ta, tb: lambda M, N, K: c.cloudaae_gemm_b16_supported(ta, tb, M, N, K))(ta, tb)
    q["b16_colstats_parts"] = c.cloudaae_gemm_b16_colstats_parts
    return q


def _plans():
    """name -> int64 [2 (knob unset, CLOUDAAE_DETERMINISTIC = 1), len(MS), len(NS), len(KS)]"""
    lib_, c = _cdll()
    out = {}
    try:
        for d, knob in enumerate((None, 1)):
            lib_.set_knob("CLOUDAAE_DETERMINISTIC", knob)
            for name, fn in _queries(c).items():
                a = out.setdefault(name, np.zeros((2, len(MS), len(NS), len(KS)), dtype=np.int64))
                for i, M in enumerate(MS):
                    for j, N in enumerate(NS):
                        for k, K in enumerate(KS):
                            a[d, i, j, k] = int(fn(M, N, K))
    finally:
        lib_.set_knob("CLOUDAAE_DETERMINISTIC", None)
    return out


def test_plans_match_the_fixture(cdll):
    ref = np.load(FIXTURE)
    got = _plans()
    assert sorted(ref.files) == sorted(got)
    for name, a in got.items():
        bad = np.argwhere(a != ref[name])
        assert bad.size == 0, "%s differs at (deterministic, M, N, K) = %r: %d, fixture %d" % (
            name, [(int(d), MS[i], NS[j], KS[k]) for d, i, j, k in bad[:5]], a[tuple(bad[0])], ref[name][tuple(bad[0])])
    # the grid reaches the rules the fixture is meant to pin
    assert (got["f32_splits"][0] > 8).any() and (got["bf16_splits"][0] > 8).any()
    assert (got["f32_splits"][1] == 1).all() and (got["f32_ordered_workspace"][1] > 0).any()
    assert got["b16_supported_00"].any() and got["b16_supported_01"].any() and got["b16_supported_10"].any()
    assert (got["b16_colstats_parts"] > 0).any()


# a fake, never dereferenced address: every call below must fail in validation, before any HIP runtime call
_X = 0x1000


def _refused(cdll, fn, args, needle):
    rc = getattr(cdll, fn)(*args)
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert msg.startswith(fn + ":") and needle in msg, msg


def _gemm(M=64, N=64, K=64, lda=None, ldb=None, ldc=None, A=_X):
    return [0, 0, M, N, K, A, K if lda is None else lda, _X, N if ldb is None else ldb, _X, N if ldc is None else ldc]


@pytest.mark.parametrize("fam", ["f32", "bf16"])
@pytest.mark.parametrize("kw, needle", [
    (dict(M=-1), "negative size"), (dict(N=-1), "negative size"), (dict(K=-1), "negative size"),
    (dict(lda=63), "leading dimension too small"), (dict(ldb=63), "leading dimension too small"),
    (dict(ldc=63), "leading dimension too small"),
])
def test_plain_refusals(cdll, fam, kw, needle):
    _refused(cdll, "cloudaae_gemm_" + fam, _gemm(**kw) + [None, 0, None], needle)
    _refused(cdll, "cloudaae_gemm_%s_ordered" % fam, _gemm(**kw) + [None, None, 0, None], needle)
    _refused(cdll, "cloudaae_gemm_%s_colstats" % fam, _gemm(**kw) + [None, _X, None], needle)


@pytest.mark.parametrize("fold_c, ldc, needle", [
    (16, 32, "leading dimension too small"), (16, 8, "leading dimension too small"),
    (12, 12, "fold width must be a power of two >= 4"), (2, 2, "fold width must be a power of two >= 4"),
])
def test_folded_output_refusals(cdll, fold_c, ldc, needle):
    assert cdll.cloudaae_gemm_f32_ordered_workspace(64, 64, 64) == 0       # stays whole: no workspace needed
    _refused(cdll, "cloudaae_gemm_f32_ordered_fold", _gemm(ldc=ldc) + [fold_c, None, 0, None], needle)


@pytest.mark.parametrize("fam", ["f32", "bf16"])
def test_colstats_needs_its_buffer(cdll, fam):
    _refused(cdll, "cloudaae_gemm_%s_colstats" % fam, _gemm() + [None, None, None], "null argument")


@pytest.mark.parametrize("fam", ["f32", "bf16"])
def test_ordered_workspace_missing_or_small(cdll, fam):
    M, N, K = 64, 64, 32768
    need = getattr(cdll, "cloudaae_gemm_%s_ordered_workspace" % fam)(M, N, K)
    assert need > M * N
    needle = "workspace missing or smaller than cloudaae_gemm_%s_ordered_workspace" % fam
    for ws, n in ((None, 0), (None, need), (_X, need - 1), (_X, 0)):
        _refused(cdll, "cloudaae_gemm_%s_ordered" % fam, _gemm(M, N, K) + [None, ws, n, None], needle)
    if fam == "f32":
        for ws, n in ((None, 0), (_X, need - 1)):
            _refused(cdll, "cloudaae_gemm_f32_ordered_fold", _gemm(M, N, K) + [0, ws, n, None], needle)


@pytest.mark.parametrize("ta, tb, M, N, K, lda, A, needle", [
    (1, 1, 128, 128, 64, 128, _X, "product not served"),
    (0, 0, 100, 128, 64, 64, _X, "product not served"),
    (0, 0, 128, 128, 96, 96, _X, "product not served"),
    (0, 0, 128, 128, 64, 68, _X, "operand rows must be 16-byte aligned"),
    (0, 0, 128, 128, 64, 64, _X + 8, "operand rows must be 16-byte aligned"),
])
def test_b16_refusals(cdll, ta, tb, M, N, K, lda, A, needle):
    _refused(cdll, "cloudaae_gemm_b16", [ta, tb, M, N, K, A, lda, _X, N, _X, N, 0, None, 0, None, None], needle)


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_gemm_host.py --regenerate   (rewrites %s from the built library)" % FIXTURE)
    np.savez_compressed(FIXTURE, **_plans())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
