"""CPU: tests/bn_reference.py is anchored before any kernel is judged by it (tests/test_20_batch_norm_paths_gpu.py).

  * at float64 it agrees with torch.autograd on a float64 restatement of oracle/model_oracle.py's batch_norm (+ReLU,
    + mean(1) / amax(1)) to 1e-12: output, every gradient, the EMA shadows;
  * dbias is the column sum of dy, the pool_stats sums reproduce the column sums of the full pass;
  * condition() leaves an empty ambiguous set on every case of the GPU file, and the float32 restatement's ReLU mask
    and tie counts then equal the float64 ones;
  * the constants of the GPU file's bounds are four times what the float32 restatement reaches against the float64
    reference over the case table, rounded up to a power of two;
  * four mutants of the reference each land far outside those bounds on every case they apply to."""
import functools

import numpy as np
import pytest
import torch

import bn_reference as R

F32, F64 = np.float32, np.float64


def _torch_bn(y, gamma, beta, training, sm, sv, decay, relu, pool_rows, pool_mode):
    """oracle/model_oracle.py: batch_norm, in float64, + ReLU + pool over groups of pool_rows rows"""
    if training:
        mean = y.mean(0)
        var = ((y - mean.detach()) ** 2).mean(0)
        om = float(F32(1.0) - F32(decay))
        with torch.no_grad():
            sm -= (sm - mean.detach()) * om
            sv -= (sv - var.detach()) * om
    else:
        mean, var = sm, sv
    inv = gamma * torch.rsqrt(var + 1e-3)
    z = y * inv + (beta - mean * inv)
    if relu:
        z = torch.relu(z)
    pooled = None
    if pool_mode:
        zg = z.view(-1, pool_rows, z.shape[1])
        pooled = zg.mean(1) if pool_mode == 1 else zg.amax(1)
    return z, pooled


AUTOGRAD_CASES = [   # M, C, relu, training, pool_rows, pool_mode, dout, duplicated rows
    (37, 5, 1, 1, 0, 0, 1, 0), (37, 5, 0, 1, 0, 0, 1, 0), (37, 5, 1, 0, 0, 0, 1, 0),
    (40, 6, 1, 1, 8, 1, 0, 0), (40, 6, 1, 1, 8, 1, 1, 0), (40, 6, 0, 0, 8, 1, 1, 0),
    (40, 6, 1, 1, 8, 2, 0, 1), (40, 6, 1, 1, 8, 2, 1, 1), (40, 6, 0, 1, 8, 2, 0, 1), (40, 6, 1, 0, 8, 2, 1, 1),
]


@pytest.mark.parametrize("M,C,relu,training,rows,mode,with_dout,dups", AUTOGRAD_CASES)
def test_float64_reference_equals_torch_autograd(M, C, relu, training, rows, mode, with_dout, dups):
    rng = np.random.default_rng(M + C + 3 * relu + 5 * training + 7 * mode + with_dout)
    y = (rng.standard_normal((M, C)) * 2 + 0.5).astype(F32)
    if dups:        # tied maxima: rows 1 and 6 of group 0 and rows 2, 3, 5 of group 1 are copies of a dominating row
        y[1] = y[6] = np.abs(y[:8]).max(0) + 1
        y[8 + 2] = y[8 + 3] = y[8 + 5] = np.abs(y[8:16]).max(0) + 1
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(F32)
    gamma[0] = np.abs(gamma[0])
    beta = (0.3 * rng.standard_normal(C)).astype(F32)
    sm, sv = (0.5 + rng.standard_normal(C)).astype(F32), (1 + np.abs(rng.standard_normal(C))).astype(F32)
    dout = rng.standard_normal((M, C)).astype(F32) if with_dout else None
    dpooled = rng.standard_normal((M // rows, C)).astype(F32) if mode else None
    fw = R.forward(y, gamma, beta, training, sm, sv, 0.9, relu, rows, mode)
    bw = R.backward(y, gamma, beta, training, sm, sv, relu, dout, rows, mode, dpooled)
    t = lambda a, g=False: torch.tensor(np.asarray(a, F64), requires_grad=g)
    ty, tg, tb = t(y, True), t(gamma, True), t(beta, True)
    tsm, tsv = t(sm), t(sv)
    z, pooled = _torch_bn(ty, tg, tb, training, tsm, tsv, 0.9, relu, rows, mode)
    loss = (z * t(dout)).sum() if with_dout else 0.0
    if mode:
        loss = loss + (pooled * t(dpooled)).sum()
    loss.backward()
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a, F64), b.detach().numpy(), rtol=1e-12, atol=1e-12)
    close(fw.z, z)
    if mode:
        close(fw.pooled, pooled)
    close(fw.ema_mean, tsm)
    close(fw.ema_var, tsv)
    close(bw.dy, ty.grad)
    close(bw.dgamma, tg.grad)
    close(bw.dbeta, tb.grad)
    close(bw.dbias, ty.grad.sum(0))
    np.testing.assert_allclose(bw.dbias, bw.dy.sum(0), rtol=0, atol=1e-13)
    if dups and mode == 2 and gamma[0] > 0:
        assert fw.ties[0, 0] == 2 and fw.ties[1, 0] == 3


def test_pool_stats_reproduce_the_column_sums_of_the_full_pass():
    c = R.CASE_BY_NAME["mean_R43"]
    x = R.make_inputs(c)
    fw, bw = R.reference(c, x)
    share = x.dpooled.astype(F64) / c.pool_rows
    np.testing.assert_allclose((share * fw.pool_stats[:, 0]).sum(0), bw.dz.sum(0), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose((share * fw.pool_stats[:, 1]).sum(0), (bw.dz * bw.xh).sum(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(fw.pool_stats[:, 2].sum(0), bw.xh.sum(0), rtol=0, atol=1e-10)
    assert np.array_equal(fw.pool_stats[:, 0].sum(0), (fw.z > 0).sum(0))


@functools.lru_cache(maxsize=None)
def _measured(name):
    """(ambiguous counts, mask of fp32 == mask of fp64, errors of the float32 restatement) of one case"""
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    fw, bw = R.reference(c, x)
    fw32, bw32 = R.reference(c, x, F32)
    same = np.array_equal(fw32.z > 0, fw.z > 0) if c.relu else True
    if c.pool_mode == 2:
        same = same and np.array_equal(fw32.ties, fw.ties) and \
            np.array_equal(fw32.z == np.repeat(fw32.pooled, c.pool_rows, 0), fw.z == np.repeat(fw.pooled, c.pool_rows, 0))
    return x.ambiguous, bool(same), R.case_errors(c, *R.outputs_of(c, fw32, bw32), fw, bw)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_is_well_posed(name):
    """the ambiguous set is empty after conditioning, and then fp32 decides every mask and every tie as fp64 does"""
    counts, same, errs = _measured(name)
    assert counts[-1] == 0, counts
    assert len(counts) <= 3, counts
    assert same
    c = R.CASE_BY_NAME[name]
    if c.relu and c.M * c.C >= 4096 and not c.clip:        # ... without the ReLU having been conditioned away
        fw, _ = R.reference(c, R.make_inputs(c))
        assert 0.05 < float((fw.z > 0).mean()) < 0.95
    for k in ("save_mean", "save_var", "stats_count", "ties"):
        if k in errs:
            assert errs[k] == 0.0, (k, errs[k])


def test_max_pool_cases_hold_the_ties_they_claim():
    for c in R.CASES:
        if not c.ties:
            continue
        fw, _ = R.reference(c, R.make_inputs(c))
        up = np.arange(c.C) % 2 == 0
        up[0] = not c.clip
        assert (fw.ties[0, up] == 2).all() and (fw.ties[1, up] == 2).all(), c.name      # one row lane; two row lanes
        assert (fw.ties[2:, up] == 1).all(), c.name                                      # the same row in two groups
        assert np.array_equal(fw.pooled[2, up], fw.pooled[3, up])
        if c.clip:
            assert (fw.pooled[:, 0] == 0).all() and (fw.ties[:, 0] == c.pool_rows).all()


def test_constants_are_four_times_the_restatement():
    worst = {k: 0.0 for k in R.ALLOWED}
    for c in R.CASES:
        for k, v in _measured(c.name)[2].items():
            if k in R.CONSTANT_OF:
                assert np.isfinite(v), (c.name, k)
                worst[R.CONSTANT_OF[k]] = max(worst[R.CONSTANT_OF[k]], v)
    print("measured:", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert R.ALLOWED[k] == R.pow2_ceil(4.0 * v), (k, v, R.ALLOWED[k])


# "far outside": more than FAR times the allowed bound (which is itself four times what the float32 restatement reaches).
# At |mean| / std = 2000 the dy bound carries the factor (1 + |mean| * rstd) and c_bwd is set by those very cases: m2 = 0
# lands 5 times outside there, every other mutant and case more than FAR (the weakest: 160).
FAR, FAR_AT_LARGE_OFFSET = 100.0, 4.0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_catch_the_mutant(mutant):
    hit = 0
    for c in R.CASES:
        if not R.mutant_applies(mutant, c):
            continue
        x = R.make_inputs(c)
        fw, bw = R.reference(c, x)
        e = R.case_errors(c, *R.outputs_of(c, *R.reference(c, x, F64, mutant)), fw, bw)
        over = max(v / max(R.allowed_of(k), 1.0 / FAR) for k, v in e.items())
        assert over > (FAR_AT_LARGE_OFFSET if abs(c.offset) > 20 * c.scale else FAR), (c.name, mutant, over, e)
        hit += 1
    assert hit >= 3


def test_unmutated_reference_has_no_error():
    c = R.CASE_BY_NAME["max_R200_out_both"]
    x = R.make_inputs(c)
    fw, bw = R.reference(c, x)
    e = R.case_errors(c, *R.outputs_of(c, fw, bw), fw, bw)
    assert e.pop("save_mean") <= 0.5 and e.pop("save_var") <= 0.5      # the moments are judged after rounding to fp32
    assert max(e.values()) == 0.0


def test_colsum_cases_name_every_shape():
    assert len(R.COLSUM_CASES) == 18
