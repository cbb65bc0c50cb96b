"""CPU: the float64 reference of tests/fc_reference.py against torch autograd in float64, the constants of the bounds of
tests/test_35_fc_paths_gpu.py measured on the reference's own float32 restatement, the conditioning of every case, the
exactness of the exact tier, and the paths the case table reaches (cloudaae_fc_plan launches nothing)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fc_reference as R

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every kind of case: with and without batch norm, training and inference, ReLU on and off, rowvec, both accumulate flags,
# each NULL, the shadows absent, every row-tile count, the coarse shapes
AUTOGRAD_CASES = [c.name for c in R.CASES if c.N < 5000 and (c.K < 900 or c.M == 40)] + sorted(R.GROUP_CASES)


def _autograd(c, i):
    t = lambda a, g=False: torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=g)
    x, w = t(i.x, True), t(i.w, True)
    bias = t(np.zeros(c.N) if i.bias is None else i.bias, True)
    y = x @ w + bias
    if i.rowvec is not None:
        y = y + t(i.rowvec)[:, torch.arange(c.N) % c.rowvec_d]
    r = {"y": y}
    out = y
    if c.bn:
        gamma, beta = t(i.gamma, True), t(i.beta, True)
        if c.training:
            mean, var = y.mean(0), y.var(0, unbiased=False)
        else:
            mean, var = t(i.ema_mean), t(i.ema_var)
            if i.tier == "exact":       # (var + eps is the float32 sum there, exactly 0.25: fc_reference.forward)
                var = t((i.ema_var + F32(R.EPS)).astype(F64) - R.EPS)
        out = (y - mean) / torch.sqrt(var + R.EPS) * gamma + beta
        if c.relu:
            out = torch.relu(out)
        r.update(mean=mean, var=var, out=out)
    (out * t(i.dout)).sum().backward()
    r.update(dx=x.grad + t(i.dx0), dw=w.grad + (t(i.dw0) if c.acc_dw else 0.0), dbias=bias.grad)
    if c.bn:
        r.update(dgamma=gamma.grad, dbeta=beta.grad)
    return {k: v.detach().numpy() for k, v in r.items()}


@pytest.mark.parametrize("tier", R.TIERS)
@pytest.mark.parametrize("name", AUTOGRAD_CASES)
def test_reference_matches_autograd(name, tier):
    """per element, to 1e-12 of the element's own magnitude term (the sum of the absolute values of what it is formed from:
    dbias under training-mode batch norm is analytically zero and has no other scale)"""
    c = R.case_by_name(name)
    i = R.make_inputs(c, tier)
    assert i.undecided == 0
    fw, bw = R.reference(c, i)
    a = _autograd(c, i)
    adz = np.abs(bw.dz)
    terms = {"y": fw.ty + fw.trow + np.abs(fw.bias64), "dx": bw.tdx, "dw": bw.tdw}
    if c.bn:
        gterm = (np.abs(bw.gr) * (adz + np.abs(bw.m1) + np.abs(bw.xh * bw.m2))).sum(0)
        terms.update(out=fw.tz, dgamma=np.abs(bw.dz * bw.xh).sum(0), dbeta=adz.sum(0), dbias=gterm)
        if c.training:      # (inference: the moments are inputs)
            terms.update(mean=np.abs(fw.y).mean(0), var=(fw.y ** 2).mean(0))
        # (the products inherit the cancellation inside d(y): judged on its magnitude term, not on |d(y)|)
        gelem = np.abs(bw.gr) * (adz + np.abs(bw.m1) + np.abs(bw.xh * bw.m2))
        terms["dw"] = np.abs(i.x.astype(F64)).T @ gelem + np.abs(i.dw0.astype(F64))
        terms["dx"] = gelem @ np.abs(i.w.astype(F64)).T + np.abs(i.dx0.astype(F64))
    else:
        terms["dbias"] = adz.sum(0)
    for k, term in terms.items():
        want = a[k]
        got = getattr(fw, k) if hasattr(fw, k) and k in ("y", "mean", "var", "out") else getattr(bw, k)
        assert R.ratio(got - want, 1e-12 * term) <= 1.0, (name, tier, k, R.ratio(got - want, 1e-12 * term))
        # Where no batch norm stands between the inputs and the output, also relative to the element itself: in the exact
        # tier both sides are exact in float64 whatever their order of summation, so they are EQUAL; in the round-off tier
        # to 1e-12 of |want| on every element that is not a cancellation (below 1e-3 of its term float64 itself, summing in
        # another order than torch, cannot promise twelve digits of the element: the term judges those, above).
        if k == "y" or (not c.bn and k in ("dw", "dx", "dbias")) or k == "dbeta" and not c.relu:
            if tier == "exact":
                assert np.array_equal(got, want), (name, k)
            else:
                solid = np.abs(want) >= 1e-3 * np.broadcast_to(term, want.shape)
                assert want.size < 100 or solid.mean() > 0.8
                assert (np.abs(got - want)[solid] <= 1e-12 * np.abs(want)[solid]).all(), (name, tier, k)


@pytest.mark.parametrize("tier", R.TIERS)
def test_every_case_is_conditioned(tier):
    """no element's pre-ReLU value lies inside its own forward bound of zero: the cap on left-out elements is zero"""
    moved = 0
    for c in list(R.CASES) + list(R.GROUP_CASES.values()):
        i = R.make_inputs(c, tier)
        assert i.undecided == 0, (c.name, tier, i.undecided)
        if c.bn and c.relu:
            fw = R.forward(c, i)
            assert (np.abs(fw.zlin) > R.zero_bound(c, i, fw)).all(), c.name
            moved += 1
    assert moved > 20


def test_exact_tier_is_exact():
    """the exact tier's claim, from the reference alone: every product output is a float32, and the magnitude sums stay
    below 2^24 units of 1/8 (so every partial sum, in any order, is a float32 too)"""
    for c in list(R.CASES) + list(R.GROUP_CASES.values()):
        i = R.make_inputs(c, "exact")
        fw, bw = R.reference(c, i)
        outs = {"y": (fw.y, fw.ty + fw.trow + np.abs(fw.bias64))}
        if not c.bn or not c.training:
            outs.update(dw=(bw.dw, bw.tdw), dx=(bw.dx, bw.tdx))
        if not c.bn:
            outs["dbias"] = (bw.dbias + i.start["dbias"].astype(F64), np.abs(bw.dz).sum(0) + np.abs(i.start["dbias"]))
        for k, (v, mag) in outs.items():
            assert np.array_equal(v.astype(F32).astype(F64), v), (c.name, k)
            assert np.array_equal(np.round(v * 16), v * 16) and (mag * 16 < 2.0 ** 24).all(), (c.name, k)


def test_constants_are_four_times_the_restatement():
    """The largest normalised error of the float32 restatement against float64 over the case table; the GPU test allows four
    times that, rounded up to a power of two (R.ALLOWED).  Never tuned to what the kernels reach."""
    worst = {}
    for c in R.CASES:
        i = R.make_inputs(c, "round")
        for k, v in R.restatement_errors(c, i).items():
            if k not in worst or v > worst[k][0]:
                worst[k] = (v, c.name)
    measured = {}
    for k, (v, name) in sorted(worst.items()):
        if k in R.FIXED:
            print("FCCONST %-12s %8.3f ulp (fixed: %g)  %s" % (k, v, R.FIXED[k], name))
            assert v <= R.FIXED[k], (k, v, name)
            continue
        const = R.CONSTANT_OF[k]
        if const not in measured or v > measured[const][0]:
            measured[const] = (v, name, k)
    for const, (v, name, k) in sorted(measured.items()):
        print("FCCONST %-9s measured %9.3f (%s of %s)  allowed %g" % (const, v, k, name, R.ALLOWED[const]))
    assert set(measured) == set(R.ALLOWED)
    for const, (v, name, k) in measured.items():
        assert R.ALLOWED[const] == R.pow2_ceil(4.0 * v), (const, v, R.pow2_ceil(4.0 * v))


def test_case_table_reaches_every_path():
    """the same statement as tests/test_35_fc_paths_gpu.py::test_case_table_reaches_every_path, where no GPU is needed"""
    import torch  # noqa: F401  (the library binds to torch's HIP runtime)
    lib = ctypes.CDLL(os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so"))
    R.assert_coverage(lib)
