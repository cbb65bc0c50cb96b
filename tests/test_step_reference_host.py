"""CPU: tests/step_reference.py is anchored before any kernel is judged by it (tests/test_34_step_paths_gpu.py).

  * evaluated in float64 on generic rows, the rotation reference equals oracle/model_oracle.py's rotation_error /
    exponential_map and torch.autograd's gradient to 1e-12 (the oracle's own conditioning is poor on the other rows: the
    reason for the 50-digit reference); the float32 restatements equal MO.translation_error and MO.AdamTF;
  * condition() holds on every case, with at most 1 % of a case's rows redrawn;
  * the constants of the GPU file's bounds are four times what the restatement (float64 for the rotation, float32 for the
    rest) reaches against the reference over the case table, rounded up to a power of two;
  * every mutant of the reference lands at least MARGIN times outside those bounds on every case it applies to."""
import functools
import math

import numpy as np
import pytest
import torch

import step_reference as R

F32, F64 = np.float32, np.float64


# ---- anchors ------------------------------------------------------------------------------------------------------------
def test_float64_rotation_equals_the_oracle_and_autograd_on_generic_rows():
    from oracle import model_oracle as MO
    rng = np.random.default_rng(11)
    pred, label = rng.standard_normal((40, 3)).astype(F32), rng.standard_normal((40, 3))
    pred[:6] *= 0.03                  # the Taylor branch of the prediction ...
    label[3:9] *= 0.03                # ... of the label, of both
    r = R.rotation(pred, label, R.FL)
    assert (r.clipped == 0).all()
    p = torch.from_numpy(pred).double().requires_grad_(True)
    mean, per = MO.rotation_error(p, torch.from_numpy(label))
    per.sum().backward()
    np.testing.assert_allclose(r.theta, per.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.jac, p.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert abs(r.mean - float(mean.detach())) < 1e-12
    np.testing.assert_allclose(R.exponential_map(label, R.FL).R.reshape(-1, 3, 3),
                               MO.exponential_map(torch.from_numpy(label)).numpy(),
                               rtol=1e-12, atol=1e-12)
    ref = R.rotation(pred, label, R.MP)       # and the 50-digit evaluation of the same code is what float64 approximates
    np.testing.assert_allclose(r.theta, ref.theta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.jac, ref.jac, rtol=1e-12, atol=1e-12)


def test_clipped_rows_have_the_clip_angle_and_no_gradient():
    c = R.CASE_BY_NAME["rot_b65"]
    x, ref = R.make_inputs(c), R.reference(c)
    hi, lo = [i for i, k in enumerate(x.kinds) if k == "equal"], [i for i, k in enumerate(x.kinds) if k == "exact_pi"]
    assert (ref.clipped[hi] == 1).all() and (ref.clipped[lo] == -1).all() and len(hi) == len(lo) == 5
    assert (ref.jac[hi + lo] == 0).all()
    assert (ref.theta[hi] == math.acos(R.LIM)).all() and (ref.theta[lo] == math.acos(-R.LIM)).all()
    near = [i for i, k in enumerate(x.kinds) if k in ("rel_1e-3", "near_pi")]
    assert (ref.clipped[near] == 0).all() and (1.0 / np.sqrt(1 - ref.t[near] ** 2)).max() > 200       # hard rows, not clipped


def test_row_kinds_are_what_they_claim():
    c = R.CASE_BY_NAME["rot_b600"]
    x = R.make_inputs(c)
    tsq = (x.pred.astype(F64) ** 2).sum(1)
    lsq = (x.label ** 2).sum(1)
    kind = np.array(x.kinds)
    assert set(kind) == set(R.ROW_KINDS)
    assert (tsq[kind == "below_switch"] >= 5e-3).all() and (tsq[kind == "below_switch"] < 1e-2).all()
    assert (tsq[kind == "above_switch"] >= 1e-2).all() and (tsq[kind == "above_switch"] < 1.5e-2).all()
    assert (tsq[kind == "pred_taylor"] < 1e-2).all() and (lsq[kind == "pred_taylor"] > 1e-2).any()
    assert (tsq[kind == "both_taylor"] < 1e-2).all() and (lsq[kind == "both_taylor"] < 1e-2).all()
    assert (tsq[kind == "large"] > math.pi ** 2).all() and (lsq[kind == "large"] > math.pi ** 2).all()
    assert (tsq[kind == "pred_zero"] == 0).all()
    ref = R.reference(c)
    for name, angle in (("rel_1e-1", 1e-1), ("rel_1e-2", 1e-2), ("rel_1e-3", 1e-3)):
        th = ref.theta[kind == name]
        assert (th > 0.79 * angle).all() and (th < 1.21 * angle).all(), name
    th = ref.theta[kind == "near_pi"]
    assert (math.pi - th < 1.01e-2).all() and (math.pi - th > 1e-3).all()


def test_float32_restatements_equal_the_oracle():
    from oracle import model_oracle as MO
    c = R.CASE_BY_NAME["rot_b63"]
    x = R.make_inputs(c)
    _, per = MO.translation_error(torch.from_numpy(x.tpred), torch.from_numpy(x.tlabel))
    # (torch sums the squares in another order)
    assert R.ulps(R.translation_error(x.tpred, x.tlabel, F32), per.numpy()) <= 1.0
    # Adam over three steps from a zero state, as the oracle starts
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(1003).astype(F32)
    params, opt = {"w": torch.from_numpy(p0.copy())}, MO.AdamTF()
    state = R.SimpleNamespace(p=p0, m=np.zeros(1003, F32), v=np.zeros(1003, F32))
    b1p, b2p = R.ADAM.beta1, R.ADAM.beta2
    for it in range(3):
        g = (rng.standard_normal(1003) * 10.0 ** (it - 1)).astype(F32)
        opt.apply(params, {"w": torch.from_numpy(g)})
        r = R.adam_step(state.p, g, state.m, state.v, b1p, b2p, dtype=F32)
        state, b1p, b2p = R.SimpleNamespace(p=r.p, m=r.m, v=r.v), r.b1p, r.b2p
        assert r.p.dtype == F32
        # (torch rounds float(lr_t) and the products once more)
        assert np.abs(r.p - params["w"].numpy()).max() <= 2.0 ** -22
        np.testing.assert_allclose(r.m, opt.m["w"].numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(r.v, opt.v["w"].numpy(), rtol=1e-6, atol=0)
    assert b1p == opt.b1p and b2p == opt.b2p
    for step, bsz in [(0, 128), (1, 128), (2, 128), (3, 32), (100, 2), (7, 40)]:
        assert float(R.bn_decay(step, bsz, dtype=F32)) == pytest.approx(MO.bn_decay_schedule(step, bsz), abs=1e-7)
        assert float(R.bn_decay(step, bsz)) == pytest.approx(MO.bn_decay_schedule(step, bsz), abs=1e-7)


def test_pool_and_edge_references_equal_autograd():
    for name in ("pool_mean_50x7x33", "pool_max_50x7x33"):
        c = R.CASE_BY_NAME[name]
        x = R.make_inputs(c)
        xs = x.x.astype(F64).reshape(c.G, c.R, c.C)
        xs[2] = np.where(np.isfinite(xs[2]), xs[2], 0.0)      # (autograd has no gradient through a group of -inf; its ties remain)
        t = torch.tensor(xs, requires_grad=True)
        out = t.mean(1) if c.mode == 1 else t.amax(1)
        (out * torch.from_numpy(x.g.astype(F64))).sum().backward()
        o, ties, _ = R.pool_rows(xs.reshape(-1, c.C).astype(F32), c.G, c.R, c.C, c.mode)
        np.testing.assert_allclose(o, out.detach().numpy(), rtol=1e-12, atol=1e-12)
        dx = R.pool_rows_grad(xs.reshape(-1, c.C).astype(F32), o, ties, x.g, c.G, c.R, c.C, c.mode)
        np.testing.assert_allclose(dx, t.grad.numpy().reshape(-1, c.C), rtol=1e-12, atol=1e-12)
    for name in R.names("edge")[:4]:
        c = R.CASE_BY_NAME[name]
        x = R.make_inputs(c)
        t = torch.tensor(x.x[:, :c.C].astype(F64).reshape(c.B, c.N, c.C), requires_grad=True)
        idx = torch.from_numpy(x.idx.astype(np.int64))
        nbr = t[torch.arange(c.B)[:, None, None], idx]
        ctr = t[:, :, None, :].expand_as(nbr)
        out = torch.cat([ctr, nbr - ctr], -1) if c.with_center else nbr - ctr
        np.testing.assert_array_equal(R.edge_feature(x.x, x.idx, c.B, c.N, c.k, c.C, c.with_center),
                                      out.detach().numpy().astype(F32).reshape(c.B * c.N * c.k, -1))
        (out.reshape(x.g.shape) * torch.from_numpy(x.g.astype(F64))).sum().backward()
        dx, _ = R.edge_feature_grad(x.g, x.idx, c.B, c.N, c.k, c.C, c.with_center)
        np.testing.assert_allclose(dx, t.grad.numpy().reshape(-1, c.C), rtol=1e-12, atol=1e-12)


def test_max_pool_cases_hold_the_ties_they_claim():
    hit = 0
    for name in R.names("pool"):
        c = R.CASE_BY_NAME[name]
        if c.mode != 2 or c.R < 2 or c.G < 3:
            continue
        out, ties, _ = R.pool_rows(R.make_inputs(c).x, c.G, c.R, c.C, 2)
        assert (ties[0] == 2).all() and (ties[1] == (3 if c.R >= 3 else 1)).all()
        assert (out[2] == -np.inf).all() and (ties[2] == c.R).all() and (ties[3:] == 1).all()
        hit += 1
    assert hit == 3


# ---- conditioning -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_is_well_posed(name):
    c = R.CASE_BY_NAME[name]
    redraws = R.condition(c)
    print("STEPPATHS redraws %s %d of %d rows" % (name, redraws, R.make_inputs(c).rows))
    assert redraws <= 0.01 * R.make_inputs(c).rows


# ---- bounds -------------------------------------------------------------------------------------------------------------
def _case_errors(c, mutant=None):
    """normalised errors of the restatement (mutant None) or of a mutant of the reference on one case"""
    x = R.make_inputs(c)
    if c.family == "rot":
        return R.rot_errors(c, x, R.rot_outputs(c, x, mutant))
    if c.family == "adam":
        return R.adam_errors_over_steps(c, x, R.adam_stepper(c, F64 if mutant else F32, mutant))[0]
    if c.family == "mean":
        return R.mean_errors(c, x, R.mean_outputs(c, x, mutant))
    if c.family == "pool":
        return R.pool_errors(c, x, R.pool_outputs(c, x, F64 if mutant else F32, mutant))
    if c.family == "edge":
        return R.edge_errors(c, x, R.edge_outputs(c, x))
    return R.elem_errors(c, x, R.elem_expected(c, x))


@functools.lru_cache(maxsize=None)
def _measured(name):
    return _case_errors(R.CASE_BY_NAME[name])


def test_constants_are_four_times_the_restatement():
    worst = {k: (0.0, None) for k in R.ALLOWED}
    for c in R.CASES:
        for k, v in _measured(c.name).items():
            if k in R.CONSTANT_OF:
                assert np.isfinite(v), (c.name, k)
                if v > worst[R.CONSTANT_OF[k]][0]:
                    worst[R.CONSTANT_OF[k]] = (v, c.name)
            else:
                assert v <= R.FIXED[k], (c.name, k, v)          # the restatement itself meets what is fixed by its meaning
    print("STEPPATHS measured:", {k: (round(v, 3), n) for k, (v, n) in worst.items()})
    for k, (v, _) in worst.items():
        assert R.ALLOWED[k] == R.pow2_ceil(4.0 * v), (k, v, R.ALLOWED[k])


def test_nan_row_of_the_translation_gradient_is_pinned():
    """a row with prediction == label: 0/0 in that row only, as TF and the oracle give; everything else stays finite"""
    c = R.CASE_BY_NAME["rot_b65"]
    x = R.make_inputs(c)
    got = R.rot_outputs(c, x)
    assert got["tper"][c.nan_row] == 0 and np.isnan(got["dtrans"][c.nan_row]).all()
    assert np.isfinite(np.delete(got["dtrans"], c.nan_row, 0)).all() and np.isfinite(got["trans_loss"])
    from oracle import model_oracle as MO
    p = torch.from_numpy(x.tpred).requires_grad_(True)
    MO.translation_error(p, torch.from_numpy(x.tlabel))[0].backward()
    assert np.array_equal(np.isnan(p.grad.numpy()), np.isnan(got["dtrans"]))


# A mutant is caught when some element lies more than MARGIN times outside its allowed bound (itself four times what the
# restatement reaches).  A margin below MARGIN means the case table lacks the rows that expose the mutant.
MARGIN = 4.0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_catch_the_mutant(mutant):
    hit, weakest = 0, (np.inf, None)
    for c in R.CASES:
        if not R.mutant_applies(mutant, c):
            continue
        e = _case_errors(c, mutant)
        over = max(v / max(R.allowed_of(k), 1.0 / MARGIN) for k, v in e.items())
        assert over >= MARGIN, (c.name, mutant, over, e)
        weakest = min(weakest, (over, c.name))
        hit += 1
    print("STEPPATHS mutant %s caught on %d cases, weakest margin %.4g (%s)" % (mutant, hit, weakest[0], weakest[1]))
    assert hit >= 3
