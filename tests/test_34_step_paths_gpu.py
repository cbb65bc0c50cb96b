"""GPU: every kernel path of the loss and optimiser entry points of csrc/step.hip and csrc/so3_dual.h against the reference
of tests/step_reference.py (50 digits for the rotation, float64 for the rest), through the C ABI, per row and per element.

Each output is compared with a bound formed from that element's own terms (u64 = 2^-53, u32 = 2^-24):
  theta                c_theta * u64 * S / sqrt(1 - t^2), S = sum |Rl[r][k] Rp[r][k]|, t the unclipped cosine; on a clipped row
                       2 ulp of acos(+-0.9999999)
  Jacobian             c_jac * u64 * max|J| * (1 + 1 / (1 - t^2)); exactly 0 on a clipped row
  exponential map      c_exp * u64 * (1 + |axag|^2) for the entries, for R^T R - I and for det R - 1
  rot_loss, trans_loss 1 ulp of the float32 rounding of the reference mean
  d rot_pred           the Jacobian bound times |g w_rot / b|, + 1 ulp float32
  translation error    c_t * u32 * per;  its gradient c_tg * u32 * |gradient|; prediction == label is NaN in that row only
  Adam                 param c_p * u32 * (|p| + |update|), m c_m * u32 * (|m| + |g|), v c_v * u32 * (|v| + g^2), beta powers
                       1 ulp; each step judged from the state it started from, with the beta powers BEFORE the step
  mean, add-mean       1 ulp of the exactly rounded mean
  pool rows            mean c_pool * u32 * sum|x| / R; max and tie count exact; gradients 1 ulp
  edge feature         exact; its gradient c_eg * u32 * sum|terms| (unordered atomics: no repeat equality)
  elementwise, SGD, loss_mix, total   bit-equal to the float32 NumPy evaluation of the same expression

The constants are not taken from the kernels.  tests/test_step_reference_host.py measures the largest normalised error of
the reference's own restatement (the rotation in float64, the rest in float32) over the case table; four times that,
rounded up to a power of two, is allowed (the factor covers the device's sin / cos / acos / sqrt, which are not correctly
rounded, and the kernels' order of summation):
  measured  c_theta 8.81  c_jac 5.80  c_exp 1.81  c_t 2.21  c_tg 3.55  c_p 10.7  c_m 1.02  c_v 0.998  c_pool 2.39  c_eg 3.02
  allowed   c_theta 64    c_jac 32    c_exp 8     c_t 16    c_tg 16    c_p 64    c_m 8     c_v 4      c_pool 16    c_eg 16
profiles/notes_step_paths.md has the case table, the mutants and what the kernels reached.

Every output sits between guards filled with a sentinel, every case runs twice into fresh buffers (bit-equal where the
kernel is deterministic), and the rotation cases run through all three routes -- the single-purpose entry points,
cloudaae_pose_losses(_grad) and cloudaae_loss_tail -- which must agree bit for bit."""
import numpy as np
import pytest
import torch

import step_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64
SENTINEL = -12345.5
_TORCH = {F32: torch.float32, F64: torch.float64, np.int32: torch.int32}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out(object):
    """`n` elements between two guards, everything set to the sentinel (or `fill`); 16-byte aligned"""

    def __init__(self, n, dtype=F32, fill=None):
        self.sentinel = int(SENTINEL) if dtype is np.int32 else SENTINEL
        self.flat = torch.full((n + 2 * GUARD,), self.sentinel, dtype=_TORCH[dtype], device="cuda")
        self.view = self.flat[GUARD:GUARD + n]
        if fill is not None:
            self.view.copy_(_dev(np.asarray(fill, dtype).reshape(n)))
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def get(self, shape=None):
        """what was written, after checking that nothing around it was"""
        flat = self.flat.cpu().numpy()
        assert (flat[:GUARD] == self.sentinel).all() and (flat[-GUARD:] == self.sentinel).all(), "a guard was overwritten"
        v = flat[GUARD:-GUARD].copy()
        return v if shape is None else (v[0] if shape == () else v.reshape(shape))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_bits(a, b, skip=()):
    for k in a:
        if k in skip or a[k] is None:
            continue
        assert np.array_equal(_bits(np.asarray(a[k])), _bits(np.asarray(b[k]))), k


def _report(tag, name, errs):
    for k in sorted(errs):
        print("STEPPATHS %s %s %s %.4g allowed %g" % (tag, name, k, errs[k], R.allowed_of(k)))
    bad = {k: v for k, v in errs.items() if not v <= R.allowed_of(k)}
    assert not bad, (tag, name, bad)


def _ws(L, which="mean"):
    n = int(getattr(L, "cloudaae_%s_workspace_bytes" % which)()) // 8
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


# ---- rotation, translation, total: three routes ------------------------------------------------------------------------
def _route_parts(hip, c, x):
    """the single-purpose entry points"""
    L, b, n, s = hip.lib(), c.b, c.n, hip.stream()
    w = c.weights
    pred, label, tp, tl, d1, d2 = (_dev(a) for a in (x.pred, x.label, x.tpred, x.tlabel, x.d1, x.d2))
    gper32, _ = R.pose_scales(c)
    per, jac, rloss = _Out(b, F64), _Out(3 * b, F64), _Out(1)
    hip.check(L.cloudaae_rotation_error(b, hip.ptr(pred), hip.ptr(label), per.ptr(), jac.ptr(), rloss.ptr(), s), "rotation_error")
    gr = _dev(np.array([F32(c.g) * F32(w[2])], F32))
    drot = _Out(3 * b)
    hip.check(L.cloudaae_rotation_error_grad(b, jac.ptr(), hip.ptr(gr), drot.ptr(), s), "rotation_error_grad")
    tper, dtr, tloss = _Out(b), _Out(3 * b), _Out(1)
    hip.check(L.cloudaae_trans_error(b, hip.ptr(tp), hip.ptr(tl), tper.ptr(), s), "trans_error")
    gper = _dev(np.full(b, gper32, F32))
    hip.check(L.cloudaae_trans_error_grad(b, hip.ptr(tp), hip.ptr(tl), tper.ptr(), hip.ptr(gper), dtr.ptr(), s), "trans_error_grad")
    ws, ws2 = _ws(L), _ws(L)
    hip.check(L.cloudaae_mean_f32(b, tper.ptr(), tloss.ptr(), hip.ptr(ws), s), "mean_f32")
    xper, xyz = _Out(n), _Out(1)
    hip.check(L.cloudaae_add_mean_f32(n, hip.ptr(d1), hip.ptr(d2), xper.ptr(), xyz.ptr(), hip.ptr(ws2), s), "add_mean_f32")
    total = _Out(1)
    hip.check(L.cloudaae_loss_mix(xyz.ptr(), tloss.ptr(), rloss.ptr(), w[0], w[1], w[2], total.ptr(), s), "loss_mix")
    g = _dev(np.array([c.g], F32))
    ga, gb, gc = _Out(1), _Out(1), _Out(1)
    hip.check(L.cloudaae_loss_mix_grad(hip.ptr(g), w[0], w[1], w[2], ga.ptr(), gb.ptr(), gc.ptr(), s), "loss_mix_grad")
    expR = _Out(9 * b, F64)
    hip.check(L.cloudaae_exponential_map(b, hip.ptr(label), expR.ptr(), s), "exponential_map")
    torch.cuda.synchronize()
    want = R.loss_mix_grad(c.g, w, F32)
    assert (ga.get(()), gb.get(()), gc.get(())) == want
    return {"theta": per.get(), "jac": jac.get((b, 3)), "rot_loss": rloss.get(()), "drot": drot.get((b, 3)), "tper": tper.get(),
            "trans_loss": tloss.get(()), "dtrans": dtr.get((b, 3)), "per": xper.get(), "xyz": xyz.get(()), "total": total.get(()),
            "dxyz": ga.get(()), "expR": expR.get((b, 9))}


def _route_pose_losses(hip, c, x, xyz):
    """cloudaae_pose_losses + cloudaae_pose_losses_grad, from the xyz loss of the first route"""
    L, b, s = hip.lib(), c.b, hip.stream()
    w = c.weights
    pred, label, tp, tl = (_dev(a) for a in (x.pred, x.label, x.tpred, x.tlabel))
    xyz_d, g = _dev(np.array([xyz], F32)), _dev(np.array([c.g], F32))
    tper, tloss, rper, rjac, rloss, total = _Out(b), _Out(1), _Out(b, F64), _Out(3 * b, F64), _Out(1), _Out(1)
    hip.check(L.cloudaae_pose_losses(b, hip.ptr(tp), hip.ptr(tl), hip.ptr(pred), hip.ptr(label), hip.ptr(xyz_d), w[0], w[1], w[2],
                                     tper.ptr(), tloss.ptr(), rper.ptr(), rjac.ptr(), rloss.ptr(), total.ptr(), s), "pose_losses")
    dxyz, dt, dr = _Out(1), _Out(3 * b), _Out(3 * b)
    hip.check(L.cloudaae_pose_losses_grad(b, hip.ptr(tp), hip.ptr(tl), tper.ptr(), rjac.ptr(), hip.ptr(g), w[0], w[1], w[2],
                                          dxyz.ptr(), dt.ptr(), dr.ptr(), s), "pose_losses_grad")
    torch.cuda.synchronize()
    return {"theta": rper.get(), "jac": rjac.get((b, 3)), "rot_loss": rloss.get(()), "drot": dr.get((b, 3)), "tper": tper.get(),
            "trans_loss": tloss.get(()), "dtrans": dt.get((b, 3)), "xyz": F32(xyz), "total": total.get(()), "dxyz": dxyz.get(())}


def _route_loss_tail(hip, c, x, with_grad=True):
    L, b, n, s = hip.lib(), c.b, c.n, hip.stream()
    w = c.weights
    pred, label, tp, tl, d1, d2 = (_dev(a) for a in (x.pred, x.label, x.tpred, x.tlabel, x.d1, x.d2))
    g = _dev(np.array([c.g], F32))
    per, xyz = _Out(n), _Out(1)
    tper, tloss, rper, rjac, rloss, total = _Out(b), _Out(1), _Out(b, F64), _Out(3 * b, F64), _Out(1), _Out(1)
    dxyz, dt, dr = _Out(1), _Out(3 * b), _Out(3 * b)
    ws, ticket = _ws(L, "loss_tail"), _Out(1, np.int32, fill=0)
    grads = (hip.ptr(g), dxyz.ptr(), dt.ptr(), dr.ptr()) if with_grad else (None, None, None, None)
    for _ in range(2):          # a second launch finds the arrival counter where the first left it
        hip.check(L.cloudaae_loss_tail(n, hip.ptr(d1), hip.ptr(d2), per.ptr(), xyz.ptr(), b, hip.ptr(tp), hip.ptr(tl),
                                       hip.ptr(pred), hip.ptr(label), w[0], w[1], w[2], tper.ptr(), tloss.ptr(), rper.ptr(),
                                       rjac.ptr(), rloss.ptr(), total.ptr(), *grads, hip.ptr(ws), ticket.ptr(), s), "loss_tail")
        torch.cuda.synchronize()
        assert ticket.get(()) == 0
    out = {"theta": rper.get(), "jac": rjac.get((b, 3)), "rot_loss": rloss.get(()), "tper": tper.get(), "trans_loss": tloss.get(()),
           "per": per.get(), "xyz": xyz.get(()), "total": total.get(())}
    if with_grad:
        out.update({"drot": dr.get((b, 3)), "dtrans": dt.get((b, 3)), "dxyz": dxyz.get(())})
    else:       # nothing was written where no gradient was asked for
        assert (dr.get() == SENTINEL).all() and (dt.get() == SENTINEL).all() and dxyz.get(()) == SENTINEL
    return out


def _judge_route(c, x, got, tag):
    errs = R.rot_errors(c, x, dict(got, drot_scale=R.pose_scales(c)[1]))
    if "per" in got:
        per = x.d1 + x.d2
        errs["per"] = R.exact(got["per"], per)
        errs["mean"] = R.ulps(got["xyz"], F32(R.mean(per)))
    # the total is the float32 expression of the three losses this route wrote; d(total)/d(xyz_loss) = g * w_xyz
    errs["exact"] = float(got["total"] != R.loss_mix(got["xyz"], got["trans_loss"], got["rot_loss"], c.weights, F32))
    if "dxyz" in got:
        errs["exact"] += float(got["dxyz"] != F32(c.g) * F32(c.weights[0]))
    _report(tag, c.name, errs)
    if c.nan_row is not None and "dtrans" in got:
        assert np.isnan(got["dtrans"][c.nan_row]).all() and got["tper"][c.nan_row] == 0
        assert np.isfinite(np.delete(got["dtrans"], c.nan_row, 0)).all()
    for k in ("theta", "jac", "rot_loss", "drot", "tper", "trans_loss", "total"):
        assert k not in got or np.isfinite(got[k]).all(), k
    return errs


@pytest.mark.parametrize("name", R.names("rot"))
def test_rotation_routes_against_50_digits(hip, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    assert R.condition(c) <= 0.01 * c.b
    parts = _route_parts(hip, c, x)
    _judge_route(c, x, parts, "parts")
    pose = _route_pose_losses(hip, c, x, parts["xyz"])
    _judge_route(c, x, pose, "pose_losses")
    tail = _route_loss_tail(hip, c, x)
    _judge_route(c, x, tail, "loss_tail")
    # the three routes agree bit for bit (the mean of the single-purpose route is formed by cloudaae_mean_f32, whose
    # workgroups split the rows otherwise once there are more than 256: there it is held by its bound alone)
    loose = ("trans_loss", "total") if c.b > 256 else ()
    _same_bits(pose, tail)
    _same_bits(pose, parts, skip=loose)
    _same_bits(tail, parts, skip=loose + ("expR",))
    # again into fresh buffers; and the loss tail without an upstream gradient writes the same losses
    _same_bits(parts, _route_parts(hip, c, x))
    _same_bits(pose, _route_pose_losses(hip, c, x, parts["xyz"]))
    again = _route_loss_tail(hip, c, x, with_grad=False)
    _same_bits(again, tail)


# ---- Adam ---------------------------------------------------------------------------------------------------------------
STEP0, BATCH = 7.0, 40.0


def _adam_stepper(hip, c, entry, trace, bn_decay_out=True):
    """one launch of cloudaae_adam_tf (advance = 1) or cloudaae_adam_tf_step into fresh guarded buffers"""
    L, s, hp, bn = hip.lib(), hip.stream(), R.ADAM, R.BN_DECAY
    step_no = [STEP0]

    def step(state, grad, b1p, b2p):
        n = c.n
        p, m, v = _Out(n, fill=state.p), _Out(n, fill=state.m), _Out(n, fill=state.v)
        g = _Out(n, fill=grad)
        q1, q2 = _Out(1, fill=b1p), _Out(1, fill=b2p)
        args = (n, p.ptr(), g.ptr(), m.ptr(), v.ptr(), float(hp.lr), float(hp.beta1), float(hp.beta2), float(hp.eps), q1.ptr(),
                q2.ptr(), c.grad_scale)
        if entry == "adam_tf":
            hip.check(L.cloudaae_adam_tf(*args, 1, s), "adam_tf")
        else:
            counter, decay, ticket = _Out(1, fill=step_no[0]), (_Out(1) if bn_decay_out else None), _Out(1, np.int32, fill=0)
            hip.check(L.cloudaae_adam_tf_step(*args, counter.ptr(), 1.0, BATCH, bn.init, bn.decay_step, bn.rate, bn.clip,
                                              decay.ptr() if decay else None, ticket.ptr(), s), "adam_tf_step")
            torch.cuda.synchronize()
            step_no[0] += 1.0
            assert ticket.get(()) == 0 and counter.get(()) == step_no[0]          # the ticket is back, the counter went up once
            if decay:           # the decay of the NEXT step: the bits of the schedule kernel at the new counter
                want = _Out(1)
                hip.check(L.cloudaae_bn_decay_schedule(counter.ptr(), BATCH, bn.init, bn.decay_step, bn.rate, bn.clip,
                                                       want.ptr(), s), "bn_decay_schedule")
                torch.cuda.synchronize()
                assert _bits(decay.get()) == _bits(want.get())
                assert abs(float(decay.get(())) - float(R.bn_decay(step_no[0], BATCH))) <= 1e-7
        torch.cuda.synchronize()
        assert np.array_equal(_bits(g.get()), _bits(np.asarray(grad, F32)))         # the gradient is read only
        got = {"p": p.get(), "m": m.get(), "v": v.get(), "b1p": q1.get(()), "b2p": q2.get(())}
        trace.append(got)
        return got
    return step


@pytest.mark.parametrize("name", R.names("adam"))
def test_adam_against_float64(hip, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    traces = {}
    for tag, entry, decay in (("adam_tf", "adam_tf", True), ("adam_tf_step", "adam_tf_step", True),
                              ("adam_tf again", "adam_tf", True), ("adam_tf_step no decay", "adam_tf_step", False)):
        traces[tag] = []
        errs, final = R.adam_errors_over_steps(c, x, _adam_stepper(hip, c, entry, traces[tag], decay))
        _report(tag, name, errs)
        assert len(traces[tag]) == 3 and all(np.isfinite(final.__dict__[k]).all() for k in "pmv")
    for tag in list(traces)[1:]:        # the two entry points, and the repeats, give the same bits step after step
        for a, b in zip(traces["adam_tf"], traces[tag]):
            _same_bits(a, b)
    last = traces["adam_tf"][-1]
    if c.exhausted:
        assert last["b1p"] == 0.0
    else:
        assert R.ulps(last["b1p"], F32(F64(R.ADAM.beta1) ** 4)) <= 3 and R.ulps(last["b2p"], F32(F64(R.ADAM.beta2) ** 4)) <= 3


# ---- the other entry points ----------------------------------------------------------------------------------------------
def _run_mean(hip, c, x):
    L, s, n = hip.lib(), hip.stream(), c.n
    a, b = _dev(x.a), _dev(x.b)
    out, per, out2 = _Out(1), _Out(n), _Out(1)
    ws, ws2 = _ws(L), _ws(L)
    hip.check(L.cloudaae_mean_f32(n, hip.ptr(a), out.ptr(), hip.ptr(ws), s), "mean_f32")
    hip.check(L.cloudaae_add_mean_f32(n, hip.ptr(a), hip.ptr(b), per.ptr(), out2.ptr(), hip.ptr(ws2), s), "add_mean_f32")
    torch.cuda.synchronize()
    return {"mean": out.get(()), "per": per.get(), "add_mean": out2.get(())}


def _run_pool(hip, c, x):
    L, s = hip.lib(), hip.stream()
    G, Rr, C = c.G, c.R, c.C
    xd, g = _dev(x.x), _dev(x.g)
    out, ties, dx = _Out(G * C), (_Out(G * C) if c.mode == 2 else None), _Out(G * Rr * C)
    tp = ties.ptr() if ties else None
    hip.check(L.cloudaae_pool_rows(G, Rr, C, c.mode, hip.ptr(xd), out.ptr(), tp, s), "pool_rows")
    hip.check(L.cloudaae_pool_rows_grad(G, Rr, C, c.mode, hip.ptr(xd), out.ptr(), tp, hip.ptr(g), dx.ptr(), s), "pool_rows_grad")
    torch.cuda.synchronize()
    return {"out": out.get((G, C)), "ties": ties.get((G, C)) if ties else None, "dx": dx.get((G * Rr, C))}


def _run_edge(hip, c, x):
    L, s = hip.lib(), hip.stream()
    W = 2 * c.C if c.with_center else c.C
    xd, idx, g = _dev(x.x), _dev(x.idx), _dev(x.g)
    out, dx = _Out(c.B * c.N * c.k * W), _Out(c.B * c.N * c.C)
    hip.check(L.cloudaae_edge_feature(c.B, c.N, c.k, c.C, c.with_center, hip.ptr(xd), c.ldx, hip.ptr(idx), out.ptr(), s),
              "edge_feature")
    hip.check(L.cloudaae_edge_feature_grad(c.B, c.N, c.k, c.C, c.with_center, hip.ptr(g), hip.ptr(idx), dx.ptr(), s),
              "edge_feature_grad")
    torch.cuda.synchronize()
    return {"out": out.get((c.B * c.N * c.k, W)), "dx": dx.get((c.B * c.N, c.C))}


def _run_elem(hip, c, x):
    L, s = hip.lib(), hip.stream()
    if c.family == "rowvec":
        xd, v = _dev(x.a), _dev(x.v)
        out = _Out(x.a.size)
        hip.check(L.cloudaae_add_rowvec(c.B, c.R, c.D, hip.ptr(xd), hip.ptr(v), out.ptr(), s), "add_rowvec")
        torch.cuda.synchronize()
        return {"add_rowvec": out.get()}
    n = c.n
    a, b, cc, scalar = _dev(x.a), _dev(x.b), _dev(x.c), _dev(np.array([x.scalar], F32))
    o = {k: _Out(n) for k in ("add", "mul_add", "mul_add_no_a", "fill", "fill_add")}
    o["sgd"] = _Out(n, fill=x.a)
    hip.check(L.cloudaae_add_f32(n, hip.ptr(a), hip.ptr(b), o["add"].ptr(), s), "add_f32")
    hip.check(L.cloudaae_mul_add_f32(n, hip.ptr(a), hip.ptr(b), hip.ptr(cc), o["mul_add"].ptr(), s), "mul_add_f32")
    hip.check(L.cloudaae_mul_add_f32(n, None, hip.ptr(b), hip.ptr(cc), o["mul_add_no_a"].ptr(), s), "mul_add_f32")
    hip.check(L.cloudaae_fill_scaled(n, hip.ptr(scalar), float(R.FILL_SCALE), None, o["fill"].ptr(), s), "fill_scaled")
    hip.check(L.cloudaae_fill_scaled(n, hip.ptr(scalar), float(R.FILL_SCALE), hip.ptr(a), o["fill_add"].ptr(), s), "fill_scaled")
    hip.check(L.cloudaae_sgd(n, o["sgd"].ptr(), hip.ptr(b), float(R.SGD_LR), float(R.SGD_SCALE), s), "sgd")
    torch.cuda.synchronize()
    return {k: v.get() for k, v in o.items()}


OTHERS = {"mean": (_run_mean, R.mean_errors), "pool": (_run_pool, R.pool_errors), "edge": (_run_edge, R.edge_errors),
          "elem": (_run_elem, R.elem_errors), "rowvec": (_run_elem, R.elem_errors)}


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.family in OTHERS])
def test_other_entry_points(hip, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    assert R.condition(c) <= 0.01 * x.rows
    run, errors = OTHERS[c.family]
    got = run(hip, c, x)
    _report(c.family, name, errors(c, x, got))
    again = run(hip, c, x)
    _report(c.family + " again", name, errors(c, x, again))
    _same_bits(got, again, skip=("dx",) if c.family == "edge" else ())      # (the edge gradient's atomics are unordered)


def test_bn_decay_schedule_against_float64(hip):
    L, bn = hip.lib(), R.BN_DECAY
    for step, bsz in [(0, 128), (1, 128), (2, 128), (3, 32), (100, 2), (7, 40), (39, 1), (40, 1), (1000, 128)]:
        counter, out = _dev(np.array([step], F32)), _Out(1)
        hip.check(L.cloudaae_bn_decay_schedule(hip.ptr(counter), float(bsz), bn.init, bn.decay_step, bn.rate, bn.clip, out.ptr(),
                                               hip.stream()), "bn_decay_schedule")
        torch.cuda.synchronize()
        assert abs(float(out.get(())) - float(R.bn_decay(step, bsz))) <= 1e-7, (step, bsz)


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_reason(hip):
    L, s, hp = hip.lib(), hip.stream(), R.ADAM
    last = lambda: L.cloudaae_last_error().decode()
    buf = [_Out(16, fill=np.ones(16)) for _ in range(4)]
    q1, q2, counter, ticket = _Out(1, fill=0.9), _Out(1, fill=0.999), _Out(1, fill=0.0), _Out(1, np.int32, fill=0)
    for odd in range(4):            # each of param / grad / m / v four bytes off a 16-byte boundary
        ptrs = [b.ptr() + (4 if i == odd else 0) for i, b in enumerate(buf)]
        rc = L.cloudaae_adam_tf(8, *ptrs, float(hp.lr), 0.9, 0.999, 1e-8, q1.ptr(), q2.ptr(), 1.0, 1, s)
        assert rc != 0 and "aligned" in last()
        rc = L.cloudaae_adam_tf_step(8, *ptrs, float(hp.lr), 0.9, 0.999, 1e-8, q1.ptr(), q2.ptr(), 1.0, counter.ptr(), 1.0, 40.0,
                                     0.5, 40.0, 0.5, 0.99, None, ticket.ptr(), s)
        assert rc != 0 and "aligned" in last()
    torch.cuda.synchronize()
    assert all((b.get() == 1).all() for b in buf) and q1.get(()) == F32(0.9) and counter.get(()) == 0 and ticket.get(()) == 0
    o = _Out(64)
    d = _Out(64, F64)
    rc = L.cloudaae_pose_losses(0, o.ptr(), o.ptr(), o.ptr(), d.ptr(), o.ptr(), 1.0, 1.0, 1.0, o.ptr(), o.ptr(), d.ptr(),
                                d.ptr(), o.ptr(), o.ptr(), s)
    assert rc != 0 and "empty batch" in last()
    rc = L.cloudaae_pose_losses_grad(0, o.ptr(), o.ptr(), o.ptr(), d.ptr(), o.ptr(), 1.0, 1.0, 1.0, o.ptr(), o.ptr(), o.ptr(), s)
    assert rc != 0 and "empty batch" in last()
    rc = L.cloudaae_rotation_error(0, o.ptr(), d.ptr(), d.ptr(), d.ptr(), o.ptr(), s)
    assert rc != 0 and "empty batch" in last()
    rc = L.cloudaae_pool_rows(2, 0, 3, 1, o.ptr(), o.ptr(), None, s)
    assert rc != 0 and "rows > 0" in last()
    rc = L.cloudaae_pool_rows(2, 2, 3, 2, o.ptr(), o.ptr(), None, s)
    assert rc != 0 and "tie_count" in last()
    torch.cuda.synchronize()
    assert (o.get() == SENTINEL).all() and (d.get() == SENTINEL).all()
