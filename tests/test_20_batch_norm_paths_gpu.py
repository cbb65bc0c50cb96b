"""GPU: every kernel path of cloudaae_bn_forward / cloudaae_bn_backward / cloudaae_colsum_f32 (csrc/bn.hip, csrc/bn_common.h)
against the float64 reference of tests/bn_reference.py, through the C ABI, per element and per channel.

Each output is compared with a bound formed from that element's own terms (u = 2^-24):
  save_mean, save_var  1 ulp of the fp64 moments rounded to fp32 (the kernels' sums are fp64)
  EMA shadows          2 ulp of a float32 evaluation of s - (s - stat) * (1 - decay) on the reference moments
  activation           c_fwd * u * (|y*inv| + |mean*inv| + |beta|)
  pooled mean          the group's mean of the activation bound + (pool_rows / 4) * u * mean|z|  (a row lane adds in fp32)
  pooled max           the activation bound of the maximum; tie count exact
  pool_stats           count exact; both x_hat sums c_stats * u * sum|x_hat| of the group
  dgamma, dbeta        c_dgamma * u * sum|dz * x_hat|,  c_dbeta * u * sum|dz|
  dy                   c_bwd * u * gr * (|dz| + |m1| + |x_hat * m2| * (1 + |mean| * rstd)),  gr = |gamma| * rstd
  dbias                c_dbias * u * gr * sum(|dz| + |m1| + |x_hat * m2|)   (the value is analytically zero in training mode)

The constants are not taken from the kernels.  tests/test_bn_reference_host.py measures the largest normalised error of
the reference's own float32 restatement against float64 over the case table; four times that, rounded up to a power of two,
is allowed (the factor covers the kernels' summation order inside their fp32 batches):
  measured  c_fwd 3.77  c_stats 474  c_bwd 297  c_dgamma 290  c_dbeta 1.13  c_dbias 148
  allowed   c_fwd 16    c_stats 2048 c_bwd 2048 c_dgamma 2048 c_dbeta 8     c_dbias 1024
c_bwd, c_dgamma and c_dbias are set by the |mean| / std = 2000 cases and by M = 2 (the rounding of the mean to fp32 moves
x_hat by u * |mean| * rstd whatever |x_hat| is), c_stats by pool_rows = 1 (a group's sum|x_hat| is one element).  Without
those cases the restatement reaches 56 (dy), 19 (dgamma), 5.5 (dbias) and 1.4 (pool_stats); profiles/notes_bn_paths.md has
the table and what the kernels reached.

Every case is conditioned (bn_reference.condition: no element whose ReLU mask or maximum fp32 cannot decide; asserted on
the CPU before anything is sent), runs twice into fresh buffers with bit-equal results (the sums have a fixed order), and
keeps the padding columns and the guards around every output untouched."""
import ctypes

import numpy as np
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64
SENTINEL = -12345.5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(a, ld):
    """a [M,C] as the first C columns of a [M,ld] device buffer whose other columns hold the sentinel"""
    if a is None:
        return None
    buf = np.full((a.shape[0], ld), SENTINEL, a.dtype)
    buf[:, :a.shape[1]] = a
    return _dev(buf)


class _Out(object):
    """an output of `rows` x `ld` elements between two guards, everything set to the sentinel"""

    def __init__(self, rows, ld, dtype=torch.float32, fill=None):
        self.flat = torch.full((rows * ld + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.flat[GUARD:GUARD + rows * ld].view(rows, ld)
        if fill is not None:
            self.view.copy_(_dev(fill))

    def ptr(self):
        return self.view.data_ptr()

    def get(self, cols):
        """the first `cols` columns, after checking that nothing else was written"""
        flat = self.flat.cpu().numpy()
        assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "a guard was overwritten"
        v = flat[GUARD:-GUARD].reshape(self.view.shape)
        assert (v[:, cols:] == SENTINEL).all(), "padding columns were overwritten"
        return v[:, :cols].copy()


def _param_start(c):
    rng = np.random.default_rng(77 + R.CASES.index(c))
    return {k: (3.0 * rng.standard_normal(c.C)).astype(F32) for k in ("dgamma", "dbeta", "dbias")}


def _run(hip, c, x, sync=None):
    """forward, then backward from what the forward saved; returns (forward outputs, backward outputs) as NumPy"""
    L = hip.lib()
    M, C, G = c.M, c.C, (c.M // c.pool_rows if c.pool_mode else 0)
    ldy, ldo, lddo, lddy = (C + p for p in c.pads)
    y, dout = _rows(x.y, ldy), _rows(x.dout, lddo)
    gamma, beta, decay = _dev(x.gamma), _dev(x.beta), _dev(np.array([x.decay], F32))
    ema_m, ema_v = _Out(1, C, fill=x.ema_mean[None]), _Out(1, C, fill=x.ema_var[None])
    save_m, save_v = _Out(1, C), _Out(1, C)
    out = _Out(M, ldo) if c.out else None
    pooled = _Out(G, C) if c.pool_mode else None
    ties = _Out(G, C) if c.pool_mode == 2 else None
    pstats = _Out(G * 3, C, torch.float64) if c.pool_stats else None
    ws = torch.full((int(L.cloudaae_bn_workspace_bytes(C)) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    p = lambda o: None if o is None else o.ptr()
    args = (M, C, y.data_ptr(), ldy, gamma.data_ptr(), beta.data_ptr(), c.training, decay.data_ptr(), ema_m.ptr(), ema_v.ptr(),
            save_m.ptr(), save_v.ptr(), c.relu, p(out), ldo, c.pool_rows, c.pool_mode, p(pooled), p(ties), p(pstats), ws.data_ptr())
    if sync is None:
        hip.check(L.cloudaae_bn_forward(*args, hip.stream()), "cloudaae_bn_forward")
    else:
        hip.check(L.cloudaae_bn_forward_sync(*args, None, 0, sync, hip.stream()), "cloudaae_bn_forward_sync")
    torch.cuda.synchronize()
    f = {"save_mean": save_m.get(C)[0], "save_var": save_v.get(C)[0], "ema_mean": ema_m.get(C)[0], "ema_var": ema_v.get(C)[0],
         "out": out.get(C) if out else None, "pooled": pooled.get(C) if pooled else None, "ties": ties.get(C) if ties else None,
         "pool_stats": pstats.get(C).reshape(G, 3, C) if pstats else None}

    start = _param_start(c)
    grads = {k: (None if c.null == k else _Out(1, C, fill=start[k][None] if c.accumulate else None)) for k in start}
    dy = _Out(M, lddy)
    dpooled = _dev(x.dpooled)
    ws.fill_(float("nan"))
    args = (M, C, y.data_ptr(), ldy, gamma.data_ptr(), beta.data_ptr(), save_m.ptr(), save_v.ptr(), c.training, c.relu,
            hip.ptr(dout), lddo, c.pool_rows, c.pool_mode, hip.ptr(dpooled), p(pooled) if c.pool_mode == 2 else None, p(ties),
            dy.ptr(), lddy, p(grads["dgamma"]), p(grads["dbeta"]), p(grads["dbias"]), c.accumulate,
            p(pstats) if c.bwd_stats else None, ws.data_ptr())
    if sync is None:
        hip.check(L.cloudaae_bn_backward(*args, hip.stream()), "cloudaae_bn_backward")
    else:
        hip.check(L.cloudaae_bn_backward_sync(*args, sync, hip.stream()), "cloudaae_bn_backward_sync")
    torch.cuda.synchronize()
    b = {"dy": dy.get(C)}
    b.update({k: (None if g is None else g.get(C)[0]) for k, g in grads.items()})
    for o in (save_m, save_v, out, pooled, ties, pstats):       # the backward pass left its inputs alone
        if o is not None:
            o.get(C)
    return f, b


def _same_bits(a, b):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        view = np.int64 if a[k].dtype == F64 else np.int32
        assert np.array_equal(a[k].view(view), b[k].view(view)), k


def _judge(c, x, f, b, fw, bw, tag):
    errs = R.case_errors(c, f, b, fw, bw, _param_start(c) if c.accumulate else None)
    if c.training:
        errs["ema_mean"] = R.ulps(f["ema_mean"], R.ema_update(x.ema_mean, fw.mean.astype(F32), x.decay, F32))
        errs["ema_var"] = R.ulps(f["ema_var"], R.ema_update(x.ema_var, fw.var.astype(F32), x.decay, F32))
    else:
        assert np.array_equal(f["ema_mean"], x.ema_mean) and np.array_equal(f["ema_var"], x.ema_var)
    for k in sorted(errs):
        print("BNPATHS %s %s %s %.4g allowed %g" % (tag, c.name, k, errs[k], R.allowed_of(k)))
    for v in list(f.values()) + list(b.values()):
        assert v is None or np.isfinite(v).all()
    bad = {k: v for k, v in errs.items() if not v <= R.allowed_of(k)}
    assert not bad, (c.name, bad)
    return errs


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_paths_against_float64(hip, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    assert x.ambiguous[-1] == 0, x.ambiguous          # the condition of every masked case, before anything is sent
    fw, bw = R.reference(c, x)
    f, b = _run(hip, c, x)
    if c.null:
        assert b[c.null] is None
    _judge(c, x, f, b, fw, bw, "plain")
    if c.const_col is not None:       # variance exactly 0: x_hat = 0, so dgamma = 0 and dy = gr * (dz - m1)
        k = c.const_col
        assert f["save_var"][k] == 0.0 and b["dgamma"][k] == 0.0
    if c.clip:                        # a channel whose rows the ReLU clips in every group passes no gradient
        assert (f["pooled"][:, 0] == 0).all() and (f["ties"][:, 0] == c.pool_rows).all() and (b["dy"][:, 0] == 0).all()
    f2, b2 = _run(hip, c, x)
    _same_bits(f, f2)
    _same_bits(b, b2)


@pytest.mark.parametrize("M,C,accumulate", R.COLSUM_CASES)
def test_colsum_against_float64(hip, M, C, accumulate):
    L = hip.lib()
    rng = np.random.default_rng(M + C + accumulate)
    xs = (rng.standard_normal((M, C)) * 2 + 0.5).astype(F32)
    start = (3.0 * rng.standard_normal(C)).astype(F32)
    want = xs.astype(F64).sum(0) + (start.astype(F64) if accumulate else 0.0)
    got = []
    for _ in range(2):
        xd = _rows(xs, C + 3)
        out = _Out(1, C, fill=start[None])
        ws = torch.full((int(L.cloudaae_bn_workspace_bytes(C)) // 8,), float("nan"), dtype=torch.float64, device="cuda")
        hip.check(L.cloudaae_colsum_f32(M, C, xd.data_ptr(), C + 3, out.ptr(), accumulate, ws.data_ptr(), hip.stream()),
                  "cloudaae_colsum_f32")
        torch.cuda.synchronize()
        got.append(out.get(C)[0])
    bound = np.spacing(np.abs(want.astype(F32))).astype(F64) + (R.U * np.abs(start.astype(F64)) if accumulate else 0.0)
    err = np.abs(got[0].astype(F64) - want)
    print("BNPATHS colsum M%d_C%d_acc%d %.4g of the bound" % (M, C, accumulate, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))


# ---- SyncBN entry points: a ctypes callback stands in for the exchange ---------------------------------------------------
SYNC_CASES = ["dense_M31_C65_relu_train", "dense_M1000_C70", "mean_R43", "mean_R43_out_both", "meanhot_3x32x64",
              "max_R200_out_both", "dense_M1000_C70_infer"]


def _sync(hip, C, world, calls):
    buf = torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")

    def allreduce(ctx, ptr, count, stream):
        calls.append(count)
        if ptr != buf.data_ptr() or count != 2 * C or (stream or 0) != (hip.stream() or 0):      # (ctypes: NULL arrives as None)
            return 1
        if world == 2:          # two ranks holding the same rows: every sum doubles (torch's current stream is `stream`)
            buf.mul_(2.0)
        return 0
    cb = hip.ALLREDUCE_FN(allreduce)
    st = hip.BnSyncStruct(cb, None, world, buf.data_ptr())
    return ctypes.pointer(st), (cb, st, buf)


@pytest.mark.parametrize("name", SYNC_CASES)
def test_sync_with_one_rank_gives_the_bits_of_the_plain_entry(hip, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    assert x.ambiguous[-1] == 0
    calls = []
    sync, keep = _sync(hip, c.C, 1, calls)
    f, b = _run(hip, c, x)
    fs, bs = _run(hip, c, x, sync)
    assert len(calls) == (2 if c.training else 0)
    if c.pool_mode == 0 and c.M <= 128:
        # the plain entry takes the one-launch kernel for small batches, the SyncBN one cannot: same formulas from the
        # same fp64 sums in another order, so both are judged by the reference instead
        fw, bw = R.reference(c, x)
        _judge(c, x, fs, bs, fw, bw, "sync1")
    else:
        _same_bits(f, fs)
        _same_bits(b, bs)


@pytest.mark.parametrize("name", SYNC_CASES)
def test_sync_with_two_ranks_of_the_same_rows_against_float64(hip, name):
    """world = 2 and a callback that doubles the sums model two ranks holding the same rows: the reference is the batch
    [y; y].  dgamma / dbeta / dbias stay this rank's sums, which are half of that batch's."""
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    assert x.ambiguous[-1] == 0
    two = lambda a: None if a is None else np.concatenate([a, a], 0)
    fw2 = R.forward(two(x.y), x.gamma, x.beta, c.training, x.ema_mean, x.ema_var, x.decay, c.relu, c.pool_rows, c.pool_mode)
    bw2 = R.backward(two(x.y), x.gamma, x.beta, c.training, x.ema_mean, x.ema_var, c.relu, two(x.dout), c.pool_rows, c.pool_mode,
                     two(x.dpooled))
    fw, bw = R.reference(c, x)      # one rank's rows: its activations and local sums ...
    for k in ("mean", "var", "m1", "m2"):       # ... which the moments and means of the doubled batch leave as they are
        a, d = getattr(fw2 if k in ("mean", "var") else bw2, k), getattr(fw if k in ("mean", "var") else bw, k)
        np.testing.assert_allclose(a, d, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(bw2.dy[:c.M], bw.dy, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(bw2.dgamma / 2, bw.dgamma, rtol=1e-11, atol=1e-13)
    calls = []
    sync, keep = _sync(hip, c.C, 2, calls)
    fs, bs = _run(hip, c, x, sync)
    assert len(calls) == (2 if c.training else 0)
    _judge(c, x, fs, bs, fw, bw, "sync2")
