"""GPU: every kernel path of the fully connected family (csrc/fc.hip) against the float64 reference of
tests/fc_reference.py, through the C ABI only, per element and per column.

Which path a shape takes is asked of cloudaae_fc_plan, never believed: test_case_table_reaches_every_path asserts that the
case table reaches every class the plan can produce (forward: CQ x vec x K whole / cut x row tiles x batch norm; backward:
RT x fine / coarse x vec x staged) and lists the ones it cannot (CQ = 4 exists exactly without batch norm at more than one
row tile; W is staged through LDS exactly on the coarse path at one row tile with whole quads).

Every case runs in two tiers.
  exact     x and dout are small integers, every other input a multiple of 1/8 (beta: of 1/16), so every partial sum of
            every product is a float32 whatever the slice, ticket or atomic order: y (all layers), and dw, dx and dbias of
            the layers whose d(y) is exact too (no batch norm; batch norm in inference mode, where the shadows' variance makes
            rstd exactly 2) must equal the reference BIT FOR BIT.  The message names the first differing (row, col) and its
            tile.  Under training-mode batch norm d(y) carries round-off: those outputs are judged as in the other tier.
  round     normal deviates, w / sqrt(K), and three cases with |mean| / std of about 50 per column.  Each output has a bound
            formed from its own terms (u = 2^-24):
              y                    c_y u (sum_k |x w| + |rowvec|) + u |bias|
              save_mean, save_var  1 ulp of the float64 moments of the device's own y (so nothing of y's bound is carried)
              EMA shadows          2 ulp of the float32 formula on those moments
              out                  c_out u (|y inv| + |mean inv| + |beta|), from the device's own y
              dgamma, dbeta, dbias the forms of tests/test_20_batch_norm_paths_gpu.py (dbias under training-mode batch norm is
                                   analytically zero and is bounded by its own term, c_dbias u gr sum(|dz| + |m1| + |x_hat m2|));
                                   without batch norm dbias: c_dbeta u sum|dout|
              dw                   c_dw u (sum_r |x| |d(y)| + |dw0|) + sum_r |x| b(d(y))
              dx                   c_dx u (sum_c |d(y)| |w| + |dx0|) + sum_c b(d(y)) |w|
            b(d(y)) = c_bwd u gr (|dz| + |m1| + |x_hat m2| (1 + |mean| rstd)) is the bound of d(y), which never leaves LDS; it
            is carried through the products in float64 from the reference (zero without batch norm).

The constants are not taken from the kernels.  tests/test_fc_reference_host.py measures the largest normalised error of the
reference's own float32 restatement (sums in index order) against float64 over the case table; four times that, rounded up to
a power of two, is allowed (the factor covers the kernels' different summation order inside fp32):
  measured  c_y 5.83  c_out 3.91  c_bwd 364   c_dgamma 94.4  c_dbeta 0.97  c_dbias 11.8  c_dw 8.66  c_dx 8.52
  allowed   c_y 32    c_out 16    c_bwd 2048  c_dgamma 512   c_dbeta 4     c_dbias 64    c_dw 64    c_dx 64
  reached   c_y 2.77  c_out 3.93  (d(y): -)   c_dgamma 21.2  c_dbeta 0.97  c_dbias 11.8  c_dw 7.49  c_dx 4.23   (the kernels)
c_bwd is set by the 4100 columns of coarsev_M40, c_dgamma by M = 2 (the fp32 rounding of the mean moves x_hat by
u |mean| rstd whatever |x_hat| is).  The |mean| / std = 50 cases stay away from M = 2, where a column of almost no variance
makes these constants a matter of the seed.  profiles/notes_fc_paths.md has the table, the cases that reached each figure
and three mutations of fc.hip the exact tier catches.

Under training-mode batch norm the exact tier only bounds dw and dx, so fc_reference.assert_coverage also requires every
backward class to hold a case whose dw, and one whose dx, IS compared bit for bit.

Contract, both tiers: every output lies between guards, with one more row and its padding columns holding a sentinel, all
unchanged afterwards; partials holds NaN before the call, afterwards exactly the rows that exist of every partial tile have
been published (the rest is still NaN) and the tickets are zero; every case runs twice into fresh
buffers (forward bit-equal always, backward bit-equal in the exact tier, where the fp32 atomics of dx add exact terms -- under
training-mode batch norm they are not, and dx is left out there); each NULL output, both
accumulate flags, absent shadows, absent scratch and pointers one float off their alignment are cases of the table."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fc_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64
SENTINEL = -12345.5
_LAYOUT_NOTE = " (by the layout of partials in csrc/fc.hip at the time of writing: [tiles][rts][splits][32][32 CQ]; if the scratch was re-laid-out, restate this check)"


class _Buf(object):
    """`rows` x `ld` floats between two guards, `off` floats past a 16-byte boundary; everything holds the sentinel except
    the first `cols` columns of the first data.shape[0] rows, which hold `data` (if given)"""

    def __init__(self, rows, cols, ld=None, off=0, data=None, dtype=np.float32, fill=SENTINEL):
        ld = cols if ld is None else ld
        host = np.full(GUARD + off + rows * ld + GUARD, fill, dtype)
        body = host[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)
        if data is not None:
            body[:data.shape[0], :cols] = data
        self.rows, self.cols, self.ld, self.off, self.fill = rows, cols, ld, off, fill
        self.before = host.copy()
        self.flat = torch.from_numpy(host).cuda()
        self.ptr = self.flat.data_ptr() + (GUARD + off) * host.itemsize
        assert self.flat.data_ptr() % 256 == 0 and (self.ptr % 16 == 0) == (off % 4 == 0)

    def get(self, rows=None):
        """the first `rows` rows of the data columns, after checking that nothing else was written"""
        rows = self.rows if rows is None else rows
        host = self.flat.cpu().numpy()
        lo, hi = GUARD + self.off, GUARD + self.off + self.rows * self.ld
        host, before = host.view(np.int32), self.before.view(np.int32)      # (bits: the scratch holds NaN)
        assert np.array_equal(host[:lo], before[:lo]) and np.array_equal(host[hi:], before[hi:]), "a guard was overwritten"
        body, was = host[lo:hi].reshape(self.rows, self.ld), before[lo:hi].reshape(self.rows, self.ld)
        assert np.array_equal(body[:, self.cols:], was[:, self.cols:]), "padding columns were overwritten"
        assert np.array_equal(body[rows:], was[rows:]), "rows past M were overwritten"
        return body[:rows, :self.cols].copy().view(self.before.dtype)

    def snapshot(self):
        """what the buffer holds now is what `unchanged` and the guards of `get` compare with from here on"""
        self.before = self.flat.cpu().numpy().copy()

    def unchanged(self):
        return np.array_equal(self.flat.cpu().numpy().view(np.int32), self.before.view(np.int32))


class _Layer(object):
    """the device buffers of one layer and its cloudaae_fc_layer record"""

    def __init__(self, hip, c, i, share=None):
        L = hip.lib()
        M, K, N = c.M, c.K, c.N
        ldx, lddo, lddx = K + c.pads[0], N + c.pads[1], K + c.pads[2]
        row = lambda a: None if a is None else a[None]
        self.c, self.i = c, i
        self.x = share.x if share else _Buf(M, K, ldx, c.offs[0], i.x)
        self.w = _Buf(K, N, N, c.offs[1], i.w)
        self.bias = None if i.bias is None else _Buf(1, N, data=row(i.bias))
        self.rowvec = None if i.rowvec is None else _Buf(M, c.rowvec_d, data=i.rowvec)
        self.dout = _Buf(M, N, lddo, 0, i.dout)
        self.y = _Buf(M + 1, N)
        self.dx = None if c.null == "dx" else (share.dx if share else _Buf(M + 1, K, lddx, 0, i.dx0))
        self.dw = None if c.null == "dw" else _Buf(K, N, N, c.offs[2], i.dw0 if c.acc_dw else None)
        grad = lambda k: None if c.null == k else _Buf(1, N, data=row(i.start[k]) if c.acc_pg else None)
        self.dbias = grad("dbias")
        self.gamma = self.beta = self.ema_mean = self.ema_var = self.save_mean = self.save_var = self.out = None
        self.dgamma = self.dbeta = None
        if c.bn:
            self.gamma, self.beta = _Buf(1, N, data=row(i.gamma)), _Buf(1, N, data=row(i.beta))
            if i.ema_mean is not None:
                self.ema_mean, self.ema_var = _Buf(1, N, data=row(i.ema_mean)), _Buf(1, N, data=row(i.ema_var))
            self.save_mean, self.save_var, self.out = _Buf(1, N), _Buf(1, N), _Buf(M + 1, N)
            self.dgamma, self.dbeta = grad("dgamma"), grad("dbeta")
        self.tickets = self.partials = None
        self.partials_floats = 0
        self.plan = R.plan_of(L._cdll, c)[0]
        if c.scratch:
            self.partials_floats =int(L.cloudaae_fc_forward_partials(M, K, N, c.bn))
            self.tickets = _Buf(1, int(L.cloudaae_fc_forward_tickets(M, N)), dtype=np.int32, fill=0)
            self.partials = _Buf(1, max(self.partials_floats, 4), fill=np.nan)
        p = lambda b: None if b is None else b.ptr
        self.record = hip.FcLayer(
            K=K, N=N, x=p(self.x), ldx=ldx, w=p(self.w), bias=p(self.bias), gamma=p(self.gamma), beta=p(self.beta),
            ema_mean=p(self.ema_mean), ema_var=p(self.ema_var), save_mean=p(self.save_mean), save_var=p(self.save_var),
            relu=c.relu, y=p(self.y), out=p(self.out), tickets=p(self.tickets), dout=p(self.dout), lddo=lddo, dx=p(self.dx),
            lddx=lddx, dw=p(self.dw), accumulate_dw=c.acc_dw, dgamma=p(self.dgamma), dbeta=p(self.dbeta), dbias=p(self.dbias),
            accumulate_param_grads=c.acc_pg, partials=p(self.partials), partials_floats=self.partials_floats,
            out_rowvec=p(self.rowvec), out_rowvec_d=c.rowvec_d)

    def forward_outputs(self):
        c, M = self.c, self.c.M
        f = {"y": self.y.get(M)}
        if c.bn:
            f.update(save_mean=self.save_mean.get()[0], save_var=self.save_var.get()[0], out=self.out.get(M))
            if self.ema_mean is not None:
                f.update(ema_mean=self.ema_mean.get()[0], ema_var=self.ema_var.get()[0])
        for k in ("y", "out", "save_mean", "save_var"):         # (the backward pass must leave them as they are now)
            if getattr(self, k) is not None:
                getattr(self, k).snapshot()
        if self.tickets is not None:
            assert not self.tickets.get().any(), "the tickets were not left at zero"
            scratch = self.partials.get()[0]
            # What met in the scratch, by the kernel's CURRENT layout (csrc/fc.hip, FcFwdArgs::partials; the header promises
            # only the size): [tiles][rts][splits] partial tiles of 32 x 32 CQ, every column of the tile included, of which
            # exactly the rows that exist were published (the last arrival reads no others: the rest still holds the NaN it
            # was given).  A re-layout of the scratch has to restate this check, not fix a kernel.
            p = self.plan
            if p["combine"]:
                tn = 32 * p["cq"]
                used = p["tiles"] * p["rts"] * p["splits"] * 32 * tn
                assert used <= self.partials_floats
                slabs = scratch[:used].reshape(p["tiles"], p["rts"], p["splits"], 32, tn)
                for rt in range(p["rts"]):
                    rows = min(32, M - 32 * rt)
                    assert np.isfinite(slabs[:, rt, :, :rows]).all(), "a partial tile was not published" + _LAYOUT_NOTE
                    assert np.isnan(slabs[:, rt, :, rows:]).all(), "rows past M were published into the scratch" + _LAYOUT_NOTE
                assert np.isnan(scratch[used:]).all()
            else:
                assert np.isnan(scratch).all(), "the scratch was written by a layer that meets in no scratch"
        return f

    def backward_outputs(self):
        c = self.c
        b = {k: (None if getattr(self, k) is None else getattr(self, k).get()[0]) for k in ("dbias", "dgamma", "dbeta")}
        b["dw"] = None if self.dw is None else self.dw.get()
        b["dx"] = None if self.dx is None else self.dx.get(c.M)
        for k in ("y", "out", "save_mean", "save_var", "x", "w", "dout", "gamma", "beta", "bias"):   # the inputs of the pass
            buf = getattr(self, k)
            assert buf is None or buf.unchanged(), k + " was written by the backward pass"
        return b


def _training(cases):
    modes = {c.training for c in cases if c.bn}
    assert len(modes) <= 1
    return modes.pop() if modes else 1


def _run(hip, cases, inputs, shared=False, wrappers=False):
    """forward then backward of a group of layers in one launch each; returns [(forward outputs, backward outputs)].
    shared: the members read one x and add into one dx.  wrappers: through cloudaae_fc_forward / cloudaae_fc_backward."""
    L = hip.lib()
    M, training = cases[0].M, _training(cases)
    layers = []
    for c, i in zip(cases, inputs):
        layers.append(_Layer(hip, c, i, share=layers[0] if shared and layers else None))
    records = (hip.FcLayer * len(layers))(*[l.record for l in layers])
    decay = torch.tensor([float(inputs[0].decay)], dtype=torch.float32, device="cuda")
    if wrappers:
        l, r = layers[0], layers[0].record
        hip.check(L.cloudaae_fc_forward(M, r.K, r.N, r.x, r.ldx, r.w, r.bias, r.gamma, r.beta, training, decay.data_ptr(),
                                        r.ema_mean, r.ema_var, r.save_mean, r.save_var, r.relu, r.y, r.out, r.tickets,
                                        r.partials, r.partials_floats, hip.stream()), "cloudaae_fc_forward")
    else:
        hip.check(L.cloudaae_fc_forward_group(M, len(layers), ctypes.addressof(records), training, decay.data_ptr(),
                                              hip.stream()), "cloudaae_fc_forward_group")
    torch.cuda.synchronize()
    fs = [l.forward_outputs() for l in layers]
    if wrappers:
        hip.check(L.cloudaae_fc_backward(M, r.K, r.N, r.x, r.ldx, r.w, r.y, r.gamma, r.beta, r.save_mean, r.save_var, training,
                                         r.relu, r.dout, r.lddo, r.dx, r.lddx, r.dw, r.accumulate_dw, r.dgamma, r.dbeta,
                                         r.dbias, r.accumulate_param_grads, hip.stream()), "cloudaae_fc_backward")
    else:
        hip.check(L.cloudaae_fc_backward_group(M, len(layers), ctypes.addressof(records), training, hip.stream()),
                  "cloudaae_fc_backward_group")
    torch.cuda.synchronize()
    bs = [l.backward_outputs() for l in layers]
    return list(zip(fs, bs))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _assert_exact(name, what, got, want64, tile_of):
    want = want64.astype(F32)
    assert np.array_equal(want.astype(F64), want64), "the reference of %s is no float32: the tier is not exact" % what
    if np.array_equal(_bits(got), _bits(want + F32(0.0))) or np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    r, col = (int(v) for v in bad[0])
    raise AssertionError("%s %s: %d elements differ, the first at (row %d, col %d) = %r, reference %r, in %s"
                         % (name, what, len(bad), r, col, float(got[r, col]), float(want[r, col]), tile_of(r, col)))


def _same_bits(a, b, keys=None):
    for k in (a if keys is None else keys):
        if a[k] is None:
            assert b[k] is None
        else:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k + " differs between two runs"


def _repeatable(*cases):
    """the backward outputs that two runs of the exact tier share bit for bit: all of them, except a dx whose slices add up
    (in fp32 atomics, in any order) products of a d(y) that is not exact -- batch norm in training mode"""
    return [k for k in ("dw", "dx", "dbias", "dgamma", "dbeta") if k != "dx" or not any(c.bn and c.training for c in cases)]


def _judge(hip, c, i, f, b, tag, dx_ref=None, dx_terms=None):
    """compare one layer's outputs with the reference; returns the normalised errors.  dx_ref / dx_terms: the reference and
    the bound's (denominator, carried d(y) bound) of a dx that several layers add into (the caller formed them)."""
    assert i.undecided == 0                 # the condition of every masked case
    plan_f, plan_b = R.plan_of(hip.lib()._cdll, c)
    fw = R.forward(c, i)
    ref_bn = R.forward(c, i, F64, f["y"]) if c.bn else fw
    bw = R.backward(c, i, ref_bn)
    for v in list(f.values()) + list(b.values()):
        assert v is None or np.isfinite(v).all()
    if i.tier == "exact":
        tn = 32 * plan_f["cq"]
        _assert_exact(c.name, "y", f["y"], fw.y, lambda r, col: "forward column tile %d (columns %d..%d), row tile %d, CQ %d, "
                      "%d K slices of %d" % (col // tn, col // tn * tn, col // tn * tn + tn - 1, r // 32, plan_f["cq"],
                                             plan_f["splits"], plan_f["kslice"]))
        if not c.bn or not c.training:
            where = "%s backward, RT %d, vec %d, staged %d" % ("fine" if plan_b["fine"] else "coarse", plan_b["RT"],
                                                               plan_b["vec"], plan_b["staged"])
            if b["dw"] is not None:
                _assert_exact(c.name, "dw", b["dw"], bw.dw, lambda r, col: "tile of W rows %d..%d, output slice %d (columns "
                              "%d..%d), %s" % (r // 32 * 32, r // 32 * 32 + 31, col // 128, col // 128 * 128, col // 128 * 128 + 127, where))
            if b["dx"] is not None and dx_ref is None:
                _assert_exact(c.name, "dx", b["dx"], bw.dx, lambda r, col: "row tile %d, tile of W rows %d..%d, %s"
                              % (r // 32, col // 32 * 32, col // 32 * 32 + 31, where))
        if not c.bn and b["dbias"] is not None:
            want = bw.dbias.astype(F64) + (i.start["dbias"].astype(F64) if c.acc_pg else 0.0)
            _assert_exact(c.name, "dbias", b["dbias"][None], want[None], lambda r, col: "output slice %d" % (col // 128))
    if c.bn and not c.training:             # inference: the shadows are read, never written, and are what is saved
        assert np.array_equal(_bits(f["ema_mean"]), _bits(i.ema_mean)) and np.array_equal(_bits(f["ema_var"]), _bits(i.ema_var))
        assert np.array_equal(_bits(f["save_mean"]), _bits(i.ema_mean)) and np.array_equal(_bits(f["save_var"]), _bits(i.ema_var))
    if c.bn:                                # the device's y decides every ReLU mask as the reference's does
        assert np.array_equal(ref_bn.zlin > 0, fw.zlin > 0)
    errs = R.forward_errors(c, i, f, fw, ref_bn)
    got_b = dict(b)
    if dx_ref is not None:
        got_b["dx"] = None
    errs.update(R.backward_errors(c, i, got_b, bw))
    for k in sorted(errs):
        print("FCPATHS %s %s %s %s %.4g allowed %g" % (tag, i.tier, c.name, k, errs[k], R.allowed_of(k)))
    bad = {k: v for k, v in errs.items() if not v <= R.allowed_of(k)}
    assert not bad, (c.name, i.tier, bad)
    return errs, bw


def test_case_table_reaches_every_path(hip):
    fwd, bwd = R.assert_coverage(hip.lib()._cdll)
    for k in sorted(fwd):
        print("FCPATHS forward (cq, vec, cut, rts, bn) = %s: %d cases, e.g. %s" % (k, len(fwd[k]), fwd[k][0]))
    for k in sorted(bwd):
        print("FCPATHS backward (RT, fine, vec, staged) = %s: %d cases, e.g. %s" % (k, len(bwd[k]), bwd[k][0]))
    for k, ok in sorted(R.forward_classes().items()):
        if not ok:
            print("FCPATHS forward class %s cannot be produced" % (k,))
    for k, ok in sorted(R.backward_classes().items()):
        if not ok:
            print("FCPATHS backward class %s cannot be produced" % (k,))


@pytest.mark.parametrize("tier", R.TIERS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_paths_against_float64(hip, name, tier):
    c = R.CASE_BY_NAME[name]
    i = R.make_inputs(c, tier)
    wrappers = not c.rowvec_d           # (the single-layer entry points have no row vector)
    (f, b), = _run(hip, [c], [i], wrappers=wrappers)
    if c.null not in (None, "bias"):
        assert b[c.null] is None
    _judge(hip, c, i, f, b, "single")
    (f2, b2), = _run(hip, [c], [i], wrappers=wrappers)
    _same_bits(f, f2)
    if tier == "exact":
        _same_bits(b, b2, _repeatable(c))


@pytest.mark.parametrize("tier", R.TIERS)
@pytest.mark.parametrize("group", [g[0] for g in R.GROUPS])
def test_groups_against_float64(hip, group, tier):
    _, members, shared = [g for g in R.GROUPS if g[0] == group][0]
    cases = [R.GROUP_CASES[n] for n in members]
    inputs = [R.make_inputs(c, tier) for c in cases]
    if shared:
        for i in inputs[1:]:
            i.x, i.dx0 = inputs[0].x, inputs[0].dx0
    got = _run(hip, cases, inputs, shared=shared)
    bws = []
    for c, i, (f, b) in zip(cases, inputs, got):
        bws.append(_judge(hip, c, i, f, b, "group " + group, dx_ref=True if shared else None)[1])
    if shared:
        # one dx: what it held plus the contribution of every member
        dx0 = inputs[0].dx0.astype(F64)
        want = dx0 + sum(bw.dx - dx0 for bw in bws)
        den = R.U * (sum(bw.tdx - np.abs(dx0) for bw in bws) + np.abs(dx0))
        carried = sum(R.dy_bound(c, bw) @ np.abs(i.w.astype(F64)).T for c, i, bw in zip(cases, inputs, bws))
        dx = got[0][1]["dx"]
        assert np.array_equal(_bits(dx), _bits(got[1][1]["dx"]))
        if tier == "exact" and all(not c.bn or not c.training for c in cases):
            _assert_exact(group, "dx", dx, want, lambda r, col: "row tile %d, tile of W rows %d.." % (r // 32, col // 32 * 32))
        e = R.ratio(dx.astype(F64) - want, den, carried)
        print("FCPATHS group %s %s shared dx %.4g allowed %g" % (group, tier, e, R.allowed_of("dx")))
        assert e <= R.allowed_of("dx")
    again = _run(hip, cases, inputs, shared=shared)
    for c, (f, b), (f2, b2) in zip(cases, got, again):
        _same_bits(f, f2)
        if tier == "exact":
            _same_bits(b, b2, _repeatable(*cases) if shared else _repeatable(c))
    if len(cases) == 1:                 # a group of one is the single-layer entry point
        (f3, b3), = _run(hip, cases, inputs, wrappers=True)
        _same_bits(got[0][0], f3)
        if tier == "exact":
            _same_bits(got[0][1], b3, _repeatable(cases[0]))


@pytest.mark.parametrize("name", ["cutv_M33_plain", "wholen_M65_plain", "coarsev_M5"])
def test_relu_is_ignored_without_batch_norm(hip, name):
    """include/cloudaae_hip.h: gamma == NULL, only y is written and `relu` is ignored in both directions"""
    c = R.CASE_BY_NAME[name]
    assert not c.bn and not c.relu
    i = R.make_inputs(c, "exact")
    with_relu = SimpleNamespace(**dict(vars(c), relu=1))
    (f0, b0), = _run(hip, [c], [i], wrappers=not c.rowvec_d)
    (f1, b1), = _run(hip, [with_relu], [i], wrappers=not c.rowvec_d)
    assert (f0["y"] < 0).any() and (i.dout < 0).any()
    _same_bits(f0, f1)
    _same_bits(b0, b1)
