"""GPU: every kernel path of cloudaae_edgeconv_forward / _backward / _revlists (csrc/edgeconv.hip) against the float64
reference of tests/edgeconv_reference.py, through the C ABI, element by element, in three stages each judged from its own
inputs (A: the [U | Q] product; B: everything between the products, from the fp32 pq; C: the two gradient products, from
the dpq the kernel returned).  Neighbour lists are constructed (a hub every point names, lists of exactly 64, 65 and 21
sources, an empty list, a self edge, one neighbour in all k slots), not computed by kNN.

Bounds, each formed from the element's own terms (u = 2^-24):
  pq                  lattice inputs: bit for bit on all three product paths; Gaussian inputs: c_pq * u * (sum|x||W_c| +
                      sum|x||W_n| + |b|) for U and the W_n term for Q
  save_mean, save_var 1 ulp;  EMA shadows 2 ulp of a float32 evaluation on the reference moments
  out                 mean: the group's mean of c_fwd * u * tz + (k / 4) * u * mean|z|;  max: c_fwd * u * tz of the maximum
  tie_count           exact;  bf16 twin: exactly the nearest-even rounding of the fp32 out the kernel stored
  edge_stats          count exact; both x_hat sums c_stats * u * sum|x_hat| over the point's k edges
  dgamma, dbeta, dbiases   c_dgamma * u * sum|dz x_hat|, c_dbeta * u * sum|dz|, c_dbias * u * gr * sum(|dz| + |m1| + |x_hat m2|)
  dpq                 S_i: c_S * u * sum_j B_ij;  T_m - S_m: c_T * u * (sum over m's list of B_ij + sum_j B_mj),
                      B_ij = gr * (|dz| + |m1| + |x_hat m2| * (1 + |mean| rstd));  an empty list gives exactly -S_m
  dx, dW              c_prod * u * sum|a||b| over the product's terms (bf16: operands rounded first; + |prior| when accumulating)

The constants are not taken from the kernels: tests/test_edgeconv_reference_host.py measures the float32 restatement of
the kernels' formulas against float64 over the case table; four times that, rounded up to a power of two, is allowed:
  measured  c_fwd 3.20  c_stats 1928  c_dgamma 2.72  c_dbeta 1.19  c_dbias 0.55  c_S 130  c_T 130  c_pq 3.79  c_prod 7.15
  allowed   c_fwd 16    c_stats 8192  c_dgamma 16    c_dbeta 8     c_dbias 4     c_S 1024 c_T 1024 c_pq 16    c_prod 32
(c_stats is set by k = 1, where a point's sum|x_hat| is one element; c_fwd and c_dbeta repeat what
tests/test_20_batch_norm_paths_gpu.py measured for the same formulas: 3.77 and 1.13.)  profiles/notes_edgeconv_paths.md has
the table and what the kernels reached.

Every output and scratch buffer sits between guards and has sentinel-filled padding columns; inputs are compared with what
was sent after the calls, pq after the backward call.  Every case runs twice into fresh buffers: everything that does not
pass through a reverse list is bit-equal; the dQ half of dpq, dx and dW are bit-equal under CLOUDAAE_DETERMINISTIC only."""
import ctypes

import numpy as np
import pytest
import torch

import bn_reference as BN
import edgeconv_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64
SENTINEL = -12345.5
FWD_KEYS = ("pq", "save_mean", "save_var", "ema_mean", "ema_var", "out", "ties", "edge_stats", "out16")
LIST_KEYS = ("dQ", "dx", "dw")          # what passes through a reverse list


class _Buf(object):
    """rows x ld elements between two guards, `off` elements past an aligned start; the first `cols` columns hold `fill`
    (or the sentinel), every other element the sentinel"""

    def __init__(self, rows, cols, ld=None, dtype=np.float32, fill=None, off=0):
        ld = cols if ld is None else ld
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, np.dtype(dtype)
        self.sent = np.array(SENTINEL if self.dtype.kind == "f" else (0xCFC7 if self.dtype.kind == "u" else -12345)).astype(dtype)
        host = np.full(2 * GUARD + off + rows * ld, self.sent, dtype)
        self.lo = GUARD + off
        if fill is not None:
            v = host[self.lo:self.lo + rows * ld].reshape(rows, ld)
            v[:, :cols] = np.asarray(fill).reshape(rows, cols)
        self.sent_host = host.copy()
        self.t = torch.from_numpy(host.view(np.int16) if dtype == np.uint16 else host).cuda()

    def ptr(self):
        return self.t.data_ptr() + self.lo * self.dtype.itemsize

    def get(self):
        """the rows x cols block, after checking that nothing around it was written"""
        flat = self.t.cpu().numpy().view(self.dtype)
        assert (flat[:self.lo] == self.sent).all() and (flat[self.lo + self.rows * self.ld:] == self.sent).all(), "a guard was overwritten"
        v = flat[self.lo:self.lo + self.rows * self.ld].reshape(self.rows, self.ld)
        assert (v[:, self.cols:] == self.sent).all(), "padding columns were overwritten"
        return v[:, :self.cols].copy()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(self.dtype).view(np.uint8), self.sent_host.view(np.uint8))


def _p(b):
    return None if b is None else b.ptr()


class _Call(object):
    """the buffers of one forward + backward pair of a case"""

    def __init__(self, hip, c, x):
        L = hip.lib()
        self.hip, self.c, self.x = hip, c, x
        P, C, cin, k = c.B * c.N, c.cout, c.cin, c.k
        self.P = P
        self.ldx, self.ldo, self.lddo, self.lddx, self.ldo16 = cin + c.ldx_pad, C + 3, C + c.lddo_pad, cin + 3, C + 8
        self.inputs = {"x": _Buf(P, cin, self.ldx, fill=x.x), "idx": _Buf(P, k, dtype=np.int32, fill=x.idx), "W": _Buf(2 * cin, C, fill=x.W),
                       "b": _Buf(1, C, fill=x.b), "gamma": _Buf(1, C, fill=x.gamma), "beta": _Buf(1, C, fill=x.beta),
                       "decay": _Buf(1, 1, fill=np.array([x.decay], F32)), "dout": _Buf(P, C, self.lddo, fill=x.dout, off=c.dout_off)}
        stats = c.estats and c.pool == 1
        self.ema_m, self.ema_v = _Buf(1, C, fill=x.ema_mean), _Buf(1, C, fill=x.ema_var)
        self.save_m, self.save_v = _Buf(1, C), _Buf(1, C)
        self.pq, self.out = _Buf(P, 2 * C), _Buf(P, C, self.ldo)
        self.ties = _Buf(P, C) if c.pool == 2 else None
        self.estats = _Buf(P * 3, C) if stats else None
        self.out16 = _Buf(P, C, self.ldo16, dtype=np.uint16) if c.b16out else None
        self.ws = torch.full((int(L.cloudaae_edgeconv_workspace_bytes(C)) // 8,), float("nan"), dtype=torch.float64, device="cuda")
        self.dpq = _Buf(P, 2 * C)
        self.rev = _Buf(1, c.B * (c.N + 1) + P * k, dtype=np.int32)
        rng = np.random.default_rng(5)
        self.dx_start = (2.0 * rng.standard_normal((P, cin))).astype(F32) if c.dx == "acc" else None
        self.dx = None if c.dx == "null" else _Buf(P, cin, self.lddx, fill=self.dx_start)
        self.dw = None if c.dw == "null" else _Buf(2 * cin, C, fill=np.zeros((2 * cin, C), F32) if c.dw == "zeroed" else None)
        self.grads = {n: (None if c.null == n else _Buf(1, C)) for n in ("dgamma", "dbeta", "dbiases")}

    def forward(self, sync=None):
        c, i, hip, L = self.c, self.inputs, self.hip, self.hip.lib()
        args = (c.B, c.N, c.k, c.cin, c.cout, i["x"].ptr(), self.ldx, i["idx"].ptr(), i["W"].ptr(), i["b"].ptr(), i["gamma"].ptr(),
                i["beta"].ptr(), c.training, i["decay"].ptr(), self.ema_m.ptr(), self.ema_v.ptr(), c.pool, self.pq.ptr(),
                self.save_m.ptr(), self.save_v.ptr(), self.out.ptr(), self.ldo, _p(self.ties), _p(self.estats), c.bf16,
                self.ws.data_ptr())
        if sync is not None:
            hip.check(L.cloudaae_edgeconv_forward_sync(*(args + (sync, hip.stream()))), "cloudaae_edgeconv_forward_sync")
        elif c.b16out:
            hip.check(L.cloudaae_edgeconv_forward_b16out(*(args + (self.out16.ptr(), self.ldo16, hip.stream()))),
                      "cloudaae_edgeconv_forward_b16out")
        else:
            hip.check(L.cloudaae_edgeconv_forward(*(args + (hip.stream(),))), "cloudaae_edgeconv_forward")
        torch.cuda.synchronize()
        P, C = self.P, c.cout
        f = {"pq": self.pq.get(), "save_mean": self.save_m.get()[0], "save_var": self.save_v.get()[0], "ema_mean": self.ema_m.get()[0],
             "ema_var": self.ema_v.get()[0], "out": self.out.get(), "ties": None if self.ties is None else self.ties.get(),
             "edge_stats": None if self.estats is None else self.estats.get().reshape(P, 3, C),
             "out16": None if self.out16 is None else self.out16.get()}
        return f

    def backward(self, sync=None, rev_ready=0, side=None):
        c, i, hip, L = self.c, self.inputs, self.hip, self.hip.lib()
        self.ws.fill_(float("nan"))
        pq_before = self.pq.t.clone()
        args = (c.B, c.N, c.k, c.cin, c.cout, i["x"].ptr(), self.ldx, i["idx"].ptr(), i["W"].ptr(), i["b"].ptr(), i["gamma"].ptr(),
                i["beta"].ptr(), c.training, c.pool, self.pq.ptr(), self.save_m.ptr(), self.save_v.ptr(),
                self.out.ptr() if c.pool == 2 else None, self.ldo, _p(self.ties), i["dout"].ptr(), self.lddo, self.dpq.ptr(),
                self.rev.ptr(), rev_ready, _p(self.dx), self.lddx, 1 if c.dx == "acc" else 0, _p(self.dw), 1 if c.dw == "zeroed" else 0,
                _p(self.grads["dbiases"]), _p(self.grads["dgamma"]), _p(self.grads["dbeta"]), _p(self.estats), c.bf16,
                self.ws.data_ptr())
        if sync is not None:
            hip.check(L.cloudaae_edgeconv_backward_sync(*(args + (sync, hip.stream(), side))), "cloudaae_edgeconv_backward_sync")
        else:
            hip.check(L.cloudaae_edgeconv_backward(*(args + (hip.stream(), side))), "cloudaae_edgeconv_backward")
        if side is not None:
            hip.stream_wait(hip.stream(), side)
        torch.cuda.synchronize()
        C = c.cout
        d = self.dpq.get()
        b = {"dS": d[:, :C].copy(), "dQ": d[:, C:].copy(), "dpq": d, "dx": None if self.dx is None else self.dx.get(),
             "dw": None if self.dw is None else self.dw.get()}
        for n, g in self.grads.items():
            b[n] = None if g is None else g.get()[0]
        b["rev"] = self.rev.get()[0]
        # the calls left their inputs alone, the backward call also what the forward call saved
        for n, buf in i.items():
            assert buf.unchanged(), "input %s was written" % n
        assert torch.equal(pq_before, self.pq.t), "the backward call wrote pq"
        for o in (self.save_m, self.save_v, self.out, self.ties, self.estats):
            if o is not None:
                o.get()
        return b


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b, keys, tag=""):
    for k in keys:
        if k not in a:
            continue
        if a[k] is None:
            assert b[k] is None, k
            continue
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _check_lists(c, x, rev, sorted_lists):
    """the reverse lists left in rev_scratch: offsets and, as sets, the sources of every list"""
    B, N, k = c.B, c.N, c.k
    off, src = rev[:B * (N + 1)].reshape(B, N + 1), rev[B * (N + 1):].reshape(B, N * k)
    for b in range(B):
        tgt = x.idx[b].ravel()
        deg = np.bincount(tgt, minlength=N)
        assert np.array_equal(off[b], np.concatenate([[0], np.cumsum(deg)])), "list offsets"
        order = np.argsort(tgt, kind="stable")
        want = order // k
        if sorted_lists:
            assert np.array_equal(src[b], want), "sorted lists"
        else:
            key = lambda s: np.lexsort((s, np.repeat(np.arange(N), deg)))
            assert np.array_equal(src[b][key(src[b])], want[key(want)]), "list contents"


def _judge(c, x, f, b, tag, ref=None):
    """stage A, B, C of one run against the reference; prints every figure before it asserts"""
    e = {}
    C = c.cout
    if c.family == "lattice":       # exact in fp32 and in bf16, in any order of summation
        e["pq_exact"] = float((f["pq"].astype(F64) != x.pq64).sum())
    else:
        a = R.stage_a(x.x, x.W, x.b, c.bf16)
        e["pq"] = R.product_errors(f["pq"], a.pq, a.t, "pq")["pq"]
    if c.family == "lattice":
        ref = R.reference(c) if ref is None else ref
        got = {"save_mean": f["save_mean"], "save_var": f["save_var"], "out": f["out"], "ties": f["ties"], "edge_stats": f["edge_stats"],
               "dgamma": b["dgamma"], "dbeta": b["dbeta"], "dbias": b["dbiases"], "dpq": b["dpq"]}
        e.update(R.stage_b_errors(got, ref))
        if c.training:
            e["ema_mean"] = BN.ulps(f["ema_mean"], BN.ema_update(x.ema_mean, ref.save_mean.astype(F32), x.decay, F32))
            e["ema_var"] = BN.ulps(f["ema_var"], BN.ema_update(x.ema_var, ref.save_var.astype(F32), x.decay, F32))
        else:
            assert np.array_equal(f["ema_mean"], x.ema_mean) and np.array_equal(f["ema_var"], x.ema_var)
            assert np.array_equal(f["save_mean"], x.ema_mean) and np.array_equal(f["save_var"], x.ema_var)
        empty = np.nonzero(ref.deg == 0)[0]
        assert np.array_equal(_bits(b["dQ"][empty]), _bits(F32(0) - b["dS"][empty])), "an empty list must give exactly 0 - S"
    if f["out16"] is not None:
        e["out16"] = float((f["out16"] != R.bf16_bits(f["out"])).sum())
    if b["dx"] is not None or b["dw"] is not None:
        cc = R.stage_c(b["dpq"], x.x, x.W, c.bf16, b.get("dx_start"))
        if b["dx"] is not None:
            e["dx"] = R.product_errors(b["dx"], cc.dx, cc.tdx, "dx")["dx"]
        if b["dw"] is not None:
            e["dw"] = R.product_errors(b["dw"], cc.dw, cc.tdw, "dw")["dw"]
    for k in sorted(e):
        print("ECPATHS %s %s %s %.4g allowed %g" % (tag, c.name, k, e[k], R.allowed_of(k)))
    for v in list(f.values()) + [b[k] for k in ("dpq", "dx", "dw", "dgamma", "dbeta", "dbiases")]:
        assert v is None or v.dtype.kind != "f" or np.isfinite(v).all()
    bad = {k: v for k, v in e.items() if not v <= R.allowed_of(k)}
    assert not bad, (c.name, tag, bad)
    return e


def _run(hip, c, x, sync=None, side=None, rev_ready=0, call=None):
    call = _Call(hip, c, x) if call is None else call
    f = call.forward(sync)
    if c.rev == 1 and not rev_ready:
        idxs = (ctypes.c_void_p * 1)(call.inputs["idx"].ptr())
        revs = (ctypes.c_void_p * 1)(call.rev.ptr())
        hip.check(hip.lib().cloudaae_edgeconv_revlists(1, c.B, c.N, c.k, idxs, revs, hip.stream()), "cloudaae_edgeconv_revlists")
        rev_ready = 1
    b = call.backward(sync, rev_ready, side)
    b["dx_start"] = call.dx_start
    return f, b


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_paths_against_float64(hip, knobs, name):
    c = R.CASE_BY_NAME[name]
    for key, want in c.why.items():        # the launcher's predicates, evaluated for this case
        assert R.launcher_paths(c)[key] == want, (key, want)
    x = R.make_inputs(c)
    assert x.ambiguous == 0 and x.seed == c.seed          # conditioned, before anything is sent
    if c.det:
        knobs("CLOUDAAE_DETERMINISTIC", 1)
    f, b = _run(hip, c, x)
    if c.null:
        assert b[c.null] is None
    _check_lists(c, x, b["rev"], c.det)
    _judge(c, x, f, b, "run1")
    if c.name == "one_point":        # a self edge, variance exactly 0: inv = gamma / sqrt(eps), z = beta
        assert (f["save_var"] == 0).all() and np.array_equal(f["out"][0] > 0, x.beta > 0)
    f2, b2 = _run(hip, c, x)
    _same_bits(f, f2, FWD_KEYS, "forward")
    _same_bits(b, b2, ("dS", "dgamma", "dbeta", "dbiases"), "backward")
    if c.det:
        _same_bits(b, b2, LIST_KEYS + ("rev",), "deterministic")
    else:
        _judge(c, x, f2, b2, "run2")


def test_lists_of_three_layers_from_one_launch(hip):
    cs = R.REV3
    xs = [R.make_inputs(c) for c in cs]
    assert not np.array_equal(xs[0].idx, xs[1].idx) and not np.array_equal(xs[1].idx, xs[2].idx)
    calls = [_Call(hip, c, x) for c, x in zip(cs, xs)]
    fs = [call.forward() for call in calls]
    c = cs[0]
    idxs = (ctypes.c_void_p * 3)(*[call.inputs["idx"].ptr() for call in calls])
    revs = (ctypes.c_void_p * 3)(*[call.rev.ptr() for call in calls])
    hip.check(hip.lib().cloudaae_edgeconv_revlists(3, c.B, c.N, c.k, idxs, revs, hip.stream()), "cloudaae_edgeconv_revlists")
    for c, x, call, f in zip(cs, xs, calls, fs):
        b = call.backward(None, 1)
        b["dx_start"] = None
        _check_lists(c, x, b["rev"], False)
        _judge(c, x, f, b, "rev3")


def test_side_stream_gives_the_bits_of_the_one_stream_call(hip):
    c = R.SIDE
    x = R.make_inputs(c)
    f, b = _run(hip, c, x)
    fs, bs = _run(hip, c, x, side=hip.side_stream())
    _same_bits(f, fs, FWD_KEYS)
    _same_bits(b, bs, ("dS", "dgamma", "dbeta", "dbiases"))
    _check_lists(c, x, bs["rev"], False)
    _judge(c, x, fs, bs, "side")


# ---- SyncBN entry points --------------------------------------------------------------------------------------------------
SYNC_CASES = ["arg_base", "inst_o128_k13_max", "nostats_o64_k20", "infer_o64_k10_mean"]


def _sync(hip, C, world, calls):
    buf = torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")

    def allreduce(ctx, ptr, count, stream):
        calls.append(count)
        if ptr != buf.data_ptr() or count != 2 * C or (stream or 0) != (hip.stream() or 0):
            return 1
        if world == 2:          # two ranks holding the same clouds: every sum doubles
            buf.mul_(2.0)
        return 0
    cb = hip.ALLREDUCE_FN(allreduce)
    st = hip.BnSyncStruct(cb, None, world, buf.data_ptr())
    return ctypes.pointer(st), (cb, st, buf)


@pytest.mark.parametrize("name", SYNC_CASES)
def test_sync_with_one_rank_gives_the_bits_of_the_plain_entry(hip, knobs, name):
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    knobs("CLOUDAAE_DETERMINISTIC", 1)
    calls = []
    sync, keep = _sync(hip, c.cout, 1, calls)
    f, b = _run(hip, c, x)
    fs, bs = _run(hip, c, x, sync)
    assert len(calls) == (2 if c.training else 0)
    _same_bits(f, fs, FWD_KEYS)
    _same_bits(b, bs, ("dS", "dgamma", "dbeta", "dbiases") + LIST_KEYS)


@pytest.mark.parametrize("name", SYNC_CASES)
def test_sync_with_two_ranks_of_the_same_clouds_against_float64(hip, name):
    """world = 2 and a callback that doubles the sums model two ranks holding the same clouds.  The moments and the means
    m1, m2 of the doubled batch are those of one rank's clouds, so are its activations and dpq; dgamma / dbeta / dbiases
    stay this rank's sums.  (Checked below on the reference itself before the kernel is judged by it.)"""
    c = R.CASE_BY_NAME[name]
    x = R.make_inputs(c)
    ref = R.reference(c)
    two = lambda a: np.concatenate([a, a], 0)
    P = c.B * c.N
    ref2 = R.stage_b(two(x.pq), two(x.idx.reshape(c.B, c.N, c.k)), 2 * c.B, c.N, c.k, x.gamma, x.beta, c.training, x.ema_mean,
                     x.ema_var, x.decay, c.pool, two(x.dout))
    np.testing.assert_allclose(ref2.save_mean, ref.save_mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref2.save_var, ref.save_var, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref2.dpq[:P], ref.dpq, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ref2.dgamma / 2, ref.dgamma, rtol=1e-11, atol=1e-13)
    calls = []
    sync, keep = _sync(hip, c.cout, 2, calls)
    fs, bs = _run(hip, c, x, sync)
    assert len(calls) == (2 if c.training else 0)
    _judge(c, x, fs, bs, "sync2")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
REFUSALS = {   # what is wrong -> (changes to the arguments, words of the message)
    "cout_96": (dict(cout=96), "64 or 128"),
    "k_33": (dict(k=33), "k must be"),
    "pool_mode_0": (dict(pool=0), "pool_mode"),
    "max_without_tie_count": (dict(pool=2, ties=None), "tie_count"),
    "inference_without_shadows": (dict(training=0, ema=None), "EMA"),
    "ldo_bf16_short": (dict(b16=1, ldo16=63), "bfloat16 output rows too short"),
    "nine_lists": (dict(lists=9), "1 to 8"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_launch_nothing(hip, what):
    L = hip.lib()
    ch, words = REFUSALS[what]
    B, N, cin = 2, 16, 8
    k, cout, pool, training = ch.get("k", 4), ch.get("cout", 64), ch.get("pool", 1), ch.get("training", 1)
    P, Cb = B * N, 128
    fill = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device="cuda")
    x, W, vec = torch.zeros(P, cin, device="cuda"), torch.zeros(2 * cin, Cb, device="cuda"), torch.ones(Cb, device="cuda")
    idx = torch.zeros(P * 33, dtype=torch.int32, device="cuda")
    outs = {n: fill(P * 2 * Cb) for n in ("pq", "out", "ties", "save_m", "save_v", "ema_m", "ema_v", "estats3", "out16")}
    outs["estats3"] = fill(P * 3 * Cb)
    ws = fill(int(L.cloudaae_edgeconv_workspace_bytes(128)) // 4)
    rev = torch.full((9, B * (N + 1) + P * 33), -12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    o = lambda n: outs[n].data_ptr()
    if "lists" in ch:
        n = ch["lists"]
        idxs = (ctypes.c_void_p * n)(*[idx.data_ptr()] * n)
        revs = (ctypes.c_void_p * n)(*[rev[i].data_ptr() for i in range(n)])
        rc = L.cloudaae_edgeconv_revlists(n, B, N, k, idxs, revs, hip.stream())
    else:
        ema = "ema" not in ch
        args = (B, N, k, cin, cout, x.data_ptr(), cin, idx.data_ptr(), W.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(),
                training, vec.data_ptr(), o("ema_m") if ema else None, o("ema_v") if ema else None, pool, o("pq"), o("save_m"),
                o("save_v"), o("out"), cout, o("ties") if "ties" not in ch else None, o("estats3"), 0, ws.data_ptr())
        if ch.get("b16"):
            rc = L.cloudaae_edgeconv_forward_b16out(*(args + (o("out16"), ch["ldo16"], hip.stream())))
        else:
            rc = L.cloudaae_edgeconv_forward(*(args + (hip.stream(),)))
    msg = L.cloudaae_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    print("ECPATHS refusal %s: rc %d, %s" % (what, rc, msg))
    assert rc != 0 and words in msg, (rc, msg)
    for n, t in outs.items():
        assert bool((t == SENTINEL).all()), n
    assert bool((ws == SENTINEL).all()) and bool((rev == -12345).all())
