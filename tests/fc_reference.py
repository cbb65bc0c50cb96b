"""NumPy restatement of the fully connected contract of include/cloudaae_hip.h (the comments above cloudaae_fc_forward,
cloudaae_fc_backward and struct cloudaae_fc_layer), written from the definition only: a yardstick for csrc/fc.hip.

  forward  : y = x w + bias (+ rowvec[r, c % d]);  with gamma the batch norm of y (bn_common.h's documented arithmetic):
             training : mean, var = biased moments over the M rows; shadows  s <- s - (s - stat) * (1 - decay)
             inference: mean, var = the shadows (save_* = those)
             inv = gamma / sqrt(var + 1e-3);  out = relu?(y * inv + (beta - mean * inv))
  backward : dz = dout * [out > 0] (ReLU mask from the forward's sign; batch norm only: without it `relu` is ignored);
             dbeta = sum dz;  dgamma = sum dz * x_hat;  d(y) = gamma * rstd * ((dz - m1) - x_hat * m2), m1 / m2 the batch means
             of dz and dz * x_hat (zero in inference mode);  dbias = sum_r d(y)  (no batch norm: d(y) = dout)
             dw (+)= x^T d(y);  dx += d(y) w^T   (each output starts from the caller's contents when its accumulate flag is
             set, dx always)

dtype = float64 is the reference.  dtype = float32 is a plain fp32 evaluation of the same formulas with every product sum
in index order (the column sums of the batch norm in fp64, the moments rounded to fp32 once, as bn_common.h documents): it
exists only so that tests/test_fc_reference_host.py can measure the constants of the bounds, never to judge a kernel.

The file also holds what the two test files share: the case table, the input generators of the two tiers (exact: every
partial sum representable in fp32; round-off: realistic magnitudes), `condition` (which chooses beta so that no ReLU mask
is undecidable in fp32), the normalised errors and the path classes of a case."""
from types import SimpleNamespace

import numpy as np

import bn_reference as B

EPS = 1e-3
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
TIERS = ("exact", "round")

# Largest normalised error of the float32 restatement against float64 over CASES (round-off tier), times four, rounded up
# to a power of two: measured by tests/test_fc_reference_host.py::test_constants_are_four_times_the_restatement, which also
# asserts that this table is what the rule gives.  The measured values are in profiles/notes_fc_paths.md.
ALLOWED = {"c_y": 32.0, "c_out": 16.0, "c_bwd": 2048.0, "c_dgamma": 512.0, "c_dbeta": 4.0, "c_dbias": 64.0, "c_dw": 64.0,
           "c_dx": 64.0}
CONSTANT_OF = {"y": "c_y", "out": "c_out", "dy": "c_bwd", "dgamma": "c_dgamma", "dbeta": "c_dbeta", "dbias": "c_dbias",
               "dbias_plain": "c_dbeta", "dw": "c_dw", "dx": "c_dx"}
FIXED = {"save_mean": 1.0, "save_var": 1.0, "ema_mean": 2.0, "ema_var": 2.0}


def allowed_of(name):
    return FIXED[name] if name in FIXED else ALLOWED[CONSTANT_OF[name]]


ratio, ulps, pow2_ceil = B._ratio, B.ulps, B.pow2_ceil


# ---- the case table -----------------------------------------------------------------------------------------------------
def case(name, M, K, N, bn=0, training=1, relu=0, pads=(0, 0, 0), offs=(0, 0, 0), rowvec_d=0, acc_dw=0, acc_pg=0, null=None,
         scratch=1, ema=1, offset=0.0):
    """pads = (ldx - K, lddo - N, lddx - K); offs = floats by which x, w and dw are moved off their 16-byte alignment;
    rowvec_d: width of the row vector added to y (no batch norm only); null: which of dx / dw / dgamma / dbeta / dbias /
    bias is passed as NULL; scratch = 0: tickets and partials NULL; ema = 0: the shadows NULL (training only); offset: the
    bias is this constant plus noise (|mean| / std of a column of y is about its size)."""
    assert not (rowvec_d and bn) and not (offset and relu) and (ema or training or not bn)
    return SimpleNamespace(name=name, M=M, K=K, N=N, bn=bn, training=training, relu=relu, pads=tuple(pads), offs=tuple(offs),
                           rowvec_d=rowvec_d, acc_dw=acc_dw, acc_pg=acc_pg, null=null, scratch=scratch, ema=ema,
                           offset=offset)


ROWS = (1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128)
# (K, N): K cut with uneven slices and an idle wave, without and with whole quads; K whole, without and with whole quads
TEMPLATES = (("cutn", 200, 37), ("cutv", 136, 64), ("wholen", 33, 130), ("wholev", 40, 132))
NULLS = (None, None, "dx", "dw", "dgamma", "bias", "dbeta", "dbias", "dw", "dx")


def _cases():
    t = []
    n = 0
    for M in ROWS:
        for tname, K, N in TEMPLATES:
            for bn in (1, 0):
                vec = tname.endswith("v")
                null = NULLS[n % len(NULLS)]
                if not bn and null in ("dgamma", "dbeta"):
                    null = None
                training = 1 if not bn else int(n % 3 != 0)
                t.append(case("%s_M%d_%s" % (tname, M, "bn" if bn else "plain"), M, K, N, bn=bn, training=training,
                              relu=int(bn and n % 4 != 1),
                              pads=((0, 4)[n % 2] if vec else (0, 4, 3)[n % 3], (0, 4, 3)[(n + 1) % 3], (0, 4, 3)[(n + 2) % 3]),
                              rowvec_d=0 if bn else (0, 5, N)[n % 3], acc_dw=int(n % 5 == 0), acc_pg=int(n % 7 < 2), null=null,
                              ema=int(not (bn and training and n % 5 == 2))))
                n += 1
    # the edges of one tile: N below a column quad, K below one group of eight
    for M in (3, 33):
        for K, N in ((5, 3), (8, 4), (7, 5), (1, 1)):
            for bn in (1, 0):
                t.append(case("tiny_M%d_K%d_N%d_%s" % (M, K, N, "bn" if bn else "plain"), M, K, N, bn=bn, relu=bn,
                              pads=(3 if K != 8 else 4, 3, 4)))
    # shapes of whole quads on pointers one float off: the non-vec bodies, either direction; dw alone unaligned
    for M in (32, 70):
        for which, offs in (("x", (1, 0, 0)), ("w", (0, 1, 0)), ("dw", (0, 0, 1))):
            for bn in (1, 0):
                t.append(case("off_%s_M%d_%s" % (which, M, "bn" if bn else "plain"), M, 136, 64, bn=bn, relu=bn, offs=offs,
                              pads=(4, 0, 0)))
    # batch norm without the tickets and the scratch (M <= 32: K stays whole in one workgroup per column tile)
    t.append(case("noscratch_M32_cutv", 32, 136, 64, bn=1, relu=1, scratch=0))
    t.append(case("noscratch_M31_cutn", 31, 200, 37, bn=1, relu=1, scratch=0, pads=(3, 4, 0)))
    t.append(case("noscratch_M17_plain", 17, 136, 64, scratch=0))
    # the backward's coarse path (a wave per tile of W): ceil(N / 128) * ceil(K / 32) > 1024
    for M in (5, 40, 100):
        t.append(case("coarsev_M%d" % M, M, 1000, 4100, bn=int(M == 40), relu=int(M == 40), acc_dw=int(M == 5),
                      pads=(0, 4, 3)))
        t.append(case("coarsen_M%d" % M, M, 993, 4097, bn=int(M == 100), relu=0, training=int(M != 100), acc_dw=int(M == 100),
                      acc_pg=1, pads=(3, 0, 4)))
    t.append(case("coarsev_M5_offdw", 5, 1000, 4100, offs=(0, 0, 1)))
    # (coarsev_M40 trains its batch norm, so its dw and dx are only bounded: the same path at two row tiles with an exact d(y))
    t.append(case("coarsev_M64_plain", 64, 1000, 4100, pads=(4, 0, 4), acc_dw=1))
    # the wide output layer of the model
    t.append(case("wide_M32", 32, 1024, 12288, rowvec_d=3, acc_dw=1))
    t.append(case("wide_M128", 128, 1024, 12288, rowvec_d=3))
    # |mean| / std of every column of y about 50 (no ReLU: the scale-and-shift form cannot decide the mask there)
    t.append(case("offset_M128_bn", 128, 136, 64, bn=1, offset=50.0))
    t.append(case("offset_M31_bn_infer", 31, 200, 37, bn=1, training=0, offset=50.0))
    # (not at M = 2: two rows can leave a column almost no variance, rstd then multiplies the fp32 rounding of the mean by up
    # to 1 / sqrt(eps), and the constants of dgamma and dbias become a matter of the seed -- 658 and 41053 for two of them)
    t.append(case("offset_M33_bn", 33, 33, 130, bn=1, offset=50.0))
    return t


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# Grouped launches: (name, member cases, members share x and dx).  Members of a group have the same M; members that share
# x have the same K, ldx and lddx.
GROUPS = (
    ("one", ("solo",), False),
    ("two", ("pairA", "pairB"), False),
    ("two_shared_x", ("shareA", "shareB"), True),
    ("four_mixed_cq", ("mixed_plain", "mixed_bn0", "mixed_bn1", "mixed_bn2"), False),
    ("four_M31", ("quad0", "quad1", "quad2", "quad3"), False),
)
GROUP_CASES = {c.name: c for c in (
    # (the batch-norm mode is an argument of the launch: the members with batch norm of one group agree on it)
    case("solo", 33, 200, 37, bn=1, relu=1, training=0, pads=(3, 4, 0)),
    case("pairA", 65, 136, 64, bn=1, relu=1, pads=(4, 3, 0)),
    case("pairB", 65, 40, 132, rowvec_d=5, acc_pg=1, pads=(0, 0, 3)),
    case("quad0", 31, 200, 37, bn=1, relu=1, training=0, pads=(0, 3, 4), acc_dw=1),
    case("quad1", 31, 136, 64, null="dx"),
    case("quad2", 31, 33, 130, bn=1, relu=0, training=0, null="dbias"),
    case("quad3", 31, 40, 132, bn=1, relu=1, training=0, scratch=0),
    # two consumers of one x whose gradients meet in one dx
    case("shareA", 40, 72, 132, bn=1, relu=1, training=0, pads=(4, 0, 3)),
    case("shareB", 40, 72, 37, pads=(4, 3, 3), acc_dw=1),
    # M = 40: a layer without batch norm takes 128-column tiles (CQ = 4), the three with it 64-column tiles (CQ = 2), in ONE
    # launch whose LDS is sized for the former
    case("mixed_plain", 40, 136, 260, rowvec_d=4),
    case("mixed_bn0", 40, 200, 37, bn=1, relu=1, pads=(3, 0, 0)),
    case("mixed_bn1", 40, 64, 64, bn=1, relu=1, training=1, ema=0),
    case("mixed_bn2", 40, 33, 130, bn=1, relu=0, acc_pg=1),
)}


def case_by_name(name):
    return CASE_BY_NAME[name] if name in CASE_BY_NAME else GROUP_CASES[name]


def seed_of(c, tier):
    """from the case's name, so that adding or removing a case leaves every other case's inputs as they are"""
    import zlib
    return zlib.crc32(("%s/%s" % (c.name, tier)).encode())


# ---- which path a case takes (what cloudaae_fc_plan is asked) -----------------------------------------------------------
def vec_of(c):
    """(forward, backward): whether the launch code finds whole quads on aligned pointers (buffers themselves are aligned)"""
    K, N, ldx = c.K, c.N, c.K + c.pads[0]
    fwd = K % 8 == 0 and ldx % 4 == 0 and N % 4 == 0 and c.offs[0] == 0 and c.offs[1] == 0
    bwd = N % 4 == 0 and c.offs[1] == 0 and (c.null == "dw" or c.offs[2] == 0)
    return int(fwd), int(bwd)


def forward_classes():
    """{(cq, vec, K cut, rts, bn): producible}: a layer without batch norm takes CQ = 4 exactly at more than one row tile,
    every other layer CQ = 2 (fc_fwd_plan); each of those exists with K whole and K cut, with and without whole quads"""
    return {(cq, vec, cut, rts, bn): (cq == 4) == (not bn and rts > 1)
            for cq in (2, 4) for vec in (0, 1) for cut in (0, 1) for rts in (1, 2, 3, 4) for bn in (0, 1)}


def backward_classes():
    """{(RT, fine, vec, staged): producible}: W goes through LDS in whole lines (staged) exactly on the coarse path at one
    row tile with whole quads (fc_bwd_body's STAGED && parts == 2)"""
    return {(rt, fine, vec, staged): staged == int(vec and rt == 1 and not fine)
            for rt in (1, 2, 4) for fine in (0, 1) for vec in (0, 1) for staged in (0, 1)}


def plan_of(lib, c):
    """what cloudaae_fc_plan says of a case: (forward dict, backward dict); lib: the loaded library (ctypes)"""
    import ctypes
    fv, bv = vec_of(c)
    out = (ctypes.c_int * 6)()
    assert lib.cloudaae_fc_plan(0, c.M, c.K, c.N, c.bn, fv, c.scratch, out) == 0
    f = dict(zip(("cq", "tiles", "rts", "splits", "kslice", "combine"), out), vec=fv, bn=c.bn)
    assert lib.cloudaae_fc_plan(1, c.M, c.K, c.N, c.bn, bv, c.scratch, out) == 0
    b = dict(zip(("RT", "fine", "parts", "tiles_per_block", "by", "staged"), out), vec=bv)
    return f, b


def classes_of(lib, c):
    f, b = plan_of(lib, c)
    return (f["cq"], f["vec"], int(f["splits"] > 1), f["rts"], f["bn"]), (b["RT"], b["fine"], b["vec"], b["staged"])


# what a few shapes of the table are there for, stated so that a changed threshold fails here and not silently
EXPECTED_PLANS = {
    "cutn_M1_bn": (dict(cq=2, splits=3, kslice=72, combine=1), dict(RT=1, fine=1, parts=4)),
    "cutv_M1_bn": (dict(cq=2, splits=2, kslice=72, combine=1), dict(RT=1, fine=1, parts=4, tiles_per_block=1)),
    "wholen_M128_bn": (dict(cq=2, rts=4, splits=1, combine=1), dict(RT=4, fine=1, tiles_per_block=2)),
    "wholen_M128_plain": (dict(cq=4, rts=4, splits=1, combine=0), dict(RT=4, fine=1)),
    "wholev_M32_plain": (dict(cq=2, rts=1, splits=1, combine=0), dict(RT=1, fine=1, staged=0)),
    "noscratch_M32_cutv": (dict(cq=2, splits=1, combine=0), dict(RT=1)),
    "coarsev_M5": (dict(cq=2, rts=1), dict(RT=1, fine=0, parts=2, staged=1)),
    "coarsev_M5_offdw": (dict(cq=2, vec=1), dict(RT=1, fine=0, vec=0, staged=0)),
    "coarsen_M100": (dict(cq=2, rts=4, bn=1), dict(RT=4, fine=0, parts=2, staged=0)),
    "coarsev_M40": (dict(cq=2, rts=2, bn=1), dict(RT=2, fine=0, staged=0)),
    "coarsev_M64_plain": (dict(cq=4, rts=2, vec=1), dict(RT=2, fine=0, parts=2, vec=1, staged=0)),
    "wide_M32": (dict(cq=2, tiles=192, rts=1, splits=1, combine=0), dict(RT=1, fine=0, parts=2, tiles_per_block=8, by=4, staged=1)),
    "wide_M128": (dict(cq=4, tiles=96, rts=4, splits=1, combine=0), dict(RT=4, fine=0, parts=2, tiles_per_block=8, by=4, staged=0)),
}


def bit_compared(c, product):
    """whether the exact tier compares this product (dw or dx) of the case with the reference bit for bit: it exists and
    d(y) is exact -- no batch norm, or batch norm in inference mode"""
    return c.null != product and not (c.bn and c.training)


def assert_coverage(lib):
    """Every path class the plan can produce is reached by a case of the table (each case runs in both tiers); the classes
    it cannot produce are listed by forward_classes / backward_classes and no case may land in one."""
    fwd, bwd = {}, {}
    for c in CASES:
        f, b = classes_of(lib, c)
        fwd.setdefault(f, []).append(c.name)
        bwd.setdefault(b, []).append(c.name)
    fc, bc = forward_classes(), backward_classes()
    assert all(fc[k] for k in fwd), [k for k in fwd if not fc[k]]
    assert all(bc[k] for k in bwd), [k for k in bwd if not bc[k]]
    missing = [("forward", k) for k, ok in fc.items() if ok and k not in fwd] + \
              [("backward", k) for k, ok in bc.items() if ok and k not in bwd]
    assert not missing, missing
    # Under training-mode batch norm d(y) carries round-off, and the exact tier only bounds dw and dx there: every backward
    # class therefore needs a case whose d(y) is exact (bit_compared) for each of the two products, or a misplaced row on
    # that path would meet a bound only.
    for k, names in bwd.items():
        for product in ("dw", "dx"):
            assert any(bit_compared(CASE_BY_NAME[n], product) for n in names), \
                "no exact-tier case compares %s bit for bit on the backward path %s: %s" % (product, k, names)
    for name, (f_want, b_want) in EXPECTED_PLANS.items():
        f, b = plan_of(lib, CASE_BY_NAME[name])
        assert {k: f[k] for k in f_want} == f_want, (name, f)
        assert {k: b[k] for k in b_want} == b_want, (name, b)
    # parts is 4 (fine) or 2 (coarse): the launch code has no third value
    for c in CASES:
        b = plan_of(lib, c)[1]
        assert b["parts"] == (4 if b["fine"] else 2)
    # a group that mixes a CQ = 4 layer with CQ = 2 layers at more than one row tile
    cqs = [plan_of(lib, GROUP_CASES[n])[0]["cq"] for n in dict((g[0], g[1]) for g in GROUPS)["four_mixed_cq"]]
    assert cqs == [4, 2, 2, 2], cqs
    # every part of the contract is some case's: each NULL, both accumulate flags, absent shadows and scratch, each offset
    have = lambda pred: any(pred(c) for c in CASES)
    for which in ("dx", "dw", "dbias", "bias", "dgamma", "dbeta"):
        assert have(lambda c: c.null == which), which
    assert have(lambda c: c.acc_dw and c.N == 12288) and have(lambda c: c.acc_pg and c.bn) and have(lambda c: c.acc_pg and not c.bn)
    assert have(lambda c: c.bn and c.training and not c.ema) and have(lambda c: c.bn and not c.training and c.relu)
    assert have(lambda c: c.bn and not c.scratch and c.M == 32)
    for k in range(3):
        assert have(lambda c: c.offs[k] == 1)
    assert {p for c in CASES for p in c.pads} == {0, 4, 3}
    return fwd, bwd


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _exact_var():
    """a float32 v with float32(v + float32(1e-3)) == 0.25: the inference-mode rstd of the exact tier is exactly 2"""
    v = F32(0.25) - F32(EPS)
    for _ in range(64):
        if F32(v + F32(EPS)) == F32(0.25):
            return v
        v = np.nextafter(v, F32(1.0) if F32(v + F32(EPS)) < F32(0.25) else F32(0.0))
    raise AssertionError("no such float32")


EXACT_VAR = _exact_var()


def make_inputs(c, tier):
    """The inputs of a case, conditioned: namespace of x [M,K], w [K,N], bias, rowvec, gamma, beta, ema_mean, ema_var (None:
    NULL), decay, dout, and what the outputs hold before the call: dx0, dw0, start (dgamma, dbeta, dbias).
    exact: x and dout small integers, the rest multiples of 1/8 (beta: of 1/16), so that every partial sum of every product
    is a float32 whatever its order: |y| <= 1024 * 3 * 8 + 24 and |dx| <= 12288 * 12 * 8 + 16 units of 1/8, below 2^24.
    round: normal deviates, w / sqrt(K)."""
    rng = np.random.default_rng(seed_of(c, tier))
    M, K, N = c.M, c.K, c.N
    assert K <= 1024 and N <= 12288
    if tier == "exact":
        ints = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(F64)
        x, dout = ints(-3, 3, M, K), ints(-3, 3, M, N)
        w, bias = ints(-8, 8, K, N) / 8, ints(-16, 16, N) / 8
        rowvec = ints(-16, 16, M, c.rowvec_d) / 8 if c.rowvec_d else None
        gamma = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, N)] * np.where(rng.random(N) < 0.25, -1.0, 1.0)
        beta = (2 * ints(-8, 7, N) + 1) / 16
        ema_mean, ema_var = ints(-16, 16, N), np.full(N, EXACT_VAR, F64)
        dx0, dw0 = ints(-16, 16, M, K) / 8, ints(-16, 16, K, N) / 8
        start = {k: ints(-16, 16, N) / 8 for k in ("dgamma", "dbeta", "dbias")}
    else:
        rnd = lambda *s: rng.standard_normal(s)
        x, dout = rnd(M, K), rnd(M, N)
        w = rnd(K, N) / np.sqrt(K)
        bias = (c.offset * np.where(rnd(N) < 0, -1.0, 1.0) + rnd(N)) if c.offset else 0.3 * rnd(N)
        rowvec = rnd(M, c.rowvec_d) if c.rowvec_d else None
        gamma = 1.0 + 0.2 * rnd(N)
        gamma[1::7] *= -1.0
        beta = 0.3 * rnd(N)
        ema_mean, ema_var = bias + 0.3 * rnd(N), 0.5 + np.abs(rnd(N))
        dx0, dw0 = rnd(M, K), rnd(K, N)
        start = {k: 3.0 * rnd(N) for k in ("dgamma", "dbeta", "dbias")}
    f = lambda a: None if a is None else np.ascontiguousarray(a, F32)
    i = SimpleNamespace(x=f(x), w=f(w), bias=None if c.null == "bias" else f(bias), rowvec=f(rowvec), dout=f(dout),
                        gamma=f(gamma) if c.bn else None, beta=f(beta) if c.bn else None,
                        ema_mean=f(ema_mean) if c.bn and c.ema else None, ema_var=f(ema_var) if c.bn and c.ema else None,
                        decay=F32(0.9), dx0=f(dx0), dw0=f(dw0), start={k: f(v) for k, v in start.items()}, tier=tier)
    return condition(c, i)


def zero_bound(c, i, fw):
    """how far the fp32 pre-ReLU value of the device may lie from the reference's: the bound of `out` itself plus what the
    bound of y moves it by -- directly (|inv| yb), through the mean (at most the column's largest yb) and through the
    variance (x_hat times that again)"""
    yb = ALLOWED["c_y"] * U * fw.ty + U * np.abs(fw.bias64)
    return ALLOWED["c_out"] * U * fw.tz + np.abs(fw.inv) * (yb + yb.max(0) * (1.0 + np.abs(fw.xh)))


def condition(c, i, tries=64):
    """Batch norm with ReLU: beta is moved per column, in steps of 1/8, to the first value at which no element's pre-ReLU
    value lies inside its own forward bound of zero (zero_bound).  Nothing is excluded: i.undecided, the number of elements
    left inside their bound, must be 0 and every user asserts it."""
    i.undecided = 0
    if not (c.bn and c.relu):
        return i
    beta0 = i.beta.astype(F64)
    done = np.zeros(c.N, bool)
    for j in range(tries):
        step = ((j + 1) // 2) * (1 if j % 2 else -1) * 0.125
        i.beta = np.where(done, i.beta, (beta0 + step).astype(F32)).astype(F32)
        fw = forward(c, i)
        bad = (np.abs(fw.zlin) <= zero_bound(c, i, fw)).sum(0)
        done = bad == 0
        if done.all():
            break
    i.undecided = int(bad.sum())
    return i


# ---- the reference ------------------------------------------------------------------------------------------------------
def _product(a, b, f, start=None):
    """a [P,Q] b [Q,R] (+ start): float64, or float32 with the sum over Q in index order, start first"""
    if f is F64:
        p = a.astype(F64) @ b.astype(F64)
        return p if start is None else p + start.astype(F64)
    a, b = a.astype(F32), b.astype(F32)
    acc = np.zeros((a.shape[0], b.shape[1]), F32) if start is None else start.astype(F32).copy()
    for q in range(a.shape[1]):
        acc += a[:, q, None] * b[q][None, :]
    return acc


def forward(c, i, dtype=F64, y=None):
    """Namespace: y, and with batch norm mean, var (the moments used), ema_mean, ema_var (what the shadows hold afterwards),
    out, plus the terms of the bounds (ty = sum_k |x w|, tz = |y inv| + |mean inv| + |beta|, inv, rstd, xh, zlin).
    y: take these values as the layer's y (the device's own) in place of x w + bias."""
    f = dtype
    M, N = c.M, c.N
    bias = np.zeros(N, f) if i.bias is None else i.bias.astype(f)
    if y is None:
        yv = _product(i.x, i.w, f) + bias
        if i.rowvec is not None:
            yv = yv + i.rowvec.astype(f)[:, np.arange(N) % c.rowvec_d]
    else:
        yv = np.asarray(y).astype(f)
    r = SimpleNamespace(y=yv, M=M, C=N, bias64=bias.astype(F64))
    if f is F64:
        r.ty = np.abs(i.x.astype(F64)) @ np.abs(i.w.astype(F64))
        r.trow = 0.0 if i.rowvec is None else np.abs(i.rowvec.astype(F64))[:, np.arange(N) % c.rowvec_d]
    if not c.bn:
        return r
    if c.training:
        y64 = yv.astype(F64)
        mean64 = y64.sum(0) / M
        var64 = ((y64 - mean64) ** 2).sum(0) / M
        r.mean, r.var = mean64.astype(f), var64.astype(f)
        r.ema_mean = r.ema_var = None
        if i.ema_mean is not None:
            r.ema_mean, r.ema_var = (B.ema_update(s, st, i.decay, f) for s, st in ((i.ema_mean, r.mean), (i.ema_var, r.var)))
    else:
        r.mean, r.var = i.ema_mean.astype(f), i.ema_var.astype(f)
        r.ema_mean, r.ema_var = r.mean, r.var
    g, b = i.gamma.astype(f), i.beta.astype(f)
    if i.tier == "exact" and not c.training:
        # the one place where the float64 reference follows fp32: var + eps as the float32 sum, which EXACT_VAR makes 0.25
        r.rstd = f(1.0) / np.sqrt((r.var.astype(F32) + F32(EPS)).astype(f))
    else:
        r.rstd = f(1.0) / np.sqrt(r.var + f(F32(EPS) if f is F32 else EPS))
    r.inv = g * r.rstd
    r.zlin = yv * r.inv + (b - r.mean * r.inv)
    r.out = r.z = np.maximum(r.zlin, f(0.0)) if c.relu else r.zlin
    r.xh = (yv - r.mean) * r.rstd
    r.tz = np.abs(yv * r.inv) + np.abs(r.mean * r.inv) + np.abs(b)
    return r


def backward(c, i, fw, dtype=F64):
    """Gradient of `forward` (fw: its result in the same dtype).  Namespace: dy, dw, dx, dbias, with batch norm dgamma and
    dbeta -- each parameter gradient WITHOUT what it is accumulated onto (start is added by whoever compares), dw and dx
    with it -- and the terms of the bounds."""
    f = dtype
    M = c.M
    dz = i.dout.astype(f)
    r = SimpleNamespace(fw=fw)
    if c.bn:
        if c.relu:
            dz = np.where(fw.zlin > 0, dz, f(0.0))
        s1, s2 = dz.astype(F64).sum(0), (dz.astype(F64) * fw.xh.astype(F64)).sum(0)
        zero = np.zeros(c.N, f)
        r.m1, r.m2 = ((s1 / M).astype(f), (s2 / M).astype(f)) if c.training else (zero, zero)
        r.gr = i.gamma.astype(f) * fw.rstd
        r.dy = r.gr * ((dz - r.m1) - fw.xh * r.m2)
        r.dgamma, r.dbeta = s2.astype(f), s1.astype(f)
        r.dbias = r.dy.astype(F64).sum(0).astype(f)
        r.xh, r.mean, r.rstd = fw.xh, fw.mean, fw.rstd
    else:
        r.dy = dz
        r.dbias = dz.astype(F64).sum(0).astype(f)
    r.dz = dz
    dw0 = i.dw0 if c.acc_dw else None
    r.dw = _product(i.x.T, r.dy, f)
    if dw0 is not None:
        r.dw = r.dw + dw0.astype(f)
    r.dx = _product(r.dy, i.w.T, f, i.dx0)
    # the same products in float64 from THIS dy: what isolates the round-off of the products in the float32 restatement
    if f is F32:
        r.dw_own = _product(i.x.T, r.dy, F64) + (0.0 if dw0 is None else dw0.astype(F64))
        r.dx_own = _product(r.dy, i.w.T, F64, i.dx0)
    ax, aw, ady = np.abs(i.x.astype(F64)), np.abs(i.w.astype(F64)), np.abs(r.dy.astype(F64))
    r.tdw = ax.T @ ady + (0.0 if dw0 is None else np.abs(dw0.astype(F64)))
    r.tdx = ady @ aw.T + np.abs(i.dx0.astype(F64))
    return r


def reference(c, i, dtype=F64, y=None):
    fw = forward(c, i, dtype, y)
    return fw, backward(c, i, fw, dtype)


# ---- normalised errors --------------------------------------------------------------------------------------------------
def dy_bound(c, bw, constant=None):
    """per element: how far the device's d(y), which never leaves LDS, may lie from the reference's (the form of
    tests/test_20_batch_norm_paths_gpu.py); zero without batch norm, where d(y) is dout itself"""
    if not c.bn:
        return np.zeros(bw.dy.shape)
    k = ALLOWED["c_bwd"] if constant is None else constant
    return k * U * _dy_den(bw)


def _dy_den(bw):
    adz, axm = np.abs(bw.dz), np.abs(bw.xh * bw.m2)
    return np.abs(bw.gr) * (adz + np.abs(bw.m1) + axm * (1.0 + np.abs(bw.mean) * bw.rstd))


def forward_errors(c, i, got, ref, ref_bn):
    """got: y, and with batch norm save_mean, save_var, ema_mean, ema_var, out.  ref: the float64 forward; ref_bn: the
    float64 forward whose batch norm starts from the y of `got` (for the restatement and the device alike, the stage is
    judged on its own input, so nothing has to be carried across it)."""
    e = {"y": ratio(got["y"].astype(F64) - ref.y, U * (ref.ty + ref.trow), U * np.abs(ref.bias64))}
    if c.bn:
        e["save_mean"], e["save_var"] = ulps(got["save_mean"], ref_bn.mean.astype(F32)), ulps(got["save_var"], ref_bn.var.astype(F32))
        if c.training and i.ema_mean is not None:
            for k, s, st in (("ema_mean", i.ema_mean, ref_bn.mean), ("ema_var", i.ema_var, ref_bn.var)):
                e[k] = ulps(got[k], B.ema_update(s, st.astype(F32), i.decay, F32))
        e["out"] = ratio(got["out"].astype(F64) - ref_bn.out, U * ref_bn.tz)
    return e


def backward_errors(c, i, got, bw, isolated=False):
    """got: whichever of dw, dx, dbias, dgamma, dbeta exist (and dy, which only the restatement has); bw: the float64
    backward from the same y.  isolated: got's products are judged against the float64 products of got's own dy (the
    restatement measuring c_dw and c_dx); otherwise against the reference's, the bound of d(y) carried through."""
    e = {}
    acc = i.start if c.acc_pg else None

    def grad(k, den, name):
        if got.get(k) is None:
            return
        want, slack = getattr(bw, k).astype(F64), 0.0
        if acc is not None:
            want = want + acc[k].astype(F64)
            slack = U * (np.abs(acc[k].astype(F64)) + np.abs(want))
        e[name] = ratio(got[k].astype(F64) - want, den, slack)
    adz = np.abs(bw.dz.astype(F64))
    if c.bn:
        axm, agr = np.abs(bw.xh * bw.m2), np.abs(bw.gr)
        if got.get("dy") is not None:
            e["dy"] = ratio(got["dy"].astype(F64) - bw.dy, U * _dy_den(bw))
        grad("dgamma", U * np.abs(bw.dz * bw.xh).sum(0), "dgamma")
        grad("dbeta", U * adz.sum(0), "dbeta")
        grad("dbias", U * agr * (adz + np.abs(bw.m1) + axm).sum(0), "dbias")
    else:
        grad("dbias", U * adz.sum(0), "dbias_plain")
    dyb = np.zeros(bw.dy.shape) if isolated else dy_bound(c, bw)
    if got.get("dw") is not None:
        want = got["dw_own"] if isolated else bw.dw
        e["dw"] = ratio(got["dw"].astype(F64) - want, U * bw.tdw, np.abs(i.x.astype(F64)).T @ dyb)
    if got.get("dx") is not None:
        want = got["dx_own"] if isolated else bw.dx
        e["dx"] = ratio(got["dx"].astype(F64) - want, U * bw.tdx, dyb @ np.abs(i.w.astype(F64)).T)
    return e


def restatement_errors(c, i):
    """normalised errors of the float32 restatement against the float64 reference on the inputs i"""
    fw, bw = reference(c, i)
    f32 = forward(c, i, F32)
    b32 = backward(c, i, f32, F32)
    got = {"y": f32.y}
    if c.bn:
        got.update(save_mean=f32.mean, save_var=f32.var, ema_mean=f32.ema_mean, ema_var=f32.ema_var, out=f32.out)
    ref_bn = forward(c, i, F64, f32.y)
    e = forward_errors(c, i, got, fw, ref_bn)
    bw_own = backward(c, i, ref_bn, F64)
    start = i.start if c.acc_pg else {k: F32(0.0) for k in i.start}
    gb = {"dy": b32.dy, "dw": b32.dw, "dx": b32.dx, "dw_own": b32.dw_own, "dx_own": b32.dx_own,
          "dbias": (b32.dbias + start["dbias"]).astype(F32)}
    if c.bn:
        gb.update(dgamma=(b32.dgamma + start["dgamma"]).astype(F32), dbeta=(b32.dbeta + start["dbeta"]).astype(F32))
    e.update(backward_errors(c, i, gb, bw_own, isolated=True))
    return e
