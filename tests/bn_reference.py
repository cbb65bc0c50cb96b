"""NumPy restatement of the batch-norm contract of include/cloudaae_hip.h (the comments above cloudaae_bn_forward and
cloudaae_bn_backward), written from the definition only: a yardstick for csrc/bn.hip and csrc/bn_common.h.

  training : mean, var = moments over all M rows (biased variance); shadows  s <- s - (s - stat) * (1 - decay)
  inference: mean, var = the shadows
  output   : inv = gamma / sqrt(var + 1e-3);  z = y * inv + (beta - mean * inv);  optional ReLU; optional pool (mean or
             max) over groups of pool_rows consecutive rows
  backward : dz = (dout + dpooled / pool_rows | dpooled * [z == max] / ties) * [z > 0];  dbeta = sum dz;
             dgamma = sum dz * x_hat;  dy = gamma * rstd * ((dz - m1) - x_hat * m2), m1 / m2 the batch means of dz and
             dz * x_hat (zero in inference mode: the statistics do not depend on the batch);  dbias = sum_r dy

dtype = float64 is the reference.  dtype = float32 performs the kernels' own formulas in fp32 (every column sum still in
fp64, the moments rounded to fp32 once): it is what the tolerances of tests/test_20_batch_norm_paths_gpu.py are measured
with (tests/test_bn_reference_host.py), never the kernels' own output.

The file also holds what the two test files share: the normalised errors (an error divided by a bound formed from that
element's own terms), `condition` (which removes the elements whose ReLU mask or maximum fp32 cannot decide), the mutants
of the reference that prove the bounds are tight, and the case table."""
from types import SimpleNamespace

import numpy as np

EPS = 1e-3
U = 2.0 ** -24                    # unit round-off of fp32
F32, F64 = np.float32, np.float64

MUTANTS = ("drop_last_row", "pool_rows_plus_one", "unshared_ties", "m2_zero")


def _colsum(a, mutant=None):
    """fp64 column sums; the mutant forgets the last row"""
    a = np.asarray(a, F64)
    return (a[:-1] if mutant == "drop_last_row" else a).sum(0)


def ema_update(s, stat, decay, dtype=F64):
    s, stat = np.asarray(s).astype(dtype), np.asarray(stat).astype(dtype)
    om = dtype(1.0) - dtype(F32(decay))
    return s - (s - stat) * om


def forward(y, gamma, beta, training, ema_mean=None, ema_var=None, decay=None, relu=0, pool_rows=0, pool_mode=0,
            dtype=F64, mutant=None):
    """y [M,C] float32.  Returns a namespace: mean, var (the moments used), ema_mean, ema_var (updated shadows, or None),
    z (activation), pooled, ties, pool_stats [groups,3,C] (rows passing the ReLU, sum of their x_hat, sum of all x_hat;
    mean pool + ReLU in training mode only), and the terms the bounds are formed from: inv, rstd, xh, zlin, tz."""
    f = dtype
    y = np.asarray(y)
    M, C = y.shape
    if training:
        y64 = y.astype(F64)
        n = M - 1 if mutant == "drop_last_row" else M
        mean64 = _colsum(y64, mutant) / n
        var64 = _colsum((y64 - mean64) ** 2, mutant) / n
        mean, var = mean64.astype(f), var64.astype(f)
        new_m = new_v = None
        if ema_mean is not None:
            new_m, new_v = ema_update(ema_mean, mean, decay, f), ema_update(ema_var, var, decay, f)
    else:
        mean, var = np.asarray(ema_mean).astype(f), np.asarray(ema_var).astype(f)
        new_m, new_v = mean, var
    yv, g, b = y.astype(f), np.asarray(gamma).astype(f), np.asarray(beta).astype(f)
    rstd = f(1.0) / np.sqrt(var + f(F32(EPS) if f is F32 else EPS))
    inv = g * rstd
    sh = b - mean * inv
    zlin = yv * inv + sh
    z = np.maximum(zlin, f(0.0)) if relu else zlin
    xh = (yv - mean) * rstd
    r = SimpleNamespace(mean=mean, var=var, ema_mean=new_m, ema_var=new_v, z=z, zlin=zlin, xh=xh, inv=inv, rstd=rstd,
                        pooled=None, ties=None, pool_stats=None, M=M, C=C)
    if f is F64:    # |y*inv| + |mean*inv| + |beta|: the magnitudes whose round-off an fp32 z carries
        r.tz = np.abs(yv * inv) + np.abs(mean * inv) + np.abs(b)
    if pool_mode:
        zg = z.reshape(M // pool_rows, pool_rows, C)
        if pool_mode == 1:
            r.pooled = (zg.astype(F64).sum(1) / pool_rows).astype(f)
            if relu and training:
                xg = xh.reshape(zg.shape).astype(F64)
                passed = zg > 0
                r.pool_stats = np.stack([passed.sum(1).astype(F64), (xg * passed).sum(1), xg.sum(1)], axis=1)
        else:
            r.pooled = zg.max(1)
            r.ties = (zg == r.pooled[:, None, :]).sum(1).astype(f)
    return r


def backward(y, gamma, beta, training, ema_mean=None, ema_var=None, relu=0, dout=None, pool_rows=0, pool_mode=0,
             dpooled=None, dtype=F64, mutant=None):
    """Gradient of `forward` for the upstreams dout [M,C] and/or dpooled [groups,C].  Returns a namespace: dy, dgamma,
    dbeta, dbias and the terms of the bounds (dz, xh, m1, m2, gr, mean, rstd)."""
    f = dtype
    fw = forward(y, gamma, beta, training, ema_mean, ema_var, 0.0 if training else None, relu, pool_rows, pool_mode, f, mutant)
    M, C = fw.M, fw.C
    dz = np.zeros((M, C), f) if dout is None else np.asarray(dout).astype(f)
    if pool_mode == 1:
        share = np.asarray(dpooled).astype(f) / f(pool_rows + (1 if mutant == "pool_rows_plus_one" else 0))
        dz = dz + np.repeat(share, pool_rows, axis=0)
    elif pool_mode == 2:
        dp = np.asarray(dpooled).astype(f)
        share = dp if mutant == "unshared_ties" else dp / fw.ties
        zg = fw.z.reshape(M // pool_rows, pool_rows, C)
        dz = dz + np.where(zg == fw.pooled[:, None, :], share[:, None, :], f(0.0)).reshape(M, C)
    if relu:
        dz = np.where(fw.z > 0, dz, f(0.0))
    n = M - 1 if mutant == "drop_last_row" else M
    s1 = _colsum(dz, mutant)
    s2 = _colsum(dz.astype(F64) * fw.xh.astype(F64), mutant)
    zero = np.zeros(C, f)
    m1 = (s1 / n).astype(f) if training else zero
    m2 = (s2 / n).astype(f) if training and mutant != "m2_zero" else zero
    gr = np.asarray(gamma).astype(f) * fw.rstd
    dy = gr * ((dz - m1) - fw.xh * m2)
    return SimpleNamespace(dy=dy, dgamma=s2.astype(f), dbeta=s1.astype(f), dbias=_colsum(dy).astype(f), dz=dz, xh=fw.xh,
                           m1=m1, m2=m2, gr=gr, mean=fw.mean, rstd=fw.rstd, fw=fw)


# ---- conditioning -------------------------------------------------------------------------------------------------------
# The kernels take the ReLU mask from their fp32 z.  An element whose fp64 z lies within fp32 round-off of zero has no
# defined mask; a maximum whose runner-up is not a bit-identical duplicate but closer than round-off has no defined tie
# count.  Such elements are moved away before a case is used, and every case asserts that none is left.
AMBIGUITY = 8.0       # |z64| <= AMBIGUITY * U * (|y*inv| + |mean*inv| + |beta|)


def ambiguous(y, gamma, beta, training, ema_mean, ema_var, relu, pool_rows, pool_mode):
    """(mask [M,C] of ambiguous elements, direction [M,C] in which y moves them away)"""
    fw = forward(y, gamma, beta, training, ema_mean, ema_var, 0.0 if training else None, 0, 0, 0, F64)
    bound = AMBIGUITY * U * fw.tz
    sgn_inv = np.where(fw.inv < 0, -1.0, 1.0)
    amb = np.zeros(fw.zlin.shape, bool)
    direction = np.where(fw.zlin < 0, -1.0, 1.0) * sgn_inv
    if relu:
        amb = np.abs(fw.zlin) <= bound
    if pool_mode == 2:
        z = np.maximum(fw.zlin, 0.0) if relu else fw.zlin
        b = np.where(z > 0, bound, 0.0) if relu else bound
        shape = (fw.M // pool_rows, pool_rows, fw.C)
        zg, bg = z.reshape(shape), b.reshape(shape)
        top1 = zg.max(1, keepdims=True)
        is1 = zg == top1
        top2 = np.where(is1, -np.inf, zg).max(1, keepdims=True)
        is2 = (zg == top2) & np.isfinite(top2)
        b1 = np.where(is1, bg, 0.0).max(1, keepdims=True)
        b2 = np.where(is2, bg, 0.0).max(1, keepdims=True)
        close = is2 & ((top1 - top2) < (b1 + b2))
        close = close.reshape(fw.M, fw.C) & ~amb
        direction = np.where(close, -sgn_inv, direction)      # the runner-up moves down
        amb = amb | close
    return amb, direction


def condition(y, gamma, beta, training, ema_mean, ema_var, relu, pool_rows, pool_mode, dup=(), max_rounds=6):
    """Nudge the ambiguous elements of y away by 1e-3 * max(1, |y|), recompute, repeat.  dup: (dst, src) row pairs that
    are bit-identical copies and stay so.  Returns (y, [ambiguous elements found in each round]); the last count is
    the size of the set that is left and must be 0."""
    y = np.array(y, F32)
    counts = []
    for _ in range(max_rounds + 1):
        amb, direction = ambiguous(y, gamma, beta, training, ema_mean, ema_var, relu, pool_rows, pool_mode)
        counts.append(int(amb.sum()))
        if counts[-1] == 0 or len(counts) > max_rounds:
            break
        for dst, src in dup:
            direction[dst] = np.where(amb[src], direction[src], direction[dst])
            amb[dst] |= amb[src]
            amb[src], direction[src] = amb[dst], direction[dst]
        step = (1e-3 * np.maximum(1.0, np.abs(y.astype(F64))) * direction).astype(F32)
        y = np.where(amb, y + step, y).astype(F32)
    return y, counts


# ---- normalised errors --------------------------------------------------------------------------------------------------
def _ratio(err, den, slack=0.0):
    """max of (err - slack) / den; where the bound is zero the value must be exact"""
    err = np.maximum(np.abs(np.asarray(err, F64)) - slack, 0.0)
    den = np.broadcast_to(np.asarray(den, F64), err.shape)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))
    q = np.where(np.isfinite(err), q, np.inf)
    return float(q.max())


def ulps(got, want32):
    """largest distance of got from the float32 array want32 in units of want32's spacing"""
    want32 = np.asarray(want32, F32)
    return _ratio(np.asarray(got, F64) - want32.astype(F64), np.spacing(np.abs(want32)).astype(F64))


def forward_errors(got, ref, pool_rows=0, pool_mode=0):
    """got: dict of whichever outputs exist (save_mean, save_var, out, pooled, ties, pool_stats [groups,3,C]); ref: the
    fp64 forward.  Moments in ulps of the rounded reference; counts as numbers of mismatches; the rest as multiples of
    U times the bound's terms (module docstring of tests/test_20_batch_norm_paths_gpu.py)."""
    e = {}
    if "save_mean" in got:
        e["save_mean"] = ulps(got["save_mean"], ref.mean.astype(F32))
        e["save_var"] = ulps(got["save_var"], ref.var.astype(F32))
    if got.get("out") is not None:
        e["out"] = _ratio(np.asarray(got["out"], F64) - ref.z, U * ref.tz)
    if pool_mode == 1:
        shape = (ref.M // pool_rows, pool_rows, ref.C)
        seq = (pool_rows / 4.0) * U * np.abs(ref.z).reshape(shape).mean(1)     # sequential fp32 accumulation of a row lane
        e["pooled"] = _ratio(np.asarray(got["pooled"], F64) - ref.pooled, U * ref.tz.reshape(shape).mean(1), seq)
        if got.get("pool_stats") is not None:
            ps = np.asarray(got["pool_stats"], F64)
            e["stats_count"] = float((ps[:, 0] != ref.pool_stats[:, 0]).sum())
            den = U * np.abs(ref.xh).reshape(shape).sum(1)
            e["stats_sum"] = max(_ratio(ps[:, 1] - ref.pool_stats[:, 1], den), _ratio(ps[:, 2] - ref.pool_stats[:, 2], den))
    elif pool_mode == 2:
        shape = (ref.M // pool_rows, pool_rows, ref.C)
        zg = ref.z.reshape(shape)
        tz_at_max = np.where(zg == ref.pooled[:, None, :], ref.tz.reshape(shape), 0.0).max(1)
        if ref.z.min() >= 0:        # after a ReLU a clipped maximum is an exact zero
            tz_at_max = np.where(ref.pooled > 0, tz_at_max, 0.0)
        e["pooled"] = _ratio(np.asarray(got["pooled"], F64) - ref.pooled, U * tz_at_max)
        if got.get("ties") is not None:
            e["ties"] = float((np.asarray(got["ties"], F64) != ref.ties).sum())
    return e


def backward_errors(got, ref, start=None):
    """got: dict of dy and whichever of dgamma / dbeta / dbias exist; ref: the fp64 backward; start: what the parameter
    gradients were accumulated onto (dict, optional): the sum with it may round once more."""
    e = {}
    adz, axm = np.abs(ref.dz), np.abs(ref.xh * ref.m2)
    agr, am1 = np.abs(ref.gr), np.abs(ref.m1)
    e["dy"] = _ratio(np.asarray(got["dy"], F64) - ref.dy, U * agr * (adz + am1 + axm * (1.0 + np.abs(ref.mean) * ref.rstd)))
    dens = {"dgamma": U * np.abs(ref.dz * ref.xh).sum(0), "dbeta": U * adz.sum(0), "dbias": U * agr * (adz + am1 + axm).sum(0)}
    for k, den in dens.items():
        if got.get(k) is None:
            continue
        want, slack = getattr(ref, k), 0.0
        if start is not None:
            want = want + start[k].astype(F64)
            slack = U * (np.abs(start[k].astype(F64)) + np.abs(want))
        e[k] = _ratio(np.asarray(got[k], F64) - want, den, slack)
    return e


# which measured constant judges which normalised error; the others are fixed by their meaning (ulps, exact counts)
CONSTANT_OF = {"out": "c_fwd", "pooled": "c_fwd", "stats_sum": "c_stats", "dy": "c_bwd", "dgamma": "c_dgamma",
               "dbeta": "c_dbeta", "dbias": "c_dbias"}
FIXED = {"save_mean": 1.0, "save_var": 1.0, "ema_mean": 2.0, "ema_var": 2.0, "stats_count": 0.0, "ties": 0.0}

# Measured by tests/test_bn_reference_host.py::test_constants_are_four_times_the_restatement (largest normalised error of
# the float32 restatement against the float64 reference over CASES), times four, rounded up to a power of two.  The
# measured values are in profiles/notes_bn_paths.md.
ALLOWED = {"c_fwd": 16.0, "c_stats": 2048.0, "c_bwd": 2048.0, "c_dgamma": 2048.0, "c_dbeta": 8.0, "c_dbias": 1024.0}


def allowed_of(name):
    return FIXED[name] if name in FIXED else ALLOWED[CONSTANT_OF[name]]


def pow2_ceil(x):
    return float(2.0 ** np.ceil(np.log2(x)))


# ---- the case table -----------------------------------------------------------------------------------------------------
def case(name, M, C, relu=1, training=1, pool_rows=0, pool_mode=0, out=None, dout=None, pool_stats=0, bwd_stats=None,
         pads=(0, 0, 0, 0), accumulate=0, null=None, scale=2.0, offset=0.5, ema_start=0, ties=0, clip=0, const_col=None):
    """out: the activation is written (default: exactly when there is no pool); dout: an upstream for it (default: as
    out); pool_stats: the forward writes the per-group sums; bwd_stats: the backward is given them (default: as
    pool_stats, and only when the pooled value is the only upstream); pads = (ldy, ldo, lddo, lddy) - C; null: which of
    dgamma / dbeta / dbias is passed as NULL; ties: duplicate rows for the max pool; clip: channel 0 gets a beta that
    clips every row; const_col: this column of y is the constant 1.5."""
    out = (pool_mode == 0) if out is None else out
    dout = out if dout is None else dout
    bwd_stats = (pool_stats and not dout) if bwd_stats is None else bwd_stats
    return SimpleNamespace(name=name, M=M, C=C, relu=relu, training=training, pool_rows=pool_rows, pool_mode=pool_mode,
                           out=int(out), dout=int(dout), pool_stats=pool_stats, bwd_stats=int(bwd_stats), pads=pads,
                           accumulate=accumulate, null=null, scale=scale, offset=offset, ema_start=ema_start, ties=ties,
                           clip=clip, const_col=const_col)


def _cases():
    t = []
    # small-batch kernels (M <= 128) and the first shape past the switch, every channel remainder
    for M in (1, 2, 3, 31, 128, 129):
        for C in (1, 63, 64, 65, 130, 1024):
            for relu in (1, 0):
                for training in (1, 0):
                    t.append(case("dense_M%d_C%d_%s_%s" % (M, C, "relu" if relu else "linear", "train" if training else "infer"),
                                  M, C, relu, training, ema_start=(M + C + relu) % 2))
    # large path: rows and channels in no whole block, parts saturating at 128 (M >= 8192), a short last slice
    t.append(case("dense_M1000_C70", 1000, 70, ema_start=1))
    t.append(case("dense_M1000_C70_infer", 1000, 70, training=0))
    t.append(case("dense_M1000_C70_linear_infer", 1000, 70, relu=0, training=0))
    t.append(case("dense_M8191_C130", 8191, 130))
    t.append(case("dense_M8192_C1024", 8192, 1024))
    t.append(case("dense_M8256_C65", 8256, 65, ema_start=1))
    t.append(case("dense_M8256_C65_infer", 8256, 65, training=0))
    # mean pool, the hot kernel (C % 64 == 0, pool_rows % 32 == 0, ReLU, training, pool_stats, no activation); backward from
    # the per-group sums, and from a pass over y (hoisted upstream: a slice inside one group, and one that crosses)
    for G, R, C in ((8, 1024, 1024), (3, 32, 64), (130, 64, 128)):
        t.append(case("meanhot_%dx%dx%d" % (G, R, C), G * R, C, pool_rows=R, pool_mode=1, pool_stats=1))
        t.append(case("meanhot_%dx%dx%d_bwd_pass" % (G, R, C), G * R, C, pool_rows=R, pool_mode=1, pool_stats=1, bwd_stats=0))
    # mean pool, the generic kernel
    for R in (200, 43, 1):
        M = 5 * R
        t.append(case("mean_R%d" % R, M, 130, pool_rows=R, pool_mode=1, pool_stats=1))
        t.append(case("mean_R%d_out_both" % R, M, 130, pool_rows=R, pool_mode=1, pool_stats=1, out=1))
        t.append(case("mean_R%d_linear" % R, M, 130, relu=0, pool_rows=R, pool_mode=1))
        t.append(case("mean_R%d_infer" % R, M, 130, training=0, pool_rows=R, pool_mode=1))
    # max pool: ties in one row lane, across row lanes, across groups; a channel clipped in every group
    for R in (200, 256):
        t.append(case("max_R%d" % R, 4 * R, 130, pool_rows=R, pool_mode=2, ties=1, clip=1))
        t.append(case("max_R%d_out_both" % R, 4 * R, 130, pool_rows=R, pool_mode=2, out=1, ties=1, clip=1))
    t.append(case("max_R200_linear", 800, 130, relu=0, pool_rows=200, pool_mode=2, ties=1))
    # strides: (ldy, ldo, lddo, lddy) - C
    t.append(case("stride_small", 31, 65, pads=(1, 2, 3, 4)))
    t.append(case("stride_large", 1000, 70, pads=(5, 3, 2, 1)))
    t.append(case("stride_mean_out_both", 215, 130, pool_rows=43, pool_mode=1, pool_stats=1, out=1, pads=(1, 4, 2, 3)))
    t.append(case("stride_max_out_both", 800, 130, pool_rows=200, pool_mode=2, out=1, ties=1, clip=1, pads=(5, 1, 3, 2)))
    t.append(case("stride_meanhot", 96, 64, pool_rows=32, pool_mode=1, pool_stats=1, pads=(5, 0, 0, 7)))
    # parameter gradients: accumulated onto what is there; each of the three not wanted
    t.append(case("accumulate_small", 31, 65, accumulate=1))
    t.append(case("accumulate_large", 1000, 70, accumulate=1))
    t.append(case("accumulate_meanhot", 96, 64, pool_rows=32, pool_mode=1, pool_stats=1, accumulate=1))
    for which in ("dgamma", "dbeta", "dbias"):
        t.append(case("null_%s_small" % which, 31, 65, null=which))
        t.append(case("null_%s_large" % which, 1000, 70, null=which))
    # |mean| / std = 2000: no ReLU (the scale-and-shift form cannot decide the mask there)
    t.append(case("offset_small", 128, 65, relu=0, scale=0.05, offset=100.0))
    t.append(case("offset_large", 1000, 70, relu=0, scale=0.05, offset=100.0))
    # a column of variance exactly 0
    t.append(case("const_small", 31, 65, relu=0, const_col=3))
    t.append(case("const_large", 1000, 70, relu=0, const_col=3))
    return t


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def tie_rows(c):
    """(dst, src) duplicate rows of a max-pool case: group 0 in one row lane (rows 8 and 12: both lane 0), group 1 in two
    row lanes (rows 5 and 6), groups 2 and 3 the same row in each (no tie inside a group)."""
    R = c.pool_rows
    return ((12, 8), (R + 6, R + 5), (3 * R + 3, 2 * R + 3)) if c.ties else ()


def make_inputs(c):
    """The conditioned inputs of a case (seed = its position in CASES): namespace of y [M,C], gamma, beta, ema_mean,
    ema_var (what the shadows hold before the call), decay, dout, dpooled, and `ambiguous`, the counts of condition()."""
    rng = np.random.default_rng(1000 + CASES.index(c))
    M, C = c.M, c.C
    rnd = lambda *s: rng.standard_normal(s)
    y = (rnd(M, C) * c.scale + c.offset + 0.25 * c.scale * rnd(1, C)).astype(F32)
    gamma = (1.0 + 0.2 * rnd(C)).astype(F32)
    gamma[1::7] *= -1.0                                       # negative scales: the larger y is the smaller z
    beta = 0.3 * rnd(C)
    beta = (np.where(beta < 0, -1.0, 1.0) * np.maximum(np.abs(beta), 0.05)).astype(F32)   # a single row has z == beta
    if c.clip:
        beta[0] = -1000.0
    if c.const_col is not None:
        y[:, c.const_col] = 1.5
    if c.training:
        ema_mean = (0.3 * rnd(C)).astype(F32) if c.ema_start else np.zeros(C, F32)
        ema_var = (0.5 + np.abs(rnd(C))).astype(F32) if c.ema_start else np.zeros(C, F32)
    else:
        ema_mean = (c.offset + 0.3 * c.scale * rnd(C)).astype(F32)
        ema_var = (c.scale ** 2 * (0.5 + np.abs(rnd(C)))).astype(F32)
    dup = tie_rows(c)
    if dup:
        # the duplicated rows win their group in every second channel
        G, R = M // c.pool_rows, c.pool_rows
        yg = y.reshape(G, R, C)
        up = gamma > 0
        for dst, src in dup:
            for r in {dst, src}:
                g = r // R
                win = np.where(up, yg[g].max(0) + 0.5, yg[g].min(0) - 0.5) + np.where(up, 1.0, -1.0) * np.abs(rnd(C))
                y[r, ::2] = win.astype(F32)[::2]
        for dst, src in dup:
            if dst // R == src // R:
                y[dst] = y[src]
            else:       # different groups: the same bits in both groups, each the only maximum of its own
                y[dst, ::2] = y[src, ::2] = np.where(up, np.maximum(y[dst], y[src]), np.minimum(y[dst], y[src]))[::2]
    y, counts = condition(y, gamma, beta, c.training, ema_mean, ema_var, c.relu, c.pool_rows, c.pool_mode, dup)
    dout = rnd(M, C).astype(F32) if c.dout else None
    dpooled = rnd(M // c.pool_rows, C).astype(F32) if c.pool_mode else None
    return SimpleNamespace(y=y, gamma=gamma, beta=beta, ema_mean=ema_mean, ema_var=ema_var, decay=F32(0.9), dout=dout,
                           dpooled=dpooled, ambiguous=counts)


def reference(c, x, dtype=F64, mutant=None):
    """(forward, backward) of a case on the inputs x"""
    fw = forward(x.y, x.gamma, x.beta, c.training, x.ema_mean, x.ema_var, x.decay, c.relu, c.pool_rows, c.pool_mode, dtype, mutant)
    bw = backward(x.y, x.gamma, x.beta, c.training, x.ema_mean, x.ema_var, c.relu, x.dout, c.pool_rows, c.pool_mode, x.dpooled,
                  dtype, mutant)
    return fw, bw


def outputs_of(c, fw, bw):
    """what the entry points would have written, had they computed (fw, bw): the `got` of forward_errors / backward_errors"""
    f = {"save_mean": fw.mean, "save_var": fw.var, "out": fw.z if c.out else None, "pooled": fw.pooled, "ties": fw.ties,
         "pool_stats": fw.pool_stats if c.pool_stats else None}
    b = {"dy": bw.dy, "dgamma": bw.dgamma, "dbeta": bw.dbeta, "dbias": bw.dbias}
    return f, b


def case_errors(c, got_f, got_b, fw, bw, start=None):
    e = forward_errors(got_f, fw, c.pool_rows, c.pool_mode)
    e.update(backward_errors(got_b, bw, start))
    return e


def mutant_applies(mutant, c):
    """the cases a mutant must be caught on"""
    if mutant == "drop_last_row":       # (inference mode: only the backward sums, and the ReLU may have clipped a lone channel)
        return c.M >= 2 and (c.training or c.C >= 63)
    if mutant == "pool_rows_plus_one":
        return c.pool_mode == 1
    if mutant == "unshared_ties":
        return c.pool_mode == 2 and c.ties
    return bool(c.training) and c.M >= 2          # m2_zero


COLSUM_CASES = [(M, C, acc) for M in (1, 129, 8256) for C in (1, 70, 1024) for acc in (0, 1)]
