"""Reference of the loss and optimiser kernels of csrc/step.hip and csrc/so3_dual.h, written from the Python reference
files only (losses/angular_distance_taylor.py:30-116, losses/trans_distance.py:4-9, losses/chamfer_loss.py:12-14,
train_cloudAAE_ycbv.py:194-273, utils/tf_util.py:635-706): a yardstick, needing NumPy and mpmath only.

  rotation   ONE implementation of exponential_map / get_rotation_error over forward-mode duals (derivatives with respect
             to the three prediction components), generic in its scalar type.  Evaluated with mpmath at 50 digits it is the
             reference; evaluated with Python floats (IEEE binary64) it is the "restatement": the same operations as the
             kernel, used ONLY to size the bounds.  Both hold the theta^2 < 1e-2 Taylor branch, the clip of the cosine at
             +-0.9999999 with a zero derivative outside and the cast of the float32 prediction to float64.
  the rest   float64 is the reference, float32 the restatement in the kernels' order of operations: translation error and
             gradient, weighted total and its fan-out, Adam in the TF ApplyAdam form (lr_t from the OLD beta powers,
             grad_scale), SGD, mean / add-mean, pool rows (mean, max with tie counts) and gradient, edge feature and
             gradient, the batch-norm decay schedule, and the one-expression elementwise kernels.

The file also holds what the CPU and the GPU test share: the named case table (every case draws from a fixed seed),
`condition`, the normalised errors (an error divided by a bound formed from that element's own terms), the allowed
constants and the mutants of the reference that prove the bounds are tight."""
import functools
import math
import zlib
from types import SimpleNamespace

import mpmath
import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24
F32, F64 = np.float32, np.float64
LIM = 0.9999999                   # clip of the cosine (angular_distance_taylor.py:81)
TAYLOR_EPS = 1e-2                 # exponential_map's EPS, on theta^2
DIGITS = 50

MUTANTS = ("taylor_drops_theta6", "no_transpose", "clip_keeps_derivative", "jacobian_column_negated",
           "adam_eps_inside_sqrt", "adam_lr_from_advanced_powers", "adam_unscaled_square", "max_grad_unshared",
           "mean_over_padded_count")


# ---- scalar kits: what the generic rotation code needs beyond + - * / ---------------------------------------------------
MP = SimpleNamespace(name="mp", c=lambda x: mpmath.mpf(float(x)), sqrt=mpmath.sqrt, sin=mpmath.sin, cos=mpmath.cos,
                     acos=mpmath.acos)
FL = SimpleNamespace(name="f64", c=float, sqrt=math.sqrt, sin=math.sin, cos=math.cos, acos=math.acos)


def _comb(ad, bd, both, only_a, only_b):
    """derivative parts; an empty tuple is a constant (all zero)"""
    if ad and bd:
        return tuple(both(x, y) for x, y in zip(ad, bd))
    if ad:
        return tuple(only_a(x) for x in ad)
    return tuple(only_b(y) for y in bd)


class Dual(object):
    """a value and its derivatives; plain numbers in an expression are constants"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=()):
        self.v, self.d = v, d

    def __add__(a, b):
        if not isinstance(b, Dual):
            return Dual(a.v + b, a.d)
        return Dual(a.v + b.v, _comb(a.d, b.d, lambda x, y: x + y, lambda x: x, lambda y: y))

    __radd__ = __add__

    def __sub__(a, b):
        if not isinstance(b, Dual):
            return Dual(a.v - b, a.d)
        return Dual(a.v - b.v, _comb(a.d, b.d, lambda x, y: x - y, lambda x: x, lambda y: -y))

    def __rsub__(a, c):
        return Dual(c - a.v, tuple(-x for x in a.d))

    def __neg__(a):
        return Dual(-a.v, tuple(-x for x in a.d))

    def __mul__(a, b):
        if not isinstance(b, Dual):
            return Dual(a.v * b, tuple(x * b for x in a.d))
        return Dual(a.v * b.v, _comb(a.d, b.d, lambda x, y: x * b.v + a.v * y, lambda x: x * b.v, lambda y: a.v * y))

    __rmul__ = __mul__

    def __truediv__(a, b):
        if not isinstance(b, Dual):
            return Dual(a.v / b, tuple(x / b for x in a.d))
        q = a.v / b.v
        return Dual(q, _comb(a.d, b.d, lambda x, y: (x - q * y) / b.v, lambda x: x / b.v, lambda y: (-(q * y)) / b.v))


def _dsqrt(a, K):
    r = K.sqrt(a.v)
    k = 0.5 / r
    return Dual(r, tuple(k * x for x in a.d))


def _dsin(a, K):
    c = K.cos(a.v)
    return Dual(K.sin(a.v), tuple(c * x for x in a.d))


def _dcos(a, K):
    s = -K.sin(a.v)
    return Dual(K.cos(a.v), tuple(s * x for x in a.d))


def _exp_map(ax, K, mutant=None):
    """angular_distance_taylor.py:30-66 on three duals; 3x3 list of duals"""
    zero = Dual(K.c(0.0))
    ss = [[zero, -ax[2], ax[1]], [ax[2], zero, -ax[0]], [-ax[1], ax[0], zero]]
    tsq = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]
    if tsq.v < TAYLOR_EPS:
        p4, p6, p8 = tsq * tsq, tsq * tsq * tsq, tsq * tsq * tsq * tsq
        t1 = 1.0 - (tsq / 6.0) + (p4 / 120.0)
        if mutant != "taylor_drops_theta6":
            t1 = t1 - (p6 / 5040.0)
        t1 = t1 + (p8 / 362880.0)
        t2 = 0.5 - (tsq / 24.0) + (p4 / 720.0) - (p6 / 40320.0) + (p8 / 3628800.0)
    else:
        th = _dsqrt(tsq, K)
        t1 = _dsin(th, K) / th
        t2 = (1.0 - _dcos(th, K)) / tsq
    R = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            sq = zero
            for k in range(3):
                sq = sq + ss[i][k] * ss[k][j]
            R[i][j] = ((1.0 if i == j else 0.0) + t1 * ss[i][j]) + t2 * sq
    return R


def _rotation_row(p32, l64, K, mutant=None):
    """get_rotation_error (:103-116) of one sample: (theta, jac[3], unclipped t, S, Sd[3], clipped in {-1, 0, 1})"""
    one, zero = K.c(1.0), K.c(0.0)
    p = [Dual(K.c(F64(p32[a])), tuple(one if a == c else zero for c in range(3))) for a in range(3)]    # tf.cast(.., float64)
    lab = [Dual(K.c(l64[a])) for a in range(3)]
    Rp, Rl = _exp_map(p, K, mutant), _exp_map(lab, K, mutant)
    tr, S, Sd = Dual(zero), zero, [zero, zero, zero]
    for r in range(3):
        e = Dual(zero)
        for k in range(3):
            term = Rl[r][k] * (Rp[k][r] if mutant == "no_transpose" else Rp[r][k])
            e = e + term
            S = S + abs(term.v)
            for a in range(3):
                Sd[a] = Sd[a] + abs(term.d[a])
        tr = tr + e
    t = (tr - 1.0) / 2.0
    tu, clipped = t.v, 0
    if t.v < -LIM or t.v > LIM:
        clipped = -1 if t.v < -LIM else 1
        t = Dual(K.c(clipped * LIM), t.d if mutant == "clip_keeps_derivative" else (zero, zero, zero))
    theta = K.acos(t.v)
    k = -1.0 / K.sqrt(1.0 - t.v * t.v)
    jac = [k * x for x in t.d]
    if mutant == "jacobian_column_negated":
        jac[1] = -jac[1]
    return theta, jac, tu, S, Sd, clipped


def rotation(pred32, label64, kit=MP, mutant=None, rows=None):
    """rows of get_rotation_error.  Namespace of float64 arrays theta [b], jac [b,3], t (unclipped), S, Sd [b,3], clipped
    [b]; mean (the float64 mean of theta, exactly rounded for the mp kit); with the mp kit also theta_mp / jac_mp, the
    unrounded values the errors are taken from."""
    pred32, label64 = np.asarray(pred32, F32), np.asarray(label64, F64)
    b = pred32.shape[0]
    out = SimpleNamespace(theta=np.zeros(b), jac=np.zeros((b, 3)), t=np.zeros(b), S=np.zeros(b), Sd=np.zeros((b, 3)),
                          clipped=np.zeros(b, int), theta_mp=None, jac_mp=None)
    with mpmath.workdps(DIGITS):
        if rows is None:
            rows = [_rotation_row(pred32[i], label64[i], kit, mutant) for i in range(b)]
        for i, (theta, jac, tu, S, Sd, clipped) in enumerate(rows):
            out.theta[i], out.jac[i], out.t[i], out.S[i], out.Sd[i], out.clipped[i] = \
                float(theta), [float(x) for x in jac], float(tu), float(S), [float(x) for x in Sd], clipped
        if kit is MP:
            out.theta_mp, out.jac_mp = [r[0] for r in rows], [r[1] for r in rows]
            out.mean = float(mpmath.fsum(out.theta_mp) / b)
        else:
            out.mean = math.fsum(out.theta) / b
    return out


def exponential_map(axag64, kit=MP, mutant=None):
    """exponential_map alone: [b,9] float64 (and .mp, the unrounded entries, for the mp kit)"""
    axag64 = np.asarray(axag64, F64)
    with mpmath.workdps(DIGITS):
        rows = [[e.v for row in _exp_map([Dual(kit.c(x)) for x in a], kit, mutant) for e in row] for a in axag64]
        R = np.array([[float(x) for x in r] for r in rows], F64).reshape(len(rows), 9)
    return SimpleNamespace(R=R, mp=rows if kit is MP else None)


# ---- everything fp32: float64 reference / float32 restatement ------------------------------------------------------------
def translation_error(pred, label, dtype=F64):
    """trans_distance.py:4-9: per = sqrt(sum (label - pred)^2)"""
    d = np.asarray(label).astype(dtype) - np.asarray(pred).astype(dtype)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def translation_grad(pred, label, per, gper, dtype=F64):
    """d per / d pred = -(label - pred) / per, times the upstream gper [b]; a row with pred == label is 0/0 = NaN"""
    d = np.asarray(label).astype(dtype) - np.asarray(pred).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.asarray(gper).astype(dtype) / np.asarray(per).astype(dtype)
        return -(g[:, None] * d)


def loss_mix(a, b, c, w, dtype=F64):
    """total = w0 * a + w1 * b + w2 * c (train...:268)"""
    f = dtype
    return (f(F32(w[0])) * f(a) + f(F32(w[1])) * f(b)) + f(F32(w[2])) * f(c)


def loss_mix_grad(g, w, dtype=F64):
    return tuple(dtype(F32(g)) * dtype(F32(x)) for x in w)


ADAM = SimpleNamespace(lr=F32(0.0008), beta1=F32(0.9), beta2=F32(0.999), eps=F32(1e-8))


def adam_step(p, g, m, v, b1p, b2p, grad_scale=1.0, hp=ADAM, dtype=F64, mutant=None):
    """TF-1.x ApplyAdam: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) from the beta powers BEFORE the step; g = grad *
    grad_scale; m += (g - m)(1 - beta1); v += (g g - v)(1 - beta2); p -= lr_t m / (sqrt(v) + eps).  Namespace: p, m, v,
    b1p, b2p (advanced, float32) and the bounds' terms update, g."""
    f = dtype
    c = lambda x: f(F32(x))
    one = f(1.0)
    q1, q2 = c(b1p), c(b2p)
    if mutant == "adam_lr_from_advanced_powers":
        q1, q2 = q1 * c(hp.beta1), q2 * c(hp.beta2)
    lr_t = c(hp.lr) * np.sqrt(one - q2) / (one - q1)
    raw = np.asarray(g).astype(f)
    gs = raw * c(grad_scale)
    m0, v0 = np.asarray(m).astype(f), np.asarray(v).astype(f)
    m1 = m0 + (gs - m0) * (one - c(hp.beta1))
    sq = raw * raw if mutant == "adam_unscaled_square" else gs * gs
    v1 = v0 + (sq - v0) * (one - c(hp.beta2))
    den = np.sqrt(v1 + c(hp.eps)) if mutant == "adam_eps_inside_sqrt" else np.sqrt(v1) + c(hp.eps)
    update = (m1 * lr_t) / den
    p0 = np.asarray(p).astype(f)
    return SimpleNamespace(p=p0 - update, m=m1, v=v1, update=update, g=gs, start=SimpleNamespace(p=p0, m=m0, v=v0),
                           b1p=F32(F64(F32(b1p)) * F64(hp.beta1)), b2p=F32(F64(F32(b2p)) * F64(hp.beta2)))


def sgd_step(p, g, lr, grad_scale, dtype=F64):
    """tf.train.GradientDescentOptimizer: var -= lr * (g * grad_scale)"""
    f = dtype
    return np.asarray(p).astype(f) - f(F32(lr)) * (np.asarray(g).astype(f) * f(F32(grad_scale)))


BN_DECAY = SimpleNamespace(init=0.5, decay_step=40.0, rate=0.5, clip=0.99)      # train...:166-169


def bn_decay(step, batch_size, hp=BN_DECAY, dtype=F64):
    """min(clip, 1 - init * rate^floor(step * batch / decay_step))   (train...:194-202)"""
    f = dtype
    p = np.floor(f(F32(step)) * f(F32(batch_size)) / f(F32(hp.decay_step)))
    return min(f(F32(hp.clip)), f(1.0) - f(F32(hp.init)) * f(F32(hp.rate)) ** p)


def mean(x, dtype=F64, mutant=None):
    """tf.reduce_mean of float32 values.  float64: the exactly rounded mean (math.fsum, one division in 50 digits);
    float32 restatement: float64 partial sums of 256 elements, summed, divided by n, rounded to float32 once."""
    x = np.asarray(x, F32).ravel()
    n = x.size
    count = -(-n // 256) * 256 if mutant == "mean_over_padded_count" else n
    if dtype is F64:
        with mpmath.workdps(DIGITS):
            return float(mpmath.mpf(math.fsum(x.astype(F64).tolist())) / count)       # (fsum rounds the exact sum once)
    pad = np.zeros(-(-n // 256) * 256, F64)
    pad[:n] = x
    return F32(pad.reshape(-1, 256).sum(1).sum() / F64(count))


def pool_rows(x, G, R, C, mode, dtype=F64):
    """tf.reduce_mean (mode 1) / tf.reduce_max (mode 2) over groups of R consecutive rows of x [G*R, C]: (out, ties,
    sum|x| / R)"""
    xg = np.asarray(x, F32).reshape(G, R, C).astype(dtype)
    if mode == 1:
        s = np.zeros((G, C), dtype)
        for r in range(R):              # a sequential sum in the working precision
            s = s + xg[:, r]
        return s / dtype(R), None, np.abs(xg.astype(F64)).sum(1) / R
    out = xg.max(1)
    return out, (xg == out[:, None, :]).sum(1).astype(dtype), None


def pool_rows_grad(x, out, ties, g, G, R, C, mode, dtype=F64, mutant=None):
    """mean: g / R to every row; max: g / ties to every row that equals the maximum (tf.reduce_max shares among ties)"""
    g = np.asarray(g).astype(dtype)
    if mode == 1:
        return np.repeat((g / dtype(R))[:, None, :], R, 1).reshape(G * R, C)
    xg = np.asarray(x, F32).reshape(G, R, C).astype(dtype)
    share = g if mutant == "max_grad_unshared" else g / np.asarray(ties).astype(dtype)
    return np.where(xg == np.asarray(out).astype(dtype)[:, None, :], share[:, None, :], dtype(0.0)).reshape(G * R, C)


def edge_feature(x, nn_idx, B, N, k, C, with_center):
    """get_edge_feature (tf_util.py:635-669) / its wo_center variant (:672-706): out[b,i,j] = [x_i, x_nbr - x_i] or only the
    second half.  x [B*N, >= C] float32 (the first C columns count); float32 subtraction is the definition."""
    xs = np.asarray(x, F32)[:, :C].reshape(B, N, C)
    nbr = xs[np.arange(B)[:, None, None], np.asarray(nn_idx).reshape(B, N, k)]          # [B,N,k,C]
    ctr = np.broadcast_to(xs[:, :, None, :], nbr.shape)
    diff = nbr - ctr
    return (np.concatenate([ctr, diff], -1) if with_center else diff).reshape(B * N * k, -1)


def edge_feature_grad(g, nn_idx, B, N, k, C, with_center, dtype=F64):
    """dx_i += sum_j (g_center[i,j] - g_diff[i,j]); dx_nbr(i,j) += g_diff[i,j].  Returns (dx [B*N,C], sum of |terms|);
    float32: the same terms added in edge order in float32."""
    g = np.asarray(g, F32).reshape(B * N, k, -1).astype(dtype)
    gd = g[:, :, C:] if with_center else g
    gc = g[:, :, :C] if with_center else np.zeros_like(gd)
    pt = np.repeat(np.arange(B * N), k)
    nb = ((np.arange(B * N) // N * N)[:, None] + np.asarray(nn_idx).reshape(B * N, k)).ravel()
    dx, mag = np.zeros((B * N, C), dtype), np.zeros((B * N, C), F64)
    np.add.at(dx, pt, (gc - gd).reshape(-1, C))
    np.add.at(dx, nb, gd.reshape(-1, C))
    np.add.at(mag, pt, (np.abs(gc) + np.abs(gd)).reshape(-1, C).astype(F64))
    np.add.at(mag, nb, np.abs(gd).reshape(-1, C).astype(F64))
    return dx, mag


# ---- normalised errors --------------------------------------------------------------------------------------------------
def _ratio(err, den, slack=0.0):
    """max of (|err| - slack) / den; where the bound is zero the value must be exact; a non-finite error is infinite"""
    err = np.abs(np.asarray(err, F64))
    bad = ~np.isfinite(err)
    err = np.maximum(np.where(bad, 0.0, err) - slack, 0.0)
    den = np.broadcast_to(np.asarray(den, F64), err.shape)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.where(bad, np.inf, q).max())


def ulps(got, want, dtype=F32):
    """largest distance of got from the dtype array `want` in units of want's spacing"""
    want = np.asarray(want, dtype)
    return _ratio(np.asarray(got, F64) - want.astype(F64), np.spacing(np.abs(want)).astype(F64))


def exact(got, want):
    """number of elements whose bits differ (any NaN equals any NaN)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bits = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return float((~((got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want)))).sum())


def _mp_err(got, ref_mp):
    """|got - ref| taken in 50 digits, as float64"""
    with mpmath.workdps(DIGITS):
        return np.array([float(abs(mpmath.mpf(float(g)) - r)) for g, r in zip(np.asarray(got, F64).ravel(), ref_mp)], F64)


def _jac_bound(ref):
    """u64 * max|J| * (1 + 1 / (1 - t^2)) per row, [b,1]"""
    with np.errstate(divide="ignore", invalid="ignore"):      # (clipped rows are judged otherwise)
        return (U64 * np.abs(ref.jac).max(1) * (1.0 + 1.0 / (1.0 - ref.t ** 2)))[:, None]


def rotation_errors(got, ref):
    """got: dict with any of theta [b], jac [b,3], rot_loss (float32 scalar), drot [b,3] (float32) + drot_scale (the float32
    upstream times w_rot, over b: a float64 number); ref: rotation(.., MP)."""
    e = {}
    un, cl = ref.clipped == 0, ref.clipped != 0
    if "theta" in got:
        err = _mp_err(got["theta"], ref.theta_mp)
        e["theta"] = _ratio(err[un], U64 * ref.S[un] / np.sqrt(1.0 - ref.t[un] ** 2))
        e["theta_clipped"] = _ratio(err[cl], np.spacing(ref.theta[cl]))
    if "jac" in got:
        err = _mp_err(got["jac"], [x for row in ref.jac_mp for x in row]).reshape(-1, 3)
        e["jac"] = _ratio(err[un], _jac_bound(ref)[un])
        e["jac_clipped"] = float((np.asarray(got["jac"])[cl] != 0.0).sum())
    if "rot_loss" in got:
        e["rot_loss"] = ulps(got["rot_loss"], F32(ref.mean))
    if "drot" in got:
        s = abs(got["drot_scale"])
        want = got["drot_scale"] * ref.jac
        e["drot"] = _ratio((np.asarray(got["drot"], F64) - want)[un], s * _jac_bound(ref)[un],
                           np.spacing(np.abs(want.astype(F32))).astype(F64)[un])
        e["drot_clipped"] = float((np.asarray(got["drot"])[cl] != 0.0).sum())
    return e


def exp_map_errors(R, axag64, ref):
    """entries, R^T R = I and det R = 1, all against u64 * (1 + |axag|^2)"""
    R = np.asarray(R, F64).reshape(-1, 9)
    den = U64 * (1.0 + (np.asarray(axag64, F64) ** 2).sum(1))
    err = _mp_err(R, [x for row in ref.mp for x in row]).reshape(-1, 9)
    M = R.reshape(-1, 3, 3)
    with mpmath.workdps(DIGITS):
        orth, det = np.zeros(len(M)), np.zeros(len(M))
        for i, m in enumerate(M):
            A = mpmath.matrix(m.tolist())
            D = A.T * A - mpmath.eye(3)
            orth[i] = float(max(abs(D[r, c]) for r in range(3) for c in range(3)))
            det[i] = float(abs(mpmath.det(A) - 1))
    return {"exp": _ratio(err, den[:, None]), "exp_orth": _ratio(orth, den), "exp_det": _ratio(det, den)}


def translation_errors(got, x, gper):
    """got: dict with any of tper [b], trans_loss, dtrans [b,3]; x holds tpred / tlabel; gper: the float32 upstream per row.
    The gradient is judged against the float64 gradient formed from the float64 per."""
    e = {}
    per = translation_error(x.tpred, x.tlabel)
    if "tper" in got:
        e["tper"] = _ratio(np.asarray(got["tper"], F64) - per, U32 * per)
    if "trans_loss" in got:
        e["trans_loss"] = ulps(got["trans_loss"], F32(mean_of_f64(per)))
    if "dtrans" in got:
        want = translation_grad(x.tpred, x.tlabel, per, np.full(len(per), gper, F32))
        dt = np.asarray(got["dtrans"])
        nan_row = per == 0
        e["dtrans_nan"] = float((np.isnan(dt) != np.repeat(nan_row[:, None], 3, 1)).sum())
        e["dtrans"] = _ratio((dt.astype(F64) - want)[~nan_row], U32 * np.abs(want)[~nan_row])
    return e


def mean_of_f64(a):
    return math.fsum(np.asarray(a, F64).tolist()) / len(a)


def adam_errors(got, ref):
    """got: dict p, m, v (float32 arrays), b1p, b2p; ref: adam_step(.., F64) from the same state (ref.start)"""
    s = ref.start
    e = {"param": _ratio(np.asarray(got["p"], F64) - ref.p, U32 * (np.abs(s.p) + np.abs(ref.update))),
         "m": _ratio(np.asarray(got["m"], F64) - ref.m, U32 * (np.abs(s.m) + np.abs(ref.g))),
         "v": _ratio(np.asarray(got["v"], F64) - ref.v, U32 * (np.abs(s.v) + ref.g ** 2))}
    if "b1p" in got:
        e["b1p"], e["b2p"] = ulps(got["b1p"], ref.b1p), ulps(got["b2p"], ref.b2p)
    return e


# which measured constant judges which normalised error; the others are fixed by their meaning (ulps, exact counts)
CONSTANT_OF = {"theta": "c_theta", "jac": "c_jac", "drot": "c_jac", "exp": "c_exp", "exp_orth": "c_exp", "exp_det": "c_exp",
               "tper": "c_t", "dtrans": "c_tg", "param": "c_p", "m": "c_m", "v": "c_v", "pool_mean": "c_pool",
               "edge_grad": "c_eg"}
FIXED = {"theta_clipped": 2.0, "jac_clipped": 0.0, "drot_clipped": 0.0, "rot_loss": 1.0, "trans_loss": 1.0, "dtrans_nan": 0.0,
         "b1p": 1.0, "b2p": 1.0, "mean": 1.0, "pool_max": 0.0, "ties": 0.0, "pool_grad": 1.0, "edge": 0.0, "exact": 0.0,
         "zero_block": 0.0, "per": 0.0}

# Measured by tests/test_step_reference_host.py::test_constants_are_four_times_the_restatement (largest normalised error of
# the restatement -- float64 for the rotation, float32 for the rest -- against the reference over CASES), times four,
# rounded up to a power of two.  The measured values are in profiles/notes_step_paths.md.
ALLOWED = {"c_theta": 64.0, "c_jac": 32.0, "c_exp": 8.0, "c_t": 16.0, "c_tg": 16.0, "c_p": 64.0, "c_m": 8.0, "c_v": 4.0,
           "c_pool": 16.0, "c_eg": 16.0}


def allowed_of(name):
    return FIXED[name] if name in FIXED else ALLOWED[CONSTANT_OF[name]]


def pow2_ceil(x):
    return float(2.0 ** np.ceil(np.log2(x)))


# ---- the case table -----------------------------------------------------------------------------------------------------
ROW_KINDS = ("generic", "large", "pred_taylor", "both_taylor", "below_switch", "above_switch", "pred_zero", "rel_1e-1",
             "rel_1e-2", "rel_1e-3", "near_pi", "equal", "exact_pi")
ROT_BATCHES = (1, 63, 64, 65, 256, 257, 600)
# the mean that cloudaae_loss_tail forms next to the pose losses takes the sizes of the mean cases
MEAN_SIZES = (1, 255, 256, 65536, 65537, 3 * 65536 + 17)
ADAM_SIZES = (1, 2, 3, 4, 7, 1003, 4096, 2048 * 256 * 4 + 4 * 300 + 3)
ELEM_SIZES = (1, 255, 257, 2048 * 256 + 77)


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _quat(w):
    a = np.linalg.norm(w)
    return np.concatenate([[math.cos(a / 2)], (math.sin(a / 2) / a) * w]) if a > 0 else np.array([1.0, 0, 0, 0])


def _qmul(a, b):
    return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])


def _compose(w, lab):
    """the axis-angle p with exp(lab) exp(p)^T = exp(w)"""
    q = _qmul(_quat(-w), _quat(lab))
    s = np.linalg.norm(q[1:])
    return (2.0 * math.atan2(s, q[0]) / s) * q[1:]


def _rot_row_inputs(kind, rng):
    """(prediction float32 [3], label float64 [3]) of one row kind"""
    lab = rng.standard_normal(3)
    if kind == "generic":
        p = rng.standard_normal(3)
    elif kind == "large":
        p, lab = 3.0 * rng.standard_normal(3), 3.0 * rng.standard_normal(3)
        for v in (p, lab):
            if np.linalg.norm(v) <= math.pi:
                v *= (math.pi + 0.5 + rng.random()) / np.linalg.norm(v)
    elif kind in ("pred_taylor", "both_taylor"):
        p = _unit(rng) * math.sqrt(rng.uniform(1e-4, 5e-3))
        if kind == "both_taylor":
            lab = _unit(rng) * math.sqrt(rng.uniform(1e-4, 9e-3))
    elif kind == "below_switch":
        p = _unit(rng) * math.sqrt(rng.uniform(5.001e-3, 9.99e-3))
    elif kind == "above_switch":
        p = _unit(rng) * math.sqrt(rng.uniform(1.001e-2, 1.499e-2))
    elif kind == "pred_zero":
        p = np.zeros(3)
    elif kind.startswith("rel_"):
        p = _compose(_unit(rng) * float(kind[4:]) * rng.uniform(0.8, 1.2), lab)
    elif kind == "near_pi":
        p = _compose(_unit(rng) * (math.pi - rng.uniform(2e-3, 1e-2)), lab)
    elif kind == "equal":
        p = lab.copy()
    else:       # exact_pi: the same axis, the angle pi apart (up to the float32 rounding of the prediction)
        p = lab * (1.0 - math.pi / np.linalg.norm(lab))
    return p.astype(F32), lab.astype(F64)


def _case(family, name, **kw):
    return SimpleNamespace(family=family, name=name, **kw)


def _cases():
    t = []
    for i, b in enumerate(ROT_BATCHES):
        # nan_row: a translation row with prediction == label (its gradient is 0/0)
        t.append(_case("rot", "rot_b%d" % b, b=b, n=(MEAN_SIZES + (4096,))[i], nan_row=5 if b in (65, 600) else None,
                       weights=(1000.0, 10.0, 1.0) if i % 2 == 0 else (1.5, 0.25, 2.0), g=0.75))
    for n in ADAM_SIZES:
        for gs, exhausted in ((1.0, 0), (0.25, 0), (1.0, 1), (0.25, 1)):
            t.append(_case("adam", "adam_n%d_gs%g_%s" % (n, gs, "exhausted" if exhausted else "step1"), n=n, grad_scale=gs,
                           exhausted=exhausted))
    for n in MEAN_SIZES:
        t.append(_case("mean", "mean_n%d" % n, n=n))
    for G, R, C in ((1, 1, 1), (50, 7, 33), (96, 10, 64), (3, 1, 5), (4100, 2, 129)):
        for mode in (1, 2):
            t.append(_case("pool", "pool_%s_%dx%dx%d" % ("mean" if mode == 1 else "max", G, R, C), G=G, R=R, C=C, mode=mode))
    for B, N, k, C, ldx, wc in ((2, 33, 5, 7, 7, 1), (2, 33, 5, 7, 12, 0), (3, 20, 1, 3, 3, 1), (3, 20, 1, 3, 4, 0),
                                (1, 1, 1, 1, 1, 1), (4, 257, 10, 64, 96, 1), (4, 257, 10, 64, 64, 0)):
        t.append(_case("edge", "edge_B%d_N%d_k%d_C%d_ld%d_%s" % (B, N, k, C, ldx, "center" if wc else "nocenter"), B=B, N=N,
                       k=k, C=C, ldx=ldx, with_center=wc))
    for n in ELEM_SIZES:
        t.append(_case("elem", "elem_n%d" % n, n=n))
    for B, R, D in ((1, 1, 3), (3, 17, 5), (2, 1000, 3), (7, 15001, 5)):
        t.append(_case("rowvec", "rowvec_%dx%dx%d" % (B, R, D), B=B, R=R, D=D))
    return t


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
assert all(c.B * c.N * c.k * c.C > 524288 for c in CASES if c.family == "edge" and c.N == 257)
assert all((c.R * c.D) % 256 for c in CASES if c.family == "rowvec")


def names(family):
    return [c.name for c in CASES if c.family == family]


def _seed(c):
    """a case's seed follows from its name: adding a case leaves the others, and the measured constants, as they are"""
    return zlib.crc32(c.name.encode())


def _rot_inputs(c):
    """rows of every kind, redrawn from the next seed while the 50-digit cosine lies within 1e-9 of the clip"""
    b, seed = c.b, _seed(c)
    pred, label, kinds, redraws = np.zeros((b, 3), F32), np.zeros((b, 3), F64), [], 0
    rows = []
    for i in range(b):
        kind = ROW_KINDS[i % len(ROW_KINDS)]
        attempt = 0
        while True:
            p, lab = _rot_row_inputs(kind, np.random.default_rng((seed, i, attempt)))
            with mpmath.workdps(DIGITS):
                row = _rotation_row(p, lab, MP)
                ok = abs(abs(row[2]) - mpmath.mpf(LIM)) > mpmath.mpf(1e-9)
            if ok:
                break
            attempt += 1
            redraws += 1
        pred[i], label[i] = p, lab
        kinds.append(kind)
        rows.append(row)
    rng = np.random.default_rng((seed, b))
    tpred, tlabel = rng.standard_normal((b, 3)).astype(F32), rng.standard_normal((b, 3)).astype(F32)
    if c.nan_row is not None:
        tpred[c.nan_row] = tlabel[c.nan_row]
    d1 = (1e4 + rng.standard_normal(c.n)).astype(F32)
    d2 = rng.random(c.n).astype(F32)
    return SimpleNamespace(pred=pred, label=label, kinds=kinds, redraws=redraws, rows=b, mp_rows=rows, tpred=tpred,
                           tlabel=tlabel, d1=d1, d2=d2)


def _adam_inputs(c):
    rng = np.random.default_rng(_seed(c))
    n = c.n
    s = 10.0 ** rng.uniform(-12, 6, n)               # gradients spanning 1e-12 .. 1e6, the state to scale
    p = rng.standard_normal(n).astype(F32)
    m = (0.5 * s * rng.standard_normal(n)).astype(F32)
    v = (s * s * (0.1 + np.abs(rng.standard_normal(n)))).astype(F32)
    grads = [(s * rng.standard_normal(n)).astype(F32) for _ in range(3)]
    # element 0 is plain whatever the draw: O(1) everywhere, moment and gradients of one sign (no cancellation in m), so the
    # step it takes is far above the round-off of its parameter (the sizes 1, 2 and 3 hold little else)
    p[0], m[0], v[0] = 0.5, 0.5, 0.5
    for a in grads:
        a[0] = 0.5 + abs(a[0]) / max(s[0], 1e-30)
    lo, hi = (n // 2, n // 2 + max(1, n // 8)) if n >= 4 else (0, 0)
    for a in [m, v] + grads:
        a[lo:hi] = 0.0
    b1p, b2p = (F32(0.0), F32(1e-30)) if c.exhausted else (ADAM.beta1, ADAM.beta2)
    return SimpleNamespace(p=p, m=m, v=v, grads=grads, zero=(lo, hi), b1p=b1p, b2p=b2p, redraws=0, rows=n)


def _pool_ambiguous(x, G, R, C):
    """groups whose maximum float32 cannot name: a NaN, or zeros of both signs at the top"""
    xg = x.reshape(G, R, C)
    top = xg.max(1)
    both = ((xg == 0) & np.signbit(xg)).any(1) & ((xg == 0) & ~np.signbit(xg)).any(1) & (top == 0)
    return np.isnan(xg).any(1) | both


def _pool_inputs(c):
    G, R, C, seed = c.G, c.R, c.C, _seed(c)
    x = np.zeros((G, R, C), F32)
    redraws = 0
    for attempt in range(4):
        rng = np.random.default_rng((seed, attempt))
        fresh = rng.standard_normal((G, R, C)).astype(F32)
        bad = _pool_ambiguous(x.reshape(G * R, C), G, R, C).any(1) if attempt else np.ones(G, bool)
        x[bad] = fresh[bad]
        if c.mode == 2 and R >= 2 and G >= 3:
            top = np.abs(x).max(1) + 1.0
            x[0, 0] = x[0, R - 1] = top[0]                       # a tie of two
            if R >= 3:
                x[1, 0] = x[1, 1] = x[1, R - 1] = top[1]         # a tie of three
            x[2] = -np.inf                                        # a group that is entirely -inf
        if not _pool_ambiguous(x.reshape(G * R, C), G, R, C).any():
            break
        redraws += int(_pool_ambiguous(x.reshape(G * R, C), G, R, C).any(1).sum())
    g = np.random.default_rng((seed, 99)).standard_normal((G, C)).astype(F32)
    return SimpleNamespace(x=x.reshape(G * R, C), g=g, redraws=redraws, rows=G)


def _edge_inputs(c):
    rng = np.random.default_rng(_seed(c))
    B, N, k, C = c.B, c.N, c.k, c.C
    x = rng.standard_normal((B * N, c.ldx)).astype(F32)
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx[:, 0, 0] = 0                                  # a neighbour list that names the point itself ...
    if k >= 3:
        idx[:, 0, 1] = idx[:, 0, 2] = N - 1          # ... and one neighbour twice
    g = rng.standard_normal((B * N * k, 2 * C if c.with_center else C)).astype(F32)
    return SimpleNamespace(x=x, idx=idx, g=g, redraws=0, rows=B * N)


def _flat_inputs(c):
    rng = np.random.default_rng(_seed(c))
    n = c.n if c.family != "rowvec" else c.B * c.R * c.D
    x = SimpleNamespace(a=(1e4 + rng.standard_normal(n)).astype(F32), b=rng.standard_normal(n).astype(F32),
                        c=rng.standard_normal(n).astype(F32), scalar=F32(rng.standard_normal()), redraws=0, rows=n)
    if c.family == "rowvec":
        x.v = rng.standard_normal((c.B, c.D)).astype(F32)
    return x


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASE_BY_NAME[name]
    return {"rot": _rot_inputs, "adam": _adam_inputs, "pool": _pool_inputs, "edge": _edge_inputs, "mean": _flat_inputs,
            "elem": _flat_inputs, "rowvec": _flat_inputs}[c.family](c)


def make_inputs(c):
    """the conditioned inputs of a case; computed once, not to be written to"""
    return _inputs(c.name)


def condition(c):
    """Number of rows that had to be redrawn from the next seed before the case was well posed: no rotation row whose
    unclipped |cosine| lies within 1e-9 of 0.9999999 at 50 digits, no pool-rows maximum that is ambiguous."""
    x = make_inputs(c)
    if c.family == "rot":
        ref = reference(c)
        assert (np.abs(np.abs(ref.t) - LIM) > 1e-9).all()
    if c.family == "pool":
        assert not _pool_ambiguous(x.x, c.G, c.R, c.C).any()
    return x.redraws


@functools.lru_cache(maxsize=None)
def _rot_reference(name):
    x = make_inputs(CASE_BY_NAME[name])
    return rotation(x.pred, x.label, MP, rows=x.mp_rows)


def reference(c):
    """the 50-digit rotation reference of a rotation case; computed once"""
    return _rot_reference(c.name)


def mutant_applies(mutant, c):
    """the cases a mutant must be caught on"""
    if c.family == "rot":
        if mutant in ("taylor_drops_theta6", "clip_keeps_derivative"):
            return c.b >= len(ROW_KINDS)
        return mutant in ("no_transpose", "jacobian_column_negated")
    if c.family == "adam":
        if mutant == "adam_lr_from_advanced_powers":
            return not c.exhausted
        if mutant == "adam_unscaled_square":
            return c.grad_scale != 1.0
        return mutant == "adam_eps_inside_sqrt" and c.n >= 1000      # (needs an element with v within reach of eps)
    if c.family == "pool":
        return mutant == "max_grad_unshared" and c.mode == 2 and c.R >= 2 and c.G >= 3
    if c.family == "mean":
        return mutant == "mean_over_padded_count" and c.n % 256 != 0
    return False


# ---- a case's outputs and their errors ------------------------------------------------------------------------------------
def pose_scales(c):
    """(float32 upstream of the translation rows gt / b, float64 scale of the rotation Jacobian gr / b) of a rotation case"""
    gt, gr = F32(c.g) * F32(c.weights[1]), F32(c.g) * F32(c.weights[2])
    return gt / F32(c.b), F64(gr) / F64(c.b)


def rot_outputs(c, x, mutant=None):
    """what the entry points would have written, had they computed the restatement (float64 rotation, float32
    translation) or a mutant of it"""
    r = rotation(x.pred, x.label, FL, mutant)
    gper, scale = pose_scales(c)
    tper = translation_error(x.tpred, x.tlabel, F32)
    return {"theta": r.theta, "jac": r.jac, "rot_loss": F32(r.mean), "drot": (scale * r.jac).astype(F32), "drot_scale": scale,
            "tper": tper, "trans_loss": F32(tper.astype(F64).sum() / c.b),
            "dtrans": translation_grad(x.tpred, x.tlabel, tper, np.full(c.b, gper, F32), F32),
            "expR": exponential_map(x.label, FL, mutant).R}


@functools.lru_cache(maxsize=None)
def _exp_reference(name):
    return exponential_map(make_inputs(CASE_BY_NAME[name]).label, MP)


def rot_errors(c, x, got):
    e = rotation_errors(got, reference(c))
    e.update(translation_errors(got, x, pose_scales(c)[0]))
    if "expR" in got:
        e.update(exp_map_errors(got["expR"], x.label, _exp_reference(c.name)))
    return e


def adam_errors_over_steps(c, x, stepper):
    """Three consecutive steps.  stepper(state, grad, b1p, b2p) -> dict p, m, v (float32 arrays), b1p, b2p (float32): the
    code under test.  Each step is judged against the float64 step from the state it actually started from, with the beta
    powers before the step.  Returns the largest error of each kind and the final state."""
    state = SimpleNamespace(p=x.p, m=x.m, v=x.v)
    b1p, b2p = x.b1p, x.b2p
    worst = {}
    lo, hi = x.zero
    for grad in x.grads:
        ref = adam_step(state.p, grad, state.m, state.v, b1p, b2p, c.grad_scale)
        got = stepper(state, grad, b1p, b2p)
        e = adam_errors(got, ref)
        e["zero_block"] = exact(np.asarray(got["p"], F32)[lo:hi], np.asarray(state.p, F32)[lo:hi]) + \
            float(np.count_nonzero(got["m"][lo:hi])) + float(np.count_nonzero(got["v"][lo:hi]))
        for k, val in e.items():
            worst[k] = max(worst.get(k, 0.0), val)
        state = SimpleNamespace(p=np.asarray(got["p"], F32), m=np.asarray(got["m"], F32), v=np.asarray(got["v"], F32))
        b1p, b2p = ref.b1p, ref.b2p
    return worst, state


def adam_stepper(c, dtype=F32, mutant=None):
    def step(state, grad, b1p, b2p):
        r = adam_step(state.p, grad, state.m, state.v, b1p, b2p, c.grad_scale, dtype=dtype, mutant=mutant)
        return {"p": r.p.astype(F32), "m": r.m.astype(F32), "v": r.v.astype(F32), "b1p": r.b1p, "b2p": r.b2p}
    return step


def mean_outputs(c, x, mutant=None):
    per = x.a + x.b
    return {"mean": mean(x.a, F32, mutant), "per": per, "add_mean": mean(per, F32, mutant)}


def mean_errors(c, x, got):
    per = x.a + x.b
    return {"mean": max(ulps(got["mean"], F32(mean(x.a))), ulps(got["add_mean"], F32(mean(per)))),
            "per": exact(np.asarray(got["per"], F32), per)}


def pool_outputs(c, x, dtype=F32, mutant=None):
    out, ties, _ = pool_rows(x.x, c.G, c.R, c.C, c.mode, dtype)
    dx = pool_rows_grad(x.x, out, ties, x.g, c.G, c.R, c.C, c.mode, dtype, mutant)
    return {"out": out.astype(F32), "ties": None if ties is None else ties.astype(F32), "dx": dx.astype(F32)}


def pool_errors(c, x, got):
    out, ties, mag = pool_rows(x.x, c.G, c.R, c.C, c.mode)
    dx = pool_rows_grad(x.x, out, ties, x.g, c.G, c.R, c.C, c.mode)
    e = {"pool_grad": ulps(got["dx"], dx.astype(F32))}
    if c.mode == 1:
        e["pool_mean"] = _ratio(np.asarray(got["out"], F64) - out, U32 * mag)
    else:
        e["pool_max"] = exact(np.asarray(got["out"], F32), out.astype(F32))
        e["ties"] = exact(np.asarray(got["ties"], F32), ties.astype(F32))
    return e


def edge_outputs(c, x):
    return {"out": edge_feature(x.x, x.idx, c.B, c.N, c.k, c.C, c.with_center),
            "dx": edge_feature_grad(x.g, x.idx, c.B, c.N, c.k, c.C, c.with_center, F32)[0]}


def edge_errors(c, x, got):
    dx, mag = edge_feature_grad(x.g, x.idx, c.B, c.N, c.k, c.C, c.with_center)
    return {"edge": exact(np.asarray(got["out"], F32), edge_feature(x.x, x.idx, c.B, c.N, c.k, c.C, c.with_center)),
            "edge_grad": _ratio(np.asarray(got["dx"], F64) - dx, U32 * mag)}


SGD_LR, SGD_SCALE, FILL_SCALE = F32(0.0008), F32(0.25), F32(1.0 / 3.0)


def elem_expected(c, x):
    """float32 NumPy evaluation of the single expression of each elementwise kernel: the kernels equal it bit for bit"""
    if c.family == "rowvec":
        return {"add_rowvec": (x.a.reshape(c.B, c.R, c.D) + x.v[:, None, :]).reshape(-1)}
    fill = x.scalar * FILL_SCALE
    return {"add": x.a + x.b, "mul_add": x.a + x.b * x.c, "mul_add_no_a": x.b * x.c, "fill": np.full(c.n, fill, F32),
            "fill_add": fill + x.a, "sgd": x.a - SGD_LR * (x.b * SGD_SCALE)}


def elem_errors(c, x, got):
    want = elem_expected(c, x)
    return {"exact": sum(exact(np.asarray(got[k], F32), want[k]) for k in want)}
