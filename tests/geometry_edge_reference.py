"""High-precision reference of the refinement kernels at degenerate and boundary geometry (csrc/icp.hip,
csrc/normals.hip, csrc/pose_math.h), written from DESIGN.md ("Pose refinement", "Surface normals") only: NumPy and
mpmath at 50 digits, as tests/step_reference.py.

  procrustes        the maximum of tr(R^T Sigma) over proper rotations and, where it is unique, its maximiser
  plane_update      the point-to-plane normal equations, solved by mpmath.lu_solve, and cond_2(A)
  covariance_eig    mean, covariance and eigen-decomposition of a neighbourhood
  rodrigues_mp / log_map_mp

Brute-force neighbours and correspondences are those of tests/normals_reference.py and tests/icp_reference.py.  The
file also holds what the CPU and the GPU test share: the input families (every one built from a fixed seed or from
dyadic coordinates), the error measures in the units the bounds are stated in, and two mutants of the restatement
(no reflection fix; `<=` in the radius test) that prove the cases can fail."""
import mpmath
import numpy as np

import icp_plane_reference as PL
import icp_reference as R
import normals_reference as NR

DIGITS = 50
U64 = 2.0 ** -53
ULP32 = 2.0 ** -23
ZERO_GAP = mpmath.mpf(10) ** -40     # s2 + d s3 below this share of s1 is zero to the reference's own precision


def _mpf(v):
    return mpmath.mpf(float(v))


def _mat(a):
    a = np.asarray(a, np.float64)
    return mpmath.matrix([[_mpf(v) for v in row] for row in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


# ---- point to point ---------------------------------------------------------------------------------------------------
def sigma_mp(P, Q):
    """(mp [3], mq [3], Sigma 3x3 = (1/n) sum (q - mq)(p - mp)^T) of the matched fp64 points, in DIGITS digits."""
    n = len(P)
    Pm, Qm = _mat(P), _mat(Q)
    mp_ = [mpmath.fsum(Pm[i, a] for i in range(n)) / n for a in range(3)]
    mq_ = [mpmath.fsum(Qm[i, a] for i in range(n)) / n for a in range(3)]
    S = mpmath.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            S[a, b] = mpmath.fsum((Qm[i, a] - mq_[a]) * (Pm[i, b] - mp_[b]) for i in range(n)) / n
    return mp_, mq_, S


def procrustes(P, Q):
    """P, Q [n,3] float64: the matched points.  Returns a dict: `s` the singular values of Sigma (descending), `d` =
    det U det V of its SVD (sign det Sigma wherever Sigma is regular; with s3 = 0 it multiplies zero), `maximum` =
    s1 + s2 + d s3 = max tr(R^T Sigma) over SO(3), `gap` = s2 + d s3, `unique` (gap > 0 to the reference's precision),
    `sigma`, `mp`, `mq` (mpmath) and, when unique, the maximiser `R` (3x3) and `t` = mq - R mp (mpmath)."""
    with mpmath.workdps(DIGITS):
        mp_, mq_, S = sigma_mp(P, Q)
        U, s, V = mpmath.svd_r(S)                          # Sigma = U diag(s) V, s descending
        d = 1 if mpmath.det(U) * mpmath.det(V) > 0 else -1
        s = [s[0], s[1], s[2]]
        out = dict(s=s, d=d, maximum=s[0] + s[1] + d * s[2], gap=s[1] + d * s[2], sigma=S, mp=mp_, mq=mq_, R=None, t=None)
        out["unique"] = bool(s[0] > 0 and out["gap"] > ZERO_GAP * s[0])
        if out["unique"]:
            Rm = U * mpmath.diag([1, 1, d]) * V
            out["R"] = Rm
            out["t"] = [mq_[a] - mpmath.fsum(Rm[a, b] * mp_[b] for b in range(3)) for a in range(3)]
        return out


def objective(ref, Rm):
    """tr(R^T Sigma) of a float64 rotation against the reference's Sigma."""
    with mpmath.workdps(DIGITS):
        return mpmath.fsum(_mpf(Rm[a][b]) * ref["sigma"][a, b] for a in range(3) for b in range(3))


def procrustes_units(ref, trans0):
    """(u, v): u = 2^-53 (s1 + |mp - c| |mq - c|) / (s2 + d s3), the unit of an error in the transform (None where
    the maximiser is not unique), and v = 2^-53 s1, the unit of an error in the objective.  c = the start translation,
    by which the one-pass sums are shifted."""
    with mpmath.workdps(DIGITS):
        c = [_mpf(v) for v in trans0]
        a = mpmath.sqrt(mpmath.fsum((ref["mp"][k] - c[k]) ** 2 for k in range(3)))
        b = mpmath.sqrt(mpmath.fsum((ref["mq"][k] - c[k]) ** 2 for k in range(3)))
        v = float(U64 * ref["s"][0])
        u = float(U64 * (ref["s"][0] + a * b) / ref["gap"]) if ref["unique"] else None
        return u, v


def transform_after_update(ref, trans0):
    """T = U T0 in DIGITS digits for T0 = [I | trans0]: (R, R trans0 + t) as float64 arrays."""
    with mpmath.workdps(DIGITS):
        c = [_mpf(v) for v in trans0]
        Rm = ref["R"]
        t = [mpmath.fsum(Rm[a, b] * c[b] for b in range(3)) + ref["t"][a] for a in range(3)]
        return _np(Rm), np.array([float(v) for v in t])


def transform_error(T, ref, trans0):
    """The error of a float64 T = U T0 against the reference, before the division by the unit u: the largest
    rotation entry's error, and the translation's error relative to |mp| + |mq| (a rotation error moves the
    translation by that lever arm)."""
    Rr, tr = transform_after_update(ref, trans0)
    with mpmath.workdps(DIGITS):
        arm = float(mpmath.sqrt(mpmath.fsum(v * v for v in ref["mp"])) + mpmath.sqrt(mpmath.fsum(v * v for v in ref["mq"])))
    return max(np.abs(T[:3, :3] - Rr).max(), np.abs(T[:3, 3] - tr).max() / arm)


def umeyama_no_reflection(p, q):
    """MUTANT of icp_reference.umeyama: U V^T without the S = diag(1, 1, -1) fix."""
    U4 = np.eye(4)
    mp_, mq_ = p.mean(axis=0), q.mean(axis=0)
    sigma = (q - mq_).T @ (p - mp_) / len(p)
    U, _, Vt = np.linalg.svd(sigma)
    U4[:3, :3] = U @ Vt
    U4[:3, 3] = mq_ - U4[:3, :3] @ mp_
    return U4


def count_inclusive(P, Q, rho):
    """MUTANT of icp_reference.correspondences: the number of source points with a target at d^2 <= rho^2."""
    d = P[:, None, :] - Q[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return int((d2 <= rho * rho).any(axis=1).sum())


# ---- point to plane ---------------------------------------------------------------------------------------------------
def plane_update(P, Q, N):
    """The 6x6 normal equations of the definition (J = [p x n; n], r = (p - q) . n, A = sum J J^T, b = sum J r) in
    DIGITS digits, A x = -b by mpmath.lu_solve.  Returns (U 4x4 float64 = [Rz(gamma) Ry(beta) Rx(alpha) | t], x [6]
    float64, cond_2(A) float)."""
    with mpmath.workdps(DIGITS):
        Pm, Qm, Nm = _mat(P), _mat(Q), _mat(N)
        A = mpmath.matrix(6, 6)
        b = mpmath.matrix(6, 1)
        for i in range(len(P)):
            p, q, n = (Pm[i, :], Qm[i, :], Nm[i, :])
            r = mpmath.fsum((p[k] - q[k]) * n[k] for k in range(3))
            J = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]]
            for a in range(6):
                b[a] += J[a] * r
                for c in range(6):
                    A[a, c] += J[a] * J[c]
        x = mpmath.lu_solve(A, -b)
        sv = mpmath.svd_r(A, compute_uv=False)
        cond = float(sv[0] / sv[5])
        ca, sa, cb, sb, cg, sg = (mpmath.cos(x[0]), mpmath.sin(x[0]), mpmath.cos(x[1]), mpmath.sin(x[1]),
                                  mpmath.cos(x[2]), mpmath.sin(x[2]))
        U = np.eye(4)
        U[0, :3] = [float(cg * cb), float(cg * sb * sa - sg * ca), float(cg * sb * ca + sg * sa)]
        U[1, :3] = [float(sg * cb), float(sg * sb * sa + cg * ca), float(sg * sb * ca - cg * sa)]
        U[2, :3] = [float(-sb), float(cb * sa), float(cb * ca)]
        U[:3, 3] = [float(x[3]), float(x[4]), float(x[5])]
        return U, np.array([float(v) for v in x]), cond


# ---- normals ------------------------------------------------------------------------------------------------------------
def covariance_eig(neigh):
    """neigh [k,3]: the exact (fp32, widened) neighbours.  Returns (mean [3], C [3,3], w [3] ascending, V [3,3]
    columns = eigenvectors) of DIGITS-digit arithmetic (mpmath.eigsy), rounded to float64 at the end."""
    with mpmath.workdps(DIGITS):
        k = len(neigh)
        X = _mat(neigh)
        mu = [mpmath.fsum(X[i, a] for i in range(k)) / k for a in range(3)]
        C = mpmath.matrix(3, 3)
        for a in range(3):
            for b in range(a, 3):
                C[a, b] = C[b, a] = mpmath.fsum((X[i, a] - mu[a]) * (X[i, b] - mu[b]) for i in range(k)) / k
        w, V = mpmath.eigsy(C)
        order = sorted(range(3), key=lambda i: w[i])
        return (np.array([float(v) for v in mu]), _np(C), np.array([float(w[i]) for i in order]),
                _np(V)[:, order])


def normals_table(support, radius, queries=None, min_neighbors=3):
    """Per query: count [K], w [K,3], C [K,3,3] and v0 [K,3] (an eigenvector of w[0]) of the reference (zeros where
    count < min_neighbors), the neighbour sets being normals_reference.neighbours.  Equal neighbour sets are decomposed
    once."""
    sup = np.asarray(support, np.float64)[:, :3]
    qs = sup if queries is None else np.asarray(queries, np.float64)[:, :3]
    K = len(qs)
    count, w, C, v0 = np.zeros(K, np.int32), np.zeros((K, 3)), np.zeros((K, 3, 3)), np.zeros((K, 3))
    seen = {}
    for i, q in enumerate(qs):
        idx = NR.neighbours(sup, q, radius)
        count[i] = len(idx)
        if len(idx) >= min_neighbors:
            key = idx.tobytes()
            if key not in seen:
                seen[key] = covariance_eig(sup[idx])
            _, C[i], w[i], V = seen[key]
            v0[i] = V[:, 0]
    return count, w, C, v0


def order_of_sums_eps(support, radius, queries=None):
    """100 x max(d, 1e-12), d = what reversing the order of the restatement's own sums changes: the eigenvalues
    relative to the largest (where that is > 0) and 1 - |n . n'| over the queries whose relative gap is >= 0.1 (the
    others have no defined direction to compare)."""
    n0, e0, c0 = NR.estimate_normals(support, radius, queries=queries)
    n1, e1, _ = NR.estimate_normals(support, radius, queries=queries, reverse=True)
    top = e0[:, 2] > 0.0
    d = 0.0
    if top.any():
        d = (np.abs(e0[top] - e1[top]) / e0[top][:, 2:3]).max()
    sharp = (c0 >= 3) & (NR.relative_gap(e0) >= 0.1)
    if sharp.any():
        d = max(d, (1.0 - np.abs((n0[sharp] * n1[sharp]).sum(axis=1))).max())
    return 100.0 * max(d, 1e-12), d


# ---- pose maps ----------------------------------------------------------------------------------------------------------
def rodrigues_mp(r):
    """axangle2mat of DESIGN.md in DIGITS digits, rounded to float64: theta = |r|, the axis normalised; theta = 0 is I."""
    with mpmath.workdps(DIGITS):
        x, y, z = (_mpf(v) for v in r)
        theta = mpmath.sqrt(x * x + y * y + z * z)
        if theta == 0:
            return np.eye(3)
        x, y, z = x / theta, y / theta, z / theta
        c, s = mpmath.cos(theta), mpmath.sin(theta)
        C = 1 - c
        M = [[x * x * C + c, x * y * C - z * s, z * x * C + y * s],
             [x * y * C + z * s, y * y * C + c, y * z * C - x * s],
             [z * x * C - y * s, y * z * C + x * s, z * z * C + c]]
        return np.array([[float(v) for v in row] for row in M])


def log_map_mp(Rm):
    """Axis-angle (angle in [0, pi]) of a float64 rotation matrix in DIGITS digits: theta = atan2(|v|, tr - 1) with v
    the skew part; the axis v / |v|, or for cos theta < -0.5 the largest column of (R + R^T) / 2 - cos I, signed
    to agree with v."""
    with mpmath.workdps(DIGITS):
        M = _mat(Rm)
        v = [M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]
        vn = mpmath.sqrt(mpmath.fsum(a * a for a in v))
        tr1 = M[0, 0] + M[1, 1] + M[2, 2] - 1
        theta = mpmath.atan2(vn, tr1)
        if tr1 > -1:
            if vn == 0:
                return np.zeros(3)
            return np.array([float(a / vn * theta) for a in v])
        cs = tr1 / 2
        B = [[(M[i, j] + M[j, i]) / 2 - (cs if i == j else 0) for j in range(3)] for i in range(3)]
        k = max(range(3), key=lambda i: B[i][i])
        a = [B[0][k], B[1][k], B[2][k]]
        an = mpmath.sqrt(mpmath.fsum(t * t for t in a))
        a = [t / an for t in a]
        if mpmath.fsum(a[i] * v[i] for i in range(3)) < 0:
            a = [-t for t in a]
        return np.array([float(t * theta) for t in a])


# ---- input families -----------------------------------------------------------------------------------------------------
F32 = np.float32
P2P_RADIUS = 0.01
GENERIC_AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


def _lattice(shape, spacing):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape], indexing="ij"), axis=-1)
    return g.reshape(-1, len(shape)) * spacing


def _moved(P, rot, shift):
    """A rigid move of the fp64 points P about their centroid, rounded to float32."""
    c = P.mean(axis=0)
    return ((P - c) @ R.rodrigues(rot).T + c + shift).astype(F32)


def pad_clouds(cases, M, N):
    """[B,M,3] sources and [B,N,3] targets: each case's clouds, filled up with points that find no partner (sources
    past +500 m, targets past -500 m, 1 m apart)."""
    B = len(cases)
    src = np.zeros((B, M, 3), F32)
    dst = np.zeros((B, N, 3), F32)
    for c, case in enumerate(cases):
        m, n = len(case["src"]), len(case["dst"])
        assert m <= M and n <= N
        src[c] = 500.0
        dst[c] = -500.0
        src[c, :, 0] += np.arange(M)
        dst[c, :, 0] -= np.arange(N)
        src[c, :m] = case["src"]
        dst[c, :n] = case["dst"]
    return src, dst


def procrustes_cases():
    """name -> dict(src [m,3] f32, dst [m,3] f32 = the source at T0 moved, trans0 [3] f32, unique, d).  `d` is None
    where Sigma is singular and the sign multiplies zero."""
    rng = np.random.default_rng(3601)
    cases = {}

    def add(name, src, trans0, unique, d, rot=None, shift=None, dst=None):
        src = np.asarray(src, np.float64).astype(F32)
        trans0 = np.asarray(trans0, np.float64).astype(F32)
        P = src.astype(np.float64) + trans0.astype(np.float64)
        if dst is None:
            dst = _moved(P, rot, shift)
        cases[name] = dict(src=src, dst=np.asarray(dst, F32), trans0=trans0, unique=unique, d=d)

    zero = np.zeros(3)
    spin = GENERIC_AXIS * 0.02
    step = np.array([1e-3, -5e-4, 8e-4])
    blob = _lattice((5, 5, 5), 0.02) + rng.uniform(-3e-3, 3e-3, (125, 3)) + [0.013, -0.021, 0.017]
    add("blob", blob, zero, True, 1, spin, step)
    tilt = np.array([0.6, 0.64, 0.48]) * 0.02                       # a unit axis out of the lattice's plane
    flat = np.concatenate([_lattice((8, 8), 0.02), np.zeros((64, 1))], axis=1) + [0.01, 0.02, -0.015]
    add("plane_square", flat, zero, True, None, tilt, step)
    flat = np.concatenate([_lattice((8, 5), 0.02), np.zeros((40, 1))], axis=1) + [0.01, 0.02, -0.015]
    add("plane_rectangle", flat, zero, True, None, tilt, step)
    line = np.arange(-8, 8)[:, None] * np.array([2.0, 1.0, -2.0]) * 2.0 ** -8 + np.array([3.0, -2.0, 5.0]) * 2.0 ** -8
    add("collinear", line, zero, False, None, spin, step)
    add("two_points", [[0.01, 0.02, -0.01], [0.03, -0.01, 0.02]], zero, False, None, spin, step)
    add("one_point", [[0.0123, -0.0456, 0.0789]], zero, False, None, spin, step)
    # 64 copies of one point, moved by one dyadic step: every sum of the one-pass form is exact, so Sigma = 0 exactly
    same = np.tile([[0.25, -0.125, 0.5]], (64, 1))
    add("coincident", same, zero, False, None, dst=same + np.array([3.0, -2.0, 1.0]) * 2.0 ** -10)
    # a thin slab, tilted, mirrored through its own plane: Sigma = C - 2 sz^2 n n^T, det < 0, the maximiser is I
    slab = np.concatenate([_lattice((8, 8), 0.02) + rng.uniform(-3e-3, 3e-3, (64, 2)),
                           rng.uniform(-1e-3, 1e-3, (64, 1))], axis=1)
    G = R.rodrigues(GENERIC_AXIS * 0.7)
    add("slab_mirrored", slab @ G.T, zero, True, -1, dst=((slab * [1.0, 1.0, -1.0]) @ G.T).astype(F32))
    # a rod of square cross-section mirrored through a plane that holds its axis, dyadic: Sigma = diag(sx^2, a^2, -a^2)
    a = 2.0 ** -9
    rod = np.stack([(2.0 * np.arange(8) - 7.0) * 2.0 ** -7, a * np.array([1, -1, -1, 1, 1, -1, -1, 1.0]),
                    a * np.array([1, -1, 1, -1, -1, 1, -1, 1.0])], axis=1)
    add("rod_mirrored", rod, zero, False, -1, dst=rod * [1.0, 1.0, -1.0])
    add("rod_mirrored_tilted", rod @ G.T, zero, True, -1, dst=((rod * [1.0, 1.0, -1.0]) @ G.T).astype(F32))
    far = np.array([30.0, -25.0, 31.25])
    add("blob_far_shifted", blob, far, True, 1, spin, step)
    add("blob_far_unshifted", blob.astype(F32).astype(np.float64) + far, zero, True, 1,
        dst=cases["blob_far_shifted"]["dst"])
    return cases


PLANE_RADIUS = 0.01
PLANE_COND_CAP = 1e12
PLANE_SPREADS = (1e-2, 1e-3, 1e-4)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _patch(normal, centre, shape, spacing):
    n = _unit(normal)
    e1 = _unit(np.cross(n, [0.0, 1.0, 0.3]))
    e2 = np.cross(n, e1)
    uv = _lattice(shape, spacing)
    return centre + uv[:, :1] * e1 + uv[:, 1:] * e2


def plane_cases():
    """name -> dict(src, dst [m,3] f32, normals [m,3] f64 of dst, regular).  The source is the target moved back by
    a small rigid motion (below half the spacing and below the radius)."""
    rng = np.random.default_rng(3602)
    cases = {}
    back, shift = -GENERIC_AXIS * 0.01, np.array([-5e-4, 3e-4, -1e-3])

    def add(name, dst, normals, regular):
        dst = np.asarray(dst, np.float64).astype(F32)
        cases[name] = dict(src=_moved(dst.astype(np.float64), back, shift), dst=dst,
                           normals=np.ascontiguousarray(normals, np.float64), regular=regular)

    ns = ([0.0, 0.0, 1.0], [0.5, 0.1, 0.8], [-0.2, 0.6, 0.7])
    cs = ([0.0, 0.0, 0.0], [0.12, 0.0, 0.02], [0.0, 0.12, -0.03])
    pts = np.concatenate([_patch(n, np.array(c), (6, 6), 0.012) for n, c in zip(ns, cs)])
    nrm = np.concatenate([np.tile(_unit(n), (36, 1)) for n in ns])
    add("three_patches", pts, nrm, True)
    flat = np.concatenate([_lattice((10, 10), 0.012), np.zeros((100, 1))], axis=1) + [0.02, -0.01, 0.0]
    for spread in PLANE_SPREADS:
        uv = rng.uniform(-1.0, 1.0, (100, 2))
        n = np.concatenate([spread * uv, np.ones((100, 1))], axis=1)
        add("nearly_flat_%g" % spread, flat, n / np.linalg.norm(n, axis=1, keepdims=True), True)
    add("normals_all_z", pts, np.tile([0.0, 0.0, 1.0], (108, 1)), False)
    add("normals_all_tilted", pts, np.tile([0.6, 0.0, 0.8], (108, 1)), False)
    few = dict(cases["three_patches"])
    few["src"] = few["src"].copy()
    few["src"][5:] += F32(1.0)                                       # five correspondences remain
    few["regular"] = False
    cases["five_correspondences"] = few
    return cases


MATCH_RADIUS = 2.0 ** -4
GRID = 2.0 ** -7


def matching_cases():
    """name -> dict(src, dst f32) for the hash grid of the matching at radius 2^-4; T0 = I, so the transformed source
    is the source.  Coordinates are multiples of 2^-7 unless the case says otherwise."""
    rng = np.random.default_rng(3603)
    cases = {}
    r = MATCH_RADIUS
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    # every source has one target, at exactly the radius along +-x, +-y, +-z in turn: none is a correspondence
    src = _lattice((4, 4, 4), 0.5) - 0.25
    cases["exact_radius"] = dict(src=src, dst=src + r * axes[np.arange(64) % 6])
    # at radius (1 - 2^-20), representable because the source's coordinate on that axis is 0: every one is
    src, dst = [], []
    for k in range(48):
        p = np.array([rng.integers(-64, 65), rng.integers(-64, 65), rng.integers(-64, 65)]) * 4.0 * GRID
        ax = axes[k % 6]
        p[np.abs(ax) > 0] = 0.0
        src.append(p)
        dst.append(p + ax * (r * (1.0 - 2.0 ** -20)))
    cases["inside_radius"] = dict(src=np.array(src), dst=np.array(dst))
    # a lattice against itself shifted by half a spacing on every axis: eight equidistant targets per source
    src = _lattice((6, 6, 6), 4 * GRID) - 2 * GRID
    dst = _lattice((7, 7, 7), 4 * GRID) - 2 * GRID
    cases["half_shift"] = dict(src=src, dst=dst[rng.permutation(len(dst))])
    # both sides of zero on every axis, zero itself and +-radius among the coordinates
    vals = np.concatenate([np.arange(-32, 33), [0, 0, 8, -8]]) * GRID
    cases["around_zero"] = dict(src=rng.choice(vals, (200, 3)), dst=rng.choice(vals, (400, 3)))
    # coordinates at the float32 neighbours of the multiples of the cell edge radius (1 + 2^-20) (not dyadic)
    h = r * (1.0 + 2.0 ** -20)
    edge = np.array([F32(k * h) for k in range(-3, 4)], F32)
    vals = np.concatenate([edge, np.nextafter(edge, F32(np.inf)), np.nextafter(edge, F32(-np.inf))]).astype(np.float64)
    cases["cell_edges"] = dict(src=rng.choice(vals, (96, 3)), dst=rng.choice(vals, (192, 3)))
    return {k: dict(src=v["src"].astype(F32), dst=v["dst"].astype(F32)) for k, v in cases.items()}


def tie_cases():
    """One source point, two targets at the same distance on opposite sides along x.  The source's cell is [0, h)
    in x; the target at +x lies in the next cell.  `low_far`: the lower index is the +x one.  `low_near`: the lower
    index is the -x one.  The update's translation is the chosen target minus the source."""
    p = np.array([[6.0, 3.0, -5.0]]) * GRID
    plus, minus = p + [4 * GRID, 0, 0], p - [4 * GRID, 0, 0]
    return {"low_far": dict(src=p.astype(F32), dst=np.concatenate([plus, minus]).astype(F32), expect=[4 * GRID, 0, 0]),
            "low_near": dict(src=p.astype(F32), dst=np.concatenate([minus, plus]).astype(F32), expect=[-4 * GRID, 0, 0])}


def colliding_case():
    """2048 targets in 256 clusters of 8 over +-50 m, sources within the radius of a tenth of them: some 250 occupied
    cells of edge 2^-4 m, metres apart, share the 4096 buckets of the hash, so buckets hold far-apart cells."""
    rng = np.random.default_rng(3604)
    centres = rng.integers(-6400, 6401, (256, 3)) * GRID
    dst = (centres[:, None, :] + rng.integers(-3, 4, (256, 8, 3)) * GRID).reshape(-1, 3)
    pick = rng.permutation(2048)[:205]
    src = dst[pick] + rng.integers(-6, 7, (205, 3)) * GRID
    return dict(src=src.astype(F32), dst=dst.astype(F32))


def huge_case():
    """Coordinates of 2e6 .. 3e8 m (cell coordinates past 2^27 and past the 2^28 clamp).  The first half of the
    sources are targets (distance 0); the second half are targets moved by one float32 step in x (>= 0.125 m)."""
    rng = np.random.default_rng(3605)
    mag = np.exp(rng.uniform(np.log(2e6), np.log(3e8), (256, 3))) * rng.choice([-1.0, 1.0], (256, 3))
    dst = mag.astype(F32)
    src = dst[rng.permutation(256)].copy()
    src[128:, 0] = np.nextafter(src[128:, 0], F32(np.inf))
    return dict(src=src, dst=dst)


def pose_map_inputs():
    """(rot [B,3] f32, nominal angle [B], unit axis [B,3]) for B = 14 axes x 22 angles."""
    pi32, third = float(F32(np.pi)), float(F32(2.0 * np.pi / 3.0))
    u_pi, u_third = float(np.spacing(F32(np.pi))), float(np.spacing(F32(2.0 * np.pi / 3.0)))
    angles = [0.0, 1e-40, 1e-20, 1e-9, 2.0 ** -149, 2.0 ** -126]
    angles += [third + k * u_third for k in (-8, -2, -1, 0, 1, 2, 8)]
    angles += [pi32 - k * u_pi for k in (64, 8, 2, 1)] + [pi32, np.pi + 1e-3, 4.0, 2.0 * np.pi - 1e-3, 7.0]
    axes = [GENERIC_AXIS, [1, 0, 0], [0, 1, 0], [0, 0, 1], _unit([1, 1, 0]), _unit([0, 1, 1]), _unit([1, 1, 1])]
    axes = [np.asarray(a, np.float64) for a in axes] + [-np.asarray(a, np.float64) for a in axes]
    rot = np.array([a * t for a in axes for t in angles]).astype(F32)
    return rot, np.array([t for _ in axes for t in angles]), np.array([a for a in axes for _ in angles])


POSE_SAFE_ANGLE = float(F32(np.pi)) - 64 * float(np.spacing(F32(np.pi)))


def normals_families():
    """name -> dict(support [n,3] f32, radius, queries [k,3] f32 or None (the support), viewpoint or None, and what
    the family must show: `planar` (w0 == 0, n == (0, 0, +-1)), `count` (every query's count), `sign` (n_z exactly)."""
    rng = np.random.default_rng(3606)
    fams = {}

    def add(name, support, radius, queries=None, viewpoint=None, **expect):
        fams[name] = dict(support=np.asarray(support, np.float64).astype(F32), radius=radius,
                          queries=None if queries is None else np.asarray(queries, np.float64).astype(F32),
                          viewpoint=viewpoint, **expect)

    plane = np.concatenate([_lattice((16, 16), 0.125), np.full((256, 1), 0.5)], axis=1)
    add("planar", plane, 0.25, planar=True)
    add("planar_seen_from_above", plane, 0.25, viewpoint=(0.1, -0.2, 2.0), planar=True, sign=1.0)
    add("planar_seen_from_below", plane, 0.25, viewpoint=(0.1, -0.2, -1.0), planar=True, sign=-1.0)
    G = R.rodrigues(GENERIC_AXIS * 0.7)
    add("planar_tilted", plane @ G.T, 0.25)
    line = np.arange(-16, 16)[:, None] * _unit([2.0, 1.0, -2.0]) * 0.05 + [0.3, 0.1, -0.2]
    add("collinear", line, 0.25)
    add("coincident", np.tile([[0.3, -0.7, 1.1]], (64, 1)), 0.25, count=64)
    cube = _lattice((6, 6, 6), 0.125)
    add("isotropic", cube, 0.25)
    add("too_few", _lattice((6, 6, 6), 0.25), 0.25, count=1)
    noisy = plane.copy()
    noisy[:, 2] += rng.standard_normal(256) * 1e-6 * 0.25
    add("nearly_planar", noisy, 0.25)
    far = np.concatenate([_lattice((16, 16), 2.0 ** -7), np.zeros((256, 1))], axis=1) + [1000.0, -1000.0, 1000.0]
    add("far_from_origin", far, 2.0 ** -6, planar=True)
    two = rng.uniform(-0.015, 0.015, (2, 256, 3))
    two[1] += [100.0, 60.0, -80.0]
    add("extent_much_larger_than_r", two.reshape(-1, 3), 0.01)
    add("extent_much_smaller_than_r", rng.uniform(-0.03, 0.03, (200, 3)) + [0.5, 0.5, 0.5], 0.25)
    r = 0.25
    lo, hi = plane.min(axis=0), plane.max(axis=0)
    out = []
    for step in (0.5 * r, 10.0 * r):
        for ax in range(3):
            for side, edge in ((-1.0, lo), (1.0, hi)):
                for a, b in ((0.0, 0.0), (0.3, -0.45), (-0.9375, 0.9375)):    # the centre, inside, a corner
                    q = np.array([a, b, 0.5])
                    q[ax] = edge[ax] + side * step
                    out.append(q)
    add("queries_outside_the_box", plane, r, queries=np.array(out))
    return fams


def packed_edge_sets():
    """Packed support sets with an empty set between two others, a 1-point and a 2-point set: (xyz [M,3] f32,
    offsets [S+1] int32, queries [S,K,3] f32, radius).  Queries: each set's own points, the rest filled with the first
    set's first point (a neighbour only in the first set)."""
    fams = normals_families()
    a, b = fams["planar_tilted"]["support"][:100], fams["isotropic"]["support"]
    sets = [a, np.zeros((0, 3), F32), b, b[:1] + F32(0.01), b[:2] - F32(0.01)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    K = max(len(s) for s in sets)
    queries = np.tile(a[:1], (len(sets), K, 1))
    for s, pts in enumerate(sets):
        queries[s, :len(pts)] = pts
    return np.concatenate(sets).astype(F32), offsets, queries.astype(F32), 0.25


# ---- the cases with their references, computed once --------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def procrustes_table():
    """name -> the case with P = the source at T0 (fp64), (I, J) = the restatement's correspondences at the radius,
    `ref` = procrustes(P[I], Q[J]), the units (u, v), and the fp64 restatement's own errors in those units: `rest_T`
    (None where the maximiser is not unique) and `rest_obj`."""
    def make():
        out = {}
        for name, c in procrustes_cases().items():
            T0 = R.initial_transform(np.zeros(3), c["trans0"])
            P, Q = R.apply(T0, c["src"].astype(np.float64)), c["dst"].astype(np.float64)
            I, J, _ = R.correspondences(P, Q, P2P_RADIUS)
            ref = procrustes(P[I], Q[J])
            u, v = procrustes_units(ref, c["trans0"])
            T = R.compose(R.umeyama(P[I], Q[J]), T0)
            rest_obj, rest_T = objective_error(T, ref, v), (transform_error(T, ref, c["trans0"]) / u if ref["unique"] else None)
            out[name] = dict(c, P=P, Q=Q, I=I, J=J, T0=T0, ref=ref, u=u, v=v, rest_T=rest_T, rest_obj=rest_obj)
        return out
    return _once("procrustes", make)


def objective_error(T, ref, v):
    """|max - tr(R^T Sigma)| in units of v = 2^-53 s1 (in absolute terms where Sigma = 0)."""
    e = abs(float(ref["maximum"] - objective(ref, T[:3, :3])))
    return e / v if v > 0.0 else e


def procrustes_allowance():
    """(units of u allowed in T, units of v allowed in the objective): 16 x the restatement's own largest error over
    the cases, at least 16."""
    tab = procrustes_table().values()
    return (max(16.0, 16.0 * max(c["rest_T"] for c in tab if c["rest_T"] is not None)),
            max(16.0, 16.0 * max(c["rest_obj"] for c in tab)))


def plane_table():
    """name -> the case with its correspondences (I, J) at T0 = I and, for the regular systems, the reference's
    (U, x, cond), the unit 2^-53 cond |x| and `rest` = the fp64 LDL^T restatement's error in U in that unit."""
    def make():
        out = {}
        for name, c in plane_cases().items():
            P, Q = c["src"].astype(np.float64), c["dst"].astype(np.float64)
            I, J, _ = R.correspondences(P, Q, PLANE_RADIUS)
            row = dict(c, P=P, Q=Q, I=I, J=J)
            if c["regular"]:
                U, x, cond = plane_update(P[I], Q[J], c["normals"][J])
                unit = U64 * cond * np.linalg.norm(x)
                rest = PL.plane_update(P[I], Q[J], c["normals"][J])
                row.update(U=U, x=x, cond=cond, unit=unit, rest=np.abs(rest - U).max() / unit)
            out[name] = row
        return out
    return _once("plane", make)


def plane_allowance():
    """K of the bound K 2^-53 cond_2(A) |x_ref|: 16 x the restatement's own largest figure over the regular cases."""
    return 16.0 * max(c["rest"] for c in plane_table().values() if c["regular"])


def normals_reference_of(name):
    """(count, w, C, v0, eps, d) of a family of normals_families(): the reference table and the order-of-sums tolerance."""
    def make():
        f = normals_families()[name]
        eps, d = order_of_sums_eps(f["support"], f["radius"], f["queries"])
        return normals_table(f["support"], f["radius"], f["queries"]) + (eps, d)
    return _once("normals:" + name, make)
