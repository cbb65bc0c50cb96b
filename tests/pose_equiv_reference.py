"""NumPy restatement of DESIGN.md "Equivalent poses": the yardstick for cloudaae_nearest_equivalent_pose
(csrc/pose_equiv.hip) and utils/pose_equiv.py.  Every product and sum is written in the definition's order, in one
floating-point type throughout (float64: the definition; numpy.longdouble: the run the tolerances are measured against);
the arrays are batched over the samples, which changes no operation of a sample.

A class is a dict: kind 'none'; or kind 'finite' with rot [n,3,3] (the identity first) and centre [3]; or kind 'axial' with
axis [3] (unit), flip (a [3,3] half-turn about a line perpendicular to the axis, or None) and centre [3].
"""
import itertools
import math

import numpy as np

NONE, FINITE, AXIAL = 0, 1, 2
MAX_MEMBERS = 64
CLAMP = 0.9999999


# ---- the two maps --------------------------------------------------------------------------------------------------------
def exp_map(ax):
    """[b,3] -> [b,3,3]: exponential_map of losses/angular_distance_taylor.py (exp_map of csrc/so3_dual.h), EPS = 1e-2."""
    ax = np.asarray(ax)
    ty = ax.dtype.type
    x, y, z = ax[:, 0], ax[:, 1], ax[:, 2]
    zero = np.zeros_like(x)
    ss = [[zero, -z, y], [z, zero, -x], [-y, x, zero]]
    tsq = (x * x + y * y) + z * z
    p4, p6, p8 = tsq * tsq, (tsq * tsq) * tsq, ((tsq * tsq) * tsq) * tsq
    t1s = (((ty(1.0) - (tsq / ty(6.0))) + (p4 / ty(120.0))) - (p6 / ty(5040.0))) + (p8 / ty(362880.0))
    t2s = (((ty(0.5) - (tsq / ty(24.0))) + (p4 / ty(720.0))) - (p6 / ty(40320.0))) + (p8 / ty(3628800.0))
    small = tsq < 1e-2
    safe = np.where(small, ty(1.0), tsq)
    th = np.sqrt(safe)
    t1 = np.where(small, t1s, np.sin(th) / th)
    t2 = np.where(small, t2s, (ty(1.0) - np.cos(th)) / safe)
    R = np.empty((len(ax), 3, 3), ax.dtype)
    for i in range(3):
        for j in range(3):
            sq = zero
            for k in range(3):
                sq = sq + ss[i][k] * ss[k][j]
            R[:, i, j] = (ty(1.0 if i == j else 0.0) + t1 * ss[i][j]) + t2 * sq
    return R


def log_map(R):
    """[b,3,3] -> [b,3]: the axis-angle of "Pose refinement" (icp_log_map of csrc/pose_math.h): theta = atan2(|v|, tr - 1);
    the axis is v / |v| while cos > -0.5, else the largest column of the symmetric part, signed to agree with v."""
    R = np.asarray(R)
    ty = R.dtype.type
    vx, vy, vz = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    tr1 = ((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - ty(1.0)
    vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
    theta = np.arctan2(vn, tr1)
    f = np.where(vn > 0.0, theta / np.where(vn > 0.0, vn, ty(1.0)), ty(0.5))
    plain = np.stack([vx * f, vy * f, vz * f], axis=1)
    cs = ty(0.5) * tr1
    b01, b02, b12 = ty(0.5) * (R[:, 0, 1] + R[:, 1, 0]), ty(0.5) * (R[:, 0, 2] + R[:, 2, 0]), ty(0.5) * (R[:, 1, 2] + R[:, 2, 1])
    b00, b11, b22 = R[:, 0, 0] - cs, R[:, 1, 1] - cs, R[:, 2, 2] - cs
    col1 = (b11 > b00) & (b11 >= b22)
    col2 = ~col1 & (b22 > b00) & (b22 > b11)
    ax = np.where(col1, b01, np.where(col2, b02, b00))
    ay = np.where(col1, b11, np.where(col2, b12, b01))
    az = np.where(col1, b12, np.where(col2, b22, b02))
    an = np.sqrt((ax * ax + ay * ay) + az * az)
    ok = an > 0.0
    an = np.where(ok, an, ty(1.0))
    ax, ay, az = np.where(ok, ax / an, ty(1.0)), np.where(ok, ay / an, ty(0.0)), np.where(ok, az / an, ty(0.0))
    sign = np.where((ax * vx + ay * vy) + az * vz < 0.0, ty(-1.0), ty(1.0))
    near_pi = np.stack([(sign * ax) * theta, (sign * ay) * theta, (sign * az) * theta], axis=1)
    return np.where((tr1 > -1.0)[:, None], plain, near_pi)


def matmul(A, B):
    """C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], batched with broadcasting."""
    A, B = np.asarray(A), np.asarray(B)
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def matvec(A, v):
    return (A[..., :, 0] * v[..., None, 0] + A[..., :, 1] * v[..., None, 1]) + A[..., :, 2] * v[..., None, 2]


def trace(A):
    return (A[..., 0, 0] + A[..., 1, 1]) + A[..., 2, 2]


def skew(a):
    z = np.zeros((), a.dtype)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], a.dtype)


# ---- the definition --------------------------------------------------------------------------------------------------------
def nearest_equivalent_pose(rot_pred, rot_label, trans_label, class_id, classes, dtype=np.float64):
    """The definition on b samples; classes: the list of class dicts (a class_id outside it is 'none').
    -> dict: rot_equiv [b,3], trans_equiv [b,3] (in `dtype`; trans_equiv32 is its float32 rounding), member [b] int32, phi,
    angle, cos (the clamped cosine angle is the acos of) [b]; and for the tests S [b,3,3] (S*), Rl, Rp [b,3,3], gap [b] (best
    minus second-best s_j of a finite class or of the two cosets, +inf elsewhere) and axial_value [b] (sqrt((tau - alpha)^2 + beta^2) of the
    chosen coset, +inf elsewhere)."""
    ty = np.dtype(dtype).type
    b = len(rot_pred)
    Rp = exp_map(np.asarray(rot_pred).astype(dtype))
    Rl = exp_map(np.asarray(rot_label, np.float64).astype(dtype))
    tl = np.asarray(trans_label, np.float32).astype(dtype)
    M = np.empty((b, 3, 3), dtype)
    for i in range(3):
        for k in range(3):
            M[:, i, k] = (Rp[:, 0, i] * Rl[:, 0, k] + Rp[:, 1, i] * Rl[:, 1, k]) + Rp[:, 2, i] * Rl[:, 2, k]
    cid = np.asarray(class_id, np.int64)
    member = np.zeros(b, np.int32)
    phi = np.zeros(b, dtype)
    s_star = trace(M)
    S = np.tile(np.eye(3, dtype=dtype), (b, 1, 1))
    rot_equiv = np.asarray(rot_label, np.float64).astype(dtype).copy()
    trans_equiv = tl.copy()
    gap = np.full(b, np.inf)
    axial_value = np.full(b, np.inf)
    for c, spec in enumerate(classes):
        sel = np.flatnonzero(cid == c)
        if spec["kind"] == "none" or len(sel) == 0:
            continue
        Mc = M[sel]
        centre = np.asarray(spec["centre"], np.float64).astype(dtype)
        if spec["kind"] == "finite":
            G = np.asarray(spec["rot"], np.float64).astype(dtype)
            assert 1 <= len(G) <= MAX_MEMBERS
            s = np.empty((len(sel), len(G)), dtype)
            for j in range(len(G)):
                t = [(Mc[:, i, 0] * G[j, 0, i] + Mc[:, i, 1] * G[j, 1, i]) + Mc[:, i, 2] * G[j, 2, i] for i in range(3)]
                s[:, j] = (t[0] + t[1]) + t[2]
            best = np.argmax(s, axis=1)                       # the first of equals
            s_star[sel] = s[np.arange(len(sel)), best]
            if len(G) > 1:
                rest = s.copy()
                rest[np.arange(len(sel)), best] = -np.inf
                gap[sel] = (s_star[sel] - rest.max(axis=1)).astype(np.float64)
            member[sel] = best
            S[sel] = G[best]
        else:
            a = np.asarray(spec["axis"], np.float64).astype(dtype)
            cosets = [None] if spec.get("flip") is None else [None, np.asarray(spec["flip"], np.float64).astype(dtype)]
            s = np.full((len(sel), len(cosets)), -np.inf, dtype)
            ph = np.zeros((len(sel), len(cosets)), dtype)
            root = np.zeros((len(sel), len(cosets)), dtype)
            for e, E in enumerate(cosets):
                N = Mc if E is None else matmul(Mc, E)
                u = matvec(N, a)
                alpha = (a[0] * u[:, 0] + a[1] * u[:, 1]) + a[2] * u[:, 2]
                tau = trace(N)
                beta = (a[0] * (N[:, 1, 2] - N[:, 2, 1]) + a[1] * (N[:, 2, 0] - N[:, 0, 2])) + a[2] * (N[:, 0, 1] - N[:, 1, 0])
                d = tau - alpha
                root[:, e] = np.sqrt(d * d + beta * beta)
                s[:, e] = alpha + root[:, e]
                ph[:, e] = np.where((d == 0.0) & (beta == 0.0), ty(0.0), np.arctan2(beta, d))
            best = np.argmax(s, axis=1)
            rows = np.arange(len(sel))
            s_star[sel] = s[rows, best]
            if len(cosets) == 2:
                gap[sel] = np.abs(s[:, 0] - s[:, 1]).astype(np.float64)
            member[sel] = best
            phi[sel] = ph[rows, best]
            axial_value[sel] = root[rows, best].astype(np.float64)
            K = skew(a)
            K2 = matmul(K, K)
            sn, vs = np.sin(phi[sel]), ty(1.0) - np.cos(phi[sel])
            R = (np.eye(3, dtype=dtype)[None] + sn[:, None, None] * K[None]) + vs[:, None, None] * K2[None]
            if len(cosets) == 2:
                R = np.where((best == 1)[:, None, None], matmul(cosets[1][None], R), R)
            S[sel] = R
        moved = sel[(S[sel] != np.eye(3, dtype=dtype)[None]).any(axis=(1, 2))]        # S* = I exactly keeps the label's bits
        Q = matmul(Rl[moved], S[moved])
        rot_equiv[moved] = log_map(Q)
        w = centre[None] - matvec(S[moved], centre[None])
        trans_equiv[moved] = tl[moved] + matvec(Rl[moved], w)
    cos = np.minimum(np.maximum((s_star - ty(1.0)) / ty(2.0), ty(-CLAMP)), ty(CLAMP))
    return dict(rot_equiv=rot_equiv, trans_equiv=trans_equiv, trans_equiv32=trans_equiv.astype(np.float32), member=member,
                phi=phi, angle=np.arccos(cos), cos=cos, S=S, Rl=Rl, Rp=Rp, gap=gap, axial_value=axial_value)


def table_arrays(classes):
    """The class dicts as cloudaae_nearest_equivalent_pose reads them: index [C,3] int32 (kind, first, count), centre
    [C,3], axis [C,3], rot [R,3,3] float64."""
    index = np.zeros((len(classes), 3), np.int32)
    centre = np.zeros((len(classes), 3))
    axis = np.zeros((len(classes), 3))
    rot = []
    for c, spec in enumerate(classes):
        if spec["kind"] == "none":
            continue
        centre[c] = spec["centre"]
        if spec["kind"] == "finite":
            index[c] = (FINITE, len(rot), len(spec["rot"]))
            rot.extend(np.asarray(spec["rot"], np.float64))
        else:
            axis[c] = spec["axis"]
            flips = 0 if spec.get("flip") is None else 1
            index[c] = (AXIAL, len(rot), flips)
            if flips:
                rot.append(np.asarray(spec["flip"], np.float64))
    return index, centre, axis, np.asarray(rot, np.float64).reshape(-1, 3, 3)


# ---- rotations and the test groups -----------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis` (normalised here), float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt(a @ a)
    K = skew(a)
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def project(R):
    """The rotation nearest R (SVD)."""
    u, _, vt = np.linalg.svd(R)
    if np.linalg.det(u @ vt) < 0.0:
        u[:, 2] = -u[:, 2]
    return u @ vt


def closure(generators, limit=120):
    """The finite group generated by the rotations given, the identity first."""
    members = [np.eye(3)]
    frontier = [np.eye(3)]
    while frontier:
        nxt = []
        for m in frontier:
            for g in generators:
                p = project(m @ g)
                if min(float(np.abs(p - q).max()) for q in members) > 1e-9:
                    members.append(p)
                    nxt.append(p)
                    assert len(members) <= limit, "not a finite group"
        frontier = nxt
    return np.stack(members)


def trivial_group():
    return np.eye(3)[None].copy()


def cyclic_group(axis, n):
    return np.stack([np.eye(3) if k == 0 else rotation(axis, 2.0 * math.pi * k / n) for k in range(n)])


def cube_group():
    """The 24 rotations of the cube: the signed permutation matrices of determinant +1 (exact), the identity first."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0.0:
                out.append(R)
    out.sort(key=lambda R: not np.array_equal(R, np.eye(3)))
    assert len(out) == 24 and np.array_equal(out[0], np.eye(3))
    return np.stack(out)


def icosahedral_group():
    """The 60 rotations of the icosahedron with vertices (0, +-1, +-g), cyclic: a five-fold turn about a vertex and a
    three-fold turn about a face centre generate them."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    G = closure([rotation([0.0, 1.0, g], 2.0 * math.pi / 5.0), rotation([1.0, 1.0, 1.0], 2.0 * math.pi / 3.0)])
    assert len(G) == 60
    return G


def duplicate_group():
    """Four members of C4 about z with member 1 repeated as member 3: an exact tie whenever the quarter turn is nearest."""
    q = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return np.stack([np.eye(3), q, q @ q, q])


TILTED_AXIS = np.array([0.36, -0.48, 0.8])          # a unit vector, exactly in decimals


def example_classes():
    """The classes of the tests, in a fixed order: none; the trivial group; C2; the cube's 24; the icosahedral 60; C64 about
    a tilted axis; the set with a duplicate; axial without and with a flip.  The centres are not zero from C2 on."""
    a = TILTED_AXIS / np.sqrt(TILTED_AXIS @ TILTED_AXIS)
    a = a / np.sqrt(a @ a)
    f = np.cross(a, [0.0, 0.0, 1.0])
    f = f / np.sqrt(f @ f)
    centre = np.array([0.01, -0.02, 0.015])
    return [dict(kind="none"),
            dict(kind="finite", rot=trivial_group(), centre=np.zeros(3)),
            dict(kind="finite", rot=cyclic_group([1.0, 2.0, -1.0], 2), centre=centre),
            dict(kind="finite", rot=cube_group(), centre=centre),
            dict(kind="finite", rot=icosahedral_group(), centre=-centre),
            dict(kind="finite", rot=cyclic_group(TILTED_AXIS, 64), centre=centre),
            dict(kind="finite", rot=duplicate_group(), centre=centre),
            dict(kind="axial", axis=a, flip=None, centre=centre),
            dict(kind="axial", axis=a, flip=2.0 * np.outer(f, f) - np.eye(3), centre=2.0 * centre)]


CLASS_NAMES = ("none", "trivial", "c2", "cube", "icosahedral", "c64", "duplicate", "axial", "axial_flip")


def random_axis_angles(rng, n, max_angle=math.pi):
    """[n,3] float64 axis-angles, uniform axes, angles uniform in [0, max_angle)."""
    v = rng.standard_normal((n, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return v * rng.uniform(0.0, max_angle, (n, 1))


def random_rotations(rng, n):
    """[n,3,3] rotations uniform over SO(3) (unit quaternions), and their axis-angles [n,3]."""
    q = rng.standard_normal((n, 4))
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    w = q[:, 0]
    v = q[:, 1:]
    vn = np.sqrt((v * v).sum(axis=1))
    theta = 2.0 * np.arctan2(vn, w)
    theta = np.where(theta > math.pi, theta - 2.0 * math.pi, theta)
    ax = v / vn[:, None] * theta[:, None]
    return exp_map(ax), ax


def geodesic(Ra, Rb):
    """The angle of Ra^T Rb, batched, by plain float64 matrix products."""
    tr = np.einsum("...ij,...ij->...", Ra, Rb)
    return np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))
