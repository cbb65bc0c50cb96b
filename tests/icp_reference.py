"""Float64 NumPy restatement of the point-to-point ICP schedule of cloudaae_icp_point_to_point ("Pose
refinement"): brute-force correspondences, sums in source order, Umeyama by np.linalg.svd.  A yardstick for the GPU
kernel, written from the definition only."""
import numpy as np


def rodrigues(rot):
    """axangle2mat form: theta = |rot|, axis = rot / theta normalised again; theta = 0 gives I."""
    rx, ry, rz = (float(v) for v in np.asarray(rot, np.float64))
    theta = np.sqrt((rx * rx + ry * ry) + rz * rz)
    if not theta > 0.0:
        return np.eye(3)
    x, y, z = rx / theta, ry / theta, rz / theta
    n = np.sqrt((x * x + y * y) + z * z)
    x, y, z = x / n, y / n, z / n
    c, s = np.cos(theta), np.sin(theta)
    C = 1.0 - c
    xs, ys, zs = x * s, y * s, z * s
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    return np.array([[x * xC + c, xyC - zs, zxC + ys],
                     [xyC + zs, y * yC + c, yzC - xs],
                     [zxC - ys, yzC + xs, z * zC + c]])


def initial_transform(rot, trans):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rot)
    T[:3, 3] = np.asarray(trans, np.float64)
    return T


def apply(T, X):
    """p = ((T00 x + T01 y) + T02 z) + T03, row by row (NumPy evaluates left to right and does not fuse)."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)


def correspondences(P, Q, rho):
    """(i, j*, d2) for every source point with a target closer than rho; ties to the smallest j."""
    rho2 = rho * rho
    I, J, D = [], [], []
    for s in range(0, len(P), 512):
        p = P[s:s + 512]
        dx = p[:, 0:1] - Q[None, :, 0]
        dy = p[:, 1:2] - Q[None, :, 1]
        dz = p[:, 2:3] - Q[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = np.where(d2 < rho2, d2, np.inf)
        j = np.argmin(d2, axis=1)                    # first minimum: the smallest j
        best = d2[np.arange(len(p)), j]
        ok = np.isfinite(best)
        I.append(np.nonzero(ok)[0] + s)
        J.append(j[ok])
        D.append(best[ok])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def _seqsum(a, axis=0):
    return np.cumsum(a, axis=axis)[-1] if len(a) else np.zeros(a.shape[1:])


def statistics(P, Q, rho, M):
    I, J, D = correspondences(P, Q, rho)
    n = len(I)
    return (I, J), n / M, (np.sqrt(_seqsum(D) / n) if n else 0.0)


def umeyama(p, q):
    """The rigid transform (4x4) that maps p onto q in the least-squares sense; I for no points."""
    U4 = np.eye(4)
    n = len(p)
    if n == 0:
        return U4
    mp, mq = _seqsum(p) / n, _seqsum(q) / n
    dp, dq = p - mp, q - mq
    sigma = _seqsum(dq[:, :, None] * dp[:, None, :]) / n
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    U4[:3, :3] = R
    U4[:3, 3] = mq - R @ mp
    return U4


def compose(U, T):
    """U T with the sums in k order: ((U_i0 T_0j + U_i1 T_1j) + U_i2 T_2j) + U_i3 T_3j."""
    N = np.eye(4)
    for i in range(3):
        for j in range(4):
            N[i, j] = ((U[i, 0] * T[0, j] + U[i, 1] * T[1, j]) + U[i, 2] * T[2, j]) + U[i, 3] * T[3, j]
    return N


def icp_round(src, Q, T, rho, max_iteration, rel_fit, rel_rmse):
    """open3d registration_icp (point to point): returns (T, fitness, rmse, updates performed)."""
    M = len(src)
    P = apply(T, src)
    (I, J), fit, rmse = statistics(P, Q, rho, M)
    its = 0
    for _ in range(max_iteration):
        if len(I):                 # an empty set gives U = I: T and P are left as they are
            U = umeyama(P[I], Q[J])
            T = compose(U, T)
            P = apply(U, P)
        (I, J), f, r = statistics(P, Q, rho, M)
        its += 1
        converged = abs(fit - f) < rel_fit and abs(rmse - r) < rel_rmse
        fit, rmse = f, r
        if converged:
            break
    return T, fit, rmse, its


def refine(src, dst, rot, trans, radius=0.01, decay=0.9, rounds=10, max_iteration=30, relative_fitness=1e-6,
           relative_rmse=1e-6):
    """One cloud: src [M,>=3], dst [N,>=3] (float32, promoted exactly), rot, trans [3].  Returns
    (T [4,4], fitness, rmse, iterations [rounds])."""
    src = np.asarray(src, np.float64)[:, :3]
    dst = np.asarray(dst, np.float64)[:, :3]
    T = initial_transform(rot, trans)
    its = []
    if rounds == 0:
        _, fit, rmse = statistics(apply(T, src), dst, radius, len(src))
        return T, fit, rmse, np.zeros(0, np.int32)
    rho = radius
    fit = rmse = 0.0
    for _ in range(rounds):
        T, fit, rmse, k = icp_round(src, dst, T, rho, max_iteration, relative_fitness, relative_rmse)
        its.append(k)
        rho = rho * decay
    return T, fit, rmse, np.array(its, np.int32)


def scene(model_xyz, rot_true, trans_true, n, noise, rng, perturb_deg, perturb_m):
    """A synthetic observation of the model: the posed model cut by a half-space (the side facing a random direction,
    to mimic visibility), n of those points (float32) with Gaussian noise of `noise` m, and an initial pose perturbed
    by perturb_deg degrees and perturb_m metres.  Returns (scene [n,3] f32, rot0 [3] f32, trans0 [3] f32)."""
    R = rodrigues(rot_true)
    posed = model_xyz.astype(np.float64) @ R.T + np.asarray(trans_true, np.float64)
    if n < len(posed):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        order = np.argsort(-(posed - posed.mean(axis=0)) @ d, kind="stable")
        pts = posed[np.sort(order[:n])]
    else:
        pts = posed
    pts = pts + rng.standard_normal(pts.shape) * noise
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    dR = rodrigues(axis * np.deg2rad(perturb_deg))
    R0 = dR @ R
    rot0 = log_map(R0)
    tdir = rng.standard_normal(3)
    tdir /= np.linalg.norm(tdir)
    trans0 = np.asarray(trans_true, np.float64) + tdir * perturb_m
    return pts.astype(np.float32), rot0.astype(np.float32), trans0.astype(np.float32)


def log_map(R):
    """Axis-angle of a rotation matrix (angle in [0, pi]), for building test poses."""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    theta = np.arctan2(np.linalg.norm(v), np.trace(R) - 1.0)
    if np.linalg.norm(v) > 1e-12 and theta < 3.0:
        return v / np.linalg.norm(v) * theta
    w, V = np.linalg.eigh((R + R.T) / 2)
    a = V[:, np.argmax(w)]
    if a @ v < 0:
        a = -a
    return a * theta
