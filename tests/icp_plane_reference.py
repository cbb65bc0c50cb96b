"""NumPy restatement of cloudaae_icp_point_to_plane ("Pose refinement", point to plane): the schedule,
matching, statistics and stopping rule of tests/icp_reference.py with the point-to-plane update -- sums in source
order, the 6x6 system by LDL^T.  Written from the definition only.  `dtype` runs the whole iteration in another
float type (numpy.longdouble: the measure of the float64 run's own rounding)."""
import numpy as np

import icp_reference as R


def _seqsum(a):
    return np.cumsum(a, axis=0)[-1]


def ldl_solve(A, b):
    """x with A x = -b by LDL^T without pivoting; None for a pivot that is not a finite number > 0 or a solution that
    is not finite."""
    dt = A.dtype
    L = np.zeros((6, 6), dt)
    d = np.zeros(6, dt)
    for j in range(6):
        dj = A[j, j]
        for k in range(j):
            dj = dj - (L[j, k] * L[j, k]) * d[k]
        if not (dj > 0.0) or not np.isfinite(dj):
            return None
        d[j] = dj
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v = v - (L[i, k] * L[j, k]) * d[k]
            L[i, j] = v / dj
    x = np.zeros(6, dt)
    for i in range(6):
        v = -b[i]
        for k in range(i):
            v = v - L[i, k] * x[k]
        x[i] = v
    x = x / d
    for i in range(5, -1, -1):
        v = x[i]
        for k in range(i + 1, 6):
            v = v - L[k, i] * x[k]
        x[i] = v
    return x if np.all(np.isfinite(x)) else None


def vector_to_matrix(x):
    """U = [Rz(gamma) Ry(beta) Rx(alpha) | t] for x = (alpha, beta, gamma, t) (open3d's TransformVector6dToMatrix4d,
    as recalled)."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4, dtype=x.dtype)
    U[0, :3] = [cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa]
    U[1, :3] = [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa]
    U[2, :3] = [-sb, cb * sa, cb * ca]
    U[:3, 3] = x[3:]
    return U


def system(p, q, n):
    """A = sum J J^T and b = sum J r over the correspondences (p_i, q_i, n_i), J = [p x n; n], r = (p - q) . n."""
    d = p - q
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    a = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
    J = np.concatenate([a, n], axis=1)
    return _seqsum(J[:, :, None] * J[:, None, :]), _seqsum(J * r[:, None]), r


def plane_update(p, q, n):
    """The update U (4x4), or None (U = I) with fewer than six correspondences or an unsolvable system."""
    if len(p) < 6:
        return None
    A, b, _ = system(p, q, n)
    x = ldl_solve(A, b)
    return None if x is None else vector_to_matrix(x)


def compose(U, T):
    N = np.eye(4, dtype=T.dtype)
    for i in range(3):
        for j in range(4):
            N[i, j] = ((U[i, 0] * T[0, j] + U[i, 1] * T[1, j]) + U[i, 2] * T[2, j]) + U[i, 3] * T[3, j]
    return N


def invert(T):
    """(R^T, -R^T t), the translation as -((R0i t0 + R1i t1) + R2i t2)."""
    N = np.eye(4, dtype=T.dtype)
    for i in range(3):
        N[i, :3] = T[:3, i]
        N[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return N


def icp_round(src, Q, Nq, T, rho, max_iteration, rel_fit, rel_rmse):
    M = len(src)
    P = R.apply(T, src)
    (I, J), fit, rmse = R.statistics(P, Q, rho, M)
    its = 0
    for _ in range(max_iteration):
        U = plane_update(P[I], Q[J], Nq[J]) if len(I) else None
        if U is not None:
            T = compose(U, T)
            P = R.apply(U, P)
        (I, J), f, r = R.statistics(P, Q, rho, M)
        its += 1
        converged = abs(fit - f) < rel_fit and abs(rmse - r) < rel_rmse
        fit, rmse = f, r
        if converged:
            break
    return T, fit, rmse, its


def refine(src, dst, normals, rot, trans, radius=0.01, decay=0.9, rounds=10, max_iteration=30, relative_fitness=1e-6,
           relative_rmse=1e-6, pose_maps_target_to_source=False, dtype=np.float64):
    """One cloud: src [M,>=3], dst [N,>=3] (float32, promoted exactly), normals [N,3] of dst, rot, trans [3].  Returns
    (T [4,4], fitness, rmse, iterations [rounds]).  pose_maps_target_to_source: [rot | trans] and T map dst onto
    src; the iteration runs on the inverse."""
    src = np.asarray(src, dtype)[:, :3]
    dst = np.asarray(dst, dtype)[:, :3]
    Nq = np.asarray(normals, dtype)
    T = R.initial_transform(rot, trans).astype(dtype)
    if pose_maps_target_to_source:
        T = invert(T)
    its = []
    rho = dtype(radius)
    if rounds == 0:
        _, fit, rmse = R.statistics(R.apply(T, src), dst, rho, len(src))
    for _ in range(rounds):
        T, fit, rmse, k = icp_round(src, dst, Nq, T, rho, max_iteration, relative_fitness, relative_rmse)
        its.append(k)
        rho = rho * dtype(decay)
    if pose_maps_target_to_source:
        T = invert(T)
    return T, fit, rmse, np.array(its, np.int32)
