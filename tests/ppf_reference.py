"""NumPy restatement of DESIGN.md "Pose proposals": the point-pair feature and its key, the local frame Q(n), the model
pair table and its direct-address CSR, the voting of a scene's pairs, the peaks and their poses, and the greedy
clustering.  Written from the definition, not from the kernels.  float64 on float32 points with + - * / sqrt only; NumPy
evaluates every expression below elementwise in the written order and never fuses a product with a sum, so integers are
compared for equality and poses bit for bit."""
import numpy as np


def tables(n_angle=15, n_alpha=30):
    """(cos_edges [n_angle-1], alpha_edges [n_alpha/2-1], alpha_cs [n_alpha,2]): the host-made tables."""
    assert n_alpha % 2 == 0
    half = n_alpha // 2
    cos_edges = np.cos(np.arange(1, n_angle, dtype=np.float64) * (np.pi / n_angle))
    alpha_edges = np.cos(np.arange(1, half, dtype=np.float64) * (np.pi / half))
    centres = -np.pi + (np.arange(n_alpha, dtype=np.float64) + 0.5) * (2.0 * np.pi / n_alpha)
    return cos_edges, alpha_edges, np.stack([np.cos(centres), np.sin(centres)], axis=1)


def angle_bin(c, edges):
    """How many of the descending edge cosines c does not exceed."""
    return (np.asarray(c, np.float64)[..., None] <= np.asarray(edges, np.float64)).sum(axis=-1).astype(np.int64)


def frame(n):
    """Q(n) [...,3,3]: the rotation that takes the unit vector n [...,3] onto +x."""
    n = np.asarray(n, np.float64)
    n0, n1, n2 = n[..., 0], n[..., 1], n[..., 2]
    pos = n0 >= 0.0
    h = np.where(pos, 1.0 + n0, 1.0 - n0)
    a = (n1 * n2) / h
    b1 = 1.0 - (n1 * n1) / h
    b2 = 1.0 - (n2 * n2) / h
    Q = np.zeros(n.shape[:-1] + (3, 3), np.float64)
    Q[..., 0, :] = n
    Q[..., 1, 0] = -n1
    Q[..., 1, 1] = np.where(pos, b1, -b1)
    Q[..., 1, 2] = np.where(pos, -a, a)
    Q[..., 2, 0] = np.where(pos, -n2, n2)
    Q[..., 2, 1] = -a
    Q[..., 2, 2] = b2
    return Q


def pair_key(p1, n1, p2, n2, dist_step, n_dist, n_angle, cos_edges):
    """-> (key, d): key -1 where the pair has none.  Arrays broadcast over their leading axes."""
    p1, p2 = np.asarray(p1, np.float32).astype(np.float64), np.asarray(p2, np.float32).astype(np.float64)
    n1, n2 = np.asarray(n1, np.float64), np.asarray(n2, np.float64)
    d = p2 - p1
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    length = np.sqrt((dx * dx + dy * dy) + dz * dz)
    with np.errstate(all="ignore"):
        t = length / dist_step
        ok = (length > 0.0) & (t >= 0.0) & (t < float(n_dist))
        qd = np.where(ok, t, 0.0).astype(np.int64)
        c1 = ((n1[..., 0] * dx + n1[..., 1] * dy) + n1[..., 2] * dz) / length
        c2 = ((n2[..., 0] * dx + n2[..., 1] * dy) + n2[..., 2] * dz) / length
    c3 = (n1[..., 0] * n2[..., 0] + n1[..., 1] * n2[..., 1]) + n1[..., 2] * n2[..., 2]
    q1, q2, q3 = angle_bin(c1, cos_edges), angle_bin(c2, cos_edges), angle_bin(c3, cos_edges)
    key = ((qd * n_angle + q1) * n_angle + q2) * n_angle + q3
    return np.where(ok, key, -1), d


def direction(Q, d):
    """-> (ok, uy, uz): the unit (y, z) part of Q d."""
    y = (Q[..., 1, 0] * d[..., 0] + Q[..., 1, 1] * d[..., 1]) + Q[..., 1, 2] * d[..., 2]
    z = (Q[..., 2, 0] * d[..., 0] + Q[..., 2, 1] * d[..., 1]) + Q[..., 2, 2] * d[..., 2]
    r = np.sqrt(y * y + z * z)
    ok = r > 0.0
    with np.errstate(all="ignore"):
        return ok, np.where(ok, y / r, 0.0), np.where(ok, z / r, 0.0)


def model_pairs(xyz, normals, dist_step, n_dist, n_angle, cos_edges):
    """One set: xyz [M,3] float32, normals [M,3] -> key [M,M] int32 (-1: skipped), ref [M,M] int32, dir [M,M,2] float32;
    row r, column i is the ordered pair (r, i)."""
    xyz, normals = np.asarray(xyz, np.float32), np.asarray(normals, np.float64)
    M = len(xyz)
    key, d = pair_key(xyz[:, None], normals[:, None], xyz[None], normals[None], dist_step, n_dist, n_angle, cos_edges)
    ok, uy, uz = direction(frame(normals)[:, None], d)
    good = (key >= 0) & ok & ~np.eye(M, dtype=bool)
    key = np.where(good, key, -1).astype(np.int32)
    dirs = np.stack([np.where(good, uy, 0.0), np.where(good, uz, 0.0)], axis=-1).astype(np.float32)
    return key, np.repeat(np.arange(M, dtype=np.int32)[:, None], M, axis=1), dirs


def build_csr(pairs, n_key):
    """pairs: [(key, ref, dir)] per set -> (bucket_start [S,n_key+1] int32 of absolute entry indices, entry_ref [E] int32,
    entry_dir [E,2] float32): the kept entries ordered by (set, key), equal keys in pair order (r, then i)."""
    starts, refs, dirs, total = [], [], [], 0
    for key, ref, d in pairs:
        k, r, d = key.reshape(-1), ref.reshape(-1), d.reshape(-1, 2)
        keep = k >= 0
        order = np.argsort(k[keep], kind="stable")
        refs.append(r[keep][order])
        dirs.append(d[keep][order])
        count = np.bincount(k[keep], minlength=n_key)
        starts.append(total + np.concatenate([[0], np.cumsum(count)]))
        total += int(keep.sum())
    return (np.stack(starts).astype(np.int32), np.concatenate(refs).astype(np.int32),
            np.concatenate(dirs).astype(np.float32).reshape(-1, 2))


def peak_pose(p_ref, n_ref, p_model, n_model, ca, sa):
    """T_s^-1 Rx T_m, [4,4]."""
    Qs, Qm = frame(n_ref), frame(n_model)
    pr = np.asarray(p_ref, np.float32).astype(np.float64)
    pm = np.asarray(p_model, np.float32).astype(np.float64)
    A = np.zeros((3, 3))
    for k in range(3):
        A[0, k] = Qm[0, k]
        A[1, k] = ca * Qm[1, k] - sa * Qm[2, k]
        A[2, k] = sa * Qm[1, k] + ca * Qm[2, k]
    T = np.eye(4)
    for i in range(3):
        for k in range(3):
            T[i, k] = (Qs[0, i] * A[0, k] + Qs[1, i] * A[1, k]) + Qs[2, i] * A[2, k]
        T[i, 3] = pr[i] - ((T[i, 0] * pm[0] + T[i, 1] * pm[1]) + T[i, 2] * pm[2])
    return T


def vote(scene, normals, mask, class_id, model, ref_step=5, peaks=2):
    """scene [B,N,3] float32, normals [B,N,3], mask [B,N], class_id [B]; model: dict(offsets [S+1], xyz [Mt,3], normals
    [Mt,3], dist_step [S], n_dist, n_angle, n_alpha, cos_edges, alpha_edges, alpha_cs, bucket_start [S,n_key+1], entry_ref,
    entry_dir, m_max) -> dict(acc [B,R,m_max,n_alpha], votes, model_index, bin [B,R,peaks] int32, pose [B,R,peaks,4,4])."""
    scene, normals = np.asarray(scene, np.float32), np.asarray(normals, np.float64)
    mask = np.asarray(mask) != 0
    B, N = mask.shape
    R = -(-N // ref_step)
    off = np.asarray(model["offsets"], np.int64)
    S, n_alpha, m_max = len(off) - 1, int(model["n_alpha"]), int(model["m_max"])
    half = n_alpha // 2
    E = len(model["entry_ref"])
    acc = np.zeros((B, R, m_max, n_alpha), np.int32)
    votes = np.zeros((B, R, peaks), np.int32)
    mi = np.full((B, R, peaks), -1, np.int32)
    bn = np.full((B, R, peaks), -1, np.int32)
    pose = np.tile(np.eye(4), (B, R, peaks, 1, 1))
    for b in range(B):
        c = int(class_id[b])
        usable = np.nonzero(mask[b])[0]
        M = 0
        if 0 <= c < S:
            first, last = int(off[c]), int(off[c + 1])
            M = last - first
            if first < 0 or last > len(model["xyz"]) or M < 1 or M > m_max:
                M = 0
        for j in range(R):
            if M == 0 or j * ref_step >= len(usable):
                continue
            ref = int(usable[j * ref_step])
            others = usable[usable != ref]
            key, d = pair_key(scene[b, ref], normals[b, ref], scene[b, others], normals[b, others], model["dist_step"][c],
                              model["n_dist"], model["n_angle"], model["cos_edges"])
            ok, uy, uz = direction(frame(normals[b, ref]), d)
            a = acc[b, j].reshape(-1)
            for k, y, z in zip(key[(key >= 0) & ok], uy[(key >= 0) & ok], uz[(key >= 0) & ok]):
                lo, hi = max(int(model["bucket_start"][c, k]), 0), min(int(model["bucket_start"][c, k + 1]), E)
                if hi <= lo:
                    continue
                rm = model["entry_ref"][lo:hi].astype(np.int64)
                w = model["entry_dir"][lo:hi].astype(np.float64)
                ca = y * w[:, 0] + z * w[:, 1]
                sa = z * w[:, 0] - y * w[:, 1]
                q = angle_bin(ca, model["alpha_edges"])
                cell = rm * n_alpha + np.where(sa >= 0.0, half + q, half - 1 - q)
                np.add.at(a, cell[(rm >= 0) & (rm < M)], 1)
            order = np.lexsort((np.arange(len(a)), -a.astype(np.int64)))[:peaks]      # votes descending, cell ascending
            for k, cell in enumerate(order):
                if a[cell] <= 0:
                    continue
                votes[b, j, k], mi[b, j, k], bn[b, j, k] = a[cell], cell // n_alpha, cell % n_alpha
                g = first + int(mi[b, j, k])
                pose[b, j, k] = peak_pose(scene[b, ref], normals[b, ref], model["xyz"][g], model["normals"][g],
                                          model["alpha_cs"][bn[b, j, k], 0], model["alpha_cs"][bn[b, j, k], 1])
    return dict(acc=acc, votes=votes, model_index=mi, bin=bn, pose=pose)


def close(Ta, Tb, trans_thresh2, rot_bound):
    d = Ta[:3, 3] - Tb[:3, 3]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    r = [(Ta[i, 0] * Tb[i, 0] + Ta[i, 1] * Tb[i, 1]) + Ta[i, 2] * Tb[i, 2] for i in range(3)]
    return bool(d2 <= trans_thresh2 and (r[0] + r[1]) + r[2] >= rot_bound)


def cluster(votes, pose, class_id, trans_thresh2, rot_bound, top):
    """votes [B,C], pose [B,C,4,4], trans_thresh2 [S] -> dict(pose [B,top,4,4], trans [B,top,3] float32, score, valid
    [B,top] int32, members: per sample the list of (representative, [member indices]))."""
    votes, pose = np.asarray(votes), np.asarray(pose, np.float64)
    B, C = votes.shape
    out = np.tile(np.eye(4), (B, top, 1, 1))
    score, valid, members = np.zeros((B, top), np.int32), np.zeros((B, top), np.int32), []
    for b in range(B):
        c = int(class_id[b])
        reps, sums, mem = [], [], []
        if 0 <= c < len(trans_thresh2):
            for i in np.lexsort((np.arange(C), -votes[b].astype(np.int64))):
                if votes[b, i] <= 0:
                    break
                for k, r in enumerate(reps):
                    if close(pose[b, r], pose[b, i], trans_thresh2[c], rot_bound):
                        sums[k] += int(votes[b, i])
                        mem[k].append(int(i))
                        break
                else:
                    reps.append(int(i))
                    sums.append(int(votes[b, i]))
                    mem.append([int(i)])
        order = np.lexsort((np.arange(len(reps)), -np.asarray(sums, np.int64)))[:top] if reps else []
        for t, k in enumerate(order):
            out[b, t], score[b, t], valid[b, t] = pose[b, reps[k]], sums[k], 1
        members.append([(reps[k], mem[k]) for k in order])
    return dict(pose=out, trans=out[:, :, :3, 3].astype(np.float32), score=score, valid=valid, members=members)


def make_model(sets, diameters, n_angle=15, n_alpha=30, n_dist=20, dist_fraction=0.05):
    """sets: [(xyz [M,3] float32, normals [M,3])] -> the model dict vote() takes, with the pairs kept under 'pairs'."""
    cos_edges, alpha_edges, alpha_cs = tables(n_angle, n_alpha)
    dist_step = dist_fraction * np.asarray(diameters, np.float64)
    pairs = [model_pairs(x, n, dist_step[i], n_dist, n_angle, cos_edges) for i, (x, n) in enumerate(sets)]
    bucket_start, entry_ref, entry_dir = build_csr(pairs, n_dist * n_angle ** 3)
    sizes = [len(x) for x, _ in sets]
    return dict(offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
                xyz=np.concatenate([np.asarray(x, np.float32) for x, _ in sets]),
                normals=np.concatenate([np.asarray(n, np.float64) for _, n in sets]), dist_step=dist_step, n_dist=n_dist,
                n_angle=n_angle, n_alpha=n_alpha, cos_edges=cos_edges, alpha_edges=alpha_edges, alpha_cs=alpha_cs,
                bucket_start=bucket_start, entry_ref=entry_ref, entry_dir=entry_dir, m_max=max(sizes), pairs=pairs,
                diameters=np.asarray(diameters, np.float64))


def thresholds(diameters, n_alpha=30, trans_fraction=0.1):
    """(trans_thresh2 [S], rot_bound): (diameter / 10)^2 and 1 + 2 cos(2 pi / n_alpha), formed on the host."""
    t = trans_fraction * np.asarray(diameters, np.float64)
    return t * t, 1.0 + 2.0 * np.cos(2.0 * np.pi / n_alpha)


def propose(model, scene, normals, mask, class_id, top=4, ref_step=5, peaks=2):
    v = vote(scene, normals, mask, class_id, model, ref_step, peaks)
    B = len(scene)
    tt2, rb = thresholds(model["diameters"], model["n_alpha"])
    r = cluster(v["votes"].reshape(B, -1), v["pose"].reshape(B, -1, 4, 4), class_id, tt2, rb, top)
    r["vote"] = v
    return r


def pose_errors(T, gt):
    """(translation distance, trace(R^T R_gt)) of a pose against the truth."""
    d = T[:3, 3] - gt[:3, 3]
    return float(np.sqrt(d @ d)), float(np.trace(T[:3, :3].T @ gt[:3, :3]))
