"""NumPy restatement of DESIGN.md, "Pose verification".  Written from the definition: the composition is float64 in the
association order the definition writes (NumPy does not fuse a product into a sum), so the matrices are expected to
equal the kernel's bit for bit; the counts are integers on the uint16 depths widened to int64; the winner is chosen with
Python's unbounded integers.  The hypotheses' images are rendered by render_reference.render."""
import numpy as np

import render_reference as R

COUNTERS = ("rendered", "consistent", "in_front", "behind", "unknown", "explained")


def flip_hypotheses(model_xyz):
    """[4,4,4]: the identity, then the half turns about the principal axes through the centroid, by descending
    eigenvalue of the covariance."""
    x = np.asarray(model_xyz, np.float64)[:, :3]
    c = x.mean(axis=0)
    y = x - c
    w, vec = np.linalg.eigh((y.T @ y) / len(x))
    out = [np.eye(4)]
    for k in np.argsort(-w, kind="stable"):
        a = vec[:, k] / np.sqrt(vec[:, k] @ vec[:, k])
        T = np.eye(4)
        T[:3, :3] = 2.0 * np.outer(a, a) - np.eye(3)
        T[:3, 3] = c - T[:3, :3] @ c
        out.append(T)
    return np.stack(out)


def compose_one(A, H):
    """base A times member H, top three rows: C[r][k] = (A[r][0] H[0][k] + A[r][1] H[1][k]) + A[r][2] H[2][k], and the
    last column ((... ) + A[r][2] H[2][3]) + A[r][3]."""
    A, H = np.asarray(A, np.float64).reshape(4, 4), np.asarray(H, np.float64).reshape(4, 4)
    C = np.zeros((4, 4), np.float64)
    for r in range(3):
        for k in range(3):
            C[r, k] = (A[r, 0] * H[0, k] + A[r, 1] * H[1, k]) + A[r, 2] * H[2, k]
        C[r, 3] = ((A[r, 0] * H[0, 3] + A[r, 1] * H[1, 3]) + A[r, 2] * H[2, 3]) + A[r, 3]
    C[3, 3] = 1.0
    return C


def compose(base, class_id, index, hyp, p):
    """-> pose [B,p,4,4], trans [B,p,3] float32, valid [B,p] int32.  index [nclass+1] offsets into hyp [n,4,4]."""
    base = np.asarray(base, np.float64).reshape(-1, 4, 4)
    index, hyp = np.asarray(index, np.int64), np.asarray(hyp, np.float64).reshape(-1, 4, 4)
    B, nclass = len(base), len(index) - 1
    pose = np.zeros((B, p, 4, 4), np.float64)
    valid = np.zeros((B, p), np.int32)
    for i in range(B):
        c = int(class_id[i])
        first = count = 0
        if 0 <= c < nclass:
            first, count = int(index[c]), int(index[c + 1] - index[c])
            if first < 0 or count < 0 or first + count > len(hyp):
                count = 0
        for j in range(p):
            ok = j < count
            H = hyp[first + (j if ok else 0)] if count > 0 else np.eye(4)
            pose[i, j] = compose_one(base[i], H)
            valid[i, j] = int(ok)
    return pose, pose[:, :, :3, 3].astype(np.float32), valid


def fit_counts(depth_test, label, frame_of, want, depth_hyp, tau):
    """-> counts [B,P,6] int32, seg_total [B] int32, abs_sum [B,P] int64."""
    dt = np.asarray(depth_test)
    dh = np.asarray(depth_hyp)
    assert dt.dtype == np.uint16 and dh.dtype == np.uint16
    F = len(dt)
    B, P = dh.shape[:2]
    counts = np.zeros((B, P, 6), np.int32)
    seg_total = np.zeros(B, np.int32)
    abs_sum = np.zeros((B, P), np.int64)
    for b in range(B):
        fr = int(frame_of[b])
        if fr < 0 or fr >= F:
            continue
        t = dt[fr].astype(np.int64)
        seg = np.zeros(t.shape, bool) if label is None else (np.asarray(label)[fr].astype(np.int64) == int(want[b])) & (t != 0)
        seg_total[b] = seg.sum()
        for j in range(P):
            d = dh[b, j].astype(np.int64)
            both = (d != 0) & (t != 0)
            consistent = both & (np.abs(d - t) <= int(tau[b]))
            counts[b, j] = [(d != 0).sum(), consistent.sum(), (both & (t - d > int(tau[b]))).sum(),
                            (both & (d - t > int(tau[b]))).sum(), ((d != 0) & (t == 0)).sum(), (seg & consistent).sum()]
            abs_sum[b, j] = np.abs(d - t)[consistent].sum()
    return counts, seg_total, abs_sum


def fraction(c, seg_total, valid, mode):
    """(num, den) of one hypothesis as Python integers; (0, 1) for "no score"."""
    c = [int(x) for x in c]
    num, den = (c[5], int(seg_total) + c[2]) if mode == 0 else (c[1], c[1] + c[2] + c[3])
    if den <= 0 or num < 0 or not valid:
        return 0, 1
    return num, den


def select(counts, seg_total, valid, pose, mode):
    """-> best [B] int32, score [B,P], pose_best [B,4,4], margin [B]."""
    counts = np.asarray(counts)
    B, P = counts.shape[:2]
    best = np.zeros(B, np.int32)
    score = np.zeros((B, P), np.float64)
    margin = np.zeros(B, np.float64)
    pose_best = np.zeros((B, 4, 4), np.float64)
    for b in range(B):
        fr = [fraction(counts[b, j], seg_total[b], valid[b, j], mode) for j in range(P)]
        w = 0
        for j in range(1, P):
            if fr[j][0] * fr[w][1] > fr[w][0] * fr[j][1]:
                w = j
        score[b] = [float(n) / float(d) for n, d in fr]
        best[b] = w
        others = [score[b, j] for j in range(P) if j != w]
        margin[b] = score[b, w] - max(others) if others else 0.0
        pose_best[b] = np.asarray(pose, np.float64).reshape(B, P, 4, 4)[b, w]
    return best, score, pose_best, margin


def tau_units(tau, factor_depth):
    return np.floor(np.asarray(tau, np.float64) * np.asarray(factor_depth, np.float64) + 0.5).astype(np.int32)


def verify(meshes, mesh_index, poses, depth_test, label, want, intrinsics, frame_of, tau=0.01, mode=0, valid=None):
    """The whole pipeline on the NumPy renderer: every hypothesis alone with its frame's intrinsics, label 1."""
    poses = np.asarray(poses, np.float64)
    B, P = poses.shape[:2]
    intr = np.asarray(intrinsics, np.float32)
    H, W = depth_test.shape[1:]
    frames = [[(int(mesh_index[b]), 1, poses[b, j])] for b in range(B) for j in range(P)]
    r = R.render(meshes, frames, intr[np.repeat(np.asarray(frame_of), P)], H, W)
    tu = tau_units(np.broadcast_to(np.asarray(tau, np.float64), (B,)), intr[np.asarray(frame_of), 4].astype(np.float64))
    counts, seg_total, abs_sum = fit_counts(depth_test, label, frame_of, want, r['depth'].reshape(B, P, H, W), tu)
    valid = np.ones((B, P), np.int32) if valid is None else valid
    best, score, pose_best, margin = select(counts, seg_total, valid, poses, mode)
    return dict(counts=counts, seg_total=seg_total, abs_sum=abs_sum, best=best, score=score, pose_best=pose_best,
                margin=margin, dropped=r['dropped'].reshape(B, P), depth_hyp=r['depth'].reshape(B, P, H, W))


# ---- the scene the host and the GPU tests share --------------------------------------------------------------------------
def l_prism():
    """An L-shaped prism with legs of 16 and 10 cm and a 4 x 4 cm section, as two boxes that share a corner block: no
    rotation but the identity maps it onto itself.  -> (vertices [16,3] float32, triangles [24,3] int32)."""
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    unit = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    tri = np.array([[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)], np.int32)
    long_leg = unit * [0.16, 0.04, 0.04]
    short_leg = unit * [0.04, 0.10, 0.04]
    v = np.concatenate([long_leg, short_leg]) - [0.05, 0.03, 0.02]
    return v.astype(np.float32), np.concatenate([tri, tri + 8]).astype(np.int32)


def plate():
    """A plate of 9 x 12 x 0.4 cm centred on the origin."""
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    unit = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    tri = np.array([[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)], np.int32)
    return ((unit - 0.5) * [0.09, 0.12, 0.004]).astype(np.float32), tri


def surface_points(vertices, triangles, per_edge=6):
    """A regular sample of every triangle (barycentric lattice): the point model the flips are taken from."""
    v = np.asarray(vertices, np.float64)
    pts = []
    for a, b, c in np.asarray(triangles):
        for i in range(per_edge + 1):
            for j in range(per_edge + 1 - i):
                u, w = i / per_edge, j / per_edge
                pts.append(v[a] * (1 - u - w) + v[b] * u + v[c] * w)
    return np.array(pts)


def scene(height=48, width=64):
    """The L prism (mesh 0, label 1) under a ground-truth pose and a nearer plate (mesh 1, label 2) that hides the end
    of its long leg, in one frame of width x height; the four flip candidates of the ground truth with the ground truth
    itself at index 2.  -> dict(meshes, intr [1,5], gt [4,4], depth [1,H,W] uint16, label [1,H,W] uint8, flips [4,4,4],
    order [4], poses [1,4,4,4])."""
    meshes = [l_prism(), plate()]
    intr = np.array([[60.0 * width / 64, 60.0 * width / 64, 0.5 * width - 0.5, 0.5 * height - 0.5, 10000.0]], np.float32)
    gt = R.pose_matrix([0.5, -0.4, 0.3], [-0.02, 0.01, 0.5])
    occ = R.pose_matrix([0.0, 0.0, 0.0], [0.075, 0.0, 0.38])
    test = R.render(meshes, [[(0, 1, gt), (1, 2, occ)]], intr, height, width)
    flips = flip_hypotheses(surface_points(*meshes[0]))
    order = np.array([1, 3, 0, 2])                            # the identity (the ground truth) comes third
    poses = np.stack([gt @ flips[k] for k in order])[None]
    return dict(meshes=meshes, intr=intr, gt=gt, depth=test['depth'], label=test['label'], flips=flips, order=order, poses=poses)
