"""NumPy/SciPy restatement of DESIGN.md "Frame segments": the segment pipeline of the reference's evaluation
(evaluate_cloudAAE_ycbv.py:164-271), which cloudaae_frame_segments, cloudaae_radius_outlier and cloudaae_ragged_fps
implement on the GPU.  Plain, slow and literal; the GPU tests compare with it bit for bit."""
import numpy as np

NUM_CLASS = 21
THRESHOLD = np.float32(0.2)       # threshold_distance_per_class (:40, :381)
NB_POINTS = 100                   # remove_radius_outlier(100, 0.02) through tf.py_func (:277)
RADIUS = np.float32(0.02)         # tf.py_func hands the literal over as float32
MIN_KEEP = 512                    # :255-256


def radius_sq(radius=RADIUS):
    """The one place of the r^2 convention: r = (double)(float32 radius), compared as d^2 < r*r in double (as the
    ICP section of DESIGN.md does; open3d's FLANN may compare in float, as recalled, not checked)."""
    r = float(np.float32(radius))
    return r * r


def back_project(depth, intrinsics):
    """:164-178 in fp32: dm = depth / factor; x = ((u - cx) * dm) / fx, y = ((v - cy) * dm) / fy; [H*W, 3]."""
    fx, fy, cx, cy, factor = (np.float32(v) for v in intrinsics)
    H, W = depth.shape
    dm = depth.astype(np.float32) / factor
    u = np.arange(W, dtype=np.float32)[None, :]
    v = np.arange(H, dtype=np.float32)[:, None]
    x = ((u - cx) * dm) / fx
    y = ((v - cy) * dm) / fy
    return np.stack([x, y, dm], axis=2).reshape(H * W, 3).astype(np.float32)


def segment_mean(pts):
    """fp64 sum in pixel order (a running sum: np.cumsum adds left to right), / count, rounded to fp32."""
    if len(pts) == 0:
        return np.zeros(3, np.float32)
    s = np.cumsum(pts.astype(np.float64), axis=0)[-1]
    return (s / float(len(pts))).astype(np.float32)


def distance_filter(pts, mean, threshold=THRESHOLD):
    """Keep sqrtf((dx^2 + dy^2) + dz^2) <= threshold, all in fp32."""
    d = (pts - mean).astype(np.float32)
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.sqrt(dd.astype(np.float32)) <= np.float32(threshold)


def frame_segments(depth, label, intrinsics, classes, threshold=THRESHOLD):
    """One frame: for each class c of `classes` (in the order given) -> dict(mask_xyz, mean, xyz) where xyz is
    xyz_org_distance_filtered (pixel order)."""
    xyz = back_project(depth, intrinsics)
    lab = label.reshape(-1).astype(np.int64) - 1
    valid = depth.reshape(-1) != 0
    out = []
    for c in classes:
        m = (lab == int(c)) & valid
        pts = xyz[m]
        mean = segment_mean(pts)
        keep = distance_filter(pts, mean, threshold) if len(pts) else np.zeros(0, bool)
        out.append(dict(mask_xyz=pts, mean=mean, xyz=pts[keep]))
    return out


def neighbour_counts(pts, radius=RADIUS):
    """For each point, the points j of the set (itself included) with ((dx^2 + dy^2) + dz^2) < r^2 in fp64.
    Candidates from scipy's cKDTree at a slightly larger radius, then the exact test."""
    from scipy.spatial import cKDTree
    n = len(pts)
    if n == 0:
        return np.zeros(0, np.int64)
    p = pts.astype(np.float64)
    r2 = radius_sq(radius)
    pairs = cKDTree(p).query_pairs(np.sqrt(r2) * (1 + 1e-6), output_type='ndarray')
    counts = np.ones(n, np.int64)
    if len(pairs):
        i, j = pairs[:, 0], pairs[:, 1]
        d = p[i] - p[j]
        ok = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2
        counts += np.bincount(i[ok], minlength=n) + np.bincount(j[ok], minlength=n)
    return counts


def neighbour_counts_brute(pts, radius=RADIUS):
    """The same by brute force (small sets)."""
    p = pts.astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return (dd < radius_sq(radius)).sum(axis=1)


def radius_outlier(pts, nb_points=NB_POINTS, radius=RADIUS, min_keep=MIN_KEEP, counts=None):
    """open3d remove_radius_outlier: keep i when its count > nb_points; fewer than min_keep kept -> all.
    Returns (inlier_idx int64, num_valid_points_in_segment = count_nonzero(inlier_idx))."""
    if counts is None:
        counts = neighbour_counts(pts, radius)
    idx = np.nonzero(counts > nb_points)[0]
    if len(idx) < min_keep:
        idx = np.arange(len(pts))
    return idx.astype(np.int64), int(np.count_nonzero(idx))


def fps(pts, k, start):
    """FPS_random (:226-247) from a given start: dist in fp64 on the widened coordinates, first argmax."""
    p = pts.astype(np.float64)

    def d2(q):
        d = q[None, :] - p
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = np.zeros(k, np.int64)
    idx[0] = start
    dist = d2(p[start])
    for i in range(1, k):
        idx[i] = int(np.argmax(dist))
        dist = np.minimum(dist, d2(p[idx[i]]))
    return idx


def extract(frames, classes_per_frame, threshold=THRESHOLD, nb_points=NB_POINTS, radius=RADIUS, min_keep=MIN_KEEP):
    """frames: list of (depth, label, intrinsics); classes_per_frame: list of class lists.  One dict per segment,
    frame-major: frame, class, xyz (filtered), mean, num_point_after_filter, inlier_idx, xyz_inlier_full,
    num_valid_points_in_segment."""
    out = []
    for f, ((depth, label, intr), classes) in enumerate(zip(frames, classes_per_frame)):
        for c, seg in zip(classes, frame_segments(depth, label, intr, classes, threshold)):
            idx, nv = radius_outlier(seg['xyz'], nb_points, radius, min_keep)
            out.append(dict(frame=f, cls=int(c), xyz=seg['xyz'], mean=seg['mean'],
                            num_point_after_filter=len(seg['xyz']), inlier_idx=idx, xyz_inlier_full=seg['xyz'][idx],
                            num_valid_points_in_segment=nv))
    return out


def extract_listed(frames, seg_frame, seg_class, threshold=THRESHOLD, nb_points=NB_POINTS, radius=RADIUS,
                   min_keep=MIN_KEEP):
    """The table rule of cloudaae_frame_segments for any segment list: segment i is the pair (seg_frame[i],
    seg_class[i]); one dict per segment, in list order, with the keys of `extract` and mask_xyz.  A pair named more than
    once keeps only its last entry; the earlier entries, and every pair whose frame lies outside [0, F) or whose class
    lies outside [0, 254], are empty segments (no point, mean 0).  A pixel whose class is not listed belongs to
    nothing."""
    F = len(frames)
    owner = {}
    for i, (f, c) in enumerate(zip(seg_frame, seg_class)):
        if 0 <= int(f) < F and 0 <= int(c) <= 254:
            owner[(int(f), int(c))] = i                      # a later entry replaces an earlier one
    none = np.zeros((0, 3), np.float32)
    out = []
    for i, (f, c) in enumerate(zip(seg_frame, seg_class)):
        f, c = int(f), int(c)
        if owner.get((f, c)) == i:
            depth, label, intr = frames[f]
            seg = frame_segments(depth, label, intr, [c], threshold)[0]
        else:
            seg = dict(mask_xyz=none, mean=np.zeros(3, np.float32), xyz=none)
        idx, nv = radius_outlier(seg['xyz'], nb_points, radius, min_keep)
        out.append(dict(frame=f, cls=c, mask_xyz=seg['mask_xyz'], xyz=seg['xyz'], mean=seg['mean'],
                        num_point_after_filter=len(seg['xyz']), inlier_idx=idx, xyz_inlier_full=seg['xyz'][idx],
                        num_valid_points_in_segment=nv))
    return out


def quat2axangle(q):
    """transforms3d.quaternions.quat2axangle (w, x, y, z) with identity_thresh None (3 float64 eps): (axis, angle)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q
    Nq = w * w + x * x + y * y + z * z
    if not np.isfinite(Nq):
        return np.array([1.0, 0, 0]), float('nan')
    if Nq < np.finfo(np.float64).eps ** 2:
        return np.array([1.0, 0, 0]), 0.0
    if Nq != 1:
        s = np.sqrt(Nq)
        w, x, y, z = w / s, x / s, y / s, z / s
    len2 = x * x + y * y + z * z
    if len2 < (3 * np.finfo(np.float64).eps) ** 2:
        return np.array([1.0, 0, 0]), 0.0
    theta = 2 * np.arccos(max(min(w, 1), -1))
    return np.array([x, y, z]) / np.sqrt(len2), theta


def quat2axag(q):
    """quat2axag_batch + quat2axag_tf (:66-79): axis and angle stored as float32, their product in float32."""
    ax, ang = quat2axangle(q)
    return (np.float32(ang) * ax.astype(np.float32)).astype(np.float32)
