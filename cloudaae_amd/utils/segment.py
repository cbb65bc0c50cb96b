"""Evaluation inputs from RGB-D frames (evaluate_cloudAAE_ycbv.py:164-271): back-projection, per-class segments, the
mean-distance filter, open3d's radius outlier removal and FPS_random -- on the GPU, the whole batch of frames in a few
launches of cloudaae_frame_segments, cloudaae_radius_outlier and cloudaae_ragged_fps.  The definition is in DESIGN.md
("Frame segments").

    r = extract_segments(depth, label, intrinsics, classes)      # ragged result, one read-back of the counts
    s = sample_segments(r, num_point, seed=0)                     # xyz_inlier, xyz [S, N, 3]
"""
import math

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

NUM_CLASS = 21
THRESHOLD = 0.2           # threshold_distance_per_class (:40, :381)
NB_POINTS = 100           # remove_radius_outlier(100, 0.02) (:277)
RADIUS = 0.02             # handed to open3d as float32 by tf.py_func; the C ABI takes a float
MIN_KEEP = 512            # fewer inliers: keep the whole segment (:255-256)
MIN_AFTER_FILTER = 100    # a segment is dropped unless num_point_after_filter > 100 (:318)


class Segments(object):
    """The ragged result of extract_segments.  Host arrays (numpy): frame, cls [S]; offsets, inlier_offsets [S+1];
    num_point_after_filter, num_valid_points_in_segment [S]; kept [S] bool; quaternion [S,4] and translation [S,3]
    (when poses were given); mean [S,3].  Device tensors: xyz [M,3] (xyz_org_distance_filtered of every segment,
    packed: segment i at offsets[i]:offsets[i+1]), xyz_inlier_full [M,3] and inlier_index [M] (index within the
    segment's filtered points) packed by inlier_offsets."""

    def segment(self, i):
        """Host copies of segment i: (xyz_org_distance_filtered, inlier_idx, xyz_inlier_full)."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        c, d = int(self.inlier_offsets[i]), int(self.inlier_offsets[i + 1])
        return (self.xyz[a:b].cpu().numpy(), self.inlier_index[c:d].cpu().numpy().astype(np.int64),
                self.xyz_inlier_full[c:d].cpu().numpy())


def _device_tensor(x, dtype, device):
    if isinstance(x, torch.Tensor):
        require(x.dtype == dtype, "expected a %s tensor, got %s" % (dtype, x.dtype))
        return x.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _segment_list(classes, F):
    """classes: None (every class of every frame), a [F, C] one-hot (class_one_hot) or a list of F class lists."""
    if classes is None:
        return [list(range(NUM_CLASS))] * F
    if isinstance(classes, np.ndarray) and classes.ndim == 2:
        require(classes.shape[0] == F, "class_one_hot must be [F, C]")
        return [list(np.nonzero(row)[0]) for row in classes]
    require(len(classes) == F, "classes must hold one list per frame")
    return [sorted(int(c) for c in cl) for cl in classes]


def extract_segments(depth, label, intrinsics, classes=None, quaternions=None, translations=None, num_point=None,
                     threshold=THRESHOLD, nb_points=NB_POINTS, radius=RADIUS, min_keep=MIN_KEEP, device=None):
    """The segments of F frames: depth [F,H,W] uint16, label [F,H,W] uint8, intrinsics [F,5] float32 (fx, fy, cx, cy,
    factor_depth); numpy arrays or tensors.  One segment per (frame, class), frame-major, classes ascending (the
    order of the reference's class_one_hot).  quaternions [F,21,4] / translations [F,21,3]: the records' poses, copied
    per segment.  kept = num_point_after_filter > 100 and, when num_point is given, num_valid_points_in_segment >=
    num_point (:318, :322).  One read-back of the counts."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if isinstance(depth, np.ndarray):
        require(depth.dtype == np.uint16, "depth must be uint16")
        d = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device)   # the same bits
    else:
        require(depth.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)), "depth must be uint16")
        d = depth.to(device).contiguous()
    lab = _device_tensor(label, torch.uint8, device)
    intr = _device_tensor(np.asarray(intrinsics, np.float32) if not isinstance(intrinsics, torch.Tensor) else intrinsics,
                          torch.float32, device)
    require(d.dim() == 3 and tuple(lab.shape) == tuple(d.shape), "depth and label must be [F, H, W]")
    F, H, W = (int(v) for v in d.shape)
    require(tuple(intr.shape) == (F, 5), "intrinsics must be [F, 5]")
    segs = _segment_list(classes, F)
    frame = np.array([f for f in range(F) for _ in segs[f]], np.int32)
    cls = np.array([c for f in range(F) for c in segs[f]], np.int32)
    S = len(cls)
    require(S >= 1, "no segment to extract")
    require(len(set(zip(frame.tolist(), cls.tolist()))) == S, "a (frame, class) pair is listed twice")
    require(cls.min() >= 0 and cls.max() < 255, "classes must lie in [0, 255)")
    M = F * H * W
    L = _lib.lib()
    seg_frame = torch.from_numpy(frame).to(device)
    seg_class = torch.from_numpy(cls).to(device)
    counts = torch.empty((3 * S + 2,), dtype=torch.int32, device=device)    # offsets | inlier offsets | num_valid
    offsets, in_offsets, num_valid = counts[:S + 1], counts[S + 1:2 * S + 2], counts[2 * S + 2:]
    xyz = torch.empty((M, 3), dtype=torch.float32, device=device)
    mean = torch.empty((S, 3), dtype=torch.float32, device=device)
    ws_bytes = int(L.cloudaae_frame_segments_workspace_bytes(F, H, W, S))
    require(ws_bytes > 0, "frame batch above the kernel's limit")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    _lib.check(L.cloudaae_frame_segments(F, H, W, d.data_ptr(), lab.data_ptr(), ptr(intr), S, ptr(seg_frame),
                                         ptr(seg_class), float(threshold), offsets.data_ptr(), ptr(xyz), ptr(mean),
                                         ptr(ws), ws_bytes, stream()), "cloudaae_frame_segments")
    in_xyz = torch.empty((M, 3), dtype=torch.float32, device=device)
    in_index = torch.empty((M,), dtype=torch.int32, device=device)
    ro_bytes = int(L.cloudaae_radius_outlier_workspace_bytes(S, M))
    ws2 = torch.empty((ro_bytes,), dtype=torch.uint8, device=device)
    _lib.check(L.cloudaae_radius_outlier(S, offsets.data_ptr(), ptr(xyz), M, int(nb_points), float(radius),
                                         int(min_keep), in_offsets.data_ptr(), ptr(in_index), ptr(in_xyz),
                                         num_valid.data_ptr(), ptr(ws2), ro_bytes, stream()),
               "cloudaae_radius_outlier")
    host = counts.cpu().numpy().astype(np.int64)             # the one read-back
    r = Segments()
    r.frame, r.cls = frame, cls
    r.offsets, r.inlier_offsets = host[:S + 1], host[S + 1:2 * S + 2]
    r.num_point_after_filter = np.diff(r.offsets)
    r.num_valid_points_in_segment = host[2 * S + 2:]
    r.kept = r.num_point_after_filter > MIN_AFTER_FILTER
    if num_point is not None:
        r.kept &= r.num_valid_points_in_segment >= int(num_point)
    r.xyz, r.xyz_inlier_full, r.inlier_index, r.mean = xyz, in_xyz, in_index, mean
    r.offsets_device, r.inlier_offsets_device = offsets, in_offsets
    r.max_points = M
    r.quaternion = np.asarray(quaternions, np.float32)[frame, cls] if quaternions is not None else None
    r.translation = np.asarray(translations, np.float32)[frame, cls] if translations is not None else None
    return r


def ragged_fps(offsets, xyz, k, starts, max_points=None):
    """cloudaae_ragged_fps: FPS_random of each packed set (offsets [S+1] int32 device, xyz [M,3]) from starts [S]
    (host or device ints).  Returns (idx [S,k] int32, picked xyz [S,k,3])."""
    require(int(k) >= 1, "k must be >= 1")
    S = int(offsets.numel()) - 1
    M = int(xyz.shape[0]) if max_points is None else int(max_points)
    dev = xyz.device
    st = starts if isinstance(starts, torch.Tensor) else torch.from_numpy(np.asarray(starts, np.int32))
    st = st.to(device=dev, dtype=torch.int32).contiguous()
    require(st.numel() == S, "one start per set")
    idx = _lib.empty((S, int(k)), dtype=torch.int32, device=dev)
    out = _lib.empty((S, int(k), 3), dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = int(L.cloudaae_ragged_fps_workspace_bytes(max(M, 1)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.check(L.cloudaae_ragged_fps(S, offsets.data_ptr(), ptr(xyz), max(M, 1), int(k), ptr(st), ptr(idx), ptr(out),
                                     ptr(ws), nbytes, stream()), "cloudaae_ragged_fps")
    return idx, out


def random_starts(sizes, rng):
    """A start index per set, uniform in [0, n) from a seeded numpy Generator (random.randint(0, n - 1) of the
    reference, :233, which is unseeded); -1 for an empty set."""
    return np.array([int(rng.integers(n)) if n > 0 else -1 for n in sizes], np.int32)


def sample_segments(result, num_point, seed=0, starts=None):
    """FPS_sample_segment (:262-271): num_point points of each segment's inliers (-> xyz_inlier) and of its filtered
    points (-> xyz).  starts: (inlier starts [S], filtered starts [S]); otherwise drawn from numpy's Generator(seed),
    inlier set first, segment by segment.  Returns dict(xyz_inlier [S,N,3], xyz [S,N,3], idx_inlier, idx [S,N],
    starts_inlier, starts)."""
    n_in = np.diff(result.inlier_offsets)
    n_f = result.num_point_after_filter
    if starts is None:
        rng = np.random.default_rng(seed)
        both = random_starts(np.stack([n_in, n_f], 1).reshape(-1), rng).reshape(-1, 2)
        s_in, s_f = both[:, 0], both[:, 1]
    else:
        s_in, s_f = (np.asarray(s, np.int32) for s in starts)
    idx_in, xyz_in = ragged_fps(result.inlier_offsets_device, result.xyz_inlier_full, num_point, s_in,
                                result.max_points)
    idx_f, xyz_f = ragged_fps(result.offsets_device, result.xyz, num_point, s_f, result.max_points)
    return dict(xyz_inlier=xyz_in, xyz=xyz_f, idx_inlier=idx_in, idx=idx_f, starts_inlier=s_in, starts=s_f)


def quat2axangle(q):
    """transforms3d.quaternions.quat2axangle (q = w, x, y, z) as the reference calls it (identity_thresh None, which
    resolves to 3 float64 eps): (axis, angle)."""
    w, x, y, z = (float(v) for v in q)
    Nq = w * w + x * x + y * y + z * z
    if not math.isfinite(Nq):
        return np.array([1.0, 0.0, 0.0]), float('nan')
    eps = np.finfo(np.float64).eps
    if Nq < eps ** 2:
        return np.array([1.0, 0.0, 0.0]), 0.0
    if Nq != 1:
        s = math.sqrt(Nq)
        w, x, y, z = w / s, x / s, y / s, z / s
    len2 = x * x + y * y + z * z
    if len2 < (3 * eps) ** 2:
        return np.array([1.0, 0.0, 0.0]), 0.0
    theta = 2 * math.acos(max(min(w, 1), -1))
    return np.array([x, y, z]) / math.sqrt(len2), theta


def quat2axag(q):
    """quat2axag_batch + quat2axag_tf (:66-79): axis and angle kept as float32, then angle * axis in float32."""
    ax, ang = quat2axangle(q)
    return (np.float32(ang) * ax.astype(np.float32)).astype(np.float32)
