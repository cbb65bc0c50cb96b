"""Detections: which of the components found in an unlabelled depth frame (utils/depth_components.py) is which object,
under which pose, or nothing -- decided without the ground truth, by verification score across the (component, class)
pairs of a frame.  Every hypothesis is rendered alone into a window around its component (utils/render.py), counted
against the observed depth inside that window (cloudaae_depth_fit_counts_window; csrc/depth_fit.hip) and the pairs of a
frame are assigned greedily by their exact fractions (cloudaae_detect_assign; csrc/detect.hip).  The definition is in
DESIGN.md ("Detections").

    d = detect_objects(depth, intrinsics, meshes, ppf_models)          # Detections; d.table['det_class'] [F,K], ...
    r = score_candidates(segments, poses, valid, meshes, mesh_of_class, intrinsics, depth)     # given hypotheses
"""
from fractions import Fraction

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .frame_inputs import check_depth, check_int32, upload_depth
from .pose_verify import COUNTERS, MODE_SEGMENT, MODE_SILHOUETTE, _fit_inputs, tau_units

# choices, not measurements
MARGIN = 0.5              # of the component's box, added on either side
MIN_SCORE = (1, 2)        # a pair below this fraction is never assigned
MAX_PER_CLASS = 1
TOP = 4                   # proposals per (component, class)
NUM_POINT = 256           # points of a component's cloud
SAMPLES_PER_LAUNCH = 64
NORMAL_RADIUS = 0.02      # neighbourhood of the component clouds' normals, metres

MAX_K, MAX_C, MAX_P = 254, 256, 64
TABLE_INT = ("det_class", "det_hyp", "det_num", "det_den", "det_rank", "alt_class", "alt_num", "alt_den")


def _ceil_times(margin, n):
    """ceil(margin n) in integers; a float margin means its decimal text (0.1 is one tenth)."""
    q = (Fraction(str(margin)) if isinstance(margin, float) else Fraction(margin)) * int(n)
    return -((-q.numerator) // q.denominator)


def windows(comp_box, n_components, H, W, margin=MARGIN):
    """One window size for the call and an origin per component, on the host in integers.  comp_box [F,K,4] = (u_min,
    v_min, u_max, v_max) and n_components [F] as segment_depth returns them.  With bw = u_max - u_min + 1 and m_u =
    ceil(margin bw) (rows alike): ww = min(max (bw + 2 m_u), W) rounded up to a multiple of 8, wh = min(max (bh + 2 m_v),
    H), the maxima over the call's components; u0 = u_min - (ww - bw) // 2, v0 = v_min - (wh - bh) // 2, so a window may
    overhang the frame.  -> (origin [F,K,2] int32, zeros past n_components; wh; ww)."""
    box = np.asarray(comp_box, np.int64)
    require(box.ndim == 3 and box.shape[2] == 4, "comp_box must be [F, K, 4]")
    F, K = box.shape[:2]
    n = np.minimum(np.asarray(n_components, np.int64).reshape(-1), K)
    require(len(n) == F, "n_components must be [F]")
    require(Fraction(str(margin)) >= 0 if isinstance(margin, float) else Fraction(margin) >= 0, "margin must be >= 0")
    live = np.arange(K)[None, :] < n[:, None]
    bw = np.where(live, box[:, :, 2] - box[:, :, 0] + 1, 1)
    bh = np.where(live, box[:, :, 3] - box[:, :, 1] + 1, 1)
    require(bw.min() >= 1 and bh.min() >= 1, "a component's box is empty")
    need_w = max([1] + [int(b) + 2 * _ceil_times(margin, b) for b in bw[live]])       # (a call without a component: 1)
    need_h = max([1] + [int(b) + 2 * _ceil_times(margin, b) for b in bh[live]])
    ww = -(-min(need_w, int(W)) // 8) * 8
    wh = min(need_h, int(H))
    origin = np.stack([box[:, :, 0] - (ww - bw) // 2, box[:, :, 1] - (wh - bh) // 2], axis=2)
    return np.where(live[:, :, None], origin, 0).astype(np.int32), wh, ww


def fit_counts_window(depth_test, label, frame_of, want, origin, depth_hyp, tau):
    """cloudaae_depth_fit_counts_window.  depth_test [F,H,W] and depth_hyp [B,P,wh,ww]: int16 tensors holding the uint16
    bits, or uint16; label [F,H,W] uint8 or None; frame_of [B] int32 (an entry outside [0, F) gives zero counts); want [B]
    int32 (ignored without a label); origin [B,2] int32 = (u0, v0), any values; tau [B] int32 in depth units.  Window
    pixel (x, y) of sample b is frame pixel (u0 + x, v0 + y); outside the frame there is no depth and no segment.
    -> dict of counts [B,P,6] int32 (pose_verify.COUNTERS), seg_total [B] int32 and abs_sum [B,P] int64 on the device."""
    dt, dh = check_depth(depth_test, "depth_test", 3), check_depth(depth_hyp, "depth_hyp", 4)
    F, H, W = (int(x) for x in dt.shape)
    B, P, wh, ww = (int(x) for x in dh.shape)
    require(B >= 1 and P >= 1 and wh >= 1 and ww >= 1, "depth_hyp must be [B, P, wh, ww], none of them 0")
    label, frame_of, want, tau, out = _fit_inputs(dt, dh, label, frame_of, want, tau)
    origin = check_int32(origin, "origin", (B, 2), dt.device)
    with torch.cuda.device(dt.device):
        _lib.check(_lib.lib().cloudaae_depth_fit_counts_window(F, H, W, ptr(dt), ptr(label), B, P, ptr(frame_of), ptr(want),
                                                               ptr(origin), wh, ww, ptr(dh), ptr(tau), ptr(out["counts"]),
                                                               ptr(out["seg_total"]), ptr(out["abs_sum"]), stream()),
                   "cloudaae_depth_fit_counts_window")
    return out


def assign(counts, seg_total, valid, pose, n_components, mode=MODE_SEGMENT, min_score=MIN_SCORE, max_per_class=MAX_PER_CLASS):
    """cloudaae_detect_assign.  counts [F,K,C,P,6], seg_total [F,K,C], valid [F,K,C,P] (None: all valid), n_components [F]
    int32 and pose [F,K,C,P,4,4] float64 on one device; min_score = (num, den).  -> dict of pair_hyp, pair_num, pair_den
    [F,K,C] int32, pair_score [F,K,C] float64, det_class, det_hyp, det_num, det_den, det_rank, alt_class, alt_num, alt_den
    [F,K] int32, det_score [F,K], det_pose [F,K,4,4] float64 and n_det [F] int32 on the device."""
    require(isinstance(counts, torch.Tensor) and counts.dtype == torch.int32 and counts.dim() == 5 and
            counts.shape[4] == len(COUNTERS) and min(counts.shape) >= 1, "counts must be an int32 [F, K, C, P, 6] tensor")
    F, K, C, P = (int(x) for x in counts.shape[:4])
    dev = counts.device
    require(K <= MAX_K and C <= MAX_C and P <= MAX_P, "at most %d components, %d classes and %d hypotheses" % (MAX_K, MAX_C, MAX_P))
    seg_total = check_int32(seg_total, "seg_total", (F, K, C), dev)
    if valid is None:
        valid = torch.ones((F, K, C, P), dtype=torch.int32, device=dev)
    valid = check_int32(valid, "valid", (F, K, C, P), dev)
    n_components = check_int32(n_components, "n_components", (F,), dev)
    require(isinstance(pose, torch.Tensor) and pose.dtype == torch.float64 and tuple(pose.shape) == (F, K, C, P, 4, 4) and
            pose.device == dev, "pose must be a float64 [F, K, C, P, 4, 4] tensor on the counts' device")
    num, den = int(min_score[0]), int(min_score[1])
    require(int(mode) in (MODE_SEGMENT, MODE_SILHOUETTE), "mode must be 0 (segment rule) or 1 (silhouette rule)")
    require(0 <= num <= den and 1 <= den <= (1 << 20), "min_score must be (num, den) with 0 <= num <= den and 1 <= den <= 2^20")
    require(int(max_per_class) >= 1, "max_per_class must be >= 1")
    out = {k: _lib.empty((F, K, C), dtype=torch.int32, device=dev) for k in ("pair_hyp", "pair_num", "pair_den")}
    out["pair_score"] = _lib.empty((F, K, C), dtype=torch.float64, device=dev)
    out.update({k: _lib.empty((F, K), dtype=torch.int32, device=dev) for k in TABLE_INT})
    out["det_score"] = _lib.empty((F, K), dtype=torch.float64, device=dev)
    out["det_pose"] = _lib.empty((F, K, 4, 4), dtype=torch.float64, device=dev)
    out["n_det"] = _lib.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_detect_assign(
            F, K, C, P, ptr(counts.contiguous()), ptr(seg_total), ptr(valid), ptr(pose.contiguous()), ptr(n_components),
            int(mode), num, den, int(max_per_class), ptr(out["pair_hyp"]), ptr(out["pair_num"]), ptr(out["pair_den"]),
            ptr(out["pair_score"]), ptr(out["det_class"]), ptr(out["det_hyp"]), ptr(out["det_num"]), ptr(out["det_den"]),
            ptr(out["det_score"]), ptr(out["det_rank"]), ptr(out["det_pose"]), ptr(out["alt_class"]), ptr(out["alt_num"]),
            ptr(out["alt_den"]), ptr(out["n_det"]), stream()), "cloudaae_detect_assign")
    return out


def window_counts(segments, poses, meshes, mesh_of_class, intrinsics, depth, tau=0.01, margin=MARGIN,
                  samples_per_launch=SAMPLES_PER_LAUNCH, window=None, keep_depth=False):
    """The render-and-count half of score_candidates (its arguments): every hypothesis of a component the frame has,
    rendered alone into the component's window and counted there.  -> dict of counts [F,K,C,P,6], seg_total [F,K,C] int32,
    abs_sum [F,K,C,P] int64, dropped [F,K,C,P] int32, n_components [F] int32 (clamped to K) on the device -- zeros for a
    component the frame does not have -- and origin [F,K,2], wh, ww; with keep_depth also depth_hyp [F,K,C,P,wh,ww] int16.
    No read-back."""
    from . import mesh_models, render
    p = mesh_models.pack_meshes(meshes)
    dev = p.device
    dt = check_depth(depth, "depth", 3)
    F, H, W = (int(x) for x in dt.shape)
    require(isinstance(poses, torch.Tensor) and poses.dim() == 6 and poses.dtype == torch.float64 and
            tuple(poses.shape[4:]) == (4, 4) and int(poses.shape[0]) == F and min(poses.shape) >= 1 and poses.device == dev,
            "poses must be a float64 [F, K, C, P, 4, 4] tensor on the meshes' device")
    K, C, P = (int(x) for x in poses.shape[1:4])
    require(K <= MAX_K and C <= MAX_C and P <= MAX_P, "at most %d components, %d classes and %d hypotheses" % (MAX_K, MAX_C, MAX_P))
    poses = poses.contiguous()
    mesh = np.asarray(mesh_of_class.cpu() if isinstance(mesh_of_class, torch.Tensor) else mesh_of_class, np.int64).reshape(-1)
    require(len(mesh) == C and mesh.min() >= 0 and mesh.max() < len(p.num_triangles), "mesh_of_class must be [C], inside the meshes")
    intr_host = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, np.float32)
    require(intr_host.shape == (F, 5), "intrinsics must be [F, 5], one row per frame")
    label = segments.label
    require(tuple(label.shape) == (F, H, W) and label.device == dev, "segments must be those of depth, on the meshes' device")
    n_comp = np.minimum(np.asarray(segments.n_components, np.int64).reshape(-1), K)
    require(len(n_comp) == F and segments.comp_box.shape[1] >= int(n_comp.max()), "segments must hold F frames' components")
    if window is None:
        box = np.full((F, K, 4), -1, np.int64)
        kk = min(K, segments.comp_box.shape[1])
        box[:, :kk] = segments.comp_box[:, :kk]
        origin, wh, ww = windows(box, n_comp, H, W, margin)
    else:
        origin, wh, ww = np.ascontiguousarray(window[0], np.int32), int(window[1]), int(window[2])
        require(origin.shape == (F, K, 2) and wh >= 1 and ww >= 1, "window must be (origin [F, K, 2], wh, ww)")
    require(P * wh * ww <= (1 << 28), "one sample's hypothesis images are above 2^28 pixels")

    # the live samples (f K + k) C + c, k < n_components[f], and their per-sample inputs, uploaded once
    fk = np.array([f * K + k for f in range(F) for k in range(int(n_comp[f]))], np.int64)
    live = (fk[:, None] * C + np.arange(C)[None, :]).reshape(-1)
    B = F * K * C
    counts = torch.zeros((B, P, len(COUNTERS)), dtype=torch.int32, device=dev)
    seg_total = torch.zeros((B,), dtype=torch.int32, device=dev)
    abs_sum = torch.zeros((B, P), dtype=torch.int64, device=dev)
    dropped = torch.zeros((B, P), dtype=torch.int32, device=dev)
    kept = torch.zeros((B, P, wh, ww), dtype=torch.int16, device=dev) if keep_depth else None
    if len(live):
        f_of, k_of = live // (K * C), (live // C) % K
        o = origin[f_of, k_of]
        rows_host = intr_host[f_of].copy()
        rows_host[:, 2] = intr_host[f_of, 2] - o[:, 0].astype(np.float32)
        rows_host[:, 3] = intr_host[f_of, 3] - o[:, 1].astype(np.float32)
        tau_host = np.broadcast_to(np.asarray(tau, np.float64), (F,))
        tu = tau_units(tau_host, intr_host[:, 4].astype(np.float64))
        ints = torch.from_numpy(np.stack([f_of, k_of + 1, tu[f_of], o[:, 0], o[:, 1]], axis=1).astype(np.int32)).to(dev)
        frame_of, want, tau_dev, org = ints[:, 0].contiguous(), ints[:, 1].contiguous(), ints[:, 2].contiguous(), ints[:, 3:].contiguous()
        rows = torch.from_numpy(np.ascontiguousarray(rows_host)).to(dev)
        live_dev = torch.from_numpy(live).to(dev)
        flat = poses.view(B, P, 16)
        n = max(min(int(samples_per_launch), (1 << 28) // (P * wh * ww)), 1)
        for lo in range(0, len(live), n):
            hi = min(lo + n, len(live))
            c = hi - lo
            J = c * P
            d, _, _, rc, _ = render.render_instances(p, rows[lo:hi].repeat_interleave(P, dim=0).contiguous(), np.arange(J + 1),
                                                     np.repeat(mesh[live[lo:hi] % C], P), np.ones(J, np.int64),
                                                     flat.index_select(0, live_dev[lo:hi]).reshape(J, 16), wh, ww)
            part = fit_counts_window(dt, label, frame_of[lo:hi], want[lo:hi], org[lo:hi], d.view(c, P, wh, ww), tau_dev[lo:hi])
            counts.index_copy_(0, live_dev[lo:hi], part["counts"])
            seg_total.index_copy_(0, live_dev[lo:hi], part["seg_total"])
            abs_sum.index_copy_(0, live_dev[lo:hi], part["abs_sum"])
            dropped.index_copy_(0, live_dev[lo:hi], rc[0].view(c, P))
            if keep_depth:
                kept.index_copy_(0, live_dev[lo:hi], d.view(c, P, wh, ww))
    out = dict(counts=counts.view(F, K, C, P, 6), seg_total=seg_total.view(F, K, C), abs_sum=abs_sum.view(F, K, C, P),
               dropped=dropped.view(F, K, C, P), n_components=torch.from_numpy(n_comp.astype(np.int32)).to(dev), origin=origin,
               wh=wh, ww=ww)
    if keep_depth:
        out["depth_hyp"] = kept.view(F, K, C, P, wh, ww)
    return out


def score_candidates(segments, poses, valid, meshes, mesh_of_class, intrinsics, depth, tau=0.01, mode=MODE_SEGMENT,
                     margin=MARGIN, min_score=MIN_SCORE, max_per_class=MAX_PER_CLASS, samples_per_launch=SAMPLES_PER_LAUNCH,
                     window=None, keep_depth=False):
    """The detection table of given hypotheses.  segments: a DepthSegments of depth [F,H,W] (int16 bits or uint16, device)
    with intrinsics [F,5]; poses [F,K,C,P,4,4] float64 (model -> camera, device): P hypotheses for every one of the first
    K components of a frame and every one of C classes, valid [F,K,C,P] int32 or None; meshes a PackedMeshes (or what
    mesh_models.pack_meshes takes) and mesh_of_class [C] host integers.  Every hypothesis of a component the frame has is
    rendered alone into the component's window (windows(); window=(origin [F,K,2], wh, ww) overrides it) with the row
    (fx, fy, cx - u0, cy - v0, factor_depth), the differences formed in float32 on the host; counted there with label =
    segments.label, want = k + 1 and tau_units of its frame; samples_per_launch (component, class) samples per launch.
    Then cloudaae_detect_assign.  -> dict of assign()'s tensors, counts [F,K,C,P,6], seg_total [F,K,C] int32, abs_sum
    [F,K,C,P] int64 (device), origin, wh, ww, and from the one read-back at the end: table, a dict of numpy arrays
    (det_class, det_hyp, det_num, det_den, det_rank, alt_class, alt_num, alt_den [F,K], det_score [F,K], det_pose
    [F,K,4,4], n_det [F]) and dropped [F,K,C,P] int32 (numpy: the triangles the renderer left out).  keep_depth adds
    depth_hyp [F,K,C,P,wh,ww] int16 (device, zeros for a component the frame does not have): the rendered windows."""
    require(int(mode) in (MODE_SEGMENT, MODE_SILHOUETTE), "mode must be 0 (segment rule) or 1 (silhouette rule)")
    w = window_counts(segments, poses, meshes, mesh_of_class, intrinsics, depth, tau, margin, samples_per_launch, window, keep_depth)
    F, K, C, P = (int(x) for x in w["counts"].shape[:4])
    B, dropped = F * K * C, w.pop("dropped")
    out = assign(w["counts"], w["seg_total"], valid, poses.contiguous(), w.pop("n_components"), mode, min_score, max_per_class)
    out.update(w)
    # the one read-back: the integers of the table, the doubles as their bits, the renderer's dropped
    parts = [out[k].reshape(-1) for k in TABLE_INT] + [out["n_det"], dropped.reshape(-1),
                                                       out["det_score"].view(torch.int32).reshape(-1),
                                                       out["det_pose"].view(torch.int32).reshape(-1)]
    host = torch.cat(parts).cpu().numpy()
    table, at = {}, 0
    for k in TABLE_INT:
        table[k] = host[at:at + F * K].reshape(F, K).copy()
        at += F * K
    table["n_det"] = host[at:at + F].copy()
    at += F
    out["dropped"] = host[at:at + B * P].reshape(F, K, C, P).copy()
    at += B * P
    table["det_score"] = host[at:at + 2 * F * K].copy().view(np.float64).reshape(F, K)
    at += 2 * F * K
    table["det_pose"] = host[at:at + 32 * F * K].copy().view(np.float64).reshape(F, K, 4, 4)
    out["table"] = table
    return out


class Detections(object):
    """The result of detect_objects.  segments: the DepthSegments; classes [C]: the class id of column c; poses [F,K,C,P,4,4]
    float64 and valid [F,K,C,P] int32 (device): the candidates that were scored; scores: score_candidates' dict (device
    tensors, and scores['table'] on the host); table = scores['table'] with det_class holding CLASS IDS (classes[c], -1:
    none) and alt_class likewise; skipped: the components that had too few points to be a candidate; dropped [F,K,C,P]."""


def component_starts(seed, frame_index, n_in, n_f):
    """The two farthest-point-sampling starts of one component's cloud, from (seed, the frame's global index, the
    component's index) alone, so that a frame's clouds do not depend on the batch it arrives in."""
    out = []
    for k, (a, b) in enumerate(zip(n_in, n_f)):
        rng = np.random.default_rng([int(seed) % (1 << 32), int(frame_index), k])
        out.append((int(rng.integers(a)) if a > 0 else -1, int(rng.integers(b)) if b > 0 else -1))
    return out


def component_clouds(depth, segments, intrinsics, num_point=NUM_POINT, seed=0, first_frame=0):
    """The clouds of every found component through the unchanged extract_segments (label = the found label image,
    "class" = the component's index) and sample_segments.  -> (frame [S], comp [S] numpy, xyz [S,num_point,3] float32 on
    the device, enough [S] bool: at least num_point inliers), S = the components of the call in frame-major order; None
    when the call has no component."""
    from . import segment as seg_util
    n_comp = np.asarray(segments.n_components, np.int64).reshape(-1)
    if int(n_comp.sum()) == 0:
        return None
    r = seg_util.extract_segments(depth, segments.label, intrinsics, classes=[list(range(int(n))) for n in n_comp],
                                  device=segments.label.device)
    n_in, n_f = np.diff(r.inlier_offsets), r.num_point_after_filter
    s_in, s_f = [], []
    for f in range(len(n_comp)):
        sel = np.nonzero(r.frame == f)[0]
        for a, b in component_starts(seed, int(first_frame) + f, n_in[sel], n_f[sel]):
            s_in.append(a)
            s_f.append(b)
    smp = seg_util.sample_segments(r, int(num_point), starts=(s_in, s_f))
    return r.frame.astype(np.int64), r.cls.astype(np.int64), smp["xyz_inlier"], r.num_valid_points_in_segment >= int(num_point)


def detect_objects(depth, intrinsics, meshes, ppf_models, classes=None, segments=None, num_point=NUM_POINT, top=TOP, icp=None,
                   mesh_of_class=None, seed=0, first_frame=0, components=None, normal_radius=NORMAL_RADIUS, ref_step=5, peaks=2,
                   tau=0.01, mode=MODE_SEGMENT, margin=MARGIN, min_score=MIN_SCORE, max_per_class=MAX_PER_CLASS,
                   samples_per_launch=SAMPLES_PER_LAUNCH):
    """depth [F,H,W] uint16 (numpy, or a tensor holding the bits as int16) and intrinsics [F,5] float32 -> Detections.
    segment_depth(depth, intrinsics, seed=seed, first_frame=first_frame, **components) unless segments is given
    (components=dict(creases=True) cuts touching objects apart first, so that each gets a class of its own); the
    clouds of its components (component_clouds: num_point points; a component with fewer inliers is no candidate, valid 0,
    and counted in skipped); their normals (ppf.scene_normals(normal_radius)); ppf.propose_poses of ppf_models (a PPFModels)
    with every cloud repeated for each of classes (default: every class of ppf_models), top proposals each; with icp (the
    parameters of icp.refine_pose_icp, point to point; needs models of one size) every candidate is refined in one call;
    then score_candidates with meshes[mesh_of_class[c]] (default: the class id) for classes[c].  Frame f is treated as
    frame first_frame + f of a sequence, so its result does not depend on the batch it arrives in."""
    from . import depth_components as dc_util
    from . import icp as icp_util
    from . import mesh_models
    from . import ppf as ppf_util
    require(isinstance(ppf_models, ppf_util.PPFModels), "ppf_models must be a PPFModels")
    dev = ppf_models.device
    packed = mesh_models.pack_meshes(meshes, device=dev)
    classes = list(range(ppf_models.num_class)) if classes is None else [int(c) for c in classes]
    C, P = len(classes), int(top)
    require(1 <= C <= MAX_C and len(set(classes)) == C and min(classes) >= 0 and max(classes) < ppf_models.num_class,
            "classes must be distinct class ids of ppf_models")
    require(1 <= P <= MAX_P, "top must lie in [1, %d]" % MAX_P)
    mesh_of_class = classes if mesh_of_class is None else [int(m) for m in mesh_of_class]
    if segments is None:
        segments = dc_util.segment_depth(depth, intrinsics, seed=seed, first_frame=first_frame, device=dev, **(components or {}))
    d = upload_depth(depth, dev)
    F = int(d.shape[0])
    n_comp = np.asarray(segments.n_components, np.int64).reshape(-1)
    K = max(int(n_comp.max()), 1)
    poses = torch.eye(4, dtype=torch.float64, device=dev).repeat(F, K, C, P, 1, 1)
    valid = torch.zeros((F, K, C, P), dtype=torch.int32, device=dev)
    skipped = 0
    clouds = component_clouds(d, segments, intrinsics, num_point, seed, first_frame)
    if clouds is not None:
        frame, comp, xyz, enough = clouds
        skipped = int((~enough).sum())
        S = len(frame)
        scene = xyz.to(torch.float32).contiguous()
        normals, mask = ppf_util.scene_normals(scene, float(normal_radius))
        cls = torch.tensor(classes, dtype=torch.int64, device=dev).repeat(S)
        prop = ppf_util.propose_poses(ppf_models, scene.repeat_interleave(C, dim=0).contiguous(),
                                      normals.repeat_interleave(C, dim=0).contiguous(), mask.repeat_interleave(C, dim=0).contiguous(),
                                      cls, top=P, ref_step=int(ref_step), peaks=int(peaks))
        cand, ok = prop["pose"], prop["valid"] * torch.from_numpy(np.repeat(enough, C).astype(np.int32)).to(dev)[:, None]
        if icp is not None:
            sizes = ppf_models.sizes[classes]
            require(len(set(int(s) for s in sizes)) == 1 and int(sizes[0]) >= 1, "icp needs point models of one size for every class")
            first = torch.from_numpy(ppf_models.offsets_host[classes].astype(np.int64)).to(dev)
            rows = first[:, None] + torch.arange(int(sizes[0]), device=dev)[None, :]
            obj = ppf_models.xyz[rows.reshape(-1)].view(C, int(sizes[0]), 3).repeat(S, 1, 1)
            r = icp_util.refine_pose_icp(obj.repeat_interleave(P, dim=0).contiguous(),
                                         scene.repeat_interleave(C * P, dim=0).contiguous(),
                                         icp_util.to_float32(prop["rot_axag"]).view(S * C * P, 3),
                                         prop["trans"].contiguous().view(S * C * P, 3), **icp)
            cand = r["transformation"].view(S * C, P, 4, 4)
        at = torch.from_numpy(frame * K + comp).to(dev)
        poses.view(F * K, C, P, 4, 4).index_copy_(0, at, cand.reshape(S, C, P, 4, 4))
        valid.view(F * K, C, P).index_copy_(0, at, ok.reshape(S, C, P).to(torch.int32))
    scores = score_candidates(segments, poses, valid, packed, mesh_of_class, intrinsics, d, tau, mode, margin, min_score,
                              max_per_class, samples_per_launch)
    r = Detections()
    r.segments, r.classes, r.poses, r.valid, r.scores, r.skipped = segments, np.asarray(classes, np.int64), poses, valid, scores, skipped
    r.dropped = scores["dropped"]
    ids = np.concatenate([r.classes, [-1]])                  # column -> class id; -1 stays -1
    r.table = dict(scores["table"])
    r.table["det_class"] = ids[scores["table"]["det_class"]].astype(np.int32)
    r.table["alt_class"] = ids[scores["table"]["alt_class"]].astype(np.int32)
    return r
