"""Tracking: known objects followed from frame to frame of a depth sequence by dense depth-image alignment.  The object is
rendered at its predicted pose into a window around it (utils/render.py), every rendered pixel is paired with the depth the
camera saw at the same pixel, one point-to-plane step is solved from the pairs (cloudaae_depth_align_step;
csrc/depth_align.hip), that is repeated, and the result is judged by the windowed counts of "Detections"
(cloudaae_depth_fit_counts_window, the silhouette rule).  Neither a segmentation nor a pose proposal is needed once a pose
of the frame before is known.  The definition is in DESIGN.md ("Tracking").

    t = track_objects(depth, intrinsics, meshes, detections_of_frame_0)           # Tracks; t.poses [F,J,4,4], t.lost [F,J]
    a = align_poses(depth, intrinsics, meshes, mesh_of, frame_of, poses)          # poses refined against their frames

    python -m cloudaae_amd.utils.track --files REC_pcnn.tfrecord --meshes DIR [--mesh_scale S] [--motion velocity] [--contour]

contour=True on either call adds the occluding-contour term of DESIGN.md, "Contours" (csrc/depth_contour.hip): the rendered
object's occluding edges are pulled onto the nearest occluding edges of the frame, which holds flat and thin objects that
point-to-plane alone lets slide.  It is off by default.
"""
import argparse

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from . import detect, mesh_models, render
from .frame_inputs import check_depth, check_int32, depth_frames, host, intrinsics_per_frame, record_intrinsics
from .pose_verify import tau_units

# choices, not measurements
ITERATIONS = 4
GATE = 0.03               # |d - t| of a pair, metres
JUMP = 0.005              # a neighbour farther than this from its pixel takes no part in the slope, metres
COS_MIN = 0.8             # |n_hyp . n_obs| of a pair
MARGIN = 0.5              # of the projected bounding box, added on either side
MIN_SCORE = (1, 2)        # a track below this fraction is lost
TAU = 0.01                # of the lost-track score, metres
Z_NEAR = 0.05
# the contour term: choices too, backed by the CPU prototype's table ("Contours")
CONTOUR_RADIUS = 16       # pixels within which an observed occluding edge is looked for
CONTOUR_STEP = 0.02       # a neighbour farther behind than this (or empty) makes a pixel an occluding edge, metres
CONTOUR_WEIGHT = 1.0 / 16.0   # of the contour sums against the plane sums
MAX_RADIUS = 32

SUMS = 28


# ---- the binding ------------------------------------------------------------------------------------------------------------
def _window_inputs(depth_test, frame_of, origin, columns, depth_hyp=None, size=None, intr_win=None):
    """The window bindings' common inputs, checked: depth_test [F,H,W]; depth_hyp [B,wh,ww], or size = (wh, ww) with B from
    frame_of; frame_of and the columns ((name, tensor), ...) int32 [B]; origin int32 [B,2]; intr_win, when given, float32 [B,5];
    one device.  -> (dt, dh or None, (F, H, W, B, wh, ww), device, frame_of, origin, [columns])."""
    dt = check_depth(depth_test, "depth_test", 3)
    dev = dt.device
    if depth_hyp is not None:
        dh = check_depth(depth_hyp, "depth_hyp", 3)
        B, wh, ww = (int(v) for v in dh.shape)
        require(B >= 1 and wh >= 1 and ww >= 1, "depth_hyp must be [B, wh, ww], none of them 0")
        require(dh.device == dev, "all inputs must be on one device")
    else:
        require(isinstance(frame_of, torch.Tensor) and frame_of.dim() == 1 and frame_of.numel() >= 1, "frame_of must be [B], B >= 1")
        dh, B, wh, ww = None, int(frame_of.numel()), int(size[0]), int(size[1])
        require(wh >= 1 and ww >= 1, "wh and ww must be >= 1")
    frame_of = check_int32(frame_of, "frame_of", (B,), dev)
    columns = [check_int32(t, n, (B,), dev) for n, t in columns]
    origin = check_int32(origin, "origin", (B, 2), dev)
    if intr_win is not None:
        require(isinstance(intr_win, torch.Tensor) and intr_win.dtype == torch.float32 and tuple(intr_win.shape) == (B, 5) and
                intr_win.device == dev, "intr_win must be a float32 [B, 5] tensor on the inputs' device")
    return dt, dh, tuple(int(v) for v in dt.shape) + (B, wh, ww), dev, frame_of, origin, columns


def _pose_in(pose_in, B, dev):
    require(isinstance(pose_in, torch.Tensor) and pose_in.dtype == torch.float64 and pose_in.numel() == 16 * B and
            pose_in.device == dev, "pose_in must be a float64 [B, 4, 4] tensor on the inputs' device")
    return pose_in.contiguous()


def align_step(depth_test, frame_of, origin, depth_hyp, intr_win, gate, jump, cos_min, pose_in):
    """cloudaae_depth_align_step.  depth_test [F,H,W] and depth_hyp [B,wh,ww]: int16 tensors holding the uint16 bits, or
    uint16; frame_of [B] int32 (an entry outside [0, F) gives status 4 and reads nothing); origin [B,2] int32 = (u0, v0), any
    values; intr_win [B,5] float32: the windows' rows (fx, fy, cx - u0, cy - v0, factor_depth); gate, jump [B] int32 in depth
    units; cos_min a number (<= 0: no normal test); pose_in [B,4,4] float64.  All on one device.  -> dict of n_pairs [B]
    int32, sums [B,28], x [B,6] float64, status [B] int32 and pose_out [B,4,4] float64 on the device.  No read-back."""
    dt, dh, (F, H, W, B, wh, ww), dev, frame_of, origin, (gate, jump) = _window_inputs(
        depth_test, frame_of, origin, (("gate", gate), ("jump", jump)), depth_hyp=depth_hyp, intr_win=intr_win)
    pose_in = _pose_in(pose_in, B, dev)
    cos_min = float(cos_min)
    require(cos_min == cos_min, "cos_min must be a number")
    L = _lib.lib()
    nbytes = int(L.cloudaae_depth_align_step_workspace_bytes(B, wh, ww))
    require(nbytes > 0, "outside the limits: wh ww <= 2^24, B wh ww <= 2^28")
    out = dict(n_pairs=_lib.empty((B,), dtype=torch.int32, device=dev), sums=_lib.empty((B, SUMS), dtype=torch.float64, device=dev),
               x=_lib.empty((B, 6), dtype=torch.float64, device=dev), status=_lib.empty((B,), dtype=torch.int32, device=dev),
               pose_out=_lib.empty((B, 4, 4), dtype=torch.float64, device=dev))
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_depth_align_step(F, H, W, ptr(dt), B, ptr(frame_of), ptr(origin), wh, ww, ptr(dh),
                                               ptr(intr_win.contiguous()), ptr(gate), ptr(jump), cos_min, ptr(pose_in),
                                               ptr(out["n_pairs"]), ptr(out["sums"]), ptr(out["x"]), ptr(out["status"]),
                                               ptr(out["pose_out"]), ptr(ws), nbytes, stream()),
                   "cloudaae_depth_align_step")
    return out


# ---- the contour term ("Contours"; csrc/depth_contour.hip) -------------------------------------------------------
def _contour_settings(contour):
    """contour=None | True | dict(radius, step, weight) -> None or the full dict."""
    if contour is None or contour is False:
        return None
    c = dict(radius=CONTOUR_RADIUS, step=CONTOUR_STEP, weight=CONTOUR_WEIGHT)
    if contour is not True:
        require(isinstance(contour, dict) and set(contour) <= set(c), "contour must be None, True or a dict of radius, step, weight")
        c.update(contour)
    c["radius"], c["weight"] = int(c["radius"]), float(c["weight"])
    require(1 <= c["radius"] <= MAX_RADIUS, "contour radius must lie in [1, %d]" % MAX_RADIUS)
    require(c["weight"] == c["weight"], "contour weight must be a number")
    return c


def edge_nearest(depth_test, frame_of, origin, wh, ww, step, radius):
    """cloudaae_depth_edge_nearest.  depth_test [F,H,W], frame_of [B], origin [B,2] as for align_step; one wh, ww per call;
    step [B] int32 in depth units (device); 1 <= radius <= 32.  -> nearest [B,wh,ww] int32 on the device: -1, or (mask_obs <<
    16) | ((j + radius) << 8) | (i + radius) of the nearest observed occluding edge (u0 + x + i, v0 + y + j) of window pixel
    (x, y).  A sample whose frame_of lies outside [0, F) is all -1.  No read-back."""
    dt, _, (F, H, W, B, wh, ww), dev, frame_of, origin, (step,) = _window_inputs(depth_test, frame_of, origin, (("step", step),),
                                                                               size=(wh, ww))
    radius = int(radius)
    require(1 <= radius <= MAX_RADIUS, "radius must lie in [1, %d]" % MAX_RADIUS)
    nearest = _lib.empty((B, wh, ww), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_depth_edge_nearest(F, H, W, ptr(dt), B, ptr(frame_of), ptr(origin), wh, ww, ptr(step), radius,
                                                          ptr(nearest), stream()), "cloudaae_depth_edge_nearest")
    return nearest


def contour_sums(depth_test, frame_of, origin, depth_hyp, intr_win, gate, step, radius, nearest):
    """cloudaae_depth_contour_sums.  The arguments of align_step without jump and cos_min, plus step [B] int32 in depth units,
    the radius and the nearest [B,wh,ww] int32 of edge_nearest for the same frames, origins, step and radius.  -> dict of
    n_rows [B] int32 (two per contour pair) and sums [B,28] float64 in align_step's layout, on the device.  No read-back."""
    dt, dh, (F, H, W, B, wh, ww), dev, frame_of, origin, (gate, step) = _window_inputs(
        depth_test, frame_of, origin, (("gate", gate), ("step", step)), depth_hyp=depth_hyp, intr_win=intr_win)
    radius = int(radius)
    require(1 <= radius <= MAX_RADIUS, "radius must lie in [1, %d]" % MAX_RADIUS)
    nearest = check_int32(nearest, "nearest", (B, wh, ww), dev)
    L = _lib.lib()
    nbytes = int(L.cloudaae_depth_contour_sums_workspace_bytes(B, wh, ww))
    require(nbytes > 0, "outside the limits: wh ww <= 2^24, B wh ww <= 2^28")
    out = dict(n_rows=_lib.empty((B,), dtype=torch.int32, device=dev), sums=_lib.empty((B, SUMS), dtype=torch.float64, device=dev))
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_depth_contour_sums(F, H, W, ptr(dt), B, ptr(frame_of), ptr(origin), wh, ww, ptr(dh),
                                                 ptr(intr_win.contiguous()), ptr(gate), ptr(step), radius, ptr(nearest),
                                                 ptr(out["n_rows"]), ptr(out["sums"]), ptr(ws), nbytes, stream()),
                   "cloudaae_depth_contour_sums")
    return out


def solve_sums(plane, contour, weight, pose_in):
    """cloudaae_depth_align_solve.  plane: what align_step returned (its sums, n_pairs and status are read); contour: what
    contour_sums returned; weight a number; pose_in [B,4,4] float64, the pose both were formed at.  total = plane sums + weight
    x contour sums; status 4 where the plane step's is 4, else 1 where n_pairs + n_rows < 6, else align_step's solve on the
    totals.  -> dict of x [B,6], status [B] int32, pose_out [B,4,4] float64 on the device (pose_in bit for bit unless status
    is 0).  No read-back."""
    ps, dev = plane["sums"], plane["sums"].device
    B = int(ps.shape[0])
    require(ps.dtype == torch.float64 and tuple(ps.shape) == (B, SUMS) and B >= 1, "plane sums must be float64 [B, 28]")
    cs = contour["sums"]
    require(isinstance(cs, torch.Tensor) and cs.dtype == torch.float64 and tuple(cs.shape) == (B, SUMS) and cs.device == dev,
            "contour sums must be float64 [B, 28] on the plane sums' device")
    n_pairs, st, n_rows = (check_int32(t, n, (B,), dev) for t, n in ((plane["n_pairs"], "n_pairs"), (plane["status"], "status"),
                                                               (contour["n_rows"], "n_rows")))
    pose_in = _pose_in(pose_in, B, dev)
    weight = float(weight)
    require(weight == weight, "weight must be a number")
    out = dict(x=_lib.empty((B, 6), dtype=torch.float64, device=dev), status=_lib.empty((B,), dtype=torch.int32, device=dev),
               pose_out=_lib.empty((B, 4, 4), dtype=torch.float64, device=dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_depth_align_solve(B, ptr(ps.contiguous()), ptr(n_pairs), ptr(st), ptr(cs.contiguous()),
                                                         ptr(n_rows), weight, ptr(pose_in), ptr(out["x"]), ptr(out["status"]),
                                                         ptr(out["pose_out"]), stream()),
                   "cloudaae_depth_align_solve")
    return out


# ---- windows of posed bounding boxes (host) ---------------------------------------------------------------------------------
def mesh_aabb(packed):
    """[S,2,3] float64 (host): the smallest and the largest vertex coordinates of every mesh of a PackedMeshes; read back
    once per PackedMeshes and kept on it."""
    if getattr(packed, "aabb", None) is None:
        v = packed.vertices.cpu().numpy().astype(np.float64)
        at = np.concatenate([[0], np.cumsum(np.asarray(packed.num_vertices, np.int64))])
        packed.aabb = np.array([[v[a:b].min(axis=0), v[a:b].max(axis=0)] if b > a else np.zeros((2, 3))
                                for a, b in zip(at[:-1], at[1:])])
    return packed.aabb


def pose_windows(poses, aabb, intrinsics, H, W, margin=MARGIN, z_near=Z_NEAR):
    """One window size for the call and an origin per track, on the host.  poses [J,4,4] float64 (model -> camera), aabb
    [J,2,3]: the low and the high corner of each track's mesh, intrinsics [J,5] (or [5]): each track's frame.  The eight
    corners (x, y, z), each the low or the high coordinate, go through X = ((A0 x + A1 y) + A2 z) + A3 (Y, Z alike), u = (fx
    X) / Z + cx, v = (fy Y) / Z + cy in float64; a track with a corner that has Z < z_near, or a value that is not finite,
    gets no window; its box is (floor min u, floor min v, ceil max u, ceil max v) clipped to the frame, and an empty box is no
    window either.  Then detect.windows over the tracks that have one.  -> (origin [J,2] int32, zeros without a window; wh;
    ww; ok [J] bool)."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    J = len(poses)
    aabb = np.asarray(aabb, np.float64)
    require(aabb.shape == (J, 2, 3), "aabb must be [J, 2, 3], one box per pose")
    intr = np.broadcast_to(np.asarray(intrinsics, np.float32), (J, 5)).astype(np.float64)
    pick = np.array([[cx, cy, cz] for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)])
    c = aabb[:, pick, np.arange(3)[None, :]]                                       # [J,8,3]
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    A = poses[:, None]
    with np.errstate(all="ignore"):
        X = ((A[..., 0, 0] * x + A[..., 0, 1] * y) + A[..., 0, 2] * z) + A[..., 0, 3]
        Y = ((A[..., 1, 0] * x + A[..., 1, 1] * y) + A[..., 1, 2] * z) + A[..., 1, 3]
        Z = ((A[..., 2, 0] * x + A[..., 2, 1] * y) + A[..., 2, 2] * z) + A[..., 2, 3]
        u = (intr[:, None, 0] * X) / Z + intr[:, None, 2]
        v = (intr[:, None, 1] * Y) / Z + intr[:, None, 3]
        ok = np.all((Z >= float(z_near)) & np.isfinite(Z) & np.isfinite(u) & np.isfinite(v), axis=1)
        u, v = np.where(ok[:, None], u, 0.0), np.where(ok[:, None], v, 0.0)
        box = np.stack([np.maximum(np.clip(np.floor(u.min(axis=1)), -1, W), 0), np.maximum(np.clip(np.floor(v.min(axis=1)), -1, H), 0),
                        np.minimum(np.clip(np.ceil(u.max(axis=1)), -1, W), W - 1),
                        np.minimum(np.clip(np.ceil(v.max(axis=1)), -1, H), H - 1)], axis=1).astype(np.int64)
    ok &= (box[:, 0] <= box[:, 2]) & (box[:, 1] <= box[:, 3])
    live = np.nonzero(ok)[0]
    packed = np.zeros((1, max(len(live), 1), 4), np.int64)
    packed[0, :len(live)] = box[live]
    o, wh, ww = detect.windows(packed, [len(live)], H, W, margin)
    origin = np.zeros((J, 2), np.int32)
    origin[live] = o[0, :len(live)]
    return origin, wh, ww, ok


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def align_windows(dev, dt, intr_host, frame_of, aabb, poses, hypothesis, iterations=ITERATIONS, gate=GATE, jump=JUMP, cos_min=COS_MIN,
                  margin=MARGIN, window=None, return_trajectory=False, contour=None, on_step=None):
    """The alignment loop: J poses refined against their frames.  Its one parameter is the hypothesis source: hypothesis(pose
    [J,4,4] float64, rows [J,5] float32, both on the device, wh, ww) -> depth [J,wh,ww], the object seen under each pose in
    its window (the meshes' renderer for align_poses, the raycast of a volume for scan.scan_object).  dt: the depth frames
    [F,H,W] on `dev`; intr_host [F,5] float32 and frame_of [J] on the host; aabb [J,2,3]: the box each window is taken of;
    poses [J,4,4] float64 (host; a device tensor costs one read-back for the windows unless window is given).  The window
    (pose_windows of the given poses; window=(origin [J,2], wh, ww) overrides it) is fixed over the iterations; gate and jump
    in metres become depth units by tau_units of the track's frame.  Per iteration: one hypothesis call for all tracks (the
    windows' rows) and one align_step; nothing is read back inside the loop.  contour=True or dict(radius=16, step=0.02,
    weight=1/16) adds the occluding-contour term ("Contours"): one edge_nearest call before the loop (step in
    metres becomes units like the gates) and per iteration, after the align_step, one contour_sums and one solve_sums, whose
    pose and status replace the step's; n_pairs stays the plane pairs'.  With contour=None nothing of that is called.  A
    track without a window is given frame_of -1: status 4, its pose unchanged.  on_step(dict(pose_in, depth_hyp, pose_out,
    n_pairs, status: device tensors; origin, wh, ww, rows, frame_of: host)) is called after every step.  -> dict of poses
    [J,4,4] float64, n_pairs and status [J] int32 of the last step (device), origin [J,2], wh, ww, ok [J] (host), device:
    dict(depth, frame_of, origin, rows) as the bindings take them; with return_trajectory also trajectory [iterations +
    1,J,4,4]: the pose before every step and after the last, and n_pairs_steps, status_steps [iterations,J] (device)."""
    F, H, W = (int(v) for v in dt.shape)
    fo = np.asarray(frame_of, np.int64).reshape(-1)
    J = len(fo)
    require(fo.min() >= 0 and fo.max() < F, "frame_of must lie in [0, F)")
    require(intr_host.shape == (F, 5), "intrinsics must be [F, 5], one row per frame")
    require(int(iterations) >= 0, "iterations must be >= 0")
    pose_dev = (poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, np.float64))).to(dev)
    require(pose_dev.dtype == torch.float64 and pose_dev.numel() == 16 * J, "poses must be float64 [J, 4, 4]")
    pose_dev = pose_dev.reshape(J, 4, 4).contiguous()
    if window is None:
        origin, wh, ww, ok = pose_windows(host(poses, np.float64), aabb, intr_host[fo], H, W, margin)
    else:
        origin, wh, ww = np.ascontiguousarray(window[0], np.int32), int(window[1]), int(window[2])
        require(origin.shape == (J, 2) and wh >= 1 and ww >= 1, "window must be (origin [J, 2], wh, ww)")
        ok = np.ones(J, bool)
    rows_host = intr_host[fo].copy()
    rows_host[:, 2] = intr_host[fo, 2] - origin[:, 0].astype(np.float32)
    rows_host[:, 3] = intr_host[fo, 3] - origin[:, 1].astype(np.float32)
    factor = intr_host[fo, 4].astype(np.float64)
    gu, ju = tau_units(np.broadcast_to(np.asarray(gate, np.float64), (J,)), factor), \
        tau_units(np.broadcast_to(np.asarray(jump, np.float64), (J,)), factor)
    con = _contour_settings(contour)
    frame_host = np.where(ok, fo, -1)
    cols = [frame_host, gu, ju, origin[:, 0], origin[:, 1]]
    if con:                                                # the edge step rides along in the one upload of the integers
        cols.append(tau_units(np.broadcast_to(np.asarray(con["step"], np.float64), (J,)), factor))
    ints = torch.from_numpy(np.stack(cols, axis=1).astype(np.int32)).to(dev)
    frame_dev, gate_dev, jump_dev, org = (ints[:, 0].contiguous(), ints[:, 1].contiguous(), ints[:, 2].contiguous(),
                                          ints[:, 3:5].contiguous())
    rows = torch.from_numpy(np.ascontiguousarray(rows_host)).to(dev)
    if con and int(iterations) > 0:
        step_dev = ints[:, 5].contiguous()
        near = edge_nearest(dt, frame_dev, org, wh, ww, step_dev, con["radius"])
    traj, n_steps, s_steps = [pose_dev], [], []
    n_pairs = torch.zeros((J,), dtype=torch.int32, device=dev)
    status = torch.zeros((J,), dtype=torch.int32, device=dev)
    for _ in range(int(iterations)):
        d = hypothesis(traj[-1], rows, wh, ww)
        r = align_step(dt, frame_dev, org, d, rows, gate_dev, jump_dev, cos_min, traj[-1])
        n_pairs = r["n_pairs"]
        if con:
            c = contour_sums(dt, frame_dev, org, d, rows, gate_dev, step_dev, con["radius"], near)
            r = solve_sums(r, c, con["weight"], traj[-1])
        status = r["status"]
        if on_step is not None:
            on_step(dict(pose_in=traj[-1], depth_hyp=d, pose_out=r["pose_out"], n_pairs=n_pairs, status=status, origin=origin, wh=wh,
                         ww=ww, rows=rows_host, frame_of=frame_host))
        if return_trajectory:
            traj.append(r["pose_out"])
            n_steps.append(n_pairs)
            s_steps.append(status)
        else:
            traj = [r["pose_out"]]
    out = dict(poses=traj[-1], n_pairs=n_pairs, status=status, origin=origin, wh=wh, ww=ww, ok=ok,
               device=dict(depth=dt, frame_of=frame_dev, origin=org, rows=rows))
    if return_trajectory:
        out["trajectory"] = torch.stack(traj)
        out["n_pairs_steps"] = torch.stack(n_steps) if n_steps else torch.zeros((0, J), dtype=torch.int32, device=dev)
        out["status_steps"] = torch.stack(s_steps) if s_steps else torch.zeros((0, J), dtype=torch.int32, device=dev)
    return out


def _mesh_source(p, mesh):
    """What known objects give the loop: the boxes [J,2,3] of the meshes mesh [J] of the PackedMeshes p, and the hypothesis
    source that draws each alone into its window (one render.render_instances call, H = wh, W = ww, the windows' rows)."""
    require(mesh.min() >= 0 and mesh.max() < len(p.num_triangles), "mesh_of must lie inside the meshes")
    J = len(mesh)
    offs, ones = np.arange(J + 1), np.ones(J, np.int64)
    return mesh_aabb(p)[mesh], lambda pose, rows, wh, ww: render.render_instances(p, rows, offs, mesh, ones, pose.view(J, 16), wh, ww)[0]


def align_poses(depth, intrinsics, meshes, mesh_of, frame_of, poses, iterations=ITERATIONS, gate=GATE, jump=JUMP, cos_min=COS_MIN,
                margin=MARGIN, window=None, return_trajectory=False, contour=None):
    """J poses refined against their frames: align_windows (its keywords and its result, device with packed: the
    PackedMeshes) with the meshes' renderer as hypothesis source -- one render.render_instances call for all tracks, H = wh, W
    = ww -- and mesh_aabb as the windows' boxes.  depth [F,H,W] uint16 (numpy, or a device tensor holding the bits as int16),
    intrinsics [F,5] float32 (host), meshes a PackedMeshes (or what mesh_models.pack_meshes takes), mesh_of and frame_of [J]
    host integers, poses [J,4,4] float64."""
    p = mesh_models.pack_meshes(meshes)
    dt = depth_frames(depth, p.device)
    mesh, fo = np.asarray(mesh_of, np.int64).reshape(-1), np.asarray(frame_of, np.int64).reshape(-1)
    require(len(mesh) >= 1 and len(fo) == len(mesh), "mesh_of and frame_of must be [J], J >= 1")
    aabb, renderer = _mesh_source(p, mesh)
    out = align_windows(p.device, dt, host(intrinsics, np.float32), fo, aabb, poses, renderer, iterations, gate, jump, cos_min, margin,
                        window, return_trajectory, contour)
    out["device"]["packed"] = p
    return out


def frame_attempt(dev, dt, intr_host, f, aabb, start, hypothesis, tau_u, min_score, label=None, want=None, **align):
    """One frame's attempt for n tracks, what tracking and scanning share: align_windows(**align) in frame f from the starts
    [n,4,4] (host), one more hypothesis at the result in the same window, detect.fit_counts_window of it (tau_u in depth
    units; label [F,H,W] uint8 with want [n] int32 on the device, or neither), one read-back -- the poses as their bits, the
    counters, the last step's pairs and status -- and the silhouette rule: (num, den) = (consistent, consistent + in_front +
    behind), 0 / 1 for den = 0; lost when num min_den < min_num den in integers, min_score = (min_num, min_den), or without
    a window.  -> (pose [n,4,4], num, den, n_pairs, status, lost [n] on the host, the poses on the device)."""
    a = align_windows(dev, dt, intr_host, np.full(len(start), f), aabb, start, hypothesis, **align)
    return score_attempt(dev, dt, a, hypothesis, tau_u, min_score, label, want)


def score_attempt(dev, dt, a, hypothesis, tau_u, min_score, label=None, want=None):
    """The second half of frame_attempt, for a loop that takes its steps otherwise (scan.scan_object with align='sdf'): a is
    what align_windows returned, with poses, n_pairs and status those of the steps taken.  -> what frame_attempt returns."""
    n = int(a["poses"].shape[0])
    dv = a["device"]
    d = hypothesis(a["poses"], dv["rows"], a["wh"], a["ww"])
    tau_dev = torch.full((n,), int(tau_u), dtype=torch.int32, device=dev)
    c = detect.fit_counts_window(dt, label, dv["frame_of"], want, dv["origin"], d.view(n, 1, a["wh"], a["ww"]), tau_dev)
    got = torch.cat([a["poses"].contiguous().view(torch.int32).reshape(-1), c["counts"].reshape(-1), a["n_pairs"],
                     a["status"]]).cpu().numpy()
    pose = got[:32 * n].copy().view(np.float64).reshape(n, 4, 4)
    counts = got[32 * n:38 * n].reshape(n, 6).astype(np.int64)
    num, den = counts[:, 1].copy(), counts[:, 1] + counts[:, 2] + counts[:, 3]
    num, den = np.where(den > 0, num, 0), np.where(den > 0, den, 1)
    lost = ~a["ok"] | (num * int(min_score[1]) < int(min_score[0]) * den)
    return pose, num, den, got[38 * n:39 * n], got[39 * n:40 * n], lost, a["poses"]


# ---- tracking ---------------------------------------------------------------------------------------------------------------
class Tracks(object):
    """The result of track_objects.  mesh_of [J]; poses [F,J,4,4] float64: the pose of every track in every frame (a lost
    track keeps its last good pose); num, den [F,J]: the silhouette rule's fraction of the frame's attempt; n_pairs, status
    [F,J]: of the attempt's last step; lost [F,J] bool; first_frame: the global index of frame 0.  All numpy."""


def _compose(U, T):
    """U T with the products of cloudaae_pose_compose (host float64)."""
    N = np.eye(4)
    for i in range(3):
        for c in range(3):
            N[i, c] = (U[i, 0] * T[0, c] + U[i, 1] * T[1, c]) + U[i, 2] * T[2, c]
        N[i, 3] = ((U[i, 0] * T[0, 3] + U[i, 1] * T[1, 3]) + U[i, 2] * T[2, 3]) + U[i, 3]
    return N


def _invert(T):
    """(R^T, -R^T t) of a rigid T."""
    N = np.eye(4)
    for i in range(3):
        N[i, :3] = T[:3, i]
        N[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return N


def predict(last, before, motion):
    """The start of a frame: the last pose, or with 'velocity' (T_{f-1} T_{f-2}^-1) T_{f-1} once two poses exist."""
    if motion == "velocity" and before is not None:
        return _compose(_compose(last, _invert(before)), last)
    return last.copy()


def _initial_tracks(init):
    if isinstance(init, detect.Detections):
        cls, pose = np.asarray(init.table["det_class"])[0], np.asarray(init.table["det_pose"], np.float64)[0]
        keep = np.nonzero(cls >= 0)[0]
        return cls[keep].astype(np.int64), pose[keep].copy()
    require(isinstance(init, (tuple, list)) and len(init) == 2, "init must be a Detections or (mesh_of [J], poses [J, 4, 4])")
    mesh = np.asarray(init[0], np.int64).reshape(-1)
    return mesh, host(init[1], np.float64).reshape(len(mesh), 4, 4).copy()


def track_objects(depth, intrinsics, meshes, init, motion="constant", min_score=MIN_SCORE, tau=TAU, on_lost=None, first_frame=0,
                  contour=None, **align):
    """Known objects followed through depth [F,H,W] uint16 (numpy, or a device tensor holding the bits as int16) with
    intrinsics [F,5] (or [5]) float32.  init: a Detections of frame 0 -- its assigned components become the tracks, mesh =
    the class id, as detect_objects assumes by default -- or (mesh_of [J], poses [J,4,4]).  Frames are taken in order, frame
    0 included.  The start of a frame is the track's last pose, or with motion='velocity' (T_{f-1} T_{f-2}^-1) T_{f-1} once
    two poses exist.  Each frame is one frame_attempt with the meshes' renderer: the loop of align_poses(**align) from the
    starts, the result rendered into the same window and counted with detect.fit_counts_window without a label (tau in
    metres); the score is the silhouette rule's (num, den) = (consistent, consistent + in_front + behind), 0 / 1 for den = 0.
    A track is lost in frame f when num min_den < min_num
    den, in integers, or when it has no window; it keeps its last good pose and is tried again from it, at rest, in the next
    frame.  on_lost(f, track_indices), called when tracks are lost, may return new poses [len(track_indices),4,4] (or None):
    they are aligned and scored in the same frame -- the hook to hang detect_objects(depth[f:f+1], ..., first_frame =
    first_frame + f) on.  contour (None, True or dict(radius, step, weight)) is align_poses': the occluding-contour term that
    holds flat and thin objects, off by default.  One read-back per frame (one more when on_lost gives poses).  -> Tracks."""
    require(motion in ("constant", "velocity"), "motion must be 'constant' or 'velocity'")
    num_min, den_min = int(min_score[0]), int(min_score[1])
    require(0 <= num_min <= den_min and den_min >= 1, "min_score must be (num, den) with 0 <= num <= den, den >= 1")
    p = mesh_models.pack_meshes(meshes)
    dev = p.device
    dt = depth_frames(depth, dev)
    F = int(dt.shape[0])
    intr = intrinsics_per_frame(intrinsics, F)
    mesh_of, last = _initial_tracks(init)
    J = len(mesh_of)
    require(J >= 1, "no track to follow")
    tau_frame = tau_units(np.broadcast_to(np.asarray(tau, np.float64), (F,)), intr[:, 4].astype(np.float64))
    before = [None] * J
    t = Tracks()
    t.mesh_of, t.first_frame = mesh_of, int(first_frame)
    t.poses = np.zeros((F, J, 4, 4))
    t.num, t.den = np.zeros((F, J), np.int64), np.ones((F, J), np.int64)
    t.n_pairs, t.status, t.lost = np.zeros((F, J), np.int32), np.zeros((F, J), np.int32), np.zeros((F, J), bool)

    def attempt(f, idx, start):
        aabb, renderer = _mesh_source(p, mesh_of[idx])
        return frame_attempt(dev, dt, intr, f, aabb, start, renderer, tau_frame[f], (num_min, den_min), contour=contour, **align)[:6]

    for f in range(F):
        idx = np.arange(J)
        start = np.array([predict(last[j], before[j], motion) for j in idx])
        pose, num, den, n_pairs, status, lost = attempt(f, idx, start)
        if lost.any() and on_lost is not None:
            again = np.nonzero(lost)[0]
            given = on_lost(f, again.copy())
            if given is not None:
                given = host(given, np.float64).reshape(len(again), 4, 4)
                pose[again], num[again], den[again], n_pairs[again], status[again], lost[again] = attempt(f, again, given)
        for j in idx:
            if lost[j]:
                before[j] = None
            else:
                before[j], last[j] = last[j].copy(), pose[j]
        t.poses[f], t.num[f], t.den[f], t.n_pairs[f], t.status[f], t.lost[f] = last, num, den, n_pairs, status, lost
    return t


# ---- command line -----------------------------------------------------------------------------------------------------------
def quat2mat(q):
    """The rotation matrix of a quaternion (w, x, y, z), normalised first, float64."""
    w, x, y, z = np.asarray(q, np.float64) / np.sqrt((np.asarray(q, np.float64) ** 2).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def record_poses(fr, classes):
    """The poses that the frame record fr holds for `classes`, model -> camera: [len(classes),4,4] float64."""
    out = np.tile(np.eye(4), (len(classes), 1, 1))
    for i, c in enumerate(classes):
        out[i, :3, :3], out[i, :3, 3] = quat2mat(fr["quaternions"][c]), fr["translations"][c]
    return out


def pose_errors(T, truth):
    """(rotation error in degrees, translation error in metres) of T against truth."""
    c = (np.trace(T[:3, :3] @ truth[:3, :3].T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(min(max(c, -1.0), 1.0)))), float(np.sqrt(((T[:3, 3] - truth[:3, 3]) ** 2).sum()))


def main(argv=None):
    parser = argparse.ArgumentParser(description="track the objects of a <seq>_pcnn.tfrecord from its first frame's poses")
    parser.add_argument("--files", required=True, help="one <seq>_pcnn.tfrecord; its frames are taken in file order")
    parser.add_argument("--meshes", required=True, help="directory of *.ply files; class i is the i-th in sorted order")
    parser.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the coordinates (0.001: millimetres to metres)")
    parser.add_argument("--motion", choices=["constant", "velocity"], default="constant")
    parser.add_argument("--iterations", type=int, default=ITERATIONS)
    parser.add_argument("--contour", action="store_true", help="add the occluding-contour term at its defaults (flat and thin objects)")
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    from .. import tfrecord_io
    from . import mesh_models
    torch.cuda.set_device(args.gpu)
    frames = list(tfrecord_io.read_frames(args.files))
    require(len(frames) >= 1, "no frame in %s" % args.files)
    packed = mesh_models.pack_meshes(mesh_models.mesh_files(args.meshes), args.mesh_scale)
    classes = [int(c) for c in np.nonzero(frames[0]["class_one_hot"])[0] if c < len(packed.num_triangles)]
    require(len(classes) >= 1, "the first frame names no class that has a mesh")

    depth = np.stack([fr["depth"] for fr in frames])
    t = track_objects(depth, record_intrinsics(frames), packed, (classes, record_poses(frames[0], classes)), motion=args.motion,
                      iterations=args.iterations, contour=True if args.contour else None)
    for f, fr in enumerate(frames):
        gt = record_poses(fr, classes)
        for i, c in enumerate(classes):
            here = bool(fr["class_one_hot"][c])
            rot, trans = pose_errors(t.poses[f, i], gt[i]) if here else (float("nan"), float("nan"))
            print("frame %d class %d score %d/%d lost %d rot_err_deg %.4f trans_err_m %.6f"
                  % (int(fr["frame_id"]), c, t.num[f, i], t.den[f, i], int(t.lost[f, i]), rot, trans))
    print("%d frames, %d tracks, %d lost track-frames" % (len(frames), len(classes), int(t.lost.sum())))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
