"""Scanning: an object that has no CAD model and no known poses is followed through a depth sequence and fused as it goes.
Each new frame is aligned against the volume fused so far -- the volume is raycast into a depth window at the current pose
(cloudaae_tsdf_raycast; csrc/tsdf.hip), track.align_step solves a point-to-plane step between that window and the frame, that
is repeated -- the result is judged by the windowed counts of "Detections" under the silhouette rule, and a frame that is not
lost is summed into the volume at its pose (fuse.integrate).  Frame 0 defines the object's frame.  The definition is in
DESIGN.md ("Scanning").  align='sdf' (experimental, opt-in) takes the steps on the volume's signed distance field instead:
every observed pixel reads the field's value as its residual and its gradient as its normal (cloudaae_tsdf_align_step;
csrc/tsdf_align.hip; DESIGN.md, "Scanning on the field"), with no raycast inside the iterations.

    s = scan_object(depth, intrinsics, 0.002)                       # Scan; s.poses [F,4,4], s.lost [F], s.volume
    vertices, triangles = s.mesh()                                  # what mesh_models.pack_meshes takes as a mesh
    d = raycast(volume, poses, intr_win, wh, ww)                    # [B,wh,ww]: the volume seen from B poses
    s = scan_object(depth, intrinsics, 0.002, align='sdf')          # the steps on the field, no raycast inside them
    pose, x, n, st = align_volume_step(volume, depth, intr_win, poses, frame_of, origin, wh, ww)    # one such step

    python -m cloudaae_amd.utils.scan --files REC_pcnn.tfrecord --target_cls C --voxel 0.002 --out model.ply [--every N]
        [--motion velocity] [--simplify METRES] [--align sdf]
"""
import argparse

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from . import fuse, render, track
from .frame_inputs import check_int32, check_poses, depth_frames, host, intrinsics_per_frame, on_device
from .pose_verify import tau_units

# a choice, not a measurement
STEP_VOXELS = 0.5         # the march's step along the camera depth, in voxels
GROW = 0.5                # of the first frame's largest side, added to its box on every side


# ---- the binding ------------------------------------------------------------------------------------------------------------
def raycast(volume, poses, intr_win, wh, ww, step=None, min_count=1, z_near=render.Z_NEAR):
    """cloudaae_tsdf_raycast.  volume a fuse.Volume; poses [B,4,4] float64, model -> camera; intr_win [B,5] float32: the
    windows' rows (fx, fy, cx - u0, cy - v0, factor_depth), both device tensors (or numpy, uploaded); step in metres of camera
    depth (default 0.5 voxel).  -> depth [B,wh,ww]: a device int16 tensor holding the uint16 bits, as the renderer returns;
    0 where the ray meets no surface from known outside.  No read-back."""
    require(isinstance(volume, fuse.Volume), "volume must be a Volume")
    dev = volume.device
    pose, rows = on_device(poses, torch.float64, dev), on_device(intr_win, torch.float32, dev)
    require(pose.dim() == 3 and tuple(pose.shape[1:]) == (4, 4) and int(pose.shape[0]) >= 1, "poses must be [B, 4, 4], B >= 1")
    B, wh, ww = int(pose.shape[0]), int(wh), int(ww)
    require(tuple(rows.shape) == (B, 5), "intr_win must be [B, 5]")
    require(wh >= 1 and ww >= 1 and wh * ww <= (1 << 24) and B * wh * ww <= (1 << 28), "outside the limits: wh ww <= 2^24, B wh ww <= 2^28")
    step = STEP_VOXELS * volume.voxel if step is None else float(step)
    nx, ny, nz = volume.dims
    ox, oy, oz = volume.origin
    out = _lib.empty((B, wh, ww), dtype=torch.int16, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_tsdf_raycast(nx, ny, nz, ox, oy, oz, volume.voxel, ptr(volume.state), int(min_count), B, wh, ww,
                                                    ptr(rows), ptr(pose), step, float(z_near), ptr(out), stream()),
                   "cloudaae_tsdf_raycast")
    return out


def align_volume_step(volume, depth, intr_win, poses, frame_of, origin, wh, ww, label=None, want=None, front=None, min_count=1):
    """cloudaae_tsdf_align_step: one Gauss-Newton step of B poses on the volume's signed distance field.  volume a
    fuse.Volume; depth [F,H,W]: an int16 tensor holding the uint16 bits, or uint16 (numpy is uploaded); intr_win [B,5] float32:
    the windows' rows (fx, fy, cx - u0, cy - v0, factor_depth) and poses [B,4,4] float64, model -> camera, device tensors (or
    numpy, uploaded); frame_of [B] int32 (an entry outside [0, F) gives status 4 and reads nothing) and origin [B,2] int32 =
    (u0, v0), any values, device tensors; one wh, ww per call; label [F,H,W] uint8 with want [F] int32 on the device, or
    neither, as fuse.integrate takes them; front in metres: what the field's 4096 stands for, the front the volume was
    integrated with (default 4 voxels).  -> (pose_out [B,4,4] float64, x [B,6] float64, n_pairs [B] int32, status [B] int32)
    on the device; status as track.align_step's.  No read-back."""
    require(isinstance(volume, fuse.Volume), "volume must be a Volume")
    dev = volume.device
    dt = depth_frames(depth, dev)
    require(dt.device == dev, "all inputs must be on the volume's device")
    F, H, W = (int(v) for v in dt.shape)
    pose = on_device(poses, torch.float64, dev)
    require(pose.dim() == 3 and int(pose.shape[0]) >= 1, "poses must be [B, 4, 4], B >= 1")
    B, wh, ww = int(pose.shape[0]), int(wh), int(ww)
    pose = check_poses(pose, "poses", (3,), B, dev)
    rows = on_device(intr_win, torch.float32, dev, (B, 5), "intr_win")
    frame_of, origin = check_int32(frame_of, "frame_of", (B,), dev), check_int32(origin, "origin", (B, 2), dev)
    require((label is None) == (want is None), "label and want come together")
    if label is not None:
        require(isinstance(label, torch.Tensor) and label.dtype == torch.uint8 and tuple(label.shape) == (F, H, W) and
                label.device == dev, "label must be a uint8 [F, H, W] tensor on the volume's device")
        label, want = label.contiguous(), check_int32(want, "want", (F,), dev)
    front = fuse.FRONT_VOXELS * volume.voxel if front is None else float(front)
    L = _lib.lib()
    nbytes = int(L.cloudaae_tsdf_align_step_workspace(B, wh, ww))
    require(nbytes > 0, "outside the limits: wh, ww >= 1, wh ww <= 2^24, B wh ww <= 2^28")
    pose_out, x = _lib.empty((B, 4, 4), dtype=torch.float64, device=dev), _lib.empty((B, 6), dtype=torch.float64, device=dev)
    n_pairs, status = _lib.empty((B,), dtype=torch.int32, device=dev), _lib.empty((B,), dtype=torch.int32, device=dev)
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    nx, ny, nz = volume.dims
    ox, oy, oz = volume.origin
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_tsdf_align_step(nx, ny, nz, ox, oy, oz, volume.voxel, ptr(volume.state), int(min_count), front, F, H, W,
                                              ptr(dt), ptr(label), ptr(want), B, ptr(frame_of), ptr(origin), wh, ww, ptr(rows),
                                              ptr(pose), ptr(n_pairs), ptr(x), ptr(status), ptr(pose_out), ptr(ws), nbytes,
                                              stream()), "cloudaae_tsdf_align_step")
    return pose_out, x, n_pairs, status


# ---- the loop ---------------------------------------------------------------------------------------------------------------
class Scan(object):
    """The result of scan_object.  poses [F,4,4] float64: the object's pose in every frame, model -> camera (a lost frame
    keeps the last good pose); num, den [F]: the silhouette rule's fraction of the frame's attempt (0 / 1 for frame 0);
    n_pairs, status [F]: of the attempt's last step; lost [F] bool, all numpy; volume: the fuse.Volume, on the device."""

    def mesh(self, simplify=None):
        """fuse.extract_mesh(volume, min_count, simplify) -> (vertices [V,3] float32, triangles [T,3] int32) on the device;
        simplify: a cell side in metres, or None for the mesh as cut."""
        return fuse.extract_mesh(self.volume, self.min_count, simplify)


def _first_pose(dt, lab, intr, want):
    """No rotation; the translation is the centre of the used pixels' box in the camera's frame (one read-back)."""
    eye = torch.eye(4, dtype=torch.float64, device=dt.device).unsqueeze(0)
    box = fuse.used_points_aabb(dt[:1], None if lab is None else lab[:1], intr[:1], eye, None if lab is None else want[:1])
    T = np.eye(4)
    T[:3, 3] = (box[0] + box[1]) / 2.0
    return T


def scan_object(depth, intrinsics, voxel, label=None, want=None, first_pose=None, aabb=None, grow=GROW, motion="constant",
                iterations=track.ITERATIONS, gate=track.GATE, jump=track.JUMP, cos_min=track.COS_MIN, margin=track.MARGIN,
                min_score=track.MIN_SCORE, tau=track.TAU, min_count=1, front=None, behind=None, step=None, on_frame=None, on_step=None,
                align="raycast"):
    """An unknown object followed through depth [F,H,W] uint16 (numpy, or a device tensor holding the bits as int16) with
    intrinsics [F,5] (or [5]) float32, and fused into a volume of `voxel` metres.  label [F,H,W] uint8 with want [F] (or one
    number) restricts the integration as in fuse.integrate and is handed to the counts.  Frame 0 defines the object's frame:
    first_pose (model -> camera; default no rotation and the centre of the used pixels' box) and aabb [2,3], the object's
    extent in that frame (default fuse.used_points_aabb of frame 0 grown on every side by `grow` times its largest side: one
    view sees only the front); the volume is fuse.volume_for(aabb, voxel) and is not resized later.  Frame 0 is integrated at
    first_pose.  Every later frame starts from the last pose (motion='velocity': track.predict) and is one track.frame_attempt
    with the raycast of the volume as hypothesis source, the box as the window's box and the label handed to the counts:
    `iterations` times raycast + track.align_step in the window of the start, one more raycast at the final pose, counted
    with detect.fit_counts_window (tau in metres); the score is the silhouette rule's, and the frame is lost when num
    min_den < min_num den or it has no window, as in track_objects.  A frame that is not lost is integrated at its pose;
    a lost one is not, the pose stays at the last good one and the next frame starts from it at rest.  Nothing is read back
    inside the iterations; one read-back per frame.  step: the raycast's, metres (default 0.5 voxel).  Two hooks for tests and
    tools: on_step(f, dict(pose_in, depth_hyp, pose_out, n_pairs, status: device tensors; origin, wh, ww, rows, frame_of:
    host)) after every step and on_frame(f, pose, volume) after every frame.
    align='sdf' (experimental; DESIGN.md, "Scanning on the field"): the `iterations` steps of a frame are align_volume_step
    calls in the window of the start pose, on the field of the volume fused so far, with the label filter of the integration
    and its front; gate, jump and cos_min have no part in them and on_step's dict has no depth_hyp.  The raycast at the final
    pose, the counts, the rule for `lost` and the integration are the same.  -> Scan."""
    require(motion in ("constant", "velocity"), "motion must be 'constant' or 'velocity'")
    require(align in ("raycast", "sdf"), "align must be 'raycast' or 'sdf'")
    num_min, den_min = int(min_score[0]), int(min_score[1])
    require(0 <= num_min <= den_min and den_min >= 1, "min_score must be (num, den) with 0 <= num <= den, den >= 1")
    require(int(iterations) >= 0 and int(min_count) >= 1, "iterations must be >= 0 and min_count >= 1")
    dev = depth.device if isinstance(depth, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    dt = depth_frames(depth, dev)
    F = int(dt.shape[0])
    intr = intrinsics_per_frame(intrinsics, F)
    require((label is None) or (want is not None), "label and want come together")
    if label is not None:
        want = np.ascontiguousarray(np.broadcast_to(host(want, np.int64).astype(np.int32).reshape(-1), (F,)))
    dt, intr_dev, _, lab, wnt = fuse._frames(dev, dt, intr, np.tile(np.eye(4), (F, 1, 1)), label, want if label is not None else None)
    first = _first_pose(dt, lab, intr_dev, wnt) if first_pose is None else host(first_pose, np.float64).reshape(4, 4).copy()

    def pose_tensor(T):
        return on_device(np.reshape(T, (1, 4, 4)), torch.float64, dev)

    def integrate(f, pose_dev):
        fuse.integrate(volume, dt[f:f + 1], intr_dev[f:f + 1], pose_dev, None if lab is None else lab[f:f + 1],
                       None if lab is None else wnt[f:f + 1], front=front, behind=behind)

    if aabb is None:
        box = fuse.used_points_aabb(dt[:1], None if lab is None else lab[:1], intr_dev[:1], pose_tensor(first),
                                    None if lab is None else wnt[:1])
        side = float((box[1] - box[0]).max())
        aabb = np.stack([box[0] - float(grow) * side, box[1] + float(grow) * side])
    aabb = host(aabb, np.float64).reshape(2, 3)
    volume = fuse.volume_for(aabb, voxel, device=dev)
    step = STEP_VOXELS * volume.voxel if step is None else float(step)

    def cast(pose, rows, wh, ww):
        return raycast(volume, pose, rows, wh, ww, step, min_count)

    def field_attempt(f, start, tau_u):
        """track.frame_attempt with the steps taken on the field: the window of the start (align_windows without a step),
        `iterations` times align_volume_step, then track.score_attempt."""
        a = track.align_windows(dev, dt, intr, np.full(1, f), aabb[None], start[None], cast, iterations=0, margin=margin)
        dv = a["device"]
        for _ in range(int(iterations)):
            pose_in = a["poses"]
            a["poses"], _, a["n_pairs"], a["status"] = align_volume_step(volume, dt, dv["rows"], pose_in, dv["frame_of"], dv["origin"],
                                                                         a["wh"], a["ww"], lab, wnt, front, min_count)
            if on_step is not None:
                on_step(f, dict(pose_in=pose_in, pose_out=a["poses"], n_pairs=a["n_pairs"], status=a["status"], origin=a["origin"],
                                wh=a["wh"], ww=a["ww"], rows=dv["rows"].cpu().numpy(), frame_of=int(f if a["ok"][0] else -1)))
        return track.score_attempt(dev, dt, a, cast, tau_u, (num_min, den_min), lab, None if lab is None else wnt[f:f + 1])

    s = Scan()
    s.volume, s.min_count, s.aabb = volume, int(min_count), aabb
    s.poses = np.zeros((F, 4, 4))
    s.num, s.den = np.zeros(F, np.int64), np.ones(F, np.int64)
    s.n_pairs, s.status, s.lost = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, bool)
    integrate(0, pose_tensor(first))
    s.poses[0] = first
    if on_frame is not None:
        on_frame(0, first, volume)
    last, before = first.copy(), None
    for f in range(1, F):
        start = track.predict(last, before, motion)
        tau_u = tau_units(np.array([tau], np.float64), intr[f:f + 1, 4].astype(np.float64))[0]
        if align == "sdf":
            pose, num, den, n_pairs, status, lost, pose_dev = field_attempt(f, start, tau_u)
        else:
            pose, num, den, n_pairs, status, lost, pose_dev = track.frame_attempt(
                dev, dt, intr, f, aabb[None], start[None], cast, tau_u, (num_min, den_min), lab, None if lab is None else wnt[f:f + 1],
                iterations=iterations, gate=gate, jump=jump, cos_min=cos_min, margin=margin,
                on_step=None if on_step is None else lambda info: on_step(f, dict(info, frame_of=int(info["frame_of"][0]))))
        if lost[0]:
            before = None
        else:
            before, last = last.copy(), pose[0]
            integrate(f, pose_dev)
        s.poses[f], s.num[f], s.den[f], s.n_pairs[f], s.status[f], s.lost[f] = last, num[0], den[0], n_pairs[0], status[0], lost[0]
        if on_frame is not None:
            on_frame(f, last, volume)
    return s


# ---- command line -----------------------------------------------------------------------------------------------------------
def main(argv=None):
    parser = argparse.ArgumentParser(description="scan one class of a <seq>_pcnn.tfrecord into a mesh from the pose of its first frame")
    parser.add_argument("--files", required=True, help="one <seq>_pcnn.tfrecord; its frames are taken in file order")
    parser.add_argument("--target_cls", type=int, required=True, help="the class to scan (its label in the frames is class + 1)")
    parser.add_argument("--voxel", type=float, default=0.002, help="voxel side in metres")
    parser.add_argument("--out", required=True, help="the PLY file to write")
    parser.add_argument("--every", type=int, default=1, help="take every N-th frame")
    parser.add_argument("--motion", choices=["constant", "velocity"], default="constant")
    parser.add_argument("--simplify", type=float, default=None, metavar="METRES", help="simplify the mesh on cells of this side")
    parser.add_argument("--align", choices=["raycast", "sdf"], default="raycast",
                        help="sdf: align on the volume's signed distance field (experimental)")
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    from . import mesh_models
    torch.cuda.set_device(args.gpu)
    c = args.target_cls
    depth, label, intr, truth, frames = fuse.class_frames(args.files, c, args.every)
    # only the first pose is used; the others are what the printed errors are measured against
    s = scan_object(depth, intr, args.voxel, label=label, want=np.full(len(frames), c + 1, np.int32), first_pose=truth[0],
                    motion=args.motion, align=args.align)
    vertices, triangles = s.mesh(args.simplify)
    mesh_models.write_ply(args.out, vertices, triangles)
    for f, fr in enumerate(frames):
        rot, trans = track.pose_errors(s.poses[f], truth[f])
        print("frame %d score %d/%d lost %d rot_err_deg %.4f trans_err_m %.6f"
              % (int(fr["frame_id"]), s.num[f], s.den[f], int(s.lost[f]), rot, trans))
    print("%d frames into %d x %d x %d voxels of %g m, %d lost" % ((len(frames),) + s.volume.dims + (s.volume.voxel, int(s.lost.sum()))))
    print("%d vertices, %d triangles, %d boundary edges, %d components written to %s"
          % (fuse.mesh_counts(vertices, triangles) + (args.out,)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
