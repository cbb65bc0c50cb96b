"""Cost of scanning ("Scanning"): cloudaae_tsdf_raycast of a 128^3 volume into B = 3 windows of 200 x 200 beside
the route the project had for the same images -- fuse.extract_mesh + mesh_models.pack_meshes + render.render_instances -- and
one whole scan_object frame, and the same two routes for the image the loop itself needs (the scanned volume, one window
of the size track.pose_windows gives).  Device events around every iteration; warm-up first; min / median / max over the iterations;
the versions alternate.  The two routes' images are compared before anything is timed: they cut the same field in two ways,
so the pixels set in both and the ones more than a voxel apart along the ray are counted, not asserted.

    python tools/bench_scan.py [--n 128] [--frames 16] [--window 200] [--iters 20] [--warmup 3] [--align raycast|sdf] [--out FILE.json]

Prints one JSON line.  The kernel's three other forms (a wave as 64 pixels of a row; the cell's values reloaded at every
sample) are timed beside the product's through the development knobs CLOUDAAE_RAYCAST_ROWS and CLOUDAAE_RAYCAST_RELOAD, their
images compared for equality first.  samples: the samples the rays take, estimated in torch from the slab interval and the
image (a ray that hits stops at its hit, any other runs to the interval's end).  --align chooses how the scan_object frame
aligns ("Scanning on the field"); either way one step of each method is timed in the loop's own window: the raycast
plus track.align_step against scan.align_volume_step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_fuse import box_mesh, look_at, timed, views  # noqa: E402


def sample_count(vol, poses, rows, wh, ww, step, depth, z_near):
    """About how many samples the rays of the B windows take."""
    dev = poses.device
    B = int(poses.shape[0])
    k = rows.to(torch.float64)
    x = torch.arange(ww, dtype=torch.float64, device=dev).view(1, 1, ww)
    y = torch.arange(wh, dtype=torch.float64, device=dev).view(1, wh, 1)
    dx, dy = (x - k[:, 2].view(B, 1, 1)) / k[:, 0].view(B, 1, 1), (y - k[:, 3].view(B, 1, 1)) / k[:, 1].view(B, 1, 1)
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    z0 = torch.full((B, wh, ww), float(z_near), dtype=torch.float64, device=dev)
    z1 = (65535.0 / k[:, 4]).view(B, 1, 1).expand(B, wh, ww).clone()
    for a in range(3):
        o = -(R[:, :, a] * t).sum(dim=1).view(B, 1, 1)
        d = R[:, 0, a].view(B, 1, 1) * dx + R[:, 1, a].view(B, 1, 1) * dy + R[:, 2, a].view(B, 1, 1)
        g0, gd = (o - vol.origin[a]) / vol.voxel - 0.5, d / vol.voxel
        ta, tb = (0.0 - g0) / gd, ((vol.dims[a] - 1) - g0) / gd
        z0, z1 = torch.maximum(z0, torch.minimum(ta, tb)), torch.minimum(z1, torch.maximum(ta, tb))
    live = z0 <= z1
    d16 = (depth.to(torch.int32) & 0xFFFF).to(torch.float64)
    end = torch.where(d16 > 0, d16 / k[:, 4].view(B, 1, 1) + step, z1)
    n = torch.where(live, torch.clamp(torch.floor((torch.minimum(end, z1) - z0) / step) + 1.0, min=0.0, max=4096.0), torch.zeros_like(z0))
    return int(live.sum()), int(n.sum())


def main(argv=None):
    parser = argparse.ArgumentParser(description="time the TSDF raycast against meshing + rasterising, and one scan_object frame")
    parser.add_argument("--n", type=int, default=128, help="voxels per side")
    parser.add_argument("--frames", type=int, default=16, help="views fused into the volume, and frames of the scanned sequence")
    parser.add_argument("--window", type=int, default=200)
    parser.add_argument("--height", type=int, default=480)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--align", choices=["raycast", "sdf"], default="raycast", help="how the scan_object frame aligns")
    parser.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan needs a GPU: nothing is measured without one")
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import fuse, mesh_models, render, scan
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    n, F, H, W, win = args.n, args.frames, args.height, args.width, args.window
    s = 0.002
    mesh = box_mesh([0.16, 0.12, 0.09])
    poses = np.stack([look_at(d, 0.7) for d in views(F)])
    intr = np.tile(np.array([600.0, 600.0, (W - 1) / 2.0, (H - 1) / 2.0, 10000.0], np.float32), (F, 1))
    depth = render.render_frames([mesh], [[(0, 1, T)] for T in poses], intr, H, W)['depth']
    vol = fuse.Volume((-0.5 * n * s,) * 3, s, (n, n, n), dev)
    fuse.integrate(vol, depth, torch.from_numpy(intr).to(dev), torch.from_numpy(poses).to(dev))

    # ---- the raycast against mesh + rasteriser: B = 3 windows around the object ------------------------------------------------
    B = 3
    view = torch.from_numpy(np.stack([look_at(d, 0.7) for d in ([0.3, -0.5, 1.0], [1.0, 0.6, -0.4], [-0.7, 0.2, -1.0])])).to(dev)
    rows = torch.from_numpy(np.tile(np.array([600.0, 600.0, (win - 1) / 2.0, (win - 1) / 2.0, 10000.0], np.float32), (B, 1))).to(dev)
    offs, which, ones = np.arange(B + 1), np.zeros(B, np.int64), np.ones(B, np.int64)

    def by_raycast():
        return scan.raycast(vol, view, rows, win, win)

    def by_mesh():
        v, t = fuse.extract_mesh(vol)
        p = mesh_models.pack_meshes([(v, t)], device=dev)
        return render.render_instances(p, rows, offs, which, ones, view.view(B, 16), win, win)[0]

    packed = mesh_models.pack_meshes([fuse.extract_mesh(vol)], device=dev)

    def rasterise_only():
        return render.render_instances(packed, rows, offs, which, ones, view.view(B, 16), win, win)[0]

    a = (by_raycast().to(torch.int32) & 0xFFFF).cpu().numpy().astype(np.int64)
    b = (by_mesh().to(torch.int32) & 0xFFFF).cpu().numpy().reshape(B, win, win).astype(np.int64)
    yy, xx = np.mgrid[0:win, 0:win]
    along = np.sqrt(((xx - (win - 1) / 2.0) / 600.0) ** 2 + ((yy - (win - 1) / 2.0) / 600.0) ** 2 + 1.0)[None]
    both, either = (a != 0) & (b != 0), (a != 0) | (b != 0)
    apart = both & (np.abs(a - b) / 10000.0 * along > s)
    rays, samples = sample_count(vol, view, rows, win, win, scan.STEP_VOXELS * s, by_raycast(), render.Z_NEAR)

    knobs = [("tile_keep", 0, 0), ("tile_reload", 0, 1), ("rows_keep", 1, 0), ("rows_reload", 1, 1)]

    def variant(r, l):
        def run():
            _lib.set_knob("CLOUDAAE_RAYCAST_ROWS", r)
            _lib.set_knob("CLOUDAAE_RAYCAST_RELOAD", l)
            return by_raycast()
        return run
    forms = [variant(r, l) for _, r, l in knobs]
    product = forms[0]()
    forms_equal = all(bool(torch.equal(f(), product)) for f in forms)
    t_forms = timed(forms, args.iters, args.warmup)
    for name in ("CLOUDAAE_RAYCAST_ROWS", "CLOUDAAE_RAYCAST_RELOAD"):
        _lib.set_knob(name, None)
    t_routes = timed([by_raycast, by_mesh, rasterise_only], args.iters, args.warmup)

    # ---- one scan_object frame: an orbit of the box, 2 degrees a frame -----------------------------------------------------------
    orbit = []
    for f in range(F):
        th = np.radians(25.0 + 2.0 * f)
        orbit.append(look_at([np.cos(th) * np.cos(0.6), np.sin(th) * np.cos(0.6), -np.sin(0.6)], 0.7))
    orbit = np.stack(orbit)
    frames = render.render_frames([mesh], [[(0, 1, T)] for T in orbit], intr, H, W)['depth']
    v32 = mesh[0].astype(np.float64)
    aabb = np.stack([v32.min(axis=0), v32.max(axis=0)])
    stamps = []

    def on_frame(f, pose, volume):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    result = None
    for _ in range(2):                                                   # the first run warms up
        del stamps[:]
        result = scan.scan_object(frames, intr, s, first_pose=orbit[0], aabb=aabb, on_frame=on_frame, align=args.align)
    per_frame = np.diff(np.array(stamps)) * 1e3
    err = np.abs(result.poses - orbit).reshape(F, -1).max(axis=1)

    # ---- the loop's own image: the scanned volume at the last pose in the window scan_object takes ------------------------------
    from cloudaae_amd.utils import track
    o2, lh, lw, _ = track.pose_windows(result.poses[-1:], aabb[None], intr[-1:], H, W)
    lrow = intr[-1:].copy()
    lrow[:, 2:4] -= o2.astype(np.float32)
    lrow, lpose = torch.from_numpy(lrow).to(dev), torch.from_numpy(result.poses[-1:].copy()).to(dev)
    lvol = result.volume
    lpacked = mesh_models.pack_meshes([result.mesh()], device=dev)

    def loop_raycast():
        return scan.raycast(lvol, lpose, lrow, lh, lw)

    def loop_mesh():
        p = mesh_models.pack_meshes([fuse.extract_mesh(lvol)], device=dev)
        return render.render_instances(p, lrow, offs[:2], which[:1], ones[:1], lpose.view(1, 16), lh, lw)[0]

    def loop_rasterise():
        return render.render_instances(lpacked, lrow, offs[:2], which[:1], ones[:1], lpose.view(1, 16), lh, lw)[0]
    t_loop = timed([loop_raycast, loop_mesh, loop_rasterise], args.iters, args.warmup)
    l_rays, l_samples = sample_count(lvol, lpose, lrow, lh, lw, scan.STEP_VOXELS * s, loop_raycast(), render.Z_NEAR)

    # ---- one alignment step of either method in that window, against the last frame -----------------------------------------
    def ints(values):
        return torch.tensor(values, dtype=torch.int32, device=dev)
    lframe, lorigin = ints([F - 1]), ints(o2.tolist())
    gate, jump = ints([int(round(track.GATE * 10000.0))]), ints([int(round(track.JUMP * 10000.0))])

    def step_raycast():
        return track.align_step(frames, lframe, lorigin, loop_raycast(), lrow, gate, jump, track.COS_MIN, lpose)["pose_out"]

    def step_field():
        return scan.align_volume_step(lvol, frames, lrow, lpose, lframe, lorigin, lh, lw)[0]
    t_step = timed([step_raycast, step_field], args.iters, args.warmup)
    step_pairs = [int(track.align_step(frames, lframe, lorigin, loop_raycast(), lrow, gate, jump, track.COS_MIN, lpose)["n_pairs"][0]),
                  int(scan.align_volume_step(lvol, frames, lrow, lpose, lframe, lorigin, lh, lw)[2][0])]

    med = t_routes[0]['median'] * 1e-3
    out = dict(voxels=[n, n, n], window=[B, win, win], mesh_triangles=int(packed.num_triangles[0]), pixels_either=int(either.sum()),
               pixels_both=int(both.sum()), pixels_more_than_a_voxel_apart=int(apart.sum()), largest_difference_units=int(np.abs(a - b)[both].max()),
               live_rays=rays, samples=samples, raycast_ms=t_routes[0], mesh_route_ms=t_routes[1], rasterise_only_ms=t_routes[2],
               forms_equal=forms_equal, forms_ms={name: t for (name, _, _), t in zip(knobs, t_forms)},
               samples_per_s=samples / med, scan_frames=F, scan_volume=list(result.volume.dims), scan_lost=int(result.lost.sum()),
               scan_frame_ms=dict(min=float(per_frame.min()), median=float(np.median(per_frame)), max=float(per_frame.max())),
               loop_window=[1, lh, lw], loop_live_rays=l_rays, loop_samples=l_samples, loop_mesh_triangles=int(lpacked.num_triangles[0]),
               loop_raycast_ms=t_loop[0], loop_mesh_route_ms=t_loop[1], loop_rasterise_only_ms=t_loop[2],
               scan_pose_error_last=float(err[-1]), scan_pose_error_max=float(err.max()), align=args.align,
               step_raycast_ms=t_step[0], step_field_ms=t_step[1], step_rows=dict(raycast=step_pairs[0], field=step_pairs[1]),
               iters=args.iters, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
