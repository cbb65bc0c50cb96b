"""Times of cloudaae_depth_normals and cloudaae_depth_sensor_noise (utils/depth_noise.py, csrc/depth_noise.hip) with HIP
events, next to the render that precedes them: eight 640 x 480 frames of tools/bench_render.py's scene, buffers allocated
once, 3 warm-ups, median and minimum of 30 launches.  Also prints, for the 'kinect1' preset on those frames, the counts
and the share of segments that pass extract_segments' two thresholds with and without the sensor.

    python tools/bench_depth_noise.py [--runs 30] [--frames 8] [--objects 5] [--scene spheres]

One JSON line per measurement.  The byte estimate: a pixel moves 2 + 1 bytes in and 2 + 1 out (the four neighbour taps
hit cache lines that neighbouring lanes load anyway), 6 B, so F H W 6 B over the HBM rate is the floor of the noise pass;
the normals pass writes 16 B per pixel (three floats and theta) on top of its 3 B."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_US = 8.0e6          # 8 TB/s peak (MI355X)


def timed(call, runs, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1000.0)
    return dict(median_us=round(float(np.median(us)), 1), min_us=round(min(us), 1), max_us=round(max(us), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--objects", type=int, default=5)
    ap.add_argument("--scene", default="spheres", choices=["spheres", "cubes"])
    args = ap.parse_args()
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import depth_noise, mesh_models, render, segment
    from tools.bench_render import scene
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    H, W = 480, 640
    meshes, frames, intr = scene(args.scene, args.frames, args.objects)
    F = len(frames)
    packed = mesh_models.pack_meshes(meshes, 1.0, dev)
    out = render.render_frames(packed, frames, intr, H, W)
    depth, label = out['depth'], out['label']
    k = torch.from_numpy(intr).to(dev)
    p = depth_noise.sensor_params('kinect1')
    L = _lib.lib()
    normals = torch.empty((F, H, W, 3), dtype=torch.float32, device=dev)
    theta = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    flat = torch.empty((F,), dtype=torch.int32, device=dev)
    d_out, l_out = torch.empty_like(depth), torch.empty_like(label)
    counts = torch.empty((F, 4), dtype=torch.int32, device=dev)
    pixels = F * H * W

    def normals_call():
        _lib.check(L.cloudaae_depth_normals(F, H, W, depth.data_ptr(), label.data_ptr(), k.data_ptr(), normals.data_ptr(),
                                            theta.data_ptr(), flat.data_ptr(), _lib.stream()), "cloudaae_depth_normals")

    def noise_call():
        _lib.check(L.cloudaae_depth_sensor_noise(F, H, W, depth.data_ptr(), label.data_ptr(), k.data_ptr(), 1, 0,
                                                 *[p[q] for q in depth_noise.PARAMS], d_out.data_ptr(), l_out.data_ptr(),
                                                 counts.data_ptr(), None, _lib.stream()), "cloudaae_depth_sensor_noise")

    def render_call():
        render.render_frames(packed, frames, intr, H, W)

    base = dict(scene=args.scene, frames=F, pixels=pixels, runs=args.runs)
    print(json.dumps(dict(base, what="cloudaae_depth_normals", bytes_per_pixel=19,
                          hbm_floor_us=round(pixels * 19 / HBM_BYTES_PER_US, 2), **timed(normals_call, args.runs, args.warmup))),
          flush=True)
    print(json.dumps(dict(base, what="cloudaae_depth_sensor_noise kinect1", bytes_per_pixel=6,
                          hbm_floor_us=round(pixels * 6 / HBM_BYTES_PER_US, 2), **timed(noise_call, args.runs, args.warmup))),
          flush=True)
    print(json.dumps(dict(base, what="render_frames (host set-up, four memsets, four launches, one read-back)",
                          **timed(render_call, args.runs, args.warmup))), flush=True)
    c = counts.cpu().numpy()
    print(json.dumps(dict(base, what="counts kinect1 seed 1", with_depth=int(c[:, 0].sum()), dropped_by_angle=int(c[:, 1].sum()),
                          dropped_by_chance=int(c[:, 2].sum()), lost_to_range_or_disparity=int(c[:, 3].sum()),
                          flat=int(flat.sum()))), flush=True)
    classes = [[int(i[1]) - 1 for i in fr] for fr in frames]
    for name, d, lab in (("clean", depth, label), ("kinect1", d_out, l_out)):
        r = segment.extract_segments(d, lab, k, classes=classes, num_point=256)
        print(json.dumps(dict(base, what="segments " + name, segments=int(len(r.kept)), kept=int(r.kept.sum()),
                              more_than_100_after_filter=int((r.num_point_after_filter > 100).sum()),
                              at_least_256_valid=int((r.num_valid_points_in_segment >= 256).sum()),
                              median_points_after_filter=float(np.median(r.num_point_after_filter)))), flush=True)


if __name__ == "__main__":
    main()
