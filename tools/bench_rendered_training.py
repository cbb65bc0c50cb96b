"""Times of the two on-line syntheses of a training batch, with HIP events, in one process and alternating: the rendered
one (utils/rendered_data.rendered_element: scene, render, optional sensor, clouds) without and with the sensor model, and
the hidden-point-removal one (train_cloudAAE_ycbv.get_small_data, object occluder) on models sampled from the same
meshes.  Buffers come from torch's caching allocator after warm-up; median (min .. max) of the timed runs, one JSON line.

    python tools/bench_rendered_training.py [--runs 30] [--batch 32] [--num_point 1024] [--height 480 --width 640]

The stages of the rendered synthesis are timed in a second loop by events between the public calls it is made of.  The
shares inside cloudaae_render_frames (z-buffer memsets, vertex, setup, queue, resolve) and inside cloudaae_frame_clouds
come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/bench_rendered_training.py
--runs 5), not from events.  The meshes: an icosphere(5) of 6 cm radius (10242 vertices, 20480 triangles), an
icosphere(3) of 5 cm (642, 1280) and a 10 x 14 x 8 cm box (8, 12); the strided bases make every instance as wide as the
largest."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def meshes():
    import mesh_models_reference as MR
    v5, t5 = MR.icosphere(5)
    v3, t3 = MR.icosphere(3)
    cv, ct, _ = MR.cube()
    return [((np.asarray(v5) * 0.06).astype(np.float32), np.asarray(t5, np.int32)),
            ((np.asarray(v3) * 0.05).astype(np.float32), np.asarray(t3, np.int32)),
            (((cv - np.float32(0.5)) * np.array([0.10, 0.14, 0.08], np.float32)).astype(np.float32), ct)]


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num_point", type=int, default=1024)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import depth_noise, mesh_models, render, rendered_data, sample_pose_in_frustum as spf
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, N, H, W, seed = args.batch, args.num_point, args.height, args.width, 123456789
    packed = mesh_models.pack_meshes(meshes(), device=dev)
    models = mesh_models.models_from_meshes(meshes(), device=dev)
    S = int(models.shape[0])

    def records(step):
        return spf.sample_poses(B, seed, step * B, num_models=S, device=dev)

    def rendered(step, sensor):
        return rendered_data.rendered_element(records(step), packed, None, N, seed, step * B, height=H, width=W, sensor=sensor)

    def hpr(step):
        return T.get_small_data(records(step), models, seed=step, occluder='object', first_index=step * B, occluder_seed=seed)

    paths = [("rendered", lambda s: rendered(s, None)), ("rendered_kinect1", lambda s: rendered(s, 'kinect1')),
             ("hpr_object_occluder", hpr)]
    times = {name: [] for name, _ in paths}
    for step in range(args.warmup + args.runs):
        for name, fn in paths:                      # alternating: the three share whatever else the machine does
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(step)
            b.record()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times[name].append(a.elapsed_time(b))
    out = {name: stats(ms) for name, ms in times.items()}
    out["visible_pixels_step0"] = dict(
        occluded=int(rendered(0, None)['num_pixels_occluded'].sum()), alone=int(rendered(0, None)['num_pixels_alone'].sum()))

    # the stages of the rendered synthesis, with the sensor
    stage = {k: [] for k in ("poses", "scene", "render", "sensor", "clouds_input", "clouds_target", "select")}
    intr = rendered_data.frame_intrinsics(2 * B, H, W, device=dev)
    ones = torch.ones((2 * B,), dtype=torch.int32, device=dev)
    for step in range(args.warmup + args.runs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        rec = records(step)
        ev[1].record()
        sc = rendered_data.rendered_scene(rec, packed, None, seed, step * B)
        ev[2].record()
        depth, label, _, _ = render.render_instances_strided(packed, intr, sc['inst_offsets'], sc['inst_mesh'], sc['inst_label'],
                                                             sc['inst_pose'], sc['vert_base'], sc['tri_base'], H, W)
        ev[3].record()
        noisy = depth_noise.apply(depth, label, intr, 'kinect1', seed=seed, first_frame=2 * step * B)
        ev[4].record()
        i = torch.arange(B, device=dev)
        g = step * B + i
        t = rec['translation']
        seen = rendered_data.frame_clouds(noisy['depth'], noisy['label'], intr, torch.cat([2 * i + 1, 2 * i]).int(), ones,
                                          torch.cat([4 * g + 1, 4 * g]), N, seed, fallback=torch.cat([t, t]))
        ev[5].record()
        rendered_data.frame_clouds(depth, label, intr, (2 * i).int(), ones[:B], 4 * g + 2, 4 * N, seed, fallback=t)
        ev[6].record()
        out_ = seen['num_pixels'][:B] < 64
        torch.where(out_[:, None, None], seen['cloud'][B:], seen['cloud'][:B])
        ev[7].record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            for k, name in enumerate(stage):
                stage[name].append(ev[k].elapsed_time(ev[k + 1]))
    out["stages_rendered_kinect1"] = {k: stats(v) for k, v in stage.items()}
    out.update(batch=B, num_point=N, height=H, width=W, runs=args.runs, device=torch.cuda.get_device_name(0),
               strided_vertices=3 * B * int(np.max(packed.num_vertices)), strided_triangles=3 * B * int(np.max(packed.num_triangles)))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
