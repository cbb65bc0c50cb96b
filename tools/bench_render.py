"""Times of cloudaae_render_frames (utils/render.py, csrc/render.hip) with HIP events: the whole call (four memsets and
four launches) through the C entry, buffers allocated once, after warm-up; median (min .. max) of the timed runs.

    python tools/bench_render.py [--runs 30] [--frames 8] [--objects 5]
    CLOUDAAE_HIP_LIB=/path/to/libcloudaae_hip_rn64.so python tools/bench_render.py --tag rn64

The scenes: (i) `objects` icosphere(5) instances per frame (20480 triangles each, a few samples per triangle) and (ii)
the same poses with 12-triangle cubes (thousands of samples per triangle), 640 x 480.  RN_SMALL is a compile-time
constant: a library built with -DCLOUDAAE_RN_SMALL=N (render.hip alone, linked with the other objects) is named through
CLOUDAAE_HIP_LIB.  The three launches sit inside one entry point, so their shares come from a kernel trace of this
script (rocprofv3 --kernel-trace, the kernels named render_*), not from events.  --restatement also times
tests/render_reference.py on one frame of each scene (NumPy, one core)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(kind, F, K):
    import mesh_models_reference as MR
    import render_reference as R
    rng = np.random.default_rng(1)
    if kind == "spheres":
        v, t = MR.icosphere(5)
        mesh = ((v * np.float32(0.06)), t)
    else:
        v, t, _ = MR.cube()
        mesh = ((v - np.float32(0.5)) * np.float32(0.12), t)
    frames = [[(0, k + 1, R.pose_matrix(rng.standard_normal(3), [rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1),
                                                                 rng.uniform(0.55, 0.95)])) for k in range(K)] for _ in range(F)]
    intr = np.array([[1066.778, 1067.487, 312.9869, 241.3109, 10000.0]] * F, np.float32)
    return [mesh], frames, intr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--objects", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    from cloudaae_amd import _lib
    import mesh_models_reference as MR
    import render_reference as R
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L, H, W = _lib.lib(), 480, 640
    for kind in ("spheres", "cubes"):
        meshes, frames, intr = scene(kind, args.frames, args.objects)
        vo, to, v, t, _ = MR.pack(meshes)
        offs, mesh, lab, poses, vb, tb = R.instance_bases(meshes, frames)
        F, J = len(frames), len(mesh)
        d = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)      # noqa: E731
        g = [d(vo, np.int32), d(to, np.int32), d(v, np.float32), d(t, np.int32), d(intr, np.float32), d(offs, np.int32),
             d(mesh, np.int32), d(lab, np.int32), d(poses, np.float64), d(vb, np.int32), d(tb, np.int32)]
        depth = torch.empty((F, H, W), dtype=torch.int16, device=dev)
        label = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty((2, J), dtype=torch.int32, device=dev)
        nbytes = int(L.cloudaae_render_workspace_bytes(F, H, W, J, int(vb[-1]), int(tb[-1])))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

        def call():
            _lib.check(L.cloudaae_render_frames(1, g[0].data_ptr(), g[1].data_ptr(), len(v), len(t), g[2].data_ptr(),
                                                g[3].data_ptr(), F, H, W, g[4].data_ptr(), g[5].data_ptr(), J, g[6].data_ptr(),
                                                g[7].data_ptr(), g[8].data_ptr(), g[9].data_ptr(), g[10].data_ptr(), int(vb[-1]),
                                                int(tb[-1]), 0.05, depth.data_ptr(), label.data_ptr(), None,
                                                counts[0].data_ptr(), counts[1].data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
                       "cloudaae_render_frames")
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1000.0)
        covered = int((label != 0).sum())
        row = dict(tag=args.tag, scene=kind, frames=F, instances=J, triangles=int(tb[-1]), covered_pixels=covered,
                   dropped=int(counts[0].sum()), runs=args.runs, median_us=round(float(np.median(us)), 1),
                   min_us=round(min(us), 1), max_us=round(max(us), 1))
        if args.restatement:
            t0 = time.perf_counter()
            R.render(meshes, frames[:1], intr[:1], H, W)
            row["restatement_one_frame_s"] = round(time.perf_counter() - t0, 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
