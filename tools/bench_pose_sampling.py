"""Times of the pose-sampling path (utils/sample_pose_in_frustum.py, csrc/pose_sample.hip) with HIP events and wall clock:
the two kernels' launch times, and one get_small_data step fed by drawn poses next to the same step fed by pose records
(host gather of the shuffled records + copy to the device included on the record side), in alternating runs.

    python tools/bench_pose_sampling.py [--reps 200] [--steps 60] [--runs 2] [--batches 32,128]
    python tools/bench_pose_sampling.py --only records --package-root /path/to/another/checkout    # e.g. the parent commit's

--only records times the record path alone and uses nothing this feature added, so with --package-root it runs against a
checkout (with its built library) from before the feature; a shell loop then alternates the two processes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_times(B, reps, dev, models):
    """Per-launch time of each entry point: `reps` calls of the C entry itself (buffers allocated once, no Python layer
    in between) back to back between two events, five times; and the same through the Python functions, which adds
    their allocations and argument handling."""
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import generate_occluder as G, sample_pose_in_frustum as S
    x = S.sample_poses(B, 1, 0, device=dev)
    x['obj_model'] = models
    y = G.get_random_object_occluder(dict(x), models.shape[0], seed=1)
    cam = S.camera_parameters('ycbv')
    _, Hnear, Wnear, _, Wfar = S.get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    L, st, p = _lib.lib()._cdll, _lib.stream(), _lib.ptr
    nm, npts = models.shape[0], models.shape[1]

    def pose_entry(i):
        L.cloudaae_sample_poses(B, i * B, 1, 0, None, nm, Wnear, Wfar, cam['nearDist'], cam['farDist'], cam['fx'], cam['fy'],
                                cam['cx'], cam['cy'], cam['width'], cam['height'], p(x['class_id']), p(x['axisangle']),
                                p(x['rot_mat64']), p(x['rot_gen_mat']), p(x['translation']), p(x['in_fov']), None, None, st)

    def occ_entry(i):
        L.cloudaae_random_object_occluder(B, i * B, 1, nm, npts, p(models), 0, None, p(x['rot_mat64']), p(x['translation']),
                                          512, Wnear, Hnear, cam['nearDist'], p(y['occluder']), None, None, st)
    torch.cuda.synchronize()
    out = {}
    for name, fn in (("sample_poses_entry_us", pose_entry), ("object_occluder_entry_us", occ_entry),
                     ("sample_poses_python_us", lambda i: S.sample_poses(B, 1, i * B, device=dev)),
                     ("object_occluder_python_us", lambda i: G.get_random_object_occluder(x, nm, seed=1, first_index=i * B))):
        per = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(reps):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            per.append(a.elapsed_time(b) * 1000.0 / reps)
        out[name] = dict(median=round(float(np.median(per)), 2), min=round(float(min(per)), 2), max=round(float(max(per)), 2))
    return out


def step_times(B, steps, dev, models, mode, occluder):
    """Per-step wall clock (synchronised) and event time of building one batch."""
    from cloudaae_amd import tfrecord_io as io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    if mode == "records":
        rng = np.random.default_rng(0)
        rec = object.__new__(io.PoseRecords)
        n = 381553
        ax = rng.standard_normal((n, 3))
        rec.axisangle = (ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.uniform(-np.pi, np.pi, (n, 1))).astype(np.float32)
        rec.translation = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.15, 0.15, n), rng.uniform(0.6, 0.9, n)], 1).astype(np.float32)
        rec.class_id = rng.integers(0, 21, n).astype(np.int64)
        batches = rec.epoch(B, seed=1)
    else:
        batches = T.SampledPoses(381553, B, device=dev).epoch(B, 0)
    wall, gpu = [], []
    for i in range(steps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        item = next(batches)
        if mode == "records":
            T.get_small_data({k: torch.as_tensor(v).to(dev, non_blocking=True) for k, v in item.items()}, models, seed=i)
        else:
            T.get_small_data(item, models, seed=i, occluder=occluder, first_index=item['first_index'], occluder_seed=1)
        b.record()
        torch.cuda.synchronize()
        if i >= 5:
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(a.elapsed_time(b))
    q = lambda v: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))   # noqa: E731
    return dict(wall_ms=q(wall), event_ms=q(gpu))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--only", default="all", choices=["all", "launch", "records", "sampled"])
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose cloudaae_amd is timed")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from cloudaae_amd import train_cloudAAE_ycbv as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    models = T.synthetic_object_models(device=dev)
    modes = {"all": [("records", "spherical"), ("sampled", "spherical"), ("sampled", "object")], "launch": [],
             "records": [("records", "spherical")], "sampled": [("sampled", "spherical"), ("sampled", "object")]}[args.only]
    for B in [int(b) for b in args.batches.split(",")]:
        if args.only in ("all", "launch"):
            print(json.dumps(dict(B=B, launch=launch_times(B, args.reps, dev, models))), flush=True)
        for run in range(args.runs):                   # alternating: records, sampled, records, sampled
            for mode, occ in modes:
                print(json.dumps(dict(tag=args.tag, B=B, run=run, poses=mode, occluder=occ,
                                      **step_times(B, args.steps, dev, models, mode, occ))), flush=True)


if __name__ == "__main__":
    main()
