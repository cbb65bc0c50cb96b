"""Batched ICP at the reference's schedule (10 rounds, 0.01 m, x0.9, 30 iterations): microseconds per launch by HIP
events after warm-up, updates performed, microseconds per update, the final pose error against the scene's true pose,
and (point to point) the NumPy restatement's CPU time per cloud for scale.  Scenes are the golden object model posed,
cut and perturbed as in tests/test_14_icp_gpu.py.  --estimation point_to_point: cloudaae_icp_point_to_point, model ->
scene.  --estimation point_to_plane: cloudaae_icp_point_to_plane, scene -> model on the model's normals
(cloudaae_estimate_normals, radius 0.015 m, outside the timed region).  --normals times the normals kernel alone.

    python tools/bench_icp.py [--estimation point_to_plane] [--batches 1 32] [--points 256 1024] [--reps 20] [--out FILE]
    python tools/bench_icp.py --normals [--sets 1 21] [--reps 20]
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--points", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--estimation", choices=["point_to_point", "point_to_plane"], default="point_to_point")
    ap.add_argument("--normals", action="store_true", help="time cloudaae_estimate_normals on S copies of the model")
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 21])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_icp.py measures on the GPU"
    import icp_reference as R
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils.icp import refine_pose_icp
    model = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))[0][0]
    rows = []
    plane = a.estimation == "point_to_plane"
    if a.normals:
        from cloudaae_amd.utils.normals import estimate_normals
        for S in a.sets:
            sets = torch.from_numpy(np.repeat(model[None], S, axis=0)).cuda()
            for _ in range(3):
                estimate_normals(sets, 0.015)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(a.reps):
                e0.record()
                estimate_normals(sets, 0.015)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            row = dict(kernel="estimate_normals", S=S, K=2048, radius=0.015, us_per_call=round(float(np.median(times)), 1),
                       us_min=round(float(np.min(times)), 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
        return

    def pose_errors(T, truth):
        deg, mm = [], []
        for c in range(len(T)):
            dR = T[c][:3, :3] @ truth[c][:3, :3].T
            deg.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))
            mm.append(np.linalg.norm(T[c][:3, 3] - truth[c][:3, 3]) * 1e3)
        return np.array(deg), np.array(mm)

    for N in a.points:
        for B in a.batches:
            rng = np.random.default_rng(B * 10000 + N)
            sc, r0, t0, truth = [], [], [], []
            for _ in range(B):
                rot = R.log_map(R.rodrigues(rng.standard_normal(3)))
                trans = np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)
                s, r, t = R.scene(model[:, :3], rot, trans, N, 1e-3, rng, rng.uniform(2, 4), rng.uniform(3, 5) * 1e-3)
                sc.append(s)
                r0.append(r)
                t0.append(t)
                truth.append(R.initial_transform(rot, trans))
            obj = torch.from_numpy(np.repeat(model[None], B, axis=0)).cuda()
            scene = torch.from_numpy(np.stack(sc)).cuda()
            rot = torch.from_numpy(np.stack(r0)).cuda()
            trans = torch.from_numpy(np.stack(t0)).cuda()
            if plane:
                from cloudaae_amd.utils.normals import estimate_normals
                nrm = estimate_normals(obj, 0.015)[0]

                def run():
                    return refine_pose_icp(scene, obj, rot, trans, estimation="point_to_plane", normals=nrm,
                                           pose_maps_target_to_source=True)
            else:
                def run():
                    return refine_pose_icp(obj, scene, rot, trans)
            for _ in range(3):
                out = run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            times = []
            for _ in range(a.reps):
                e0.record()
                out = run()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            updates = int(out["iterations"].sum())
            us = float(np.median(times))
            cpu_ms = 0.0
            if not plane:
                t = time.perf_counter()
                R.refine(model, sc[0], r0[0], t0[0])
                cpu_ms = (time.perf_counter() - t) * 1e3
            deg, mm = pose_errors(out["transformation"].cpu().numpy(), truth)
            deg0, mm0 = pose_errors([R.initial_transform(r, t) for r, t in zip(r0, t0)], truth)
            row = dict(estimation=a.estimation, B=B, N=N, M=2048, us_per_launch=round(us, 1), us_min=round(float(np.min(times)), 1),
                       updates=updates, updates_max_cloud=int(out["iterations"].sum(dim=1).max()),
                       us_per_update=round(us / max(1, int(out["iterations"].sum(dim=1).max())), 2),
                       restatement_cpu_ms_per_cloud=round(cpu_ms, 1),
                       mean_fitness=round(float(out["fitness"].mean()), 4),
                       start_deg_mean=round(float(deg0.mean()), 3), start_mm_mean=round(float(mm0.mean()), 3),
                       final_deg_mean=round(float(deg.mean()), 3), final_deg_max=round(float(deg.max()), 3),
                       final_mm_mean=round(float(mm.mean()), 3), final_mm_max=round(float(mm.max()), 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
