"""Pose scores (cloudaae_pose_score: ADD, ADD-S) at M = 2048: microseconds per launch by HIP events (median and min of
--reps launches after 3 warm-ups), pairs per second, and two yardsticks measured in the same run: (a) the library's
Chamfer search (tf_nndistance.nn_distance) on the same two transformed clouds materialised in float32 -- both
directions, float32-exact: a lower-precision, twice-the-work neighbour, a scale only; (b) the replayed evaluate_batch
pass at B = 1, N = 256 without and with score (and with icp).  Also the NumPy restatement's CPU time per sample.

    python tools/bench_pose_score.py [--reps 20] [--out FILE]
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


def timed(fn, reps, warm=3):
    """(median, min) microseconds of fn() between two HIP events, and of `reps` calls back to back divided by reps."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return float(np.median(times)), float(np.min(times)), e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose_score.py measures on the GPU"
    import icp_reference as IR
    import pose_score_reference as R
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.tf_ops.nn_distance import tf_nndistance
    from cloudaae_amd.utils import pose_score as S
    model = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))[0][0]
    M = len(model)
    rows = []
    for B, P in ((1, 1), (1, 2), (32, 1), (32, 2)):
        rng = np.random.default_rng(100 * B + P)
        gt, est = np.empty((B, 4, 4)), np.empty((B, P, 4, 4))
        for s in range(B):
            rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
            gt[s] = IR.initial_transform(rot, np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3))
            for k in range(P):
                axis = rng.standard_normal(3)
                dR = IR.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(rng.uniform(2, 4)))
                est[s, k] = gt[s]
                est[s, k, :3, :3] = dR @ gt[s, :3, :3]
                est[s, k, :3, 3] += rng.standard_normal(3) * 2e-3
        obj = torch.from_numpy(np.repeat(model[None], B, axis=0)).cuda()
        e, g = torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda()
        med, low, b2b = timed(lambda: S.score_poses(obj, e, g), a.reps)
        # yardstick (a): the same clouds in float32 through the Chamfer search, one call per pose
        X = model[:, :3].astype(np.float64)
        gc = torch.from_numpy(np.stack([IR.apply(gt[s], X) for s in range(B)]).astype(np.float32)).cuda()
        ec = [torch.from_numpy(np.stack([IR.apply(est[s, k], X) for s in range(B)]).astype(np.float32)).cuda()
              for k in range(P)]
        cmed, clow, cb2b = timed(lambda: [tf_nndistance.nn_distance(gc, c) for c in ec], a.reps)
        pairs = B * P * M * M
        row = dict(B=B, P=P, M=M, grid=B * P * ((M + 63) // 64), us_per_launch=round(med, 1), us_min=round(low, 1),
                   us_back_to_back=round(b2b, 1), gpairs_per_s=round(pairs / low * 1e-3, 1),
                   chamfer_f32_us=round(cmed, 1), chamfer_f32_us_min=round(clow, 1),
                   chamfer_f32_us_back_to_back=round(cb2b, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    t = time.perf_counter()
    R.score(model, est[0, 0], gt[0])
    rows.append(dict(restatement_cpu_ms_per_sample=round((time.perf_counter() - t) * 1e3, 1)))
    print(json.dumps(rows[-1]), flush=True)
    # yardstick (b): the replayed evaluation pass at B = 1, N = 256
    N = 256
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": 1})
    rng = np.random.default_rng(3)
    rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
    trans = np.array([0.01, -0.02, 0.8])
    sc, _, _ = IR.scene(model[:, :3], rot, trans, N, 1e-3, rng, 3.0, 0.004)
    el = dict(xyz_inlier=torch.from_numpy(sc[None]), visiblePoints_org=torch.from_numpy(sc[None]).clone(),
              class_id=torch.zeros(1, dtype=torch.int64), translation=torch.from_numpy(trans[None]).float(),
              axisangle=torch.from_numpy(rot[None]), obj_batch=torch.from_numpy(model[None]))
    el = {k: v.cuda() for k, v in el.items()}
    for icp in (None, True):
        row = dict(evaluate_batch="replay", B=1, N=N, icp=bool(icp))
        for score in (None, True):
            med, low, b2b = timed(lambda: E.evaluate_batch(graph, el, replay=True, icp=icp, score=score), a.reps)
            tag = "scored" if score else "unscored"
            row.update({tag + "_us": round(med, 1), tag + "_us_min": round(low, 1), tag + "_us_back_to_back": round(b2b, 1)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
