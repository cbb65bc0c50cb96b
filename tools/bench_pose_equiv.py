"""The nearest equivalent pose (cloudaae_nearest_equivalent_pose): microseconds per launch by HIP events (median and min
of --reps launches after 3 warm-ups, and --reps launches back to back divided by --reps) at b = 32, 128 and 256 with the
icosahedral set of 60 members and with an axial class with a flip; then the replayed training step of bench.py's shape
(batch 32, 1024 points, all 21 classes, fp32) without a symmetry table and with one, in the same run.

    python tools/bench_pose_equiv.py [--reps 50] [--step_reps 30] [--out FILE]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step_reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose_equiv.py measures on the GPU"
    import pose_equiv_reference as PR
    from cloudaae_amd import _lib
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import pose_equiv as PE
    dev = torch.device("cuda:0")
    classes = PR.example_classes()
    names = {n: i for i, n in enumerate(PR.CLASS_NAMES)}
    table = PE.SymmetryTable(*PR.table_arrays(classes), device=dev)
    rows = []
    for kind in ("icosahedral", "axial_flip"):
        for b in (32, 128, 256):
            rng = np.random.default_rng(b)
            rp = torch.from_numpy(PR.random_rotations(rng, b)[1].astype(np.float32)).to(dev)
            rl = torch.from_numpy(PR.random_rotations(rng, b)[1]).to(dev)
            tl = torch.from_numpy(rng.standard_normal((b, 3)).astype(np.float32)).to(dev)
            ids = torch.full((b,), names[kind], dtype=torch.int64, device=dev)
            # the launch alone: outputs allocated once, the C entry called directly
            out = PE.nearest_equivalent_pose(rp, rl, tl, ids, table)
            index, centre, axis, rot = table.on(dev)
            L, s = _lib.lib(), _lib.stream()
            args = (b, rp.data_ptr(), 0, rl.data_ptr(), tl.data_ptr(), ids.data_ptr(), table.num_class, index.data_ptr(),
                    centre.data_ptr(), axis.data_ptr(), table.num_rot, rot.data_ptr(), out["rot_equiv"].data_ptr(),
                    out["trans_equiv"].data_ptr(), out["member"].data_ptr(), out["phi"].data_ptr(), out["angle"].data_ptr(), s)
            med, low, b2b = timed(lambda: L.cloudaae_nearest_equivalent_pose(*args), a.reps)
            wmed, wlow, wb2b = timed(lambda: PE.nearest_equivalent_pose(rp, rl, tl, ids, table), a.reps)
            row = dict(kind=kind, b=b, grid=(b + 3) // 4, us_per_launch=round(med, 1), us_min=round(low, 1),
                       us_back_to_back=round(b2b, 2), wrapper_us=round(wmed, 1), wrapper_us_back_to_back=round(wb2b, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    # the replayed training step of bench.py's shape, without and with a table over the 21 classes
    B, N = 32, 1024
    el = T.synthetic_element(B, N, dev)
    full = PE.SymmetryTable(*PR.table_arrays([classes[c % len(classes)] for c in range(21)]), device=dev)
    for name, sym in (("without", None), ("with", full), ("without_again", None)):
        graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=True, symmetries=sym)
        graph.reuse_staged_inputs = True
        med, low, b2b = timed(lambda: graph.train_step(el), a.step_reps, warm=5)
        row = dict(train_step="replay", B=B, N=N, symmetries=name, launches=len(graph._plan.entries),
                   us_per_step=round(med, 1), us_min=round(low, 1), us_back_to_back=round(b2b, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del graph
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
