"""Stage times of the frame-segment pipeline (utils/segment.py): cloudaae_frame_segments, cloudaae_radius_outlier and
the two cloudaae_ragged_fps launches, timed with HIP events, for B frames of 640x480 holding one segment of about
5k, 20k or 60k points each; against the host restatement (tests/segment_reference.py: NumPy, scipy cKDTree, NumPy FPS)
on one frame.

    python tools/bench_segment.py [--reps 20] [--num_point 256] [--no-host]
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

H, W = 480, 640
INTR = np.array([1066.778, 1067.487, 312.9869, 241.3109, 10000.0], np.float32)


def frame(n_points, seed):
    """One class (0) on a sphere cap of about n_points pixels at 0.8 m, a background plane, 2 % holes."""
    rng = np.random.default_rng(seed)
    side = int(round(np.sqrt(n_points / 0.98)))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = np.full((H, W), 1.3)
    label = np.zeros((H, W), np.uint8)
    u0, v0 = (W - side) // 2, (H - side) // 2
    box = (u >= u0) & (u < u0 + side) & (v >= v0) & (v < v0 + side)
    r = np.sqrt((u - W / 2) ** 2 + (v - H / 2) ** 2) / side
    depth[box] = (0.8 - 0.05 * np.sqrt(np.clip(1 - r ** 2, 0, 1)))[box]
    label[box] = 1
    d16 = np.round(depth * INTR[4]).astype(np.uint16)
    d16[rng.random((H, W)) < 0.02] = 0
    return d16, label


def gpu_stages(B, n_points, num_point, reps):
    from cloudaae_amd.utils import segment as S
    frames = [frame(n_points, s) for s in range(B)]
    depth = np.stack([f[0] for f in frames])
    label = np.stack([f[1] for f in frames])
    intr = np.stack([INTR] * B)
    r = S.extract_segments(depth, label, intr, classes=[[0]] * B)
    smp = S.sample_segments(r, num_point, seed=0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    times = {"extract_ms": [], "fps_inlier_ms": [], "fps_filtered_ms": []}
    for _ in range(reps):
        ev[0].record()
        r = S.extract_segments(depth, label, intr, classes=[[0]] * B)      # ends with the counts' read-back
        ev[1].record()
        S.ragged_fps(r.inlier_offsets_device, r.xyz_inlier_full, num_point, smp["starts_inlier"], r.max_points)
        ev[2].record()
        S.ragged_fps(r.offsets_device, r.xyz, num_point, smp["starts"], r.max_points)
        ev[3].record()
        torch.cuda.synchronize()
        times["extract_ms"].append(ev[0].elapsed_time(ev[1]))
        times["fps_inlier_ms"].append(ev[1].elapsed_time(ev[2]))
        times["fps_filtered_ms"].append(ev[2].elapsed_time(ev[3]))
    out = {k: float(np.median(v)) for k, v in times.items()}
    out.update(B=B, points=int(r.num_point_after_filter.mean()), inliers=int(np.diff(r.inlier_offsets).mean()))
    return out, (depth[0], label[0])


def kernel_stages(B, n_points, reps):
    """The launches of extract_segments one by one (frame segments, radius outlier), events around each call."""
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import segment as S
    frames = [frame(n_points, s) for s in range(B)]
    dev = torch.device("cuda")
    d = torch.from_numpy(np.stack([f[0] for f in frames]).view(np.int16)).to(dev)
    lab = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
    intr = torch.from_numpy(np.stack([INTR] * B)).to(dev)
    M = B * H * W
    L = _lib.lib()
    sf = torch.arange(B, dtype=torch.int32, device=dev)
    sc = torch.zeros(B, dtype=torch.int32, device=dev)
    off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    xyz = torch.empty((M, 3), device=dev)
    mean = torch.empty((B, 3), device=dev)
    n1 = int(L.cloudaae_frame_segments_workspace_bytes(B, H, W, B))
    ws1 = torch.empty(n1, dtype=torch.uint8, device=dev)
    in_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    in_idx = torch.empty(M, dtype=torch.int32, device=dev)
    in_xyz = torch.empty((M, 3), device=dev)
    nv = torch.empty(B, dtype=torch.int32, device=dev)
    n2 = int(L.cloudaae_radius_outlier_workspace_bytes(B, M))
    ws2 = torch.empty(n2, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t = {"frame_segments_ms": [], "radius_outlier_ms": []}
    for _ in range(reps + 1):
        ev[0].record()
        _lib.check(L.cloudaae_frame_segments(B, H, W, d.data_ptr(), lab.data_ptr(), intr.data_ptr(), B, sf.data_ptr(),
                                             sc.data_ptr(), float(S.THRESHOLD), off.data_ptr(), xyz.data_ptr(),
                                             mean.data_ptr(), ws1.data_ptr(), n1, _lib.stream()), "frame_segments")
        ev[1].record()
        _lib.check(L.cloudaae_radius_outlier(B, off.data_ptr(), xyz.data_ptr(), M, S.NB_POINTS, float(S.RADIUS),
                                             S.MIN_KEEP, in_off.data_ptr(), in_idx.data_ptr(), in_xyz.data_ptr(),
                                             nv.data_ptr(), ws2.data_ptr(), n2, _lib.stream()), "radius_outlier")
        ev[2].record()
        torch.cuda.synchronize()
        t["frame_segments_ms"].append(ev[0].elapsed_time(ev[1]))
        t["radius_outlier_ms"].append(ev[1].elapsed_time(ev[2]))
    return {k: float(np.median(v[1:])) for k, v in t.items()}


def host_stages(depth, label, num_point):
    import segment_reference as R
    t0 = time.perf_counter()
    seg = R.frame_segments(depth, label, INTR, [0])[0]
    t1 = time.perf_counter()
    idx, _ = R.radius_outlier(seg["xyz"])
    t2 = time.perf_counter()
    R.fps(seg["xyz"][idx], num_point, 0)
    R.fps(seg["xyz"], num_point, 0)
    t3 = time.perf_counter()
    return {"host_segment_ms": (t1 - t0) * 1e3, "host_radius_ms": (t2 - t1) * 1e3, "host_fps_x2_ms": (t3 - t2) * 1e3}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--num_point", type=int, default=256)
    p.add_argument("--no-host", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    for n in (5000, 20000, 60000):
        for B in (1, 8):
            row, first = gpu_stages(B, n, a.num_point, a.reps)
            row.update(kernel_stages(B, n, a.reps))
            if B == 1 and not a.no_host:
                row.update(host_stages(first[0], first[1], a.num_point))
            print(json.dumps(row))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
