"""Times of cloudaae_vsd_counts, cloudaae_pose_max_dist and bop_score.vsd() end to end (B = 32, P = 2, 640 x 480): HIP
events around the Python wrappers, warm-up calls first, min / median / max in microseconds, one JSON document
(profiles/notes_bop_score.md).

    python tools/bench_bop_score.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_models_reference as MR
from cloudaae_amd.utils import bop_score as BS, mesh_models as mm, pose_score, render
from cloudaae_amd.utils import sample_pose_in_frustum as spf

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
B, P, H, W = 32, 2, 480, 640
iv, it = MR.icosphere(4)                       # 5120 triangles, radius 0.06 m
packed = mm.pack_meshes([((iv.astype(np.float64) * 0.06).astype(np.float32), it)], device=dev)
cam = spf.camera_parameters('ycbv')
intr = torch.tensor([[cam['fx'], cam['fy'], cam['cx'], cam['cy'], 10000.0]] * B, dtype=torch.float32, device=dev)
s = spf.sample_poses(B, 7, 0, device=dev)
gt = pose_score.pose_matrix(s['axisangle'], s['translation'])
est = gt.unsqueeze(1).repeat(1, P, 1, 1).contiguous()
est[:, 0, 0, 3] += 0.004
est[:, 1, 2, 3] += 0.01
test = render.render_frames(packed, [[(0, 1, gt[b].cpu().numpy())] for b in range(B)], intr, H, W)['depth']

def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return dict(min_us=min(ts), median_us=float(np.median(ts)), max_us=max(ts), n=n)

out = {}
r = BS.vsd(packed, [0] * B, est, gt, test, intr, np.arange(B), 0.12)
out['sample0'] = dict(visib_gt=int(r['visib_gt'][0]), union=r['union'][0].tolist(), errors=r['errors'][0].tolist())
out['vsd_end_to_end'] = timed(lambda: BS.vsd(packed, [0] * B, est, gt, test, intr, np.arange(B), 0.12), n=15, warm=3)
# the two halves of vsd(): the render of one chunk of 8 samples (24 frames), and the count of the whole batch
c = 8
poses = torch.cat([gt[:c].reshape(c, 16), est[:c].reshape(c * P, 16)])
J = c * (1 + P)
rows = intr[:1].repeat(J, 1).contiguous()
ren = lambda: render.render_instances(packed, rows, np.arange(J + 1), np.zeros(J, np.int64), np.ones(J, np.int64), poses, H, W)
out['render_chunk_8_samples_24_frames'] = timed(ren)
dg = test.clone()
de = test.unsqueeze(1).repeat(1, P, 1, 1).contiguous()
tau = torch.full((B, 10), 0.006, dtype=torch.float64, device=dev) * torch.arange(1, 11, device=dev)
fo = torch.arange(B, dtype=torch.int32, device=dev)
out['vsd_counts_b32_p2'] = timed(lambda: BS.vsd_counts(test, intr, fo, dg, de, 0.015, tau, check_frames=False))
out['vsd_counts_b8_p2'] = timed(lambda: BS.vsd_counts(test, intr, fo[:8], dg[:8], de[:8], 0.015, tau[:8], check_frames=False))
out['vsd_counts_b1_p2'] = timed(lambda: BS.vsd_counts(test, intr, fo[:1], dg[:1], de[:1], 0.015, tau[:1], check_frames=False))
model = torch.randn(B, 2048, 6, device=dev) * 0.05
sym = [BS.symmetry_rotations((0, 0, 1), (0, 0, 0), 4)] * B
for name, b, sy in (("max_dist_b32_p2_m2048_s1", B, None), ("max_dist_b32_p2_m2048_s4", B, sym), ("max_dist_b1_p2_m2048_s1", 1, None)):
    m_, e_, g_, i_ = model[:b], est[:b], gt[:b], intr[:b]
    sy_ = None if sy is None else sy[:b]
    out[name] = timed(lambda: BS.mssd_mspd(m_, e_, g_, i_, sy_))
print(json.dumps(out, indent=1))
