"""Times of cloudaae_depth_fit_counts on rendered 640 x 480 frames (B samples, P = 4 flip hypotheses of an L-shaped
prism): HIP events around the Python wrapper, warm-up calls first, min / median / max in microseconds, and the bytes the
kernel has to read per second of the median.  The same launch is timed on a copy of the images that starts 2 bytes past
a 16-byte boundary, where every workgroup takes the pixel-by-pixel path: the scalar-only form of the same kernel.  One
chunk's render and verify_poses end to end stand beside them (profiles/notes_pose_verify.md).

    python tools/bench_pose_verify.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_verify_reference as V
from cloudaae_amd.utils import mesh_models as mm, pose_score, pose_verify as PV, render
from cloudaae_amd.utils import sample_pose_in_frustum as spf

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
B, P, H, W = 32, 4, 480, 640
lv, lt = V.l_prism()
packed = mm.pack_meshes([((lv.astype(np.float64) * 1.5).astype(np.float32), lt)], device=dev)
cam = spf.camera_parameters('ycbv')
intr = torch.tensor([[cam['fx'], cam['fy'], cam['cx'], cam['cy'], 10000.0]] * B, dtype=torch.float32, device=dev)
s = spf.sample_poses(B, 7, 0, device=dev)
gt = pose_score.pose_matrix(s['axisangle'], s['translation'])
table = PV.HypothesisTable.from_sets({0: PV.flip_hypotheses(V.surface_points(lv * 1.5, lt))})
c = PV.compose(gt, torch.zeros(B, dtype=torch.int64, device=dev), table)
out = render.render_frames(packed, [[(0, 1, gt[b].cpu().numpy())] for b in range(B)], intr, H, W)
test, label = out['depth'], out['label']
J = B * P
hyp = render.render_instances(packed, intr.repeat_interleave(P, 0).contiguous(), np.arange(J + 1), np.zeros(J, np.int64),
                              np.ones(J, np.int64), c['pose'].reshape(J, 16), H, W)[0].view(B, P, H, W)
fo = torch.arange(B, dtype=torch.int32, device=dev)
want = torch.ones(B, dtype=torch.int32, device=dev)
tau = torch.full((B,), 100, dtype=torch.int32, device=dev)


def shifted(t):
    """A copy of t whose first element lies one element past the start of its allocation."""
    buf = torch.zeros((t.numel() + 1,), dtype=t.dtype, device=dev)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return dict(min_us=min(ts), median_us=float(np.median(ts)), max_us=max(ts), n=n)


res = {}
r = PV.fit_counts(test, label, fo, want, hyp, tau, check_frames=False)
res['sample0'] = dict(counts=r['counts'][0].tolist(), seg_total=int(r['seg_total'][0]))
test_s, label_s, hyp_s = shifted(test), shifted(label), shifted(hyp)
assert test_s.data_ptr() % 16 == 2 and hyp_s.data_ptr() % 16 == 2
rs = PV.fit_counts(test_s, label_s, fo, want, hyp_s, tau, check_frames=False)
assert all(torch.equal(r[k], rs[k]) for k in r)
for b in (32, 8, 1):
    nbytes = b * H * W * (2 * P + 3)
    for name, (t_, l_, h_) in (("aligned", (test, label, hyp)), ("scalar", (test_s, label_s, hyp_s))):
        t = timed(lambda: PV.fit_counts(t_, l_, fo[:b], want[:b], h_[:b], tau[:b], check_frames=False))
        t['bytes'] = nbytes
        t['tb_per_s_of_median'] = nbytes / t['median_us'] * 1e-6
        res['fit_counts_b%d_p%d_%s' % (b, P, name)] = t
rows = intr[:1].repeat(8 * P, 1).contiguous()
res['render_chunk_8_samples_%d_frames' % (8 * P)] = timed(lambda: render.render_instances(
    packed, rows, np.arange(8 * P + 1), np.zeros(8 * P, np.int64), np.ones(8 * P, np.int64), c['pose'][:8].reshape(8 * P, 16), H, W))
res['verify_poses_end_to_end_b%d' % B] = timed(lambda: PV.verify_poses(packed, [0] * B, c['pose'], test, label, want, intr,
                                                                          np.arange(B), valid=c['valid']), n=15, warm=3)
v = PV.verify_poses(packed, [0] * B, c['pose'], test, label, want, intr, np.arange(B), valid=c['valid'])
res['best'] = v['best'].tolist()
print(json.dumps(res, indent=1))
