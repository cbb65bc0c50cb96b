"""Device-event times of detection (csrc/detect.hip, utils/detect.py), F = 8 rendered frames of 480 x 640: the table scene
of tests/detect_reference.py (a plane, the L prism, the standing plate and a cube) seen by a camera of five times its
resolution, the scene a centimetre further away per frame; four classes (the three and a sphere no frame shows), the
defaults of utils/detect.py.  Warm-up calls first, then timed calls each; prints min / median / max microseconds.
  (a) the windowed render + count of all F K C P hypotheses (detect.window_counts) against the same hypotheses through
      the full-frame path that exists without it: render_instances into whole frames + cloudaae_depth_fit_counts, in
      verify_poses' chunks of 8 samples;
  (b) cloudaae_detect_assign alone;
  (c) detect_objects as a whole and its stages one by one.
The numbers of profiles/notes_detect.md come from this script.

    python tools/bench_detect.py [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_reference as DR
import render_reference as R
from cloudaae_amd.utils import depth_components as DC, detect, pose_verify as PV, ppf, render

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
F, H, W = 8, 480, 640
CALLS = int(os.environ.get("BENCH_DETECT_CALLS", "10"))
s = DR.scene()
meshes = [(m[0], m[1]) for m in s['meshes']]
intr = np.tile(np.array([[750.0, 750.0, 319.5, 239.5, 10000.0]], np.float32), (F, 1))
T = R.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])
inst = []
for f in range(F):
    fr = []
    for m, lab, pose in [(4, 1, T)] + [(c, c + 2, s['gt'][c]) for c in range(3)]:
        pose = np.array(pose)
        pose[2, 3] += 0.01 * f
        fr.append((m, lab, pose))
    inst.append(fr)
packed = render.mesh_models.pack_meshes(meshes, device=dev)
out = render.render_frames(packed, inst, intr, H, W, device=dev)
depth, label = out['depth'], out['label']
models = ppf.PPFModels.from_meshes(meshes[:4], num_point=256, device=dev)


def timed(fn, calls=CALLS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    return dict(min_us=min(ts), median_us=float(np.median(ts)), max_us=max(ts), calls=len(ts))


res = {}
det = detect.detect_objects(depth, intr, packed, models)
seg, poses, valid = det.segments, det.poses, det.valid
Fk, K, C, P = (int(x) for x in poses.shape[:4])
w = detect.window_counts(seg, poses, packed, [0, 1, 2, 3], intr, depth)
n_live = int(np.minimum(seg.n_components, K).sum()) * C
res["shape"] = dict(F=F, H=H, W=W, K=K, C=C, P=P, n_components=seg.n_components.tolist(), wh=w["wh"], ww=w["ww"],
                    live_samples=n_live, hypotheses=n_live * P, window_over_frame=w["wh"] * w["ww"] / float(H * W))
print(json.dumps(res["shape"]), flush=True)

# (a) the same live hypotheses through whole frames
fk = np.array([f * K + k for f in range(F) for k in range(int(min(seg.n_components[f], K)))], np.int64)
live = (fk[:, None] * C + np.arange(C)[None, :]).reshape(-1)
live_dev = torch.from_numpy(live).to(dev)
flat = poses.view(F * K * C, P, 16).index_select(0, live_dev)
frame_of = torch.from_numpy((live // (K * C)).astype(np.int32)).to(dev)
want = torch.from_numpy(((live // C) % K + 1).astype(np.int32)).to(dev)
tau = torch.from_numpy(PV.tau_units(np.full(len(live), 0.01), intr[live // (K * C), 4].astype(np.float64))).to(dev)
rows = torch.from_numpy(intr).to(dev).index_select(0, frame_of.to(torch.int64))
mesh = live % C


def full_frame(n=8):
    parts = []
    for lo in range(0, len(live), n):
        hi = min(lo + n, len(live))
        c = hi - lo
        J = c * P
        d = render.render_instances(packed, rows[lo:hi].repeat_interleave(P, dim=0).contiguous(), np.arange(J + 1),
                                    np.repeat(mesh[lo:hi], P), np.ones(J, np.int64), flat[lo:hi].reshape(J, 16), H, W)[0]
        parts.append(PV.fit_counts(depth, seg.label, frame_of[lo:hi], want[lo:hi], d.view(c, P, H, W), tau[lo:hi],
                                   check_frames=False))
    return parts


res["a_windowed"] = timed(lambda: detect.window_counts(seg, poses, packed, [0, 1, 2, 3], intr, depth))
print("a_windowed", res["a_windowed"], flush=True)
for n in (16, 256):                               # 6 chunks and 1 instead of 2: what the launch count costs
    res["a_windowed_%d_per_launch" % n] = timed(lambda: detect.window_counts(seg, poses, packed, [0, 1, 2, 3], intr, depth,
                                                                              samples_per_launch=n))
    print("a_windowed_%d_per_launch" % n, res["a_windowed_%d_per_launch" % n], flush=True)
res["a_full_frame"] = timed(full_frame, calls=max(CALLS // 2, 3), warm=1)
print("a_full_frame", res["a_full_frame"], flush=True)
# what the two agree on: a window that holds the whole of a hypothesis' pixels counts what the frame counts
full = torch.cat([q["counts"] for q in full_frame()])
win = w["counts"].view(F * K * C, P, 6).index_select(0, live_dev)
res["a_check"] = dict(samples=len(live), equal_rows=int((full == win).all(dim=2).sum()), rows=int(full.shape[0] * P))
print("a_check", res["a_check"], flush=True)

# the two counting calls alone, on images rendered beforehand: all live samples in windows, the first 8 in whole frames
kept = detect.window_counts(seg, poses, packed, [0, 1, 2, 3], intr, depth, samples_per_launch=256, keep_depth=True)
dh_win = kept["depth_hyp"].view(F * K * C, P, w["wh"], w["ww"]).index_select(0, live_dev).contiguous()
org = torch.from_numpy(w["origin"].reshape(F * K, 2)[live // C].astype(np.int32)).to(dev)
res["a_count_windowed_all"] = timed(lambda: detect.fit_counts_window(depth, seg.label, frame_of, want, org, dh_win, tau),
                                    calls=3 * CALLS)
res["a_count_windowed_all"]["samples"] = len(live)
res["a_count_windowed_all"]["hypothesis_bytes"] = int(dh_win.numel()) * 2
print("a_count_windowed_all", res["a_count_windowed_all"], flush=True)
J = 8 * P
dh_full = render.render_instances(packed, rows[:8].repeat_interleave(P, dim=0).contiguous(), np.arange(J + 1), np.repeat(mesh[:8], P),
                                  np.ones(J, np.int64), flat[:8].reshape(J, 16), H, W)[0].view(8, P, H, W)
res["a_count_full_frame_8"] = timed(lambda: PV.fit_counts(depth, seg.label, frame_of[:8], want[:8], dh_full, tau[:8],
                                                          check_frames=False), calls=3 * CALLS)
res["a_count_full_frame_8"]["samples"] = 8
res["a_count_full_frame_8"]["hypothesis_bytes"] = int(dh_full.numel()) * 2
print("a_count_full_frame_8", res["a_count_full_frame_8"], flush=True)

# (b) the decision alone
res["b_assign"] = timed(lambda: detect.assign(w["counts"], w["seg_total"], valid, poses, w["n_components"]), calls=3 * CALLS)
print("b_assign", res["b_assign"], flush=True)

# (c) the whole and its stages
clouds = detect.component_clouds(depth, seg, intr, detect.NUM_POINT)
scene = clouds[2].to(torch.float32).contiguous()
normals, mask = ppf.scene_normals(scene, detect.NORMAL_RADIUS)
S = scene.shape[0]
cls = torch.arange(C, device=dev, dtype=torch.int64).repeat(S)
sc, nc, mc = (t.repeat_interleave(C, dim=0).contiguous() for t in (scene, normals, mask))
stages = {
    "c_detect_objects": lambda: detect.detect_objects(depth, intr, packed, models),
    "c_segment_depth": lambda: DC.segment_depth(depth, intr, device=dev),
    "c_component_clouds": lambda: detect.component_clouds(depth, seg, intr, detect.NUM_POINT),
    "c_scene_normals": lambda: ppf.scene_normals(scene, detect.NORMAL_RADIUS),
    "c_propose_poses": lambda: ppf.propose_poses(models, sc, nc, mc, cls, top=detect.TOP),
    "c_score_candidates": lambda: detect.score_candidates(seg, poses, valid, packed, [0, 1, 2, 3], intr, depth),
}
for name, fn in stages.items():
    res[name] = timed(fn)
    print(name, res[name], flush=True)
# the class each component really shows (label value c + 2), from the rendered labels: a report, no input of the detection
true_class = np.full((F, K), -1, np.int64)
for c in range(3):
    k, _ = DC.match_components(seg.label, label, depth, c + 2)
    for f in range(F):
        if 0 < k[f] <= K:
            true_class[f, k[f] - 1] = c
res["check"] = dict(true_class=true_class.tolist(), correct=int((det.table["det_class"] == true_class).sum()),
                    components=int(np.minimum(seg.n_components, K).sum()),
                    det_class=det.table["det_class"].tolist(), det_score=det.table["det_score"].tolist(),
                    alt_class=det.table["alt_class"].tolist(), n_det=det.table["n_det"].tolist(), skipped=det.skipped,
                    valid_proposals=int(valid.sum()), dropped=int(det.dropped.sum()))
print(json.dumps(res["check"]))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
