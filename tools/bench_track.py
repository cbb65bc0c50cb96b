"""Device-event times of tracking (csrc/depth_align.hip, utils/track.py) on the scene of tools/bench_detect.py: F = 8 rendered
frames of 480 x 640 of the table scene of tests/detect_reference.py (a plane, the L prism, the standing plate and a cube), with
the cube sliding 1.1 cm and turning 2 degrees per frame.  The tracks are the three objects, started from their true poses of
frame 0.  Warm-up calls first, then timed calls each; prints min / median / max microseconds of
  (a) cloudaae_depth_align_step alone, on windows rendered beforehand;
  (b) one align_poses call (the defaults: 4 x (one render + one step)) for the three tracks of frame 1;
  (c) track_objects over the 8 frames (per frame: its time / 8);
  (d) detect_objects on the same frames in the same session: the figure to hold tracking against -- all 8 frames in one call,
      which a tracker cannot do (frame f starts from the result of frame f - 1), and one frame per call, as frames arrive;
  (e) the pieces of an iteration alone: render_instances of the three windows, and the windowed count of the score.
The numbers of profiles/notes_track.md come from this script (its output: profiles/track_bench_8x480x640.json).
With --contour, (b) and (c) run with the occluding-contour term at its defaults ("Contours"), and
  (f) the term's three entries alone: edge_nearest (once per frame), contour_sums and solve_sums (once per iteration)
is added; (a), (d) and (e) are what they are without it.  The numbers of profiles/notes_track_contour.md come from one run
with and one without the flag in the same session.

    python tools/bench_track.py [--contour] [OUT.json]
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
from cloudaae_amd.utils import detect, ppf, render, track

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
F, H, W = 8, 480, 640
CALLS = int(os.environ.get("BENCH_TRACK_CALLS", "10"))
CONTOUR = True if "--contour" in sys.argv[1:] else None
ARGS = [a for a in sys.argv[1:] if a != "--contour"]
s = DR.scene()
meshes = [(m[0], m[1]) for m in s['meshes']]
intr = np.tile(np.array([[750.0, 750.0, 319.5, 239.5, 10000.0]], np.float32), (F, 1))
T = R.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])
truth = np.zeros((F, 3, 4, 4))
inst = []
for f in range(F):
    truth[f, 0], truth[f, 1] = s['gt'][0], s['gt'][1]
    truth[f, 2] = DR._on_table(T, 0.23 - 0.011 * f, -0.02, 0.035, [0.0, 0.0, 0.7 + np.radians(2.0) * f])
    inst.append([(4, 1, T)] + [(c, c + 2, truth[f, c]) for c in range(3)])
packed = render.mesh_models.pack_meshes(meshes, device=dev)
depth = render.render_frames(packed, inst, intr, H, W, device=dev)['depth']
models = ppf.PPFModels.from_meshes(meshes[:4], num_point=256, device=dev)
mesh_of = [0, 1, 2]


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
a = track.align_poses(depth, intr, packed, mesh_of, [1, 1, 1], truth[0], return_trajectory=True)
dv = a["device"]
hyp = render.render_instances(packed, dv["rows"], np.arange(4), np.array(mesh_of), np.ones(3, np.int64),
                              a["trajectory"][0].reshape(3, 16), a["wh"], a["ww"])[0]
factor = intr[[1, 1, 1], 4].astype(np.float64)
gate = torch.from_numpy(track.tau_units(np.full(3, track.GATE), factor)).to(dev)
jump = torch.from_numpy(track.tau_units(np.full(3, track.JUMP), factor)).to(dev)
res["shape"] = dict(F=F, H=H, W=W, tracks=3, wh=a["wh"], ww=a["ww"], window_over_frame=a["wh"] * a["ww"] / float(H * W),
                    n_pairs_steps=a["n_pairs_steps"].cpu().numpy().tolist(), status_steps=a["status_steps"].cpu().numpy().tolist())
print(json.dumps(res["shape"]), flush=True)

res["a_align_step"] = timed(lambda: track.align_step(depth, dv["frame_of"], dv["origin"], hyp, dv["rows"], gate, jump, track.COS_MIN,
                                                     a["trajectory"][0]), calls=3 * CALLS)
print("a_align_step", res["a_align_step"], flush=True)
res["contour"] = bool(CONTOUR)
res["b_align_poses"] = timed(lambda: track.align_poses(depth, intr, packed, mesh_of, [1, 1, 1], truth[0], contour=CONTOUR))
print("b_align_poses", res["b_align_poses"], flush=True)
res["c_track_objects_8_frames"] = timed(lambda: track.track_objects(depth, intr, packed, (mesh_of, truth[0]), contour=CONTOUR))
res["c_track_objects_per_frame_median_us"] = res["c_track_objects_8_frames"]["median_us"] / F
print("c_track_objects_8_frames", res["c_track_objects_8_frames"], res["c_track_objects_per_frame_median_us"], flush=True)
res["d_detect_objects_8_frames"] = timed(lambda: detect.detect_objects(depth, intr, packed, models))
res["d_detect_objects_per_frame_median_us"] = res["d_detect_objects_8_frames"]["median_us"] / F
print("d_detect_objects_8_frames", res["d_detect_objects_8_frames"], res["d_detect_objects_per_frame_median_us"], flush=True)
res["d_detect_objects_1_frame"] = timed(lambda: detect.detect_objects(depth[1:2], intr[1:2], packed, models, first_frame=1))
print("d_detect_objects_1_frame", res["d_detect_objects_1_frame"], flush=True)
res["e_render_windows"] = timed(lambda: render.render_instances(packed, dv["rows"], np.arange(4), np.array(mesh_of), np.ones(3, np.int64),
                                                                a["trajectory"][0].reshape(3, 16), a["wh"], a["ww"]), calls=3 * CALLS)
print("e_render_windows", res["e_render_windows"], flush=True)
tau = torch.from_numpy(track.tau_units(np.full(3, track.TAU), factor)).to(dev)
res["e_count_windows"] = timed(lambda: detect.fit_counts_window(depth, None, dv["frame_of"], None, dv["origin"],
                                                                hyp.view(3, 1, a["wh"], a["ww"]), tau), calls=3 * CALLS)
print("e_count_windows", res["e_count_windows"], flush=True)
if CONTOUR:
    step = torch.from_numpy(track.tau_units(np.full(3, track.CONTOUR_STEP), factor)).to(dev)
    R = track.CONTOUR_RADIUS
    res["f_edge_nearest"] = timed(lambda: track.edge_nearest(depth, dv["frame_of"], dv["origin"], a["wh"], a["ww"], step, R), calls=3 * CALLS)
    print("f_edge_nearest", res["f_edge_nearest"], flush=True)
    near = track.edge_nearest(depth, dv["frame_of"], dv["origin"], a["wh"], a["ww"], step, R)
    plane = track.align_step(depth, dv["frame_of"], dv["origin"], hyp, dv["rows"], gate, jump, track.COS_MIN, a["trajectory"][0])
    res["f_contour_sums"] = timed(lambda: track.contour_sums(depth, dv["frame_of"], dv["origin"], hyp, dv["rows"], gate, step, R, near),
                                  calls=3 * CALLS)
    print("f_contour_sums", res["f_contour_sums"], flush=True)
    con = track.contour_sums(depth, dv["frame_of"], dv["origin"], hyp, dv["rows"], gate, step, R, near)
    res["f_solve_sums"] = timed(lambda: track.solve_sums(plane, con, track.CONTOUR_WEIGHT, a["trajectory"][0]), calls=3 * CALLS)
    print("f_solve_sums", res["f_solve_sums"], flush=True)
    res["f_n_rows"] = con["n_rows"].cpu().numpy().tolist()

t = track.track_objects(depth, intr, packed, (mesh_of, truth[0]), contour=CONTOUR)
res["check"] = dict(error=[[float(np.abs(t.poses[f, j] - truth[f, j]).max()) for j in range(3)] for f in range(F)],
                    lost=t.lost.astype(int).tolist(), num=t.num.tolist(), den=t.den.tolist(), n_pairs=t.n_pairs.tolist())
print(json.dumps(res["check"]))
if ARGS:
    with open(ARGS[0], "w") as fh:
        json.dump(res, fh, indent=1)
