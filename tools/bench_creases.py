"""Device-event times of cloudaae_depth_creases (csrc/creases.hip) through the C ABI and of segment_depth with and without
the cut, F = 8 frames of 480 x 640 from render_frames with sensor='kinect1': the table of
tests/depth_components_reference.py with the touching spheres of tests/creases_reference.py, seen by a camera of eight
times its resolution, the plane a centimetre further away per frame.  Warm-up calls first, then 30 timed calls each;
prints min / median / max microseconds and, as a check, what was found.  The numbers of profiles/notes_creases.md come
from this script.

    python tools/bench_creases.py [OUT.json]
    python tools/bench_creases.py --plain [OUT.json]     # segment_depth without the cut only: runs on a tree without it

--plain with --package DIR imports cloudaae_amd from DIR (a checkout of another commit with its library built): the
comparison of the unchanged path against the parent commit, one fresh process per measurement.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
plain_only = "--plain" in args
package = ROOT
if "--package" in args:
    package = os.path.abspath(args[args.index("--package") + 1])
    args = [a for i, a in enumerate(args) if a != "--package" and (i == 0 or args[i - 1] != "--package")]
args = [a for a in args if a != "--plain"]
sys.path.insert(0, package)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import creases_reference as C
import depth_noise_reference as DN
import mesh_models_reference as MR
from cloudaae_amd import _lib
from cloudaae_amd.utils import depth_components as DC, render

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
F, H, W = 8, 480, 640
meshes = [MR.icosphere(2), DN.plane_mesh()]
frame = [(1, 1, C.table_pose())]
for i, (centre, (_, _, rad)) in enumerate(zip(C.sphere_centres(C.TOUCHING_SPHERES), C.TOUCHING_SPHERES)):
    S = np.eye(4)
    S[:3, :3] *= rad
    S[:3, 3] = centre
    frame.append((0, 2 + i, S))
intr = np.tile(np.array([[600.0, 592.0, 314.4, 236.8, 1000.0]], np.float32), (F, 1))
inst = []
for f in range(F):
    fr = []
    for m, lab, T in frame:
        T = np.array(T)
        T[2, 3] += 0.01 * f
        fr.append((m, lab, T))
    inst.append(fr)
out = render.render_frames([(m[0], m[1]) for m in meshes], inst, intr, H, W, device=dev, sensor='kinect1', sensor_seed=3)
depth, label = out['depth'], out['label']


def timed(fn, calls=30, warm=5):
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
res["segment_depth"] = timed(lambda: DC.segment_depth(depth, intr, device=dev))
print("segment_depth", res["segment_depth"], flush=True)
plain = DC.segment_depth(depth, intr, device=dev)
res["check"] = dict(n_components=plain.n_components.tolist(), comp_size=plain.comp_size[:, :4].tolist(), fg=int(plain.fg.sum()))
if not plain_only:
    L = _lib.lib()
    st = _lib.stream()
    intr_t = torch.from_numpy(intr).to(dev)
    ju = plain.jump_units
    img = [torch.empty((F, H, W), dtype=torch.uint8, device=dev) for _ in range(3)]
    n_crease = torch.empty((F,), dtype=torch.int32, device=dev)
    nbytes = int(L.cloudaae_depth_creases_workspace_bytes(F, H, W))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    for name, step, smooth in (("creases_3_1", DC.STEP, DC.SMOOTH), ("creases_8_7", 8, 7)):
        c = np.cos(np.radians(DC.ANGLE))

        def call():
            assert L.cloudaae_depth_creases(F, H, W, depth.data_ptr(), plain.fg.data_ptr(), intr_t.data_ptr(), ju.data_ptr(), step, smooth,
                                            float(c * c), img[0].data_ptr(), img[1].data_ptr(), img[2].data_ptr(), n_crease.data_ptr(),
                                            ws.data_ptr(), nbytes, st) == 0
        res[name] = timed(call)
        res[name]["n_crease"] = n_crease.tolist()
        print(name, res[name], flush=True)
    res["segment_depth_creases"] = timed(lambda: DC.segment_depth(depth, intr, device=dev, creases=True))
    print("segment_depth_creases", res["segment_depth_creases"], flush=True)
    cut = DC.segment_depth(depth, intr, device=dev, creases=True)
    k, iou = zip(*[DC.match_components(cut.label, label, depth, v) for v in (2, 3, 4)])
    res["check"].update(cut_n_components=cut.n_components.tolist(), cut_comp_size=cut.comp_size[:, :4].tolist(),
                        n_crease=cut.n_crease.tolist(), iou=[x.tolist() for x in iou], k=[x.tolist() for x in k])
print(json.dumps(res["check"]))
if args:
    with open(args[0], "w") as fh:
        json.dump(res, fh, indent=1)
