"""Device-event times of the four depth-components stages (csrc/depth_components.hip) through the C ABI and of
segment_depth as a whole, F = 8 rendered frames of 480 x 640: the table scene of tests/depth_components_reference.py (a
plane and three spheres) seen by a camera of eight times its resolution, the plane a centimetre further away per frame.
Warm-up calls first, then 30 timed calls each; prints min / median / max microseconds and, as a check, what was found.
The numbers of profiles/notes_depth_components.md come from this script.

    python tools/bench_depth_components.py [OUT.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_components_reference as D
from cloudaae_amd import _lib
from cloudaae_amd.utils import depth_components as DC, render

torch.cuda.set_device(0)
dev = torch.device("cuda:0")
F, H, W = 8, 480, 640
meshes, frames = D.scene_frames()
intr = np.tile(np.array([[600.0, 592.0, 314.4, 236.8, 1000.0]], np.float32), (F, 1))
inst = []
for f in range(F):
    fr = []
    for m, lab, T in frames[0]:
        T = np.array(T)
        T[2, 3] += 0.01 * f
        fr.append((m, lab, T))
    inst.append(fr)
out = render.render_frames([(m[0], m[1]) for m in meshes], inst, intr, H, W, device=dev)
depth, label = out['depth'], out['label']
intr_t = torch.from_numpy(intr).to(dev)
L = _lib.lib()
st = _lib.stream()
n_hyp = DC.N_HYP
count = torch.empty((F, n_hyp), dtype=torch.int32, device=dev)
tested = torch.empty((F,), dtype=torch.int32, device=dev)
plane = torch.empty((F, 4), dtype=torch.float64, device=dev)
hyp = torch.empty((F,), dtype=torch.int32, device=dev)
fg = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
root = torch.empty((F, H, W), dtype=torch.int32, device=dev)
status = torch.empty((F,), dtype=torch.int32, device=dev)
lab_out = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
K = DC.MAX_COMPONENTS
tab = [torch.empty((F, K * c), dtype=torch.int32, device=dev) for c in (1, 1, 4)]
nc = [torch.empty((F,), dtype=torch.int32, device=dev) for _ in range(2)]
ju = torch.full((F,), 20, dtype=torch.int32, device=dev)
b1 = int(L.cloudaae_depth_components_workspace_bytes(F, H, W))
w1 = torch.empty((b1,), dtype=torch.uint8, device=dev)
b2 = int(L.cloudaae_component_labels_workspace_bytes(F, H, W))
w2 = torch.empty((b2,), dtype=torch.uint8, device=dev)
stages = {
    "plane": lambda: L.cloudaae_depth_plane(F, H, W, depth.data_ptr(), intr_t.data_ptr(), 0, 0, n_hyp, DC.STRIDE, DC.TOL, DC.MIN_PLANE_PERCENT,
                                            count.data_ptr(), tested.data_ptr(), plane.data_ptr(), hyp.data_ptr(), st),
    "foreground": lambda: L.cloudaae_depth_foreground(F, H, W, depth.data_ptr(), intr_t.data_ptr(), plane.data_ptr(), hyp.data_ptr(), DC.TOL,
                                                      DC.MAX_HEIGHT, fg.data_ptr(), st),
    "components": lambda: L.cloudaae_depth_components(F, H, W, depth.data_ptr(), fg.data_ptr(), ju.data_ptr(), root.data_ptr(),
                                                      status.data_ptr(), w1.data_ptr(), b1, st),
    "labels": lambda: L.cloudaae_component_labels(F, H, W, root.data_ptr(), DC.MIN_PIXELS, K, lab_out.data_ptr(), nc[0].data_ptr(),
                                                  nc[1].data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(), w2.data_ptr(), b2, st),
    "segment_depth": lambda: DC.segment_depth(depth, intr, device=dev) and 0,
}
res = {}
for name, fn in stages.items():
    for _ in range(5):
        assert fn() == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    res[name] = dict(min_us=min(ts), median_us=float(np.median(ts)), max_us=max(ts), calls=len(ts))
    print(name, res[name], flush=True)
s = DC.segment_depth(depth, intr, device=dev)
k, iou = zip(*[DC.match_components(s.label, label, depth, v) for v in (2, 3, 4)])
res["check"] = dict(plane_hyp=s.plane_hyp.tolist(), tested=s.tested.tolist(), n_components=s.n_components.tolist(),
                    n_candidates=s.n_candidates.tolist(), comp_size=s.comp_size[:, :4].tolist(), fg=int(s.fg.sum()),
                    status=status.tolist(), iou=[x.tolist() for x in iou], k=[x.tolist() for x in k],
                    valid=int((depth != 0).sum()))
print(json.dumps(res["check"]))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
