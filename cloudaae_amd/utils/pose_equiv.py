"""The nearest equivalent ground-truth pose of a symmetric object: of the label poses T_label o [S | c - S c], S in the
object's rotational symmetry set, the one whose rotation is closest to the predicted rotation
(cloudaae_nearest_equivalent_pose, csrc/pose_equiv.hip).  Minimising a pose loss over the symmetry set is evaluating it
at that label with the choice held constant, so the training step and the evaluation pass the equivalent labels to the
loss and error kernels they already have.  The definition is in DESIGN.md ("Equivalent poses").

    table = SymmetryTable.from_results(symmetries_of_meshes(paths), device='cuda')     # class i = entry i
    table = load_symmetry_table('symmetries.json', num_class=21, device='cuda')        # a save_symmetries file
    d = nearest_equivalent_pose(rot_pred, rot_label, trans_label, class_id, table)
    d['rot_equiv'], d['trans_equiv'], d['member'], d['phi'], d['angle']
"""
import json

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

KIND_NONE, KIND_FINITE, KIND_AXIAL = 0, 1, 2          # CLOUDAAE_SYMMETRY_* of include/cloudaae_hip.h
MAX_MEMBERS = 64                                       # CLOUDAAE_SYMMETRY_MAX_MEMBERS: one member per lane of a wave
IDENTITY_TOL = 1e-12                                   # the first member of a finite set against the identity
ROTATION_TOL = 1e-6                                    # R R^T against the identity, det against 1


def half_turn(f):
    """[3,3]: the rotation by pi about the line along f (re-normalised): 2 f f^T - I."""
    f = np.asarray(f, np.float64).reshape(3)
    n = float(np.sqrt(f @ f))
    require(n > 0.0 and np.isfinite(n), "a flip axis must be a finite vector that is not zero")
    f = f / n
    return 2.0 * np.outer(f, f) - np.eye(3)


class SymmetryTable(object):
    """The symmetry sets of num_class classes as the kernel reads them: index [num_class,3] int32 (kind, first, count),
    centre and axis [num_class,3] float64, rot [num_rot,3,3] float64.  Built on the host (NumPy), checked there, and
    uploaded once per device (on(); device= uploads at once)."""

    def __init__(self, index, centre, axis, rot, device=None):
        index = np.ascontiguousarray(index, np.int32).reshape(-1, 3)
        num_class = len(index)
        require(num_class >= 1, "a symmetry table describes at least one class")
        centre = np.ascontiguousarray(centre, np.float64).reshape(num_class, 3)
        axis = np.ascontiguousarray(axis, np.float64).reshape(num_class, 3)
        rot = np.ascontiguousarray(rot, np.float64).reshape(-1, 3, 3)
        require(np.isfinite(centre).all() and np.isfinite(axis).all() and np.isfinite(rot).all(),
                "a symmetry table holds finite numbers only")
        for c, (kind, first, count) in enumerate(index.tolist()):
            require(kind in (KIND_NONE, KIND_FINITE, KIND_AXIAL), "class %d: unknown kind %d" % (c, kind))
            if kind == KIND_NONE:
                continue
            require(first >= 0 and count >= 0 and first + count <= len(rot),
                    "class %d: rotations %d .. %d leave the table's %d" % (c, first, first + count, len(rot)))
            if kind == KIND_FINITE:
                require(1 <= count <= MAX_MEMBERS, "class %d: a finite set has 1 .. %d members, not %d" % (c, MAX_MEMBERS, count))
            else:
                require(count <= 1, "class %d: an axial class has at most one flip" % c)
                require(abs(float(np.sqrt(axis[c] @ axis[c])) - 1.0) <= 1e-12, "class %d: the axis must be a unit vector" % c)
        self.index, self.centre, self.axis, self.rot = index, centre, axis, rot
        self.num_class, self.num_rot = num_class, len(rot)
        self._dev = {}
        if device is not None:
            self.on(device)

    def on(self, device):
        """(index, centre, axis, rot) on `device`: uploaded the first time a device asks, kept from then on (fixed
        addresses, as a recorded step needs)."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got device %s" % dev)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.index).to(dev), torch.from_numpy(self.centre).to(dev),
                              torch.from_numpy(self.axis).to(dev),
                              torch.from_numpy(self.rot).to(dev) if self.num_rot else None)
        return self._dev[dev]

    @classmethod
    def from_results(cls, results, num_class=None, classes=None, device=None):
        """From find_symmetries results (or the class entries of a save_symmetries file): result i describes class
        classes[i] (default i) of num_class (default: one past the largest).  Classes without a result are 'none'."""
        return cls(*table_arrays(results, num_class, classes), device=device)

    def kinds(self):
        return [("none", "finite", "axial")[k] for k in self.index[:, 0].tolist()]


def table_arrays(results, num_class=None, classes=None):
    """(index, centre, axis, rot) NumPy arrays of a SymmetryTable from find_symmetries results: a finite set gives the
    rotations of its transforms (at most 64, the identity first), an axial one axes[0] re-normalised and, when there is
    an axes[1], the half-turn about it; 'none' and 'spherical' have no members."""
    results = list(results)
    classes = list(range(len(results))) if classes is None else [int(c) for c in classes]
    require(len(classes) == len(results), "one class id per result")
    require(len(set(classes)) == len(classes) and all(c >= 0 for c in classes), "class ids must be distinct and >= 0")
    num_class = (max(classes) + 1 if classes else 1) if num_class is None else int(num_class)
    require(num_class >= 1 and all(c < num_class for c in classes), "a class id outside [0, num_class)")
    index = np.zeros((num_class, 3), np.int32)
    centre = np.zeros((num_class, 3))
    axis = np.zeros((num_class, 3))
    rot = []
    for c, r in zip(classes, results):
        kind = r["kind"]
        require(kind in ("none", "finite", "axial", "spherical"), "class %d: unknown kind %r" % (c, kind))
        if kind in ("none", "spherical"):
            continue
        centre[c] = np.asarray(r["centre"], np.float64).reshape(3)
        if kind == "finite":
            R = np.asarray(r["transforms"], np.float64).reshape(-1, 4, 4)[:, :3, :3]
            require(1 <= len(R) <= MAX_MEMBERS, "class %d: a finite set of %d members, the limit is %d" % (c, len(R), MAX_MEMBERS))
            require(float(np.abs(R[0] - np.eye(3)).max()) <= IDENTITY_TOL, "class %d: a finite set must start with the identity" % c)
            err = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)[None]).max()
            require(err <= ROTATION_TOL and float(np.abs(np.linalg.det(R) - 1.0).max()) <= ROTATION_TOL,
                    "class %d: the members of a finite set must be rotations" % c)
            R = R.copy()
            R[0] = np.eye(3)
            index[c] = (KIND_FINITE, len(rot), len(R))
            rot.extend(R)
        else:
            axes = np.asarray(r["axes"], np.float64).reshape(-1, 3)
            require(len(axes) >= 1, "class %d: an axial class needs its axis" % c)
            n = float(np.sqrt(axes[0] @ axes[0]))
            require(n > 0.0 and np.isfinite(n), "class %d: the axis must be a finite vector that is not zero" % c)
            a = axes[0] / n
            axis[c] = a / np.sqrt(a @ a)
            flips = 0
            if len(axes) >= 2:
                f = axes[1] - float(axes[1] @ axis[c]) * axis[c]        # perpendicular to the axis, as the search made it
                flips = 1
                rot.append(half_turn(f))
            index[c] = (KIND_AXIAL, len(rot) - flips, flips)
    return index, centre, axis, np.asarray(rot, np.float64).reshape(-1, 3, 3)


def load_symmetry_table(path, num_class=None, device=None):
    """The SymmetryTable of a file written by symmetry.save_symmetries (its kind, centre, axes and transforms per class)."""
    with open(path) as f:
        data = json.load(f)
    entries = data["classes"]
    return SymmetryTable.from_results(entries, num_class, [int(e["class"]) for e in entries], device)


def nearest_equivalent_pose(rot_pred, rot_label, trans_label, class_id, table):
    """cloudaae_nearest_equivalent_pose: rot_pred [B,3] float32 or float64, rot_label [B,3] (float64), trans_label [B,3]
    (float32), class_id [B] (int64), all on one GPU.  -> dict(rot_equiv [B,3] float64, trans_equiv [B,3] float32,
    member [B] int32, phi [B] float64, angle [B] float64): the label equivalent under the class's symmetries that is
    nearest rot_pred, which member it is, and the angle left.  No gradient flows through it.  One launch; the outputs
    come from _lib.empty, so the call records into a StepPlan and replays."""
    require(isinstance(table, SymmetryTable), "table must be a SymmetryTable")
    require(rot_pred.dim() == 2 and rot_pred.shape[1] == 3 and rot_pred.shape[0] >= 1, "rot_pred must be [B,3], B >= 1")
    require(rot_pred.dtype in (torch.float32, torch.float64), "rot_pred must be float32 or float64")
    B = int(rot_pred.shape[0])
    for t, name in ((rot_label, "rot_label"), (trans_label, "trans_label")):
        require(tuple(t.shape) == (B, 3), "%s must be [B,3]" % name)
    require(tuple(class_id.shape) == (B,), "class_id must be [B]")
    dev = rot_pred.device
    require(rot_label.device == dev and trans_label.device == dev and class_id.device == dev,
            "the poses and the class ids must be on one GPU")
    index, centre, axis, rot = table.on(dev)
    with torch.no_grad():
        rp = rot_pred.detach().contiguous()
        rl = rot_label.detach().to(torch.float64).contiguous()
        tl = trans_label.detach().to(torch.float32).contiguous()
        cls = class_id.to(torch.int64).contiguous()
        out = dict(rot_equiv=_lib.empty((B, 3), dtype=torch.float64, device=dev),
                   trans_equiv=_lib.empty((B, 3), dtype=torch.float32, device=dev),
                   member=_lib.empty((B,), dtype=torch.int32, device=dev),
                   phi=_lib.empty((B,), dtype=torch.float64, device=dev),
                   angle=_lib.empty((B,), dtype=torch.float64, device=dev))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cloudaae_nearest_equivalent_pose(
                B, ptr(rp), int(rp.dtype == torch.float64), ptr(rl), ptr(tl), ptr(cls), table.num_class,
                ptr(index), ptr(centre), ptr(axis), table.num_rot, ptr(rot),
                ptr(out["rot_equiv"]), ptr(out["trans_equiv"]), ptr(out["member"]), ptr(out["phi"]), ptr(out["angle"]),
                stream()), "cloudaae_nearest_equivalent_pose")
    return out
