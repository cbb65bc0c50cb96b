"""Pose verification: judge candidate poses of an object against the depth the camera saw, without the ground truth,
and keep the best.  A small set of hypotheses is composed from a base pose (cloudaae_pose_compose), every hypothesis is
rendered alone with its frame's intrinsics (utils/render.py), each rendering is compared per pixel with the observed
depth and with the object's segment (cloudaae_depth_fit_counts; csrc/depth_fit.hip), and the winner is chosen exactly
(cloudaae_select_pose; csrc/pose_verify.hip).  The definition is in DESIGN.md ("Pose verification").

    table = HypothesisTable.from_models(models)                      # identity + the three principal half turns per class
    c = compose(base, class_id, table)                               # c['pose'] [B,P,4,4], c['valid'] [B,P]
    r = verify_poses(meshes, mesh_index, c['pose'], depth_test, label, want, intrinsics, frame_of, valid=c['valid'])
    r['best'], r['pose_best'], r['score'], r['margin']

The failure this answers: a depth-only encoder returns a pose half a turn about one of the object's long axes from the
truth, ICP converges from it to the wrong local minimum, and its fitness does not tell."""
import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .frame_inputs import check_depth, check_int32, check_poses

COUNTERS = ("rendered", "consistent", "in_front", "behind", "unknown", "explained")      # the order of counts [..., 6]
MODE_SEGMENT, MODE_SILHOUETTE = 0, 1
IDENTITY_TOL = 1e-12                                      # the first member of a set against the identity


def flip_hypotheses(model_xyz):
    """[4,4,4] float64: the identity (exactly) and the half turns about the three principal axes of the points model_xyz
    [M,>=3] through their centroid, by descending eigenvalue of the covariance (numpy.linalg.eigh): H = [R | c - R c],
    R = 2 a a^T - I.  NumPy float64 on the host, once per class."""
    x = np.asarray(model_xyz.detach().cpu() if isinstance(model_xyz, torch.Tensor) else model_xyz, np.float64)
    require(x.ndim == 2 and x.shape[1] >= 3 and len(x) >= 1, "model_xyz must be [M, >=3]")
    x = x[:, :3]
    c = x.mean(axis=0)
    y = x - c
    _, vec = np.linalg.eigh((y.T @ y) / len(x))           # eigenvalues ascending
    out = np.zeros((4, 4, 4), np.float64)
    out[0] = np.eye(4)
    for k in range(3):
        a = vec[:, 2 - k]
        a = a / np.sqrt(a @ a)
        R = 2.0 * np.outer(a, a) - np.eye(3)
        out[1 + k, :3, :3] = R
        out[1 + k, :3, 3] = c - R @ c
        out[1 + k, 3, 3] = 1.0
    return out


class HypothesisTable(object):
    """The transform sets of num_class classes as the kernel reads them: index [num_class+1] int32, offsets into hyp
    [n_total,4,4] float64; class c owns hyp[index[c]:index[c+1]], whose first member is the identity (so that hypothesis 0
    is the base pose itself; identity_first=False lifts the check for a caller who wants another order).  Built on the
    host (NumPy) and uploaded once per device (on(); device= uploads at once)."""

    def __init__(self, index, hyp, device=None, identity_first=True):
        index = np.ascontiguousarray(index, np.int32).reshape(-1)
        hyp = np.ascontiguousarray(hyp, np.float64).reshape(-1, 4, 4)
        require(len(index) >= 2 and index[0] == 0 and (np.diff(index) >= 0).all() and index[-1] == len(hyp),
                "index must be [num_class + 1] offsets from 0 to the number of transforms, not decreasing")
        require(np.isfinite(hyp).all(), "a hypothesis table holds finite numbers only")
        for c in range(len(index) - 1):
            if identity_first and index[c + 1] > index[c]:
                require(np.array_equal(hyp[index[c]], np.eye(4)), "class %d: the first member must be the identity" % c)
        self.index, self.hyp = index, hyp
        self.num_class, self.num_total = len(index) - 1, len(hyp)
        self.max_members = int(np.diff(index).max())
        self._dev = {}
        if device is not None:
            self.on(device)

    def on(self, device):
        """(index, hyp) on `device`: uploaded the first time a device asks, kept from then on."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got device %s" % dev)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        if dev not in self._dev:
            self._dev[dev] = (torch.from_numpy(self.index).to(dev),
                              torch.from_numpy(self.hyp).to(dev) if self.num_total else None)
        return self._dev[dev]

    def members(self, c):
        """[n,4,4]: the set of class c (empty for a class without one)."""
        return self.hyp[self.index[c]:self.index[c + 1]]

    @classmethod
    def from_sets(cls, sets, num_class=None, device=None, identity_first=True):
        """From {class: [n,4,4] transforms}; the first member of every set must be the identity (to 1e-12: it is stored
        as the identity exactly) unless identity_first is False.  Classes without a set get none: compose gives them the
        base pose alone."""
        sets = {int(c): np.asarray(s, np.float64).reshape(-1, 4, 4) for c, s in sets.items()}
        require(all(c >= 0 for c in sets), "class ids must be >= 0")
        num_class = (max(sets) + 1 if sets else 1) if num_class is None else int(num_class)
        require(num_class >= 1 and all(c < num_class for c in sets), "a class id outside [0, num_class)")
        index, rows = [0], []
        for c in range(num_class):
            s = sets.get(c)
            if s is not None and len(s):
                s = s.copy()
                if identity_first:
                    require(float(np.abs(s[0] - np.eye(4)).max()) <= IDENTITY_TOL,
                            "class %d: a set must start with the identity" % c)
                    s[0] = np.eye(4)
                s[:, 3] = (0.0, 0.0, 0.0, 1.0)
                rows.extend(s)
            index.append(len(rows))
        return cls(index, np.asarray(rows, np.float64).reshape(-1, 4, 4), device, identity_first)

    @classmethod
    def from_models(cls, models, classes=None, num_class=None, device=None):
        """flip_hypotheses of each model of models [C,M,>=3]; model i is class classes[i] (default i)."""
        m = np.asarray(models.detach().cpu() if isinstance(models, torch.Tensor) else models)
        require(m.ndim == 3 and m.shape[2] >= 3, "models must be [C, M, >=3]")
        classes = list(range(len(m))) if classes is None else [int(c) for c in classes]
        require(len(classes) == len(m) and len(set(classes)) == len(classes), "one distinct class id per model")
        return cls.from_sets({c: flip_hypotheses(m[i]) for i, c in enumerate(classes)}, num_class, device)


def compose(base, class_id, table, p=None):
    """cloudaae_pose_compose: base [B,4,4] float64 and class_id [B] (int64) on one GPU, table a HypothesisTable; p
    hypotheses per sample (default: the largest set's count).  -> dict of pose [B,P,4,4] float64, rot_axag [B,P,3]
    float64 (angle in [0, pi]), trans [B,P,3] float32 and valid [B,P] int32: hypothesis j of sample i is base_i H_{c,j};
    past the class's count it repeats member 0 with valid 0.  One launch."""
    require(isinstance(table, HypothesisTable), "table must be a HypothesisTable")
    require(isinstance(base, torch.Tensor) and base.dim() == 3 and base.shape[0] >= 1, "base must be a float64 [B, 4, 4] tensor")
    B, dev = int(base.shape[0]), base.device
    base = check_poses(base, "base", (3,), B, dev)
    require(isinstance(class_id, torch.Tensor) and tuple(class_id.shape) == (B,) and class_id.device == dev,
            "class_id must be [B], on the poses' device")
    P = max(table.max_members, 1) if p is None else int(p)
    require(P >= 1, "p must be >= 1")
    index, hyp = table.on(dev)
    cls = class_id.to(torch.int64).contiguous()
    out = dict(pose=_lib.empty((B, P, 4, 4), dtype=torch.float64, device=dev),
               rot_axag=_lib.empty((B, P, 3), dtype=torch.float64, device=dev),
               trans=_lib.empty((B, P, 3), dtype=torch.float32, device=dev),
               valid=_lib.empty((B, P), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_pose_compose(B, ptr(base), ptr(cls), table.num_class, ptr(index), table.num_total,
                                                    ptr(hyp), P, ptr(out["pose"]), ptr(out["rot_axag"]), ptr(out["trans"]),
                                                    ptr(out["valid"]), stream()), "cloudaae_pose_compose")
    return out


def _fit_inputs(dt, dh, label, frame_of, want, tau):
    """What fit_counts and detect.fit_counts_window share: the checks of label [F,H,W], want (None without a label),
    frame_of and tau [B] against the test frames dt [F,H,W] and the hypothesis images dh [B,P,..], and the outputs.
    -> (label, frame_of, want, tau, out), out the dict of counts [B,P,6] int32, seg_total [B] int32, abs_sum [B,P] int64."""
    B, P, dev = int(dh.shape[0]), int(dh.shape[1]), dt.device
    require(dh.device == dev, "all inputs must be on one device")
    if label is not None:
        require(isinstance(label, torch.Tensor) and label.dtype == torch.uint8 and label.shape == dt.shape and
                label.device == dev, "label must be a uint8 [F, H, W] tensor on the inputs' device, or None")
        label = label.contiguous()
        want = check_int32(want, "want", (B,), dev)
    else:
        want = None
    frame_of, tau = check_int32(frame_of, "frame_of", (B,), dev), check_int32(tau, "tau", (B,), dev)
    out = {"counts": _lib.empty((B, P, len(COUNTERS)), dtype=torch.int32, device=dev),
           "seg_total": _lib.empty((B,), dtype=torch.int32, device=dev),
           "abs_sum": _lib.empty((B, P), dtype=torch.int64, device=dev)}
    return label, frame_of, want, tau, out


def fit_counts(depth_test, label, frame_of, want, depth_hyp, tau, check_frames=True):
    """cloudaae_depth_fit_counts.  depth_test [F,H,W], depth_hyp [B,P,H,W]: int16 tensors holding the uint16 bits (what
    render_frames returns) or uint16; label [F,H,W] uint8 or None; frame_of [B] int32 in [0, F) (checked here with one
    read-back unless check_frames is False: the kernel gives an entry outside zero counts); want [B] int32 (ignored
    without a label); tau [B] int32 in depth units.  -> dict of counts [B,P,6] int32 (COUNTERS), seg_total [B] int32 and
    abs_sum [B,P] int64 on the device."""
    dt, dh = check_depth(depth_test, "depth_test", 3), check_depth(depth_hyp, "depth_hyp", 4)
    F, H, W = (int(x) for x in dt.shape)
    B, P = int(dh.shape[0]), int(dh.shape[1])
    require(tuple(dh.shape) == (B, P, H, W) and B >= 1 and P >= 1, "depth_hyp must be [B, P, H, W] with the test frames' H and W")
    label, frame_of, want, tau, out = _fit_inputs(dt, dh, label, frame_of, want, tau)
    if check_frames:
        fo = frame_of.cpu().numpy()
        require(fo.min() >= 0 and fo.max() < F, "a frame_of entry outside [0, F)")
    with torch.cuda.device(dt.device):
        _lib.check(_lib.lib().cloudaae_depth_fit_counts(F, H, W, ptr(dt), ptr(label), B, P, ptr(frame_of), ptr(want), ptr(dh),
                                                        ptr(tau), ptr(out["counts"]), ptr(out["seg_total"]),
                                                        ptr(out["abs_sum"]), stream()), "cloudaae_depth_fit_counts")
    return out


def select(counts, seg_total, valid, pose, mode=MODE_SEGMENT):
    """cloudaae_select_pose.  counts [B,P,6], seg_total [B] int32 as fit_counts returns them, valid [B,P] int32 (None:
    all valid), pose [B,P,4,4] float64; mode 0: explained / (seg_total + in_front), mode 1: consistent / (consistent +
    in_front + behind).  -> dict of best [B] int32, score [B,P], margin [B] and pose_best [B,4,4] float64."""
    require(isinstance(counts, torch.Tensor) and counts.dtype == torch.int32 and counts.dim() == 3 and
            counts.shape[2] == len(COUNTERS) and counts.shape[0] >= 1 and counts.shape[1] >= 1,
            "counts must be an int32 [B, P, 6] tensor")
    B, P, dev = int(counts.shape[0]), int(counts.shape[1]), counts.device
    seg_total = check_int32(seg_total, "seg_total", (B,), dev)
    if valid is None:
        valid = torch.ones((B, P), dtype=torch.int32, device=dev)
    require(isinstance(valid, torch.Tensor) and valid.dtype == torch.int32 and tuple(valid.shape) == (B, P) and
            valid.device == dev, "valid must be an int32 [B, P] tensor on the counts' device")
    pose = check_poses(pose, "pose", (4,), B, dev)
    require(int(pose.shape[1]) == P, "pose must hold P poses per sample")
    require(int(mode) in (MODE_SEGMENT, MODE_SILHOUETTE), "mode must be 0 (segment rule) or 1 (silhouette rule)")
    out = dict(best=_lib.empty((B,), dtype=torch.int32, device=dev), score=_lib.empty((B, P), dtype=torch.float64, device=dev),
               pose_best=_lib.empty((B, 4, 4), dtype=torch.float64, device=dev),
               margin=_lib.empty((B,), dtype=torch.float64, device=dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_select_pose(B, P, ptr(counts.contiguous()), ptr(seg_total), ptr(valid.contiguous()),
                                                   ptr(pose), int(mode), ptr(out["best"]), ptr(out["score"]),
                                                   ptr(out["pose_best"]), ptr(out["margin"]), stream()),
                   "cloudaae_select_pose")
    return out


def tau_units(tau, factor_depth):
    """floor(tau factor_depth + 0.5) in float64, clamped into [0, 2^31 - 1]: tau in metres -> depth units, [B] int32."""
    t = np.floor(np.asarray(tau, np.float64) * np.asarray(factor_depth, np.float64) + 0.5)
    return np.clip(np.nan_to_num(t, nan=0.0), 0.0, 2147483647.0).astype(np.int32)


def verify_poses(meshes, mesh_index, poses, depth_test, label, want, intrinsics, frame_of, tau=0.01, mode=MODE_SEGMENT,
                 samples_per_launch=8, valid=None):
    """The best of the hypotheses poses [B,P,4,4] (float64, model -> camera, on the device) in the test frames depth_test
    [F,H,W] (int16 bits or uint16, device) with label [F,H,W] uint8 (or None: mode 1 then) and intrinsics [F,5];
    frame_of [B]: each sample's frame; want [B]: the label value of each sample's object; meshes: a PackedMeshes (or what
    mesh_models.pack_meshes takes) and mesh_index [B] (host integers): each sample's mesh.  tau in metres (a number or
    [B]): tau_units = floor(tau factor_depth + 0.5) of the sample's frame, formed in float64 on the host.  Every
    hypothesis is rendered alone with its frame's intrinsics (label 1, samples_per_launch samples per launch), counted by
    cloudaae_depth_fit_counts and the winner chosen by cloudaae_select_pose.  valid [B,P] int32 (compose's; None: all
    valid).  -> dict of counts [B,P,6], seg_total [B] int32, abs_sum [B,P] int64, score [B,P], margin [B], pose_best
    [B,4,4] float64, best [B] int32 (device) and dropped [B,P] int32 (numpy, one read-back at the end: the triangles
    the renderer left out under each hypothesis)."""
    from . import mesh_models, render
    p = mesh_models.pack_meshes(meshes)
    dev = p.device
    dt = check_depth(depth_test, "depth_test", 3)
    F, H, W = (int(x) for x in dt.shape)
    require(isinstance(poses, torch.Tensor) and poses.dim() == 4, "poses must be a float64 [B, P, 4, 4] tensor")
    B, P = int(poses.shape[0]), int(poses.shape[1])
    poses = check_poses(poses, "poses", (4,), B, dev)
    mesh = np.asarray(mesh_index.cpu() if isinstance(mesh_index, torch.Tensor) else mesh_index, np.int64).reshape(-1)
    require(len(mesh) == B and mesh.min() >= 0 and mesh.max() < len(p.num_triangles), "mesh_index must be [B], inside the meshes")
    fo_host = np.asarray(frame_of.cpu() if isinstance(frame_of, torch.Tensor) else frame_of, np.int64).reshape(-1)
    require(len(fo_host) == B and fo_host.min() >= 0 and fo_host.max() < F, "frame_of must be [B] with entries in [0, F)")
    intr_host = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, np.float32)
    require(intr_host.shape == (F, 5), "intrinsics must be [F, 5], one row per test frame")
    intr = torch.from_numpy(np.ascontiguousarray(intr_host)).to(dev)
    require(int(mode) in (MODE_SEGMENT, MODE_SILHOUETTE), "mode must be 0 (segment rule) or 1 (silhouette rule)")
    require(label is not None or int(mode) == MODE_SILHOUETTE, "the segment rule (mode 0) needs the label image")
    if label is not None:
        want_host = np.asarray(want.cpu() if isinstance(want, torch.Tensor) else want, np.int64).reshape(-1)
        want_host = np.ascontiguousarray(np.broadcast_to(want_host, (B,)) if len(want_host) == 1 else want_host)
        require(len(want_host) == B, "want must be [B]")
        want_dev = torch.from_numpy(want_host.astype(np.int32)).to(dev)
    else:
        want_dev = None
    tau_host = np.asarray(tau.cpu() if isinstance(tau, torch.Tensor) else tau, np.float64)
    tau_host = np.broadcast_to(tau_host.reshape(-1) if tau_host.ndim else tau_host, (B,))
    tau_dev = torch.from_numpy(tau_units(tau_host, intr_host[fo_host, 4].astype(np.float64))).to(dev)
    fo = torch.from_numpy(fo_host.astype(np.int32)).to(dev)
    fo64 = fo.to(torch.int64)
    n = max(int(samples_per_launch), 1)
    parts, dropped = [], []
    for lo in range(0, B, n):
        hi = min(lo + n, B)
        c = hi - lo
        idx = np.repeat(np.arange(lo, hi), P)
        J = len(idx)
        rows = intr.index_select(0, fo64[torch.from_numpy(idx).to(dev)])
        depth, _, _, counts, _ = render.render_instances(p, rows, np.arange(J + 1), mesh[idx], np.ones(J, np.int64),
                                                         poses[lo:hi].reshape(J, 16), H, W)
        parts.append(fit_counts(dt, label, fo[lo:hi], None if want_dev is None else want_dev[lo:hi],
                                depth.view(c, P, H, W), tau_dev[lo:hi], check_frames=False))
        dropped.append(counts[0].view(c, P))
    out = {k: torch.cat([q[k] for q in parts]) for k in ("counts", "seg_total", "abs_sum")}
    out.update(select(out["counts"], out["seg_total"], valid, poses, mode))
    out["dropped"] = torch.cat(dropped).cpu().numpy()
    return out
