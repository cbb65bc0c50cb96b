"""Pose scores: ADD, ADD-S, their area under the accuracy-threshold curve and the shares below 2 cm / a tenth of the
object's diameter -- the numbers 6D pose results on YCB-Video are reported in.  The per-sample distances come from
cloudaae_pose_score (one HIP launch for the batch and all scored poses); the data-set summary is NumPy float64 on
the host: it runs once over a few thousand numbers.  The definition is in DESIGN.md ("Pose scores")."""
import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .icp import _points

# the symmetric objects of YCB-Video, 0-based (bowl, wood block, large clamp, extra large clamp, foam brick; as recalled
# from PoseCNN's list 13, 16, 19, 20, 21)
SYMMETRIC_CLASSES = (12, 15, 18, 19, 20)
AUC_LIMIT = 0.1          # metres


def pose_matrix(rot, trans):
    """[B,4,4] float64 poses [Rodrigues(rot) | trans; 0 0 0 1] from an axis-angle rot [B,3] (float32 or float64) and a
    float32 translation [B,3]: T0 of DESIGN.md "Pose refinement" (a zero rot is the identity)."""
    require(isinstance(rot, torch.Tensor) and rot.dim() == 2 and rot.shape[1] == 3 and
            rot.dtype in (torch.float32, torch.float64), "rot must be a float32 or float64 [B, 3] tensor")
    B = int(rot.shape[0])
    require(isinstance(trans, torch.Tensor) and tuple(trans.shape) == (B, 3) and trans.dtype == torch.float32,
            "trans must be a float32 [B, 3] tensor")
    require(trans.device == rot.device, "all inputs must be on one device")
    out = _lib.empty((B, 4, 4), dtype=torch.float64, device=rot.device)
    _lib.check(_lib.lib().cloudaae_pose_matrix(B, ptr(rot.contiguous()), int(rot.dtype == torch.float64),
                                               ptr(trans.contiguous()), ptr(out), stream()), "cloudaae_pose_matrix")
    return out


def stack_poses(first, second):
    """[B,2,4,4] from two [B,4,4] float64 pose sets: the est of one score_poses call with two poses per sample."""
    for t in (first, second):
        require(isinstance(t, torch.Tensor) and t.dim() == 3 and tuple(t.shape[1:]) == (4, 4) and
                t.dtype == torch.float64, "poses must be float64 [B, 4, 4] tensors")
    require(first.shape == second.shape and first.device == second.device, "the two pose sets must match")
    B = int(first.shape[0])
    out = _lib.empty((B, 2, 4, 4), dtype=torch.float64, device=first.device)
    _lib.check(_lib.lib().cloudaae_pose_stack(B, ptr(first.contiguous()), ptr(second.contiguous()), ptr(out), stream()),
               "cloudaae_pose_stack")
    return out


def score_poses(model_xyz, est, gt, return_nn_d2=False):
    """ADD and ADD-S of the estimates est [B,P,4,4] (or [B,4,4]: P = 1) against the ground truth gt [B,4,4], float64,
    on the object models model_xyz [B,M,>=3] float32 (row strides allowed: obj_batch [B,2048,6]).  Returns a dict of
    add, adds [B,P] float64 and, on request, nn_d2 [B,P,M].  Only the library's kernels run (outputs from
    _lib.empty), so the call records into a StepPlan and replays."""
    mp, mps, mcs, M = _points(model_xyz, "model_xyz")
    B = int(model_xyz.shape[0])
    require(isinstance(est, torch.Tensor) and est.dtype == torch.float64 and est.dim() in (3, 4) and
            tuple(est.shape[-2:]) == (4, 4) and est.shape[0] == B, "est must be a float64 [B, P, 4, 4] tensor")
    P = int(est.shape[1]) if est.dim() == 4 else 1
    require(isinstance(gt, torch.Tensor) and gt.dtype == torch.float64 and tuple(gt.shape) == (B, 4, 4),
            "gt must be a float64 [B, 4, 4] tensor")
    dev = model_xyz.device
    require(est.device == dev and gt.device == dev, "all inputs must be on one device")
    L = _lib.lib()
    add = _lib.empty((B, P), dtype=torch.float64, device=dev)
    adds = _lib.empty((B, P), dtype=torch.float64, device=dev)
    nn = _lib.empty((B, P, M), dtype=torch.float64, device=dev) if return_nn_d2 else None
    ws = _lib.empty((int(L.cloudaae_pose_score_workspace_bytes(B, P, M)) // 8,), dtype=torch.float64, device=dev)
    _lib.check(L.cloudaae_pose_score(B, P, M, mp, mps, mcs, ptr(est.contiguous()), ptr(gt.contiguous()), ptr(add),
                                     ptr(adds), ptr(nn), ptr(ws), stream()), "cloudaae_pose_score")
    out = dict(add=add, adds=adds)
    if return_nn_d2:
        out["nn_d2"] = nn
    return out


def model_diameter(models):
    """[C] float64: the largest distance between two points of each model [C,M,>=3] float32 (row strides allowed)."""
    mp, mps, mcs, M = _points(models, "models")
    C = int(models.shape[0])
    L = _lib.lib()
    diam = _lib.empty((C,), dtype=torch.float64, device=models.device)
    ws = _lib.empty((int(L.cloudaae_cloud_diameter_workspace_bytes(C, M)) // 8,), dtype=torch.float64,
                    device=models.device)
    _lib.check(L.cloudaae_cloud_diameter(C, M, mp, mps, mcs, ptr(diam), ptr(ws), stream()), "cloudaae_cloud_diameter")
    return diam


# ---- the data-set summary (host, NumPy float64) ----------------------------------------------------------------------

def auc(d, limit=AUC_LIMIT):
    """Area under the accuracy-threshold curve up to `limit`, the YCB-Video toolbox's VOCap (as recalled, not checked):
    distances above the limit dropped, the rest sorted; accuracy k / n with n counting the dropped ones; the step
    priced at its right end, a run of equal distances at the accuracy of its first member; divided by the limit."""
    d = np.asarray(d, np.float64).reshape(-1)
    n = len(d)
    kept = np.sort(d[d <= limit])
    if n == 0 or len(kept) == 0:
        return 0.0
    acc = np.arange(1, len(kept) + 1, dtype=np.float64) / n
    mrec = np.concatenate([[0.0], kept, [limit]])
    mpre = np.concatenate([[0.0], acc, [acc[-1]]])
    mpre = np.maximum.accumulate(mpre)
    i = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]) / limit)


def summarize(d, diameter=None, limit=AUC_LIMIT):
    """dict(n, mean, auc, acc_2cm, acc_0.1d) of distances d [n]; diameter: a number or [n] (each sample's class's);
    acc_0.1d is None without one.  Strict <."""
    d = np.asarray(d, np.float64).reshape(-1)
    n = len(d)
    out = {"n": n, "mean": float(d.mean()) if n else 0.0, "auc": auc(d, limit),
           "acc_2cm": float(np.mean(d < 0.02)) if n else 0.0, "acc_0.1d": None}
    if diameter is not None:
        out["acc_0.1d"] = float(np.mean(d < 0.1 * np.broadcast_to(np.asarray(diameter, np.float64), d.shape))) if n else 0.0
    return out


METRICS = ("add", "adds", "add(-s)")


class PoseScoreLog(object):
    """Collects the per-sample rows of an evaluation (class, seq, frame, ADD and ADD-S of each scored pose) on the
    device, reads them back once and summarises them per class and over all.
    poses: the names of the scored poses in the order of P (e.g. ("pred", "icp")); diameters: [C] model diameters
    (model_diameter; None: no acc_0.1d)."""

    def __init__(self, poses=("pred",), diameters=None, symmetric=SYMMETRIC_CLASSES, limit=AUC_LIMIT):
        self.poses = tuple(poses)
        self.symmetric = frozenset(int(c) for c in symmetric)
        self.limit = float(limit)
        if isinstance(diameters, torch.Tensor):
            diameters = diameters.detach().cpu().numpy()
        self.diameters = None if diameters is None else np.asarray(diameters, np.float64)
        self._dev = []           # (class_id [B], add [B,P], adds [B,P]) device copies
        self._host = []          # (seq [B], frame [B]) host
        self._rows = None

    def append(self, class_id, add, adds, seq=None, frame=None):
        B = int(class_id.shape[0])
        require(tuple(add.shape) == (B, len(self.poses)) and tuple(adds.shape) == (B, len(self.poses)),
                "add and adds must be [B, %d]" % len(self.poses))
        # copies: a replayed evaluation overwrites its outputs in place
        self._dev.append((class_id.detach().to(torch.int64).clone(), add.detach().clone(), adds.detach().clone()))
        fill = np.full(B, -1, np.int64)
        self._host.append((fill if seq is None else np.asarray(seq, np.int64).reshape(B),
                           fill if frame is None else np.asarray(frame, np.int64).reshape(B)))
        self._rows = None

    def rows(self):
        """dict of class_id, seq, frame [n] int64 and add, adds [n,P] float64 (NumPy): one read-back."""
        if self._rows is None:
            P = len(self.poses)
            if self._dev:
                cls = torch.cat([c for c, _, _ in self._dev]).cpu().numpy()
                both = torch.cat([torch.cat([a, s], dim=1) for _, a, s in self._dev]).cpu().numpy()
                seq = np.concatenate([s for s, _ in self._host])
                frame = np.concatenate([f for _, f in self._host])
            else:
                cls = seq = frame = np.zeros(0, np.int64)
                both = np.zeros((0, 2 * P))
            self._rows = dict(class_id=cls, seq=seq, frame=frame, add=both[:, :P], adds=both[:, P:])
        return self._rows

    def _block(self, r, sel):
        cls = r["class_id"][sel]
        sym = np.isin(cls, sorted(self.symmetric))
        diam = None if self.diameters is None else self.diameters[cls]
        out = {}
        for k, pose in enumerate(self.poses):
            a, s = r["add"][sel, k], r["adds"][sel, k]
            dist = {"add": a, "adds": s, "add(-s)": np.where(sym, s, a)}
            out[pose] = {m: summarize(dist[m], diam, self.limit) for m in METRICS}
        return out

    def summary(self):
        """{'classes': {c: block}, 'all': block}; block[pose][metric] = summarize(...), metric in METRICS."""
        r = self.rows()
        classes = {int(c): self._block(r, r["class_id"] == c) for c in np.unique(r["class_id"])}
        return {"classes": classes, "all": self._block(r, np.ones(len(r["class_id"]), bool))}

    def lines(self):
        """The summary as text: one line per class (and one over all), pose and metric."""
        s = self.summary()
        out = []
        for name, block in [("class %d" % c, b) for c, b in sorted(s["classes"].items())] + [("all", s["all"])]:
            for pose in self.poses:
                for m in METRICS:
                    v = block[pose][m]
                    line = "score %s %s %s n %d mean %f auc %f acc_2cm %f" % (name, pose, m, v["n"], v["mean"], v["auc"],
                                                                               v["acc_2cm"])
                    if v["acc_0.1d"] is not None:
                        line += " acc_0.1d %f" % v["acc_0.1d"]
                    out.append(line)
        return out
