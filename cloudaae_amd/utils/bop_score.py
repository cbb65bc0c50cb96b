"""BOP's pose errors: the visible surface discrepancy (VSD), the maximum symmetry-aware surface distance (MSSD) and
projection distance (MSPD), and the average recall the BOP benchmark reports since 2019.  The per-pixel comparison is
cloudaae_vsd_counts, the maximum distances cloudaae_pose_max_dist (csrc/bop_score.hip); the images VSD compares are
rendered by cloudaae_render_frames (utils/render.py).  The data-set summary is NumPy float64 on the host.  The
definition is in DESIGN.md ("BOP pose errors (VSD, MSSD, MSPD)"): BOP's, as recalled, not checked -- bop_toolkit was
not available.

    r = vsd(meshes, mesh_index, est, gt, depth_test, intrinsics, frame_of, diameters)     # r['errors'] [B,P,K]
    d = mssd_mspd(model_xyz, est, gt, intrinsics, symmetries=[symmetry_rotations((0, 0, 1), (0, 0, 0), 4)] * B)

The symmetry transforms of an object are the caller's: BOP keeps them in models_info.json, which is not part of this
project, and the transform sets of pose_score.SYMMETRIC_CLASSES are not known here.  The default is the identity alone.
"""
import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .frame_inputs import check_depth, check_poses
from .icp import _points

VSD_DELTA = 0.015                                        # metres
VSD_TAUS = tuple(0.05 * k for k in range(1, 11))         # times the object's diameter
THETAS = tuple(0.05 * j for j in range(1, 11))           # correctness thresholds of VSD; times the diameter: of MSSD
MSPD_PIXELS = tuple(5.0 * j for j in range(1, 11))       # times width / 640
MAX_TAUS = 16


def vsd_counts(depth_test, intrinsics, frame_of, depth_gt, depth_est, delta, taus, check_frames=True):
    """cloudaae_vsd_counts.  depth_test [F,H,W], depth_gt [B,H,W], depth_est [B,P,H,W]: int16 tensors holding the uint16
    bits (what render_frames returns) or uint16; intrinsics [F,5] float32; frame_of [B] int32 in [0, F) (checked here
    with one read-back unless check_frames is False: the kernel gives an entry outside zero counts); taus [B,K] float64
    in metres, K <= 16.  -> dict of inter, union [B,P], over [B,P,K], visib_gt [B] int32 on the device."""
    dt, dg, de = check_depth(depth_test, "depth_test", 3), check_depth(depth_gt, "depth_gt", 3), check_depth(depth_est, "depth_est", 4)
    F, H, W = (int(x) for x in dt.shape)
    B, P = int(de.shape[0]), int(de.shape[1])
    dev = dt.device
    require(tuple(dg.shape) == (B, H, W) and tuple(de.shape) == (B, P, H, W) and B >= 1 and P >= 1,
            "depth_gt must be [B, H, W] and depth_est [B, P, H, W] with the test frames' H and W")
    require(isinstance(intrinsics, torch.Tensor) and intrinsics.dtype == torch.float32 and tuple(intrinsics.shape) == (F, 5),
            "intrinsics must be a float32 [F, 5] tensor")
    require(isinstance(frame_of, torch.Tensor) and frame_of.dtype == torch.int32 and tuple(frame_of.shape) == (B,),
            "frame_of must be an int32 [B] tensor")
    require(isinstance(taus, torch.Tensor) and taus.dtype == torch.float64 and taus.dim() == 2 and taus.shape[0] == B and
            1 <= taus.shape[1] <= MAX_TAUS, "taus must be a float64 [B, K] tensor with 1 <= K <= 16")
    require(all(t.device == dev for t in (dg, de, intrinsics, frame_of, taus)), "all inputs must be on one device")
    if check_frames:
        fo = frame_of.cpu().numpy()
        require(fo.min() >= 0 and fo.max() < F, "a frame_of entry outside [0, F)")
    K = int(taus.shape[1])
    inter = _lib.empty((B, P), dtype=torch.int32, device=dev)
    uni = _lib.empty((B, P), dtype=torch.int32, device=dev)
    over = _lib.empty((B, P, K), dtype=torch.int32, device=dev)
    visib = _lib.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_vsd_counts(F, H, W, ptr(dt), ptr(intrinsics.contiguous()), B, P,
                                                  ptr(frame_of.contiguous()), ptr(dg), ptr(de), float(delta), K,
                                                  ptr(taus.contiguous()), ptr(inter), ptr(uni), ptr(over), ptr(visib),
                                                  stream()), "cloudaae_vsd_counts")
    return {"inter": inter, "union": uni, "over": over, "visib_gt": visib}


def vsd_errors(inter, union, over):
    """e_k = (over[k] + union - inter) / union in float64, 1.0 where union = 0: [B,P,K] from the counts (tensors or
    arrays; the result is of the same kind)."""
    if isinstance(over, torch.Tensor):
        u = union.to(torch.float64).unsqueeze(-1)
        num = (over + (union - inter).unsqueeze(-1)).to(torch.float64)
        return torch.where(u == 0, torch.ones_like(num), num / torch.where(u == 0, torch.ones_like(u), u))
    u = np.asarray(union, np.float64)[..., None]
    num = (np.asarray(over, np.int64) + (np.asarray(union, np.int64) - np.asarray(inter, np.int64))[..., None]).astype(np.float64)
    return np.where(u == 0, 1.0, num / np.where(u == 0, 1.0, u))


def vsd(meshes, mesh_index, est, gt, depth_test, intrinsics, frame_of, diameters, delta=VSD_DELTA, taus=VSD_TAUS,
        samples_per_launch=8):
    """VSD of the estimates est [B,P,4,4] (or [B,4,4]: P = 1) against the ground truth gt [B,4,4] (float64, model ->
    camera, on the device) in the test frames depth_test [F,H,W] (int16 bits or uint16, device) with intrinsics [F,5];
    frame_of [B]: each sample's frame; meshes: a PackedMeshes (or what mesh_models.pack_meshes takes) and mesh_index [B]
    (host integers): each sample's mesh; diameters [B] in metres (a number, an array or a tensor): tau_k = taus[k] *
    diameter, formed in float64 on the host.  The mesh is rendered alone under the ground truth and under every
    estimate with its frame's intrinsics (label 1, B (1 + P) one-instance frames, samples_per_launch samples per
    launch) and counted by cloudaae_vsd_counts.  -> dict of errors [B,P,K] float64 (device), inter, union [B,P], over
    [B,P,K], visib_gt [B] int32 (device) and dropped [B,1+P] int32 (numpy, one read-back at the end: the triangles the
    renderer left out under the ground truth (column 0) and each estimate -- a pose that puts the mesh through the near
    plane shows here)."""
    from . import mesh_models, render
    p = mesh_models.pack_meshes(meshes)
    dev = p.device
    dt = check_depth(depth_test, "depth_test", 3)
    F, H, W = (int(x) for x in dt.shape)
    require(isinstance(gt, torch.Tensor) and gt.dim() == 3, "gt must be a float64 [B, 4, 4] tensor")
    B = int(gt.shape[0])
    gt = check_poses(gt, "gt", (3,), B, dev)
    est = check_poses(est, "est", (3, 4), B, dev)
    P = int(est.shape[1]) if est.dim() == 4 else 1
    est = est.view(B, P, 16)
    mesh = np.asarray(mesh_index.cpu() if isinstance(mesh_index, torch.Tensor) else mesh_index, np.int64).reshape(-1)
    require(len(mesh) == B and mesh.min() >= 0 and mesh.max() < len(p.num_triangles), "mesh_index must be [B], inside the meshes")
    fo_host = np.asarray(frame_of.cpu() if isinstance(frame_of, torch.Tensor) else frame_of, np.int64).reshape(-1)
    require(len(fo_host) == B and fo_host.min() >= 0 and fo_host.max() < F, "frame_of must be [B] with entries in [0, F)")
    intr = intrinsics if isinstance(intrinsics, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(intrinsics, np.float32))
    intr = intr.to(device=dev, dtype=torch.float32).contiguous()
    require(tuple(intr.shape) == (F, 5), "intrinsics must be [F, 5], one row per test frame")
    diam = np.asarray(diameters.cpu() if isinstance(diameters, torch.Tensor) else diameters, np.float64)
    diam = np.ascontiguousarray(np.broadcast_to(diam.reshape(-1) if diam.ndim else diam, (B,)))
    tk = np.asarray(taus, np.float64).reshape(-1)
    require(1 <= len(tk) <= MAX_TAUS, "1 to 16 thresholds tau")
    tau = torch.from_numpy(tk[None, :] * diam[:, None]).to(dev)          # [B,K] float64, the product formed here
    fo = torch.from_numpy(fo_host.astype(np.int32)).to(dev)
    fo64 = fo.to(torch.int64)
    n = max(int(samples_per_launch), 1)
    parts, dropped = [], []
    for lo in range(0, B, n):
        hi = min(lo + n, B)
        c = hi - lo
        # the ground-truth frames of the chunk first, then its estimates: both blocks are contiguous
        poses = torch.cat([gt[lo:hi].reshape(c, 16), est[lo:hi].reshape(c * P, 16)])
        idx = np.concatenate([np.arange(lo, hi), np.repeat(np.arange(lo, hi), P)])
        J = len(idx)
        rows = intr.index_select(0, fo64[torch.from_numpy(idx).to(dev)])
        depth, _, _, counts, _ = render.render_instances(p, rows, np.arange(J + 1), mesh[idx], np.ones(J, np.int64), poses,
                                                         H, W)
        parts.append(vsd_counts(dt, intr, fo[lo:hi], depth[:c], depth[c:].view(c, P, H, W), delta, tau[lo:hi],
                                check_frames=False))
        dropped.append(torch.cat([counts[0, :c].view(c, 1), counts[0, c:].view(c, P)], dim=1))
    out = {k: torch.cat([q[k] for q in parts]) for k in ("inter", "union", "over", "visib_gt")}
    out["errors"] = vsd_errors(out["inter"], out["union"], out["over"])
    out["dropped"] = torch.cat(dropped).cpu().numpy()
    return out


def symmetry_rotations(axis, offset, n):
    """[n,4,4] float64: the rotations by 2 pi k / n (k = 0 .. n - 1; k = 0 is the identity exactly) about the line
    through `offset` along `axis` -- a discrete rotational symmetry of order n, and how BOP discretises a continuous
    one (there with n chosen so that the surface moves by at most a small share of the diameter between steps)."""
    a = np.asarray(axis, np.float64).reshape(3)
    o = np.asarray(offset, np.float64).reshape(3)
    n = int(n)
    require(n >= 1 and float(np.sqrt((a * a).sum())) > 0.0, "n >= 1 and a non-zero axis")
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    out = np.zeros((n, 4, 4), np.float64)
    for k in range(n):
        T = np.eye(4)
        if k:
            th = 2.0 * np.pi * k / n
            T[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
            T[:3, 3] = o - T[:3, :3] @ o
        out[k] = T
    return out


def pack_symmetries(symmetries, B):
    """Per-sample transform sets (a list of B arrays [n_b,4,4]; None or an entry None: the identity alone) ->
    (sym [B,smax,4,4] float64 padded with identities, num_sym [B] int32), NumPy."""
    sets = [None] * B if symmetries is None else list(symmetries)
    require(len(sets) == B, "symmetries: one transform set per sample")
    sets = [np.eye(4)[None] if s is None else np.asarray(s, np.float64).reshape(-1, 4, 4) for s in sets]
    require(all(len(s) >= 1 for s in sets), "a transform set must hold the identity at least")
    smax = max(len(s) for s in sets)
    sym = np.tile(np.eye(4), (B, smax, 1, 1))
    for b, s in enumerate(sets):
        sym[b, :len(s)] = s
    return sym, np.array([len(s) for s in sets], np.int32)


def mssd_mspd(model_xyz, est, gt, intrinsics=None, symmetries=None):
    """MSSD and MSPD of the estimates est [B,P,4,4] (or [B,4,4]) against gt [B,4,4] (float64) on the model points
    model_xyz [B,M,>=3] float32 (row strides allowed), by cloudaae_pose_max_dist.  intrinsics [B,5] float32: each
    sample's frame's; None: no MSPD.  symmetries: per sample an array [n_b,4,4] that holds the identity (see
    pack_symmetries), or None.  -> dict of mssd [B,P] (metres) and, with intrinsics, mspd [B,P] (pixels; +inf when a
    point lies at Z <= 0 under a pose), float64 on the device."""
    mp, mps, mcs, M = _points(model_xyz, "model_xyz")
    B, dev = int(model_xyz.shape[0]), model_xyz.device
    gt = check_poses(gt, "gt", (3,), B, dev)
    est = check_poses(est, "est", (3, 4), B, dev)
    P = int(est.shape[1]) if est.dim() == 4 else 1
    if intrinsics is not None:
        require(isinstance(intrinsics, torch.Tensor) and intrinsics.dtype == torch.float32 and
                tuple(intrinsics.shape) == (B, 5) and intrinsics.device == dev, "intrinsics must be a float32 [B, 5] tensor")
        intrinsics = intrinsics.contiguous()
    sym, num = pack_symmetries(symmetries, B)
    smax = int(sym.shape[1])
    sym_d, num_d = torch.from_numpy(sym).to(dev), torch.from_numpy(num).to(dev)
    L = _lib.lib()
    mssd = _lib.empty((B, P), dtype=torch.float64, device=dev)
    mspd = _lib.empty((B, P), dtype=torch.float64, device=dev) if intrinsics is not None else None
    ws = _lib.empty((int(L.cloudaae_pose_max_dist_workspace_bytes(B, P, smax)) // 8,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_pose_max_dist(B, P, M, mp, mps, mcs, ptr(est), ptr(gt), smax, ptr(num_d), ptr(sym_d),
                                            ptr(intrinsics), ptr(mssd), ptr(mspd), ptr(ws), stream()),
                   "cloudaae_pose_max_dist")
    out = {"mssd": mssd}
    if mspd is not None:
        out["mspd"] = mspd
    return out


# ---- the data-set summary (host, NumPy float64) ----------------------------------------------------------------------

def recall(errors, thetas):
    """[n]: per sample the share of (k, j) with errors[i, k] < thetas[i, j] (strict).  errors [n] or [n,K]; thetas [J]
    (the same for every sample) or [n,J]."""
    e = np.asarray(errors, np.float64)
    e = e.reshape(len(e), -1)
    t = np.asarray(thetas, np.float64)
    t = np.broadcast_to(t.reshape(1, -1) if t.ndim == 1 else t, (len(e), t.shape[-1]))
    if len(e) == 0:
        return np.zeros(0, np.float64)
    return (e[:, :, None] < t[:, None, :]).mean(axis=(1, 2))


class BopScoreLog(object):
    """Collects the per-sample rows of an evaluation (class, seq, frame, the VSD errors, MSSD and MSPD of each scored
    pose) on the device, reads them back once and summarises them per class and over all: AR_VSD, AR_MSSD, AR_MSPD
    (each the mean over the samples of recall(...)) and AR, their mean.  poses: the names of the scored poses in the
    order of P; diameters: [C] model diameters in metres (the MSSD thresholds are THETAS times the class's)."""

    def __init__(self, poses=("pred",), diameters=None, thetas=THETAS, mspd_pixels=MSPD_PIXELS):
        self.poses = tuple(poses)
        require(diameters is not None, "BopScoreLog needs the classes' diameters")
        if isinstance(diameters, torch.Tensor):
            diameters = diameters.detach().cpu().numpy()
        self.diameters = np.asarray(diameters, np.float64).reshape(-1)
        self.thetas = np.asarray(thetas, np.float64)
        self.mspd_pixels = np.asarray(mspd_pixels, np.float64)
        self._dev = []           # (class_id [B], [B, P (K + 2)] float64) device copies
        self._host = []          # (seq, frame, width [B]) host
        self._k = None
        self._rows = None

    def append(self, class_id, vsd, mssd, mspd, width, seq=None, frame=None):
        """vsd [B,P,K], mssd, mspd [B,P] float64 device tensors; width: the frames' width in pixels (the MSPD
        thresholds are mspd_pixels * width / 640)."""
        B, P = int(class_id.shape[0]), len(self.poses)
        require(vsd.dim() == 3 and tuple(vsd.shape[:2]) == (B, P) and tuple(mssd.shape) == (B, P) and
                tuple(mspd.shape) == (B, P), "vsd must be [B, %d, K], mssd and mspd [B, %d]" % (P, P))
        K = int(vsd.shape[2])
        require(self._k in (None, K), "the number of VSD thresholds changed between batches")
        self._k = K
        row = torch.cat([vsd.detach().reshape(B, P * K), mssd.detach(), mspd.detach()], dim=1)
        self._dev.append((class_id.detach().to(torch.int64).clone(), row))
        fill = np.full(B, -1, np.int64)
        self._host.append((fill if seq is None else np.asarray(seq, np.int64).reshape(B),
                           fill if frame is None else np.asarray(frame, np.int64).reshape(B),
                           np.full(B, float(width), np.float64)))
        self._rows = None

    def rows(self):
        """dict of class_id, seq, frame [n] int64, width [n], vsd [n,P,K], mssd, mspd [n,P] float64 (NumPy): one
        read-back."""
        if self._rows is None:
            P, K = len(self.poses), self._k or 0
            if self._dev:
                cls = torch.cat([c for c, _ in self._dev]).cpu().numpy()
                allr = torch.cat([r for _, r in self._dev]).cpu().numpy()
                seq, frame, width = (np.concatenate([h[i] for h in self._host]) for i in range(3))
            else:
                cls = seq = frame = np.zeros(0, np.int64)
                width = np.zeros(0, np.float64)
                allr = np.zeros((0, P * (K + 2)))
            n = len(cls)
            self._rows = dict(class_id=cls, seq=seq, frame=frame, width=width, vsd=allr[:, :P * K].reshape(n, P, K),
                              mssd=allr[:, P * K:P * K + P], mspd=allr[:, P * K + P:])
        return self._rows

    def _block(self, r, sel):
        cls = r["class_id"][sel]
        n = int(len(cls))
        out = {}
        for k, pose in enumerate(self.poses):
            if n == 0:
                out[pose] = {"n": 0, "ar_vsd": 0.0, "ar_mssd": 0.0, "ar_mspd": 0.0, "ar": 0.0}
                continue
            v = float(recall(r["vsd"][sel, k], self.thetas).mean())
            s = float(recall(r["mssd"][sel, k], self.thetas[None, :] * self.diameters[cls][:, None]).mean())
            p = float(recall(r["mspd"][sel, k], self.mspd_pixels[None, :] * (r["width"][sel] / 640.0)[:, None]).mean())
            out[pose] = {"n": n, "ar_vsd": v, "ar_mssd": s, "ar_mspd": p, "ar": (v + s + p) / 3.0}
        return out

    def summary(self):
        """{'classes': {c: block}, 'all': block}; block[pose] = dict(n, ar_vsd, ar_mssd, ar_mspd, ar)."""
        r = self.rows()
        classes = {int(c): self._block(r, r["class_id"] == c) for c in np.unique(r["class_id"])}
        return {"classes": classes, "all": self._block(r, np.ones(len(r["class_id"]), bool))}

    def lines(self):
        """The summary as text: one line per class (and one over all) and pose."""
        s = self.summary()
        out = []
        for name, block in [("class %d" % c, b) for c, b in sorted(s["classes"].items())] + [("all", s["all"])]:
            for pose in self.poses:
                v = block[pose]
                out.append("bop %s %s n %d ar_vsd %f ar_mssd %f ar_mspd %f ar %f"
                           % (name, pose, v["n"], v["ar_vsd"], v["ar_mssd"], v["ar_mspd"], v["ar"]))
        return out
