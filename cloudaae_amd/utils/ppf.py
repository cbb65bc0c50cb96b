"""Pose proposals by point-pair-feature voting (Drost, Ulrich, Navab, Ilic 2010, as recalled): hypotheses for the pose
of a known object in a depth segment from nothing but oriented points -- no network, no ground truth.  The pairs of an
object model are tabulated once by a quantised feature (cloudaae_ppf_model_pairs, a direct-address CSR built with
torch.sort); the pairs of a scene vote for (model point, rotation about the normal) cells (cloudaae_ppf_vote); the voted
poses are clustered greedily (cloudaae_ppf_cluster; csrc/ppf.hip).  The definition is in DESIGN.md ("Pose proposals").

    models = PPFModels.from_meshes(mesh_files, num_point=256, scale=0.001)        # class i is mesh i
    normals, mask = scene_normals(scene, radius=0.01)                             # scene [B,N,3] float32, camera frame
    r = propose_poses(models, scene, normals, mask, class_id, top=4)
    r['pose'] [B,top,4,4], r['score'] [B,top], r['valid'] [B,top]                 # model -> camera, best first

The model normals must point out of the object: from_meshes takes the face normals, whose sign is the winding's, so a
mesh whose winding is not consistently outward is the caller's to repair.  Scene normals face the camera."""
import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

N_ANGLE, N_ALPHA, N_DIST = 15, 30, 20      # 12 degree feature bins, 12 degree rotation bins, 20 distance bins
DIST_FRACTION = 0.05                       # dist_step = 0.05 diameter
TRANS_FRACTION = 0.1                       # trans_thresh = diameter / 10; rot_thresh = 2 pi / n_alpha
MAX_LDS_BYTES = 158 * 1024                 # the accumulator's share of a workgroup's LDS (csrc/ppf.hip)
MAX_CANDIDATES = 4096


def quantisation_tables(n_angle=N_ANGLE, n_alpha=N_ALPHA):
    """The host-made tables (NumPy float64): cos_edges [n_angle-1] = cos(k pi / n_angle), alpha_edges [n_alpha/2-1] =
    cos(k pi / (n_alpha/2)), alpha_cs [n_alpha,2] = cosine and sine of the bin centres -pi + (j + 1/2) 2 pi / n_alpha."""
    require(1 <= int(n_angle) <= 64, "n_angle must lie in [1, 64]")
    require(int(n_alpha) % 2 == 0 and 2 <= int(n_alpha) <= 128, "n_alpha must be even, in [2, 128]")
    half = int(n_alpha) // 2
    cos_edges = np.cos(np.arange(1, int(n_angle), dtype=np.float64) * (np.pi / int(n_angle)))
    alpha_edges = np.cos(np.arange(1, half, dtype=np.float64) * (np.pi / half))
    centres = -np.pi + (np.arange(int(n_alpha), dtype=np.float64) + 0.5) * (2.0 * np.pi / int(n_alpha))
    return cos_edges, alpha_edges, np.stack([np.cos(centres), np.sin(centres)], axis=1)


def _table(a, dev, n):
    """A table on the device, never empty (a table without entries is one unread zero)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(n, a.dtype)).to(dev)


class PPFModels(object):
    """The oriented point models of num_class classes and their pair tables, on one device: offsets [num_class+1] int32
    into xyz [Mt,3] float32 and normals [Mt,3] float64 (a class without a model owns no point), diameters, dist_step,
    trans_thresh2 [num_class] float64, the three quantisation tables, and the CSR bucket_start [num_class, n_key+1] int32,
    entry_ref [E] int32, entry_dir [E,2] float32; pair_key / pair_ref / pair_dir are what cloudaae_ppf_model_pairs wrote."""

    @classmethod
    def from_points(cls, xyz, normals, diameters, classes=None, num_class=None, n_angle=N_ANGLE, n_alpha=N_ALPHA,
                    n_dist=N_DIST, dist_fraction=DIST_FRACTION, trans_fraction=TRANS_FRACTION, device=None):
        """xyz: [S,M,>=3] or a list of [M_i,>=3] point sets (float32), normals alike (float64 unit vectors, outward),
        diameters [S] (metres); set i is class classes[i] (default i) of num_class."""
        def rows(t, ty):
            return [np.ascontiguousarray(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)[:, :3], ty) for x in t]
        xs, ns = rows(xyz, np.float32), rows(normals, np.float64)
        S = len(xs)
        require(S >= 1 and len(ns) == S and all(len(x) == len(n) and len(x) >= 2 for x, n in zip(xs, ns)),
                "one normal per point and at least two points per set")
        diam = np.asarray(diameters.detach().cpu() if isinstance(diameters, torch.Tensor) else diameters, np.float64).reshape(-1)
        require(len(diam) == S and np.isfinite(diam).all() and (diam > 0).all(), "one positive diameter per set")
        classes = list(range(S)) if classes is None else [int(c) for c in classes]
        require(len(classes) == S and len(set(classes)) == S and min(classes) >= 0, "one distinct class id >= 0 per set")
        C = max(classes) + 1 if num_class is None else int(num_class)
        require(C > max(classes), "a class id outside [0, num_class)")
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self = cls()
        self.device, self.num_class = device, C
        self.n_angle, self.n_alpha, self.n_dist = int(n_angle), int(n_alpha), int(n_dist)
        self.n_key = self.n_dist * self.n_angle ** 3
        require(self.n_dist >= 1 and self.n_key <= (1 << 24), "n_dist must be >= 1 and n_dist * n_angle^3 <= 2^24")
        self.tables = quantisation_tables(n_angle, n_alpha)
        order = np.argsort(classes)                              # the sets in class order
        sizes = np.zeros(C, np.int64)
        d_all = np.ones(C, np.float64)
        for i in order:
            sizes[classes[i]] = len(xs[i])
            d_all[classes[i]] = diam[i]
        self.sizes, self.diameters = sizes, d_all
        self.m_max, self.m_total = int(sizes.max()), int(sizes.sum())
        require(4 * self.m_max * self.n_alpha <= MAX_LDS_BYTES,
                "a model of %d points with %d rotation bins does not fit the voting kernel's LDS (%d bytes)"
                % (self.m_max, self.n_alpha, MAX_LDS_BYTES))
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        pair_offsets = np.concatenate([[0], np.cumsum(sizes * sizes)])
        self.n_pairs = int(pair_offsets[-1])
        require(self.n_pairs <= (1 << 28), "more than 2^28 model pairs")
        self.rot_bound = float(1.0 + 2.0 * np.cos(2.0 * np.pi / self.n_alpha))
        t = float(trans_fraction) * d_all
        self.offsets_host = offsets
        self.offsets = torch.from_numpy(offsets.astype(np.int32)).to(device)
        self.pair_offsets = torch.from_numpy(pair_offsets.astype(np.int64)).to(device)
        self.xyz = torch.from_numpy(np.concatenate([xs[i] for i in order])).to(device)
        self.normals = torch.from_numpy(np.concatenate([ns[i] for i in order])).to(device)
        self.dist_step = torch.from_numpy(float(dist_fraction) * d_all).to(device)
        self.trans_thresh2 = torch.from_numpy(t * t).to(device)
        self.cos_edges = _table(self.tables[0], device, 1)
        self.alpha_edges = _table(self.tables[1], device, 1)
        self.alpha_cs = _table(self.tables[2], device, 2)
        self._build()
        return self

    @classmethod
    def from_meshes(cls, meshes, num_point=256, scale=1.0, seed=None, classes=None, num_class=None, device=None, **kw):
        """num_point surface points with the faces' normals per mesh (mesh_models.models_from_meshes(return_normals=True),
        so the normals point where the winding says), the diameters of the point models, then from_points."""
        from . import mesh_models, pose_score
        seed = mesh_models.DEFAULT_SEED if seed is None else seed
        models, normals = mesh_models.models_from_meshes(meshes, num_point=int(num_point), seed=seed, scale=scale,
                                                         return_normals=True, device=device)
        return cls.from_points(models, normals, pose_score.model_diameter(models), classes, num_class, device=models.device, **kw)

    def _build(self):
        """The pair table (one launch) and its CSR (torch: a stable sort by (class, key), a count and a prefix sum)."""
        dev, P = self.device, self.n_pairs
        self.pair_key = _lib.empty((P,), dtype=torch.int32, device=dev)
        self.pair_ref = _lib.empty((P,), dtype=torch.int32, device=dev)
        self.pair_dir = _lib.empty((P, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cloudaae_ppf_model_pairs(
                self.num_class, ptr(self.offsets), ptr(self.pair_offsets), self.m_total, P, ptr(self.xyz), ptr(self.normals),
                ptr(self.dist_step), self.n_dist, self.n_angle, ptr(self.cos_edges), ptr(self.pair_key), ptr(self.pair_ref),
                ptr(self.pair_dir), stream()), "cloudaae_ppf_model_pairs")
        sizes2 = torch.from_numpy(self.sizes * self.sizes).to(dev)
        owner = torch.repeat_interleave(torch.arange(self.num_class, device=dev), sizes2)
        keep = self.pair_key >= 0
        flat = owner[keep] * self.n_key + self.pair_key[keep].to(torch.int64)
        flat, order = torch.sort(flat, stable=True)
        self.entry_ref = self.pair_ref[keep][order].contiguous()
        self.entry_dir = self.pair_dir[keep][order].contiguous()
        self.n_entries = int(flat.numel())
        count = torch.bincount(flat, minlength=self.num_class * self.n_key)
        start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(count, 0)])
        idx = (torch.arange(self.num_class, device=dev)[:, None] * self.n_key + torch.arange(self.n_key + 1, device=dev)[None])
        self.bucket_start = start[idx].to(torch.int32).contiguous()
        if self.n_entries == 0:
            self.entry_ref, self.entry_dir = None, None


def scene_normals(scene, radius):
    """Normals of the scene clouds scene [B,N,>=3] (float32, camera frame) from their neighbours within `radius`, flipped
    towards the camera at the origin (normals.estimate_normals(viewpoint=(0, 0, 0))).  -> (normals [B,N,3] float64, mask
    [B,N] uint8: 1 where the point had the three neighbours an estimate needs)."""
    from . import normals as normals_util
    n, _, count = normals_util.estimate_normals(scene, radius, viewpoint=(0.0, 0.0, 0.0))
    return n, (count >= 3).to(torch.uint8)


def vote(models, scene_xyz, scene_normals, mask, class_id, ref_step=5, peaks=2, return_acc=False):
    """cloudaae_ppf_vote -> dict(votes, model_index, bin [B,R,peaks] int32, pose [B,R,peaks,4,4] float64 and, with
    return_acc, acc [B,R,m_max,n_alpha] int32), R = ceil(N / ref_step)."""
    require(isinstance(models, PPFModels), "models must be a PPFModels")
    dev = models.device
    require(isinstance(scene_xyz, torch.Tensor) and scene_xyz.dim() == 3 and scene_xyz.shape[2] >= 3 and
            scene_xyz.dtype == torch.float32, "scene_xyz must be a float32 [B, N, >=3] tensor")
    if not scene_xyz.is_cuda:
        raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got a %s tensor" % scene_xyz.device)
    B, N = int(scene_xyz.shape[0]), int(scene_xyz.shape[1])
    require(B >= 1 and N >= 2 and scene_xyz.device == dev, "scene_xyz must hold >= 2 points per sample, on the models' device")
    xyz = scene_xyz[:, :, :3].contiguous()
    require(isinstance(scene_normals, torch.Tensor) and tuple(scene_normals.shape) == (B, N, 3) and
            scene_normals.dtype == torch.float64 and scene_normals.device == dev, "scene_normals must be a float64 [B, N, 3] tensor")
    require(isinstance(mask, torch.Tensor) and tuple(mask.shape) == (B, N) and mask.device == dev and
            mask.dtype in (torch.uint8, torch.bool), "mask must be a uint8 or bool [B, N] tensor")
    require(isinstance(class_id, torch.Tensor) and tuple(class_id.shape) == (B,) and class_id.device == dev,
            "class_id must be [B], on the models' device")
    ref_step, peaks = int(ref_step), int(peaks)
    require(1 <= ref_step <= N and 1 <= peaks <= 4, "ref_step must lie in [1, N] and peaks in [1, 4]")
    R = -(-N // ref_step)
    m8 = mask.to(torch.uint8).contiguous()
    cls = class_id.to(torch.int64).contiguous()
    out = dict(votes=_lib.empty((B, R, peaks), dtype=torch.int32, device=dev),
               model_index=_lib.empty((B, R, peaks), dtype=torch.int32, device=dev),
               bin=_lib.empty((B, R, peaks), dtype=torch.int32, device=dev),
               pose=_lib.empty((B, R, peaks, 4, 4), dtype=torch.float64, device=dev))
    acc = _lib.empty((B, R, models.m_max, models.n_alpha), dtype=torch.int32, device=dev) if return_acc else None
    m = models
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_ppf_vote(
            B, N, ptr(xyz), ptr(scene_normals.contiguous()), ptr(m8), ptr(cls), ref_step, peaks, m.num_class, ptr(m.offsets),
            m.m_total, m.m_max, ptr(m.xyz), ptr(m.normals), ptr(m.dist_step), m.n_dist, m.n_angle, m.n_alpha, ptr(m.cos_edges),
            ptr(m.alpha_edges), ptr(m.alpha_cs), ptr(m.bucket_start), m.n_entries, ptr(m.entry_ref), ptr(m.entry_dir),
            ptr(out["votes"]), ptr(out["model_index"]), ptr(out["bin"]), ptr(out["pose"]), ptr(acc), stream()),
            "cloudaae_ppf_vote")
    if return_acc:
        out["acc"] = acc
    return out


def cluster(models, votes, pose, class_id, top=4):
    """cloudaae_ppf_cluster on votes [B,C] int32 and pose [B,C,4,4] float64 -> dict(pose [B,top,4,4], rot_axag [B,top,3]
    float64, trans [B,top,3] float32, score, valid [B,top] int32)."""
    require(isinstance(models, PPFModels), "models must be a PPFModels")
    dev = models.device
    require(isinstance(votes, torch.Tensor) and votes.dim() == 2 and votes.dtype == torch.int32 and votes.device == dev,
            "votes must be an int32 [B, C] tensor on the models' device")
    B, C = int(votes.shape[0]), int(votes.shape[1])
    require(B >= 1 and 1 <= C <= MAX_CANDIDATES, "at most %d candidates per sample (ceil(N / ref_step) * peaks)" % MAX_CANDIDATES)
    require(isinstance(pose, torch.Tensor) and tuple(pose.shape) == (B, C, 4, 4) and pose.dtype == torch.float64 and
            pose.device == dev, "pose must be a float64 [B, C, 4, 4] tensor")
    top = int(top)
    require(1 <= top <= 64, "top must lie in [1, 64]")
    cls = class_id.to(torch.int64).contiguous()
    out = dict(pose=_lib.empty((B, top, 4, 4), dtype=torch.float64, device=dev),
               rot_axag=_lib.empty((B, top, 3), dtype=torch.float64, device=dev),
               trans=_lib.empty((B, top, 3), dtype=torch.float32, device=dev),
               score=_lib.empty((B, top), dtype=torch.int32, device=dev),
               valid=_lib.empty((B, top), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_ppf_cluster(
            B, C, ptr(votes.contiguous()), ptr(pose.contiguous()), ptr(cls), models.num_class, ptr(models.trans_thresh2),
            models.rot_bound, top, ptr(out["pose"]), ptr(out["rot_axag"]), ptr(out["trans"]), ptr(out["score"]),
            ptr(out["valid"]), stream()), "cloudaae_ppf_cluster")
    return out


def propose_poses(models, scene_xyz, scene_normals, mask, class_id, top=4, ref_step=5, peaks=2):
    """The `top` best pose clusters of each sample, best first: dict(pose [B,top,4,4] float64 (model -> camera), rot_axag
    [B,top,3] float64, trans [B,top,3] float32, score [B,top] int32 (votes), valid [B,top] int32).  Two launches."""
    v = vote(models, scene_xyz, scene_normals, mask, class_id, ref_step, peaks)
    B = int(scene_xyz.shape[0])
    return cluster(models, v["votes"].view(B, -1), v["pose"].view(B, -1, 4, 4), class_id, top)
