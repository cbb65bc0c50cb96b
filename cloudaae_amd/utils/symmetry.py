"""The geometric symmetries of an object, found from two surface samples of it: the rigid transforms under which a
depth-only method cannot tell two poses apart, and the transform sets that bop_score.mssd_mspd and
evaluate_batch(bop=...) take.  Every candidate transform is scored by cloudaae_transform_hausdorff
(csrc/symmetry.hip): the directed Hausdorff distance of the moved queries from the targets.  Candidates are sharpened by
the project's ICP (utils/icp.py); the bookkeeping is NumPy float64 on the host over small arrays.  The definition, the
procedure and its limits are in DESIGN.md ("Object symmetries").

    s = hausdorff_scores(queries, targets, transforms, limit=0.01)        # [C] float64 (device), +inf above the limit
    r = find_symmetries(targets, queries)                                 # r['transforms'] [n,4,4], r['kind'], ...
    sets = symmetries_of_meshes(paths, scale=0.001)                       # one result per mesh
    d = mssd_mspd(model_xyz, est, gt, intr, symmetries=[sets[c]['transforms'] for c in classes])

    python -m cloudaae_amd.utils.symmetry --meshes DIR [--mesh_scale X] --out symmetries.json
    python -m cloudaae_amd.utils.symmetry --object_model FILE --out symmetries.json

Reflections are not rigid poses and are not looked for; texture is not seen; an object with two continuous axes is
flagged 'spherical' and keeps the identity alone.
"""
import argparse
import json
import math

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .bop_score import symmetry_rotations

ORDER_STEPS = 120                          # L: every order that divides it can be told
COARSE_ANGLES = (2.0 * math.pi / 2.0, 2.0 * math.pi / 3.0, 2.0 * math.pi / 5.0)
NUM_AXES = 2048
NUM_QUERIES = 512
NUM_TARGETS = 4096
TOL = 0.02
REFINE = 256
MERGE_DEG = 5.0
DISC_STEP = 0.01
MAX_MEMBERS = 60
MAX_CANDIDATES = 1 << 20                   # of one launch (csrc/symmetry.hip)
ICP_MAX_POINTS = 4096                      # CLOUDAAE_ICP_MAX_POINTS
QUERY_SEED_OFFSET = 1                      # the queries of a mesh are drawn with seed + 1
KINDS = ("none", "finite", "axial", "spherical")


# ---- the kernel ------------------------------------------------------------------------------------------------------
def _cloud(t, name):
    require(isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] >= 3 and t.shape[0] >= 1,
            "%s must be a [P, >=3] tensor with P >= 1" % name)
    require(t.dtype == torch.float32, "%s must be float32" % name)
    if not t.is_cuda:
        raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got a %s tensor" % t.device)
    require(t.stride(1) == 1, "%s: the coordinates of a point must be contiguous" % name)
    return t.data_ptr(), int(t.stride(0)), int(t.shape[0])


def hausdorff_scores(queries, targets, transforms, limit=math.inf):
    """cloudaae_transform_hausdorff: out[c] = max_i min_j |T_c x_i - y_j| of the queries x [M,>=3] against the targets y
    [N,>=3] (float32 on one GPU, row strides allowed) under each of the transforms [C,4,4] (float64; a tensor on that
    GPU or an array); +inf where it exceeds `limit` (the kernel compares the squares: limit * limit, formed here in
    float64).  -> [C] float64 on the device."""
    qp, qs, M = _cloud(queries, "queries")
    tp, ts, N = _cloud(targets, "targets")
    dev = queries.device
    require(targets.device == dev, "queries and targets must be on one device")
    if not isinstance(transforms, torch.Tensor):
        transforms = torch.from_numpy(np.ascontiguousarray(np.asarray(transforms, np.float64).reshape(-1, 4, 4))).to(dev)
    require(transforms.dtype == torch.float64 and transforms.dim() == 3 and tuple(transforms.shape[1:]) == (4, 4) and
            transforms.shape[0] >= 1 and transforms.device == dev, "transforms must be a float64 [C, 4, 4] tensor, C >= 1")
    limit = float(limit)
    require(limit >= 0.0, "limit must be >= 0 (inf allowed)")
    T = transforms.contiguous()
    C = int(T.shape[0])
    out = _lib.empty((C,), dtype=torch.float64, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for lo in range(0, C, MAX_CANDIDATES):
            c = min(MAX_CANDIDATES, C - lo)
            ws = _lib.empty((int(L.cloudaae_transform_hausdorff_workspace_bytes(c)) // 8,), dtype=torch.int64, device=dev)
            _lib.check(L.cloudaae_transform_hausdorff(c, M, qp, qs, N, tp, ts, ptr(T[lo:lo + c]), limit * limit,
                                                      ptr(out[lo:lo + c]), ptr(ws), stream()),
                       "cloudaae_transform_hausdorff")
    return out


# ---- rotations (host, NumPy float64) ---------------------------------------------------------------------------------
def fibonacci_hemisphere(k):
    """[k,3] unit vectors spread over the hemisphere z > 0 (a rotation axis and its opposite name the same line)."""
    i = np.arange(int(k), dtype=np.float64)
    z = (i + 0.5) / float(k)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def rotations_about(axes, angles, centre):
    """[n,4,4]: the rotation by angles[i] about the line through `centre` along axes[i] (Rodrigues; axes [n,3] or [3],
    angles [n] or a number, broadcast)."""
    a = np.atleast_2d(np.asarray(axes, np.float64))
    th = np.atleast_1d(np.asarray(angles, np.float64))
    n = max(len(a), len(th))
    a = np.broadcast_to(a, (n, 3))
    th = np.broadcast_to(th, (n,))
    a = a / np.sqrt((a * a).sum(axis=1))[:, None]
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
    R = np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1.0 - np.cos(th))[:, None, None] * (K @ K)
    return about_centre(R, centre)


def about_centre(R, centre):
    """[n,4,4]: x -> R (x - centre) + centre for rotation matrices R [n,3,3]."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    c = np.asarray(centre, np.float64).reshape(3)
    T = np.tile(np.eye(4), (len(R), 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = c[None] - R @ c
    return T


def rotation_distance_deg(Ra, Rb):
    """[a,b] degrees: the angle of Ra[i]^T Rb[j] (rotation matrices [a,3,3], [b,3,3])."""
    Ra = np.asarray(Ra, np.float64).reshape(-1, 3, 3)
    Rb = np.asarray(Rb, np.float64).reshape(-1, 3, 3)
    tr = np.einsum("aij,bij->ab", Ra, Rb)
    return np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


def rotation_axis(R):
    """The unit axis of a rotation matrix that is not the identity: the eigenvector of (R + R^T) / 2 to the eigenvalue
    1 (well conditioned also at a half-turn, where the skew part vanishes), signed by the skew part when there is one,
    else so that its largest component is positive."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w, v = np.linalg.eigh((R + R.T) / 2.0)
    a = v[:, int(np.argmax(w))]
    skew = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if float(np.abs(skew).max()) > 1e-6:
        return a if float(a @ skew) >= 0.0 else -a
    return a if a[int(np.argmax(np.abs(a)))] > 0.0 else -a


def nearest_rotation(M):
    """The rotation matrix nearest to M [n,3,3] (SVD, determinant +1)."""
    u, _, vt = np.linalg.svd(np.asarray(M, np.float64).reshape(-1, 3, 3))
    d = np.sign(np.linalg.det(u @ vt))
    u[:, :, 2] *= d[:, None]
    return u @ vt


def line_angle_deg(a, b):
    """[n,m] degrees between the lines along a [n,3] and b [m,3] (unit vectors; a line has no sign)."""
    c = np.abs(np.atleast_2d(a) @ np.atleast_2d(b).T)
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))


def order_from_mask(passed, steps=ORDER_STEPS):
    """passed[k - 1]: whether the rotation by 2 pi k / steps was accepted, k = 1 .. steps - 1.  -> the largest n dividing
    `steps` whose multiples of 2 pi / n all passed (1: none; steps: every angle, a continuous axis)."""
    p = np.asarray(passed, bool).reshape(-1)
    require(len(p) == steps - 1, "one flag per angle 2 pi k / steps, k = 1 .. steps - 1")
    for n in range(steps, 1, -1):
        if steps % n == 0 and all(p[k * (steps // n) - 1] for k in range(1, n)):
            return n
    return 1


def discretisation_count(r_max, diameter, disc_step=DISC_STEP):
    """The smallest n >= 2 with 2 r_max sin(pi / n) <= disc_step * diameter: the steps of a continuous axis, chosen as
    BOP does (as recalled) so that the farthest surface point moves by at most that share of the diameter per step."""
    step = float(disc_step) * float(diameter)
    require(step > 0.0 and r_max >= 0.0, "disc_step * diameter must be > 0 and r_max >= 0")
    if 2.0 * r_max <= step:
        return 2
    n = max(2, int(math.ceil(math.pi / math.asin(step / (2.0 * r_max)))))
    while 2.0 * r_max * math.sin(math.pi / n) > step:
        n += 1
    while n > 2 and 2.0 * r_max * math.sin(math.pi / (n - 1)) <= step:
        n -= 1
    return n


def _greedy_merge(R, scores, merge_deg, seed_R=None):
    """Indices kept when the rotations R [n,3,3] are visited by ascending score and one within merge_deg of a kept one
    (or of a rotation of seed_R) is dropped."""
    order = np.argsort(scores, kind="stable")
    kept = []
    ref = np.zeros((0, 3, 3)) if seed_R is None else np.asarray(seed_R, np.float64).reshape(-1, 3, 3)
    for i in order:
        if len(ref) and float(rotation_distance_deg(R[i:i + 1], ref).min()) <= merge_deg:
            continue
        kept.append(int(i))
        ref = np.concatenate([ref, R[i:i + 1]])
    return kept


def is_closed(R, merge_deg=MERGE_DEG):
    """Whether every product of two of the rotations R [n,3,3] lies within merge_deg of one of them."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    prod = np.einsum("aij,bjk->abik", R, R).reshape(-1, 3, 3)
    return bool((rotation_distance_deg(prod, R).min(axis=1) <= merge_deg).all())


# ---- the search ------------------------------------------------------------------------------------------------------
def find_symmetries(targets, queries, diameter=None, tol=TOL, epsilon=None, num_axes=NUM_AXES, refine=REFINE,
                    merge_deg=MERGE_DEG, disc_step=DISC_STEP, max_members=MAX_MEMBERS, icp=None):
    """The rotational symmetries of the object of which targets [N,>=3] and queries [M,>=3] (float32, one GPU) are two
    independent surface samples.  Every candidate is a rotation about a line through the targets' mean; one is accepted
    when its score (hausdorff_scores) is <= epsilon = h0 + tol * diameter, h0 being the identity's score -- the
    sampling's own noise floor (epsilon= overrides the rule, e.g. BOP's max(0.015, 0.1 diameter)).  diameter: default
    the targets' (pose_score.model_diameter).  icp: parameters of icp.refine_pose_icp for the sharpening (default:
    radius 0.1 diameter, the reference's decay, rounds and iterations).  Procedure: DESIGN.md, "Object symmetries".
    -> dict(transforms [n,4,4] float64 with the identity first, axes [A,3], orders [A] (ORDER_STEPS: continuous),
    continuous [A] bool, kind ('none' | 'finite' | 'axial' | 'spherical'), closed, epsilon, h0, diameter, centre [3],
    steps (the discretisation of an axial object, else 0)).  More than max_members members of a finite group raise."""
    from . import icp as icp_util
    from . import pose_score
    _cloud(targets, "targets")
    _cloud(queries, "queries")
    centre = targets[:, :3].to(torch.float64).mean(dim=0).cpu().numpy()
    if diameter is None:
        diameter = float(pose_score.model_diameter(targets.unsqueeze(0))[0])
    diameter = float(diameter)
    require(diameter > 0.0 and math.isfinite(diameter), "the object's diameter must be a finite number > 0")

    def score(T, limit=math.inf):
        return hausdorff_scores(queries, targets, T, limit).cpu().numpy()

    h0 = float(score(np.eye(4)[None])[0])
    eps = float(h0 + float(tol) * diameter) if epsilon is None else float(epsilon)
    result = dict(epsilon=eps, h0=h0, diameter=diameter, centre=centre, steps=0)

    def done(kind, T, axes, orders, closed):
        axes = np.asarray(axes, np.float64).reshape(-1, 3)
        orders = np.asarray(orders, np.int64).reshape(-1)
        result.update(kind=kind, transforms=np.ascontiguousarray(T, np.float64), axes=axes, orders=orders,
                      continuous=orders == ORDER_STEPS, closed=bool(closed))
        return result

    # (a) the coarse pass
    grid = fibonacci_hemisphere(num_axes)
    cand = np.concatenate([rotations_about(grid, a, centre) for a in COARSE_ANGLES])
    s = score(cand, eps)
    hit = np.flatnonzero(np.isfinite(s))
    if len(hit) == 0:
        return done("none", np.eye(4)[None], [], [], True)
    # (b) sharpen: the best-scoring candidate of every neighbourhood, `refine` of them at most, by ICP of the queries
    # onto the targets; what comes back is put about the centre again, scored again and merged
    keep = _greedy_merge(cand[hit, :3, :3], s[hit], merge_deg)[:int(refine)]
    start = cand[hit[keep]]
    refined = _sharpen(icp_util, queries, targets, start, centre, diameter, icp)
    s2 = score(refined, eps)
    ok = np.flatnonzero(np.isfinite(s2))
    R, s2 = refined[ok, :3, :3], s2[ok]
    keep = _greedy_merge(R, s2, merge_deg, seed_R=np.eye(3)[None])
    R, s2 = R[keep], s2[keep]
    if len(R) == 0:
        return done("none", np.eye(4)[None], [], [], True)
    # (c) the order of every axis
    axes_all = np.stack([rotation_axis(r) for r in R])
    axes = []
    for i in np.argsort(s2, kind="stable"):
        if not axes or float(line_angle_deg(axes_all[i:i + 1], np.stack(axes)).min()) > merge_deg:
            axes.append(axes_all[i])
    axes = np.stack(axes)
    k = np.arange(1, ORDER_STEPS)
    sweep = np.concatenate([rotations_about(a, 2.0 * math.pi * k / ORDER_STEPS, centre) for a in axes])
    passed = np.isfinite(score(sweep, eps)).reshape(len(axes), ORDER_STEPS - 1)
    orders = np.array([order_from_mask(p) for p in passed], np.int64)
    axes, passed, orders = axes[orders > 1], passed[orders > 1], orders[orders > 1]
    if len(axes) == 0:
        return done("none", np.eye(4)[None], [], [], True)
    # (d) assemble
    cont = np.flatnonzero(orders == ORDER_STEPS)
    if len(cont) >= 2:
        return done("spherical", np.eye(4)[None], axes[cont], orders[cont], True)
    if len(cont) == 1:
        a = axes[cont[0]]
        t_host = targets[:, :3].to(torch.float64).cpu().numpy() - centre[None]
        r_max = float(np.sqrt(((t_host - (t_host @ a)[:, None] * a[None]) ** 2).sum(axis=1)).max())
        n = discretisation_count(r_max, diameter, disc_step)
        result["steps"] = n
        T = symmetry_rotations(a, centre, n)
        out_axes, out_orders = [a], [ORDER_STEPS]
        # at most one half-turn about a line perpendicular to the axis: the first in the order of the scores
        for i in range(len(axes)):
            if i != cont[0] and passed[i][ORDER_STEPS // 2 - 1] and \
                    float(line_angle_deg(axes[i:i + 1], a[None])[0, 0]) >= 90.0 - merge_deg:
                f = axes[i] - float(axes[i] @ a) * a
                F = symmetry_rotations(f, centre, 2)[1]
                T = np.concatenate([T, F[None] @ T])
                out_axes.append(f / np.sqrt(f @ f))
                out_orders.append(2)
                break
        return done("axial", T, out_axes, out_orders, True)
    members = np.concatenate([symmetry_rotations(a, centre, int(n))[1:] for a, n in zip(axes, orders)])
    keep = _greedy_merge(members[:, :3, :3], np.arange(len(members), dtype=np.float64), merge_deg, seed_R=np.eye(3)[None])
    T = np.concatenate([np.eye(4)[None], members[keep]])
    require(len(T) <= int(max_members), "a finite symmetry group of %d members, more than max_members = %d: lower tol or "
                                        "pass a smaller epsilon" % (len(T), int(max_members)))
    return done("finite", T, axes, orders, is_closed(T[:, :3, :3], merge_deg))


def _sharpen(icp_util, queries, targets, start, centre, diameter, icp):
    """start [B,4,4] -> [B,4,4]: each refined by point-to-point ICP of the queries onto the targets (at most 4096 of
    either: a prefix of a surface sample is a surface sample), its rotation made a rotation again and put about the
    centre."""
    B = len(start)
    q = queries[:ICP_MAX_POINTS, :3].contiguous()
    t = targets[:ICP_MAX_POINTS, :3].contiguous()
    dev = queries.device
    rot = np.zeros((B, 3))
    for i in range(B):
        R = start[i, :3, :3]
        ang = math.acos(min(1.0, max(-1.0, (float(np.trace(R)) - 1.0) / 2.0)))
        rot[i] = rotation_axis(R) * ang
    params = dict(radius=0.1 * diameter)
    params.update(icp or {})
    out = icp_util.refine_pose_icp(q.unsqueeze(0).repeat(B, 1, 1), t.unsqueeze(0).repeat(B, 1, 1),
                                   torch.from_numpy(rot.astype(np.float32)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(start[:, :3, 3], np.float32)).to(dev), **params)
    T = out["transformation"].cpu().numpy()
    return about_centre(nearest_rotation(T[:, :3, :3]), centre)


# ---- samples -----------------------------------------------------------------------------------------------------------
def samples_of_model(model):
    """A class model [P,>=3] without a mesh -> (targets, queries): its even and its odd rows."""
    require(isinstance(model, torch.Tensor) and model.dim() == 2 and model.shape[0] >= 2, "a model is a [P, >=3] tensor, P >= 2")
    return model[0::2], model[1::2]


def symmetries_of_meshes(meshes, scale=1.0, seed=None, num_targets=NUM_TARGETS, num_queries=NUM_QUERIES, device=None,
                         mesh_ids=None, **kw):
    """find_symmetries for every mesh (paths, (vertices, triangles) pairs or a PackedMeshes): targets and queries are two
    sample_meshes draws, with seed and seed + 1 (mesh_ids: the ids the draws are made under, default the positions, so
    that a mesh searched alone gives what it gives among the others).  -> a list of results."""
    from . import mesh_models
    seed = mesh_models.DEFAULT_SEED if seed is None else int(seed)
    p = mesh_models.pack_meshes(meshes, scale, device)
    t = mesh_models.sample_meshes(p, int(num_targets), seed=seed, mesh_ids=mesh_ids)
    q = mesh_models.sample_meshes(p, int(num_queries), seed=seed + QUERY_SEED_OFFSET, mesh_ids=mesh_ids, cum=t["cum"])
    return [find_symmetries(t["xyzrgb"][i], q["xyzrgb"][i], **kw) for i in range(len(p.num_triangles))]


def symmetries_of_models(models, **kw):
    """find_symmetries for every class model of models [C,P,>=3] (float32, on the GPU or an array)."""
    if not isinstance(models, torch.Tensor):
        models = torch.from_numpy(np.ascontiguousarray(models, np.float32)).cuda()
    return [find_symmetries(*samples_of_model(models[i]), **kw) for i in range(int(models.shape[0]))]


# ---- files -------------------------------------------------------------------------------------------------------------
def save_symmetries(path, results, names=None):
    """The results of a list of find_symmetries calls, class i being entry i, as JSON."""
    classes = []
    for i, r in enumerate(results):
        classes.append({"class": i, "name": None if names is None else names[i], "kind": r["kind"],
                        "closed": bool(r["closed"]), "epsilon": float(r["epsilon"]), "h0": float(r["h0"]),
                        "diameter": float(r["diameter"]), "steps": int(r["steps"]),
                        "centre": [float(x) for x in r["centre"]], "axes": np.asarray(r["axes"]).tolist(),
                        "orders": [int(x) for x in r["orders"]], "continuous": [bool(x) for x in r["continuous"]],
                        "transforms": np.asarray(r["transforms"], np.float64).tolist()})
    with open(path, "w") as f:
        json.dump({"classes": classes}, f)


def load_symmetries(path):
    """{class: [n,4,4] float64} of a file written by save_symmetries: what evaluate_batch(bop=...)'s 'symmetries' takes."""
    with open(path) as f:
        data = json.load(f)
    out = {}
    for c in data["classes"]:
        T = np.asarray(c["transforms"], np.float64).reshape(-1, 4, 4)
        require(len(T) >= 1 and np.array_equal(T[0], np.eye(4)), "a transform set must start with the identity")
        out[int(c["class"])] = T
    return out


def kind_lines(results, classes=None):
    """One line of text per class (default: the positions): what was found."""
    out = []
    for i, r in zip(range(len(results)) if classes is None else classes, results):
        orders = ",".join("inf" if n == ORDER_STEPS else str(int(n)) for n in r["orders"]) or "-"
        out.append("symmetry class %d kind %s transforms %d orders %s epsilon %f h0 %f"
                   % (i, r["kind"], len(r["transforms"]), orders, r["epsilon"], r["h0"]))
    return out


def main(argv=None):
    from . import mesh_models
    parser = argparse.ArgumentParser(description="the geometric symmetries of every mesh of a directory, or of every class model")
    parser.add_argument("--meshes", default=None, help="directory of *.ply files; class i is the i-th in sorted order")
    parser.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the coordinates (0.001: millimetres to metres)")
    parser.add_argument("--object_model", default=None, help="obj_models.tfrecords: the class models, when there are no meshes")
    parser.add_argument("--out", required=True, help="the JSON file to write")
    parser.add_argument("--tol", type=float, default=TOL)
    parser.add_argument("--seed", type=int, default=mesh_models.DEFAULT_SEED)
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    if (args.meshes is None) == (args.object_model is None):
        parser.error("give --meshes DIR or --object_model FILE")
    torch.cuda.set_device(args.gpu)
    if args.meshes:
        import os
        files = mesh_models.mesh_files(args.meshes)
        results = symmetries_of_meshes(files, scale=args.mesh_scale, seed=args.seed, tol=args.tol)
        names = [os.path.basename(f) for f in files]
    else:
        from .. import tfrecord_io
        models, _ = tfrecord_io.read_and_decode_obj_model(args.object_model)
        results = symmetries_of_models(models, tol=args.tol)
        names = None
    save_symmetries(args.out, results, names)
    for line in kind_lines(results):
        print(line)
    print("%d classes written to %s" % (len(results), args.out))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
