"""GPU: the refinement kernels (csrc/icp.hip, csrc/normals.hip, csrc/pose_math.h) at degenerate and boundary
geometry, against the 50-digit reference of tests/geometry_edge_reference.py.  The input families, the units of the
bounds and the preconditions (identity matching, rank and sign of Sigma, neighbour counts, conditioning) are those of
that file; tests/test_geometry_edge_reference_host.py proves the preconditions on the CPU.

Bounds.  One Procrustes update: the transform in units of u = 2^-53 (s1 + |mp - c| |mq - c|) / (s2 + d s3), the
objective tr(R^T Sigma) in units of 2^-53 s1; allowed is 16 x the fp64 restatement's own largest error over the same
cases, at least 16 units.  One plane update: K 2^-53 cond_2(A) |x_ref| with K = 16 x the restatement's own figure.
Normals: eps = 100 x max(order-of-sums difference of the restatement, 1e-12) per family, for the eigenvalues and for
the gap-free residual |C n - w0 n|, both relative to the largest eigenvalue; no query is left out.  Pose maps and
matching statistics: the bounds of tests/test_14_icp_gpu.py.  profiles/notes_geometry_edges.md has the figures."""
import numpy as np
import pytest
import torch

import geometry_edge_reference as G
import icp_plane_reference as PL
import icp_reference as R
import normals_reference as NR

pytestmark = pytest.mark.gpu

ONE_FACTOR = 8.0 * 2.0 ** -52                 # orthonormality of one rotation factor (tests/test_19_icp_plane_gpu.py)


def _icp(src, dst, rot, trans, normals=None, **kw):
    from cloudaae_amd.utils.icp import refine_pose_icp
    if normals is not None:
        kw.update(estimation="point_to_plane", normals=torch.from_numpy(np.ascontiguousarray(normals)).cuda())
    out = refine_pose_icp(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (src, dst, rot, trans)), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_pose(out, c):
    """One factor: R orthonormal and proper to 8 x 2^-52, the last row exact, rot_axag and trans consistent with T."""
    T = out["transformation"][c]
    Rm = T[:3, :3]
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= ONE_FACTOR, c
    assert abs(np.linalg.det(Rm) - 1.0) <= ONE_FACTOR, c
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.abs(G.rodrigues_mp(out["rot_axag"][c]) - Rm).max() < 1e-12
    assert np.linalg.norm(out["rot_axag"][c]) <= np.pi + 1e-12
    assert np.array_equal(out["trans"][c], T[:3, 3].astype(np.float32))


# ---- 3a: one Procrustes update -------------------------------------------------------------------------------------
def test_one_procrustes_update(hip):
    tab = G.procrustes_table()
    names = list(tab)
    M = 128
    src, dst = G.pad_clouds([tab[n] for n in names], M, M)
    trans = np.stack([tab[n]["trans0"] for n in names])
    got = _icp(src, dst, np.zeros_like(trans), trans, radius=G.P2P_RADIUS, rounds=1, max_iteration=1)
    kT, kobj = G.procrustes_allowance()
    print("allowed: %.1f units in T, %.1f units in the objective" % (kT, kobj))
    worst_T = worst_obj = 0.0
    for c, name in enumerate(names):
        case, T = tab[name], got["transformation"][c]
        ref = case["ref"]
        assert np.array_equal(got["iterations"][c], [1]), name
        assert got["fitness"][c] * M == len(case["src"]), name
        _check_pose(got, c)
        e_obj = G.objective_error(T, ref, case["v"])
        e_T = G.transform_error(T, ref, case["trans0"]) / case["u"] if ref["unique"] else None
        print("%-20s objective %.2f units (restatement %.2f), T %s units (restatement %s)"
              % (name, e_obj, case["rest_obj"], "none" if e_T is None else "%.2f" % e_T,
                 "none" if e_T is None else "%.2f" % case["rest_T"]))
        assert e_obj <= kobj, name
        worst_obj = max(worst_obj, e_obj)
        assert ref["unique"] == case["unique"]
        if ref["unique"]:
            assert e_T <= kT, name
            worst_T = max(worst_T, e_T)
        if name in ("one_point", "coincident"):                     # Sigma = 0: R = I, t = mq - mp
            assert np.array_equal(T[:3, :3], np.eye(3)), name
            t = np.array([float(ref["mq"][k] - ref["mp"][k]) for k in range(3)])
            ulp = np.spacing(np.maximum(np.abs([float(v) for v in ref["mq"]]), np.abs([float(v) for v in ref["mp"]])))
            assert np.all(np.abs(T[:3, 3] - t) <= ulp), name
    print("kernel: largest %.2f units in T, %.2f units in the objective" % (worst_T, worst_obj))


# ---- 3b: one plane update -------------------------------------------------------------------------------------------
def _plane_batch(names, M=128):
    tab = G.plane_table()
    src, dst = G.pad_clouds([tab[n] for n in names], M, M)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (len(names), M, 1))
    for c, n in enumerate(names):
        nrm[c, :len(tab[n]["normals"])] = tab[n]["normals"]
    return tab, src, dst, nrm


def test_one_plane_update_of_a_regular_system(hip):
    names = ["three_patches"] + ["nearly_flat_%g" % s for s in G.PLANE_SPREADS]
    tab, src, dst, nrm = _plane_batch(names)
    zero = np.zeros((len(names), 3), np.float32)
    got = _icp(src, dst, zero, zero, normals=nrm, radius=G.PLANE_RADIUS, rounds=1, max_iteration=1)
    K = G.plane_allowance()
    print("allowed: K = %.3e" % K)
    for c, name in enumerate(names):
        case = tab[name]
        assert case["regular"] and case["cond"] < G.PLANE_COND_CAP
        assert np.array_equal(got["iterations"][c], [1]), name
        err = np.abs(got["transformation"][c] - case["U"]).max() / case["unit"]
        print("%-20s cond %.3e: U off by %.3e of 2^-53 cond |x| (restatement %.3e)" % (name, case["cond"], err, case["rest"]))
        assert err <= K, name
        _check_pose(got, c)


def test_a_plane_update_that_cannot_be_solved_keeps_the_pose(hip):
    """Normals all (0, 0, 1): the third pivot is exactly zero.  Five correspondences: fewer than six.  T is the
    rounds = 0 transform bit for bit, every round counts one (empty) update.  Normals all (0.6, 0, 0.8): the fourth
    pivot is rounding noise, so the pose may move, by a finite amount."""
    names = ["normals_all_z", "five_correspondences", "normals_all_tilted"]
    tab, src, dst, nrm = _plane_batch(names)
    rot = np.tile(np.array([2e-3, -1e-3, 1.5e-3], np.float32), (3, 1))
    trans = np.tile(np.array([2.0 ** -10, 0.0, -2.0 ** -10], np.float32), (3, 1))
    kw = dict(radius=G.PLANE_RADIUS, rounds=3, max_iteration=5)
    got = _icp(src, dst, rot, trans, normals=nrm, **kw)
    start = _icp(src, dst, rot, trans, normals=nrm, radius=G.PLANE_RADIUS, rounds=0)
    for c, name in enumerate(names[:2]):
        T, fit, rmse, its = PL.refine(src[c], dst[c], nrm[c], rot[c], trans[c], **kw)
        assert np.array_equal(T, R.initial_transform(rot[c], trans[c])) and np.array_equal(its, [1, 1, 1]), name
        assert got["transformation"][c].tobytes() == start["transformation"][c].tobytes(), name
        assert np.abs(got["transformation"][c] - T).max() <= 1e-15, name
        assert np.array_equal(got["iterations"][c], [1, 1, 1]), name
        assert got["fitness"][c] * 128 == round(fit * 128) and got["fitness"][c] > 0.0, name
    for k in ("transformation", "rot_axag", "trans", "fitness", "inlier_rmse"):
        assert np.all(np.isfinite(got[k])), k


# ---- 3c: matching ----------------------------------------------------------------------------------------------------
def _check_statistics(got, c, src, dst, name):
    M = len(src)
    I, J, D = R.correspondences(src.astype(np.float64), dst.astype(np.float64), G.MATCH_RADIUS)
    rmse = np.sqrt(np.cumsum(D)[-1] / len(I)) if len(I) else 0.0
    print("%-14s %d of %d matched, rmse %.9e vs %.9e" % (name, got["fitness"][c] * M, M, got["inlier_rmse"][c], rmse))
    assert got["fitness"][c] * M == len(I), name
    assert abs(got["inlier_rmse"][c] - rmse) <= 1e-9 * rmse, name
    assert np.array_equal(got["transformation"][c], np.eye(4)), name


def _check_one_update(got, c, src, dst, name):
    kw = dict(radius=G.MATCH_RADIUS, rounds=1, max_iteration=1)
    T, fit, rmse, its = R.refine(src, dst, np.zeros(3), np.zeros(3), **kw)
    print("%-14s one update: max |T - T_ref| %.3e" % (name, np.abs(got["transformation"][c] - T).max()))
    assert np.array_equal(got["iterations"][c], its), name
    assert np.abs(got["transformation"][c] - T).max() <= 1e-9, name       # another partner in a tie moves T by far more
    assert got["fitness"][c] * len(src) == round(fit * len(src)), name
    assert abs(got["inlier_rmse"][c] - rmse) <= 1e-9 * rmse, name


def test_matching_at_cell_and_radius_boundaries(hip):
    cases = G.matching_cases()
    names = list(cases)
    src, dst = G.pad_clouds([cases[n] for n in names], 256, 512)
    zero = np.zeros((len(names), 3), np.float32)
    got = _icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=0)
    for c, name in enumerate(names):
        _check_statistics(got, c, src[c], dst[c], name)
    assert got["fitness"][names.index("exact_radius")] == 0.0
    assert got["fitness"][names.index("inside_radius")] * 256 == 48
    got = _icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=1, max_iteration=1)
    for c, name in enumerate(names):
        _check_one_update(got, c, src[c], dst[c], name)
    assert np.array_equal(got["transformation"][names.index("exact_radius")], np.eye(4))


def test_a_tie_goes_to_the_lowest_index_wherever_it_is_probed(hip):
    cases = G.tie_cases()
    names = list(cases)
    src = np.stack([cases[n]["src"] for n in names])
    dst = np.stack([cases[n]["dst"] for n in names])
    zero = np.zeros((len(names), 3), np.float32)
    got = _icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=1, max_iteration=1)
    for c, name in enumerate(names):
        T = got["transformation"][c]
        assert np.array_equal(T[:3, :3], np.eye(3)), name
        assert np.array_equal(T[:3, 3], cases[name]["expect"]), (name, T[:3, 3])
        assert got["fitness"][c] == 1.0 and got["inlier_rmse"][c] == 0.0, name


def test_matching_with_far_apart_cells_in_one_bucket(hip):
    c = G.colliding_case()
    src, dst = c["src"][None], c["dst"][None]
    zero = np.zeros((1, 3), np.float32)
    _check_statistics(_icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=0), 0, src[0], dst[0], "colliding")
    _check_one_update(_icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=1, max_iteration=1), 0, src[0], dst[0],
                      "colliding")


def test_matching_beyond_the_cell_clamp(hip):
    c = G.huge_case()
    src, dst = c["src"][None], c["dst"][None]
    zero = np.zeros((1, 3), np.float32)
    got = _icp(src, dst, zero, zero, radius=G.MATCH_RADIUS, rounds=0)
    _check_statistics(got, 0, src[0], dst[0], "huge")
    assert got["fitness"][0] * 256 == 128 and got["inlier_rmse"][0] == 0.0


# ---- 3d: pose maps ---------------------------------------------------------------------------------------------------
def test_pose_maps_at_their_branch_points(hip):
    rot, angle, axis = G.pose_map_inputs()
    B = len(rot)
    assert B >= 256
    src = np.zeros((B, 1, 3), np.float32)
    dst = np.ones((B, 1, 3), np.float32)                      # 1 m (and more) from the transformed source: no partner
    trans = np.zeros((B, 3), np.float32)
    got = _icp(src, dst, rot, trans)
    start = _icp(src, dst, rot, trans, rounds=0)
    assert got["transformation"].tobytes() == start["transformation"].tobytes()
    assert np.all(got["fitness"] == 0.0) and np.all(got["inlier_rmse"] == 0.0) and np.all(got["iterations"] == 1)
    worst = [0.0, 0.0, 0.0]
    for c in range(B):
        Rm = got["transformation"][c][:3, :3]
        r64 = rot[c].astype(np.float64)
        e0 = np.abs(Rm - G.rodrigues_mp(rot[c])).max()
        e1 = np.abs(G.rodrigues_mp(got["rot_axag"][c]) - Rm).max()
        assert e0 <= 1e-15, (c, angle[c], axis[c], e0)
        assert e1 < 1e-12, (c, angle[c], axis[c], e1)
        assert np.linalg.norm(got["rot_axag"][c]) <= np.pi + 1e-12, (c, angle[c], axis[c])
        worst[0], worst[1] = max(worst[0], e0), max(worst[1], e1)
        if np.linalg.norm(r64) <= G.POSE_SAFE_ANGLE:
            e2 = np.abs(got["rot_axag"][c] - r64).max()
            assert e2 <= 1e-12, (c, angle[c], axis[c], e2)
            assert np.abs(got["rot_axag"][c] - G.log_map_mp(Rm)).max() <= 1e-12, (c, angle[c], axis[c])
            worst[2] = max(worst[2], e2)
        if not np.any(r64):
            assert np.array_equal(Rm, np.eye(3)) and not np.any(got["rot_axag"][c])
        assert np.array_equal(got["transformation"][c][3], [0.0, 0.0, 0.0, 1.0])
    print("pose maps, %d poses: R vs mp %.3e, Rodrigues(rot_out) vs R %.3e, rot_out vs rot (angles <= pi - 64 ulp) %.3e"
          % (B, worst[0], worst[1], worst[2]))


# ---- 3e: normals -----------------------------------------------------------------------------------------------------
def _normals(xyz, radius, **kw):
    from cloudaae_amd.utils.normals import estimate_normals
    kw = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out = estimate_normals(torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), radius, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_normals(name, got, ref, queries, viewpoint=None):
    """Every query: count, ascending eigenvalues within eps l2 of the reference's, a unit normal, the residual
    |C n - w0 n| <= eps l2, and where the relative gap is >= 0.1 also the direction.  No query is left out."""
    (n, e, cnt), (count, w, C, v0, eps, d) = got, ref
    assert np.array_equal(cnt, count), name
    few = count < 3
    ok = ~few
    assert np.all(n[few] == [0.0, 0.0, 1.0]) and np.all(e[few] == 0.0), name
    assert np.all(np.diff(e, axis=1) >= 0.0), name
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-14, name
    top = w[:, 2]
    e_w = np.abs(e - w).max(axis=1)
    res = np.linalg.norm(np.einsum("kab,kb->ka", C, n) - w[:, :1] * n, axis=1)
    sharp = ok & (NR.relative_gap(w) >= 0.1)
    dot = 1.0 - np.abs((n * v0).sum(axis=1))
    scale = np.where(top > 0.0, top, 1.0)
    print("%-28s eps %.1e: %d queries, %d estimated, %d with a direction; eigenvalues off by %.2e l2, residual %.2e l2, "
          "1 - |dot| %.2e" % (name, eps, len(count), ok.sum(), sharp.sum(), (e_w[ok] / scale[ok]).max() if ok.any() else 0.0,
                              (res[ok] / scale[ok]).max() if ok.any() else 0.0, dot[sharp].max() if sharp.any() else 0.0))
    assert np.all(e_w[ok] <= eps * top[ok]), name
    assert np.all(res[ok] <= eps * top[ok]), name
    assert np.all(dot[sharp] <= eps), name
    if viewpoint is not None:
        side = (n * (queries.astype(np.float64) - np.asarray(viewpoint, np.float64))).sum(axis=1)
        assert np.all(side[ok] <= 1e-9), name
    return ok


@pytest.mark.parametrize("name", list(G.normals_families()))
def test_normals_of_a_degenerate_or_boundary_family(hip, name):
    f = G.normals_families()[name]
    ref = G.normals_reference_of(name)
    sup, q = f["support"], f["queries"]
    kw = {} if f["viewpoint"] is None else dict(viewpoint=f["viewpoint"])
    batched = _normals(sup[None], f["radius"], **(kw if q is None else dict(kw, queries=q[None])))
    qs = sup if q is None else q
    got = [t[0] for t in batched]
    ok = _check_normals(name, got, ref, qs, f["viewpoint"])
    n, e, cnt = got
    if f.get("planar"):
        assert ok.all() and np.all(e[:, 0] == 0.0), name
        assert np.all(np.abs(n) == [0.0, 0.0, 1.0]), name
    if "sign" in f:
        assert np.all(n[:, 2] == f["sign"]), name
    if name == "coincident":                                   # C = 0: the first of equal diagonal entries
        assert np.all(e == 0.0) and np.all(n == [1.0, 0.0, 0.0])
    if name == "isotropic":
        inner = cnt == 27
        assert inner.sum() == 64 and np.all(e[inner] == e[inner][:, :1]) and np.all(n[inner] == [1.0, 0.0, 0.0])
    # the packed form: the family's set between a three-point set and an empty one; the set's result is the same bits
    xyz = np.concatenate([sup[:3] + np.float32(7.0), sup])
    offsets = torch.tensor([0, 3, 3 + len(sup), 3 + len(sup)], dtype=torch.int32).cuda()
    packed = _normals(xyz, f["radius"], queries=np.stack([qs, qs, qs]), offsets=offsets, **kw)
    for a, b in zip(packed, got):
        assert a[1].tobytes() == b.tobytes(), name
    assert np.all(packed[2][2] == 0) and np.all(packed[0][2] == [0.0, 0.0, 1.0]) and np.all(packed[1][2] == 0.0)
    assert np.all(packed[2][0] == 0)


def test_normals_of_packed_edge_sets(hip):
    xyz, offsets, queries, radius = G.packed_edge_sets()
    out = _normals(xyz, radius, queries=queries, offsets=torch.from_numpy(offsets).cuda())
    for s in range(len(offsets) - 1):
        pts = xyz[offsets[s]:offsets[s + 1]]
        got = [t[s] for t in out]
        if len(pts) == 0:
            assert np.all(got[2] == 0) and np.all(got[0] == [0.0, 0.0, 1.0]) and np.all(got[1] == 0.0)
            continue
        ref = G.normals_table(pts, radius, queries[s]) + G.order_of_sums_eps(pts, radius, queries[s])
        _check_normals("packed set %d (%d points)" % (s, len(pts)), got, ref, queries[s])
        if len(pts) < 3:
            assert got[2].max() == len(pts) and np.all(got[0] == [0.0, 0.0, 1.0])
