"""CPU: the high-precision reference of tests/geometry_edge_reference.py agrees with numpy.linalg where that is
trustworthy and reproduces closed-form cases, and every input family of tests/test_36_geometry_edges_gpu.py satisfies
the preconditions its GPU assertions rest on (identity matching, the rank and sign of Sigma, neighbour counts, the
conditioning of the regular plane systems) -- checked with the fp64 restatements alone.  Two mutants of the
restatement (no reflection fix; `<=` in the radius test) fail the cases written for them."""
import numpy as np

import geometry_edge_reference as G
import icp_plane_reference as PL
import icp_reference as R
import normals_reference as NR


def test_reference_agrees_with_numpy_on_well_conditioned_inputs():
    rng = np.random.default_rng(1)
    for _ in range(3):
        P = rng.standard_normal((40, 3)) * 0.05
        Rt = R.rodrigues(rng.standard_normal(3))
        Q = P @ Rt.T + rng.standard_normal(3) * 0.1 + rng.standard_normal((40, 3)) * 1e-3
        ref = G.procrustes(P, Q)
        assert ref["unique"] and ref["d"] == 1
        U = R.umeyama(P, Q)
        Rr, tr = G.transform_after_update(ref, np.zeros(3))
        assert np.abs(U[:3, :3] - Rr).max() < 1e-13 and np.abs(U[:3, 3] - tr).max() < 1e-13
        sv = np.linalg.svd((Q - Q.mean(0)).T @ (P - P.mean(0)) / 40, compute_uv=False)
        assert np.abs(np.array([float(v) for v in ref["s"]]) - sv).max() < 1e-15
        assert abs(float(ref["maximum"]) - sv.sum()) < 1e-15
        # plane: three random surface patches' worth of normals, a well-conditioned system
        N = rng.standard_normal((40, 3))
        N /= np.linalg.norm(N, axis=1, keepdims=True)
        A, b, _ = PL.system(P, Q, N)
        U, x, cond = G.plane_update(P, Q, N)
        assert cond < 1e6 and abs(cond - np.linalg.cond(A)) < 1e-8 * cond
        assert np.abs(x - np.linalg.solve(A, -b)).max() < 1e-10 * np.abs(x).max()
        assert np.abs(U - PL.vector_to_matrix(x)).max() < 1e-15
        # covariance
        mu, C, w, V = G.covariance_eig(P)
        assert np.abs(mu - P.mean(0)).max() < 1e-16 and np.abs(C - np.cov(P.T, bias=True)).max() < 1e-16
        assert np.abs(w - np.linalg.eigvalsh(C)).max() < 1e-16
        assert np.abs(C @ V - V * w).max() < 1e-16 and np.abs(V.T @ V - np.eye(3)).max() < 1e-15
        # pose maps
        r = rng.standard_normal(3)
        r *= rng.uniform(0.1, 3.0) / np.linalg.norm(r)
        assert np.abs(G.rodrigues_mp(r) - R.rodrigues(r)).max() < 1e-15
        assert np.abs(G.log_map_mp(G.rodrigues_mp(r)) - r).max() < 1e-14
    assert np.array_equal(G.rodrigues_mp(np.zeros(3)), np.eye(3))
    assert np.array_equal(G.log_map_mp(np.eye(3)), np.zeros(3))
    half_turn = G.log_map_mp(np.diag([-1.0, 1.0, -1.0]))
    assert np.abs(np.abs(half_turn) - [0.0, np.pi, 0.0]).max() < 1e-15


def test_reference_reproduces_closed_forms():
    tab = G.procrustes_table()
    slab = tab["slab_mirrored"]
    Rr, _ = G.transform_after_update(slab["ref"], slab["trans0"])
    assert slab["ref"]["d"] == -1 and slab["ref"]["unique"]
    # Sigma = H C (H the mirror, C the slab's covariance): the maximiser is I where the slab's plane normal is an
    # eigenvector of C, i.e. up to the sample correlation of the 64 heights with x and y (1 mm against 80 mm)
    assert np.abs(Rr - np.eye(3)).max() < 1e-2
    rod = tab["rod_mirrored"]["ref"]                                 # diag(sx^2, a^2, -a^2), exactly
    assert [float(v) for v in rod["s"]] == [21.0 * 2.0 ** -14, 2.0 ** -18, 2.0 ** -18] and rod["d"] == -1
    assert float(rod["maximum"]) == 21.0 * 2.0 ** -14 and not rod["unique"]
    # an exactly planar lattice: lambda0 = 0 and the normal +-z; 27 lattice neighbours: three equal eigenvalues
    fams = G.normals_families()
    plane = fams["planar"]["support"].astype(np.float64)
    _, C, w, V = G.covariance_eig(plane[NR.neighbours(plane, plane[17], 0.25)])
    assert w[0] == 0.0 and w[1] > 0.0 and np.array_equal(np.abs(V[:, 0]), [0.0, 0.0, 1.0])
    cube = fams["isotropic"]["support"].astype(np.float64)
    inner = np.abs(cube).max(axis=1) < 0.25
    assert inner.sum() == 64
    for q in cube[inner][:4]:
        idx = NR.neighbours(cube, q, 0.25)
        _, C, w, _ = G.covariance_eig(cube[idx])
        assert len(idx) == 27 and w[0] == w[1] == w[2] == 2.0 * 0.125 ** 2 / 3.0


def test_procrustes_families_meet_their_preconditions():
    tab = G.procrustes_table()
    assert len(tab) == 12
    for name, c in tab.items():
        m = len(c["src"])
        assert np.array_equal(c["I"], np.arange(m)), name           # every source point is matched ...
        assert np.array_equal(c["Q"][c["J"]], c["Q"][c["I"]]), name  # ... with its own moved copy
        assert (name == "coincident") != np.array_equal(c["I"], c["J"]), name   # (64 equal targets: the lowest index)
        moved = np.linalg.norm(c["Q"] - c["P"], axis=1).max()
        assert moved < G.P2P_RADIUS
        if m > 1 and name != "coincident":
            d = np.linalg.norm(c["P"][:, None] - c["P"][None], axis=2) + np.eye(m)
            assert moved < 0.5 * d.min(), name
        ref = c["ref"]
        assert ref["unique"] == c["unique"], name
        if c["d"] is not None:
            assert ref["d"] == c["d"], name
        s = [float(v) for v in ref["s"]]
        rank = sum(v > 1e-30 for v in s)
        want = dict(collinear=1, two_points=1, one_point=0, coincident=0, plane_square=2, plane_rectangle=2)
        assert rank == want.get(name, 3), (name, s)
        print("%-20s s = %.3e %.3e %.3e d = %+d gap / s1 = %.2e  restatement: T %s units, objective %.2f units"
              % (name, s[0], s[1], s[2], ref["d"], float(ref["gap"] / ref["s"][0]) if s[0] > 0 else 0.0,
                 "none" if c["rest_T"] is None else "%.2f" % c["rest_T"], c["rest_obj"]))
    assert abs(float(tab["plane_square"]["ref"]["s"][0] / tab["plane_square"]["ref"]["s"][1]) - 1.0) < 1e-6
    assert float(tab["plane_rectangle"]["ref"]["s"][1] / tab["plane_rectangle"]["ref"]["s"][0]) < 0.5
    assert float(tab["rod_mirrored_tilted"]["ref"]["gap"] / tab["rod_mirrored_tilted"]["ref"]["s"][0]) < 1e-8
    for far in ("blob_far_shifted", "blob_far_unshifted"):
        assert np.linalg.norm(tab[far]["P"].mean(axis=0)) > 50.0
    assert np.array_equal(tab["coincident"]["ref"]["sigma"], tab["coincident"]["ref"]["sigma"] * 0)
    kT, kobj = G.procrustes_allowance()
    print("allowed: %.1f units in T, %.1f units in the objective" % (kT, kobj))
    assert 16.0 <= kT < 1024.0 and 16.0 <= kobj < 1024.0             # the restatement itself is a few units off


def test_plane_families_meet_their_preconditions():
    tab = G.plane_table()
    for name, c in tab.items():
        if name == "five_correspondences":
            assert np.array_equal(c["I"], np.arange(5)) and np.array_equal(c["J"], np.arange(5))
            assert PL.plane_update(c["P"][c["I"]], c["Q"][c["J"]], c["normals"][c["J"]]) is None
            continue
        assert np.array_equal(c["I"], np.arange(len(c["src"]))) and np.array_equal(c["I"], c["J"]), name
        if c["regular"]:
            assert c["cond"] < G.PLANE_COND_CAP, (name, c["cond"])
            print("%-20s cond %.3e |x| %.3e restatement %.3e of 2^-53 cond |x|" % (name, c["cond"], np.linalg.norm(c["x"]), c["rest"]))
    conds = [tab["nearly_flat_%g" % s]["cond"] for s in G.PLANE_SPREADS]
    assert tab["three_patches"]["cond"] < 1e5 < conds[0] < 1e8 < conds[1] < 1e10 < conds[2]
    # all normals along z: rows and columns 2, 3, 4 of A are zero, the third pivot is exactly zero
    c = tab["normals_all_z"]
    A, b, _ = PL.system(c["P"], c["Q"], c["normals"])
    assert np.all(A[2:5] == 0.0) and A[0, 0] > 0.0 and A[1, 1] > 0.0
    assert PL.ldl_solve(A, b) is None
    print("allowed: K = %.3e" % G.plane_allowance())
    assert 0.0 < G.plane_allowance() < 16.0                          # the restatement is inside the bound with K = 1


def _stats(c, radius):
    P, Q = c["src"].astype(np.float64), c["dst"].astype(np.float64)
    I, J, D = R.correspondences(P, Q, radius)
    return P, Q, I, J, D


def test_matching_families_meet_their_preconditions():
    r = G.MATCH_RADIUS
    cases = G.matching_cases()
    for name in ("exact_radius", "inside_radius", "half_shift", "around_zero"):
        for k in ("src", "dst"):
            x = cases[name][k].astype(np.float64) / G.GRID
            if name == "inside_radius" and k == "dst":
                x = x[np.abs(x - np.round(x)) == 0.0]
            assert np.array_equal(x, np.round(x)), name              # multiples of 2^-7: every d^2 is exact
    P, Q, I, J, D = _stats(cases["exact_radius"], r)
    assert len(I) == 0 and np.all(np.linalg.norm(P - Q, axis=1) == r)
    assert np.all((P.min(axis=0) < 0) & (P.max(axis=0) > 0))
    P, Q, I, J, D = _stats(cases["inside_radius"], r)
    assert len(I) == 48 and np.all(np.abs(P - Q).max(axis=1) == r * (1.0 - 2.0 ** -20))
    assert (D == (r * (1.0 - 2.0 ** -20)) ** 2).sum() >= 40
    P, Q, I, J, D = _stats(cases["half_shift"], r)
    d = P[:, None] - Q[None]
    d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
    assert len(I) == 216 and np.all((d2 == 3.0 * 2.0 ** -12).sum(axis=1) == 8) and np.all(D == 3.0 * 2.0 ** -12)
    assert np.array_equal(J, np.argmax(d2 == 3.0 * 2.0 ** -12, axis=1))             # the lowest of the eight indices
    P, Q, I, J, D = _stats(cases["around_zero"], r)
    assert 0 < len(I) < len(P) and np.all((P.min(axis=0) < 0) & (P.max(axis=0) > 0)) and (P == 0.0).any()
    P, Q, I, J, D = _stats(cases["cell_edges"], r)
    h = r * (1.0 + 2.0 ** -20)
    k = np.concatenate([P, Q]) / h
    assert np.abs(k - np.round(k)).max() < 1e-6 and len(np.unique(np.floor(k))) >= 7 and 0 < len(I) < len(P)
    for name, c in G.tie_cases().items():
        P, Q, I, J, D = _stats(c, r)
        assert np.array_equal(J, [0]) and np.array_equal(Q[0] - P[0], c["expect"]), name
        assert np.linalg.norm(Q[0] - P[0]) == np.linalg.norm(Q[1] - P[0]) == 4 * G.GRID
        assert np.floor(P[0, 0] / h) == 0 and sorted(np.floor(Q[:, 0] / h)) == [0, 1]
    c = G.colliding_case()
    P, Q, I, J, D = _stats(c, r)
    cells = np.unique(np.floor(Q / h), axis=0)
    assert len(Q) == 2048 and len(cells) > 200 and np.abs(Q).max() > 49.0 and 100 < len(I) < len(P)
    c = G.huge_case()
    P, Q, I, J, D = _stats(c, r)
    f = np.abs(Q / h)
    assert f.min() > 2e6 / h and (f >= 2.0 ** 27).any() and (f >= 2.0 ** 28).any() and (f.max(axis=1) < 2.0 ** 27).any()
    assert np.array_equal(I, np.arange(128)) and np.all(D == 0.0)


def test_pose_map_inputs_cover_the_branches():
    rot, angle, axis = G.pose_map_inputs()
    assert len(rot) >= 256
    theta = np.linalg.norm(rot.astype(np.float64), axis=1)
    cos = np.cos(theta)
    assert (theta == 0.0).any() and ((theta > 0.0) & (theta < 1e-44)).any()
    assert ((cos > -0.5) & (cos < -0.5 + 1e-6)).any() and ((cos < -0.5) & (cos > -0.5 - 1e-6)).any()
    assert (theta > np.pi).sum() >= 4 * 14 and ((theta > G.POSE_SAFE_ANGLE) & (theta <= np.pi)).any()
    worst = 0.0
    for r in rot:
        Rm = R.rodrigues(r)
        assert np.abs(Rm - G.rodrigues_mp(r)).max() <= 1e-15
        back = G.log_map_mp(Rm)
        assert np.abs(G.rodrigues_mp(back) - Rm).max() < 1e-12 and np.linalg.norm(back) <= np.pi + 1e-12
        if np.linalg.norm(r.astype(np.float64)) <= G.POSE_SAFE_ANGLE:
            worst = max(worst, np.abs(back - r.astype(np.float64)).max())
    assert worst <= 1e-12


def test_normals_families_meet_their_preconditions():
    fams = G.normals_families()
    gapless = {}
    for name, f in fams.items():
        count, w, C, v0, eps, d = G.normals_reference_of(name)
        assert eps == 1e-10, (name, d)                               # the floor decides in every family
        if "count" in f:
            assert np.all(count == f["count"]), name
        ok = count >= 3
        gapless[name] = int((ok & (NR.relative_gap(w) < 0.1)).sum()), int(ok.sum())
        if f.get("planar"):
            assert ok.all() and np.all(w[:, 0] == 0.0) and np.all(C[:, 2, :] == 0.0), name
        print("%-28s K %4d, count %d..%d, %d of %d estimated queries have a relative gap below 0.1, d = %.2e"
              % (name, len(count), count.min(), count.max(), gapless[name][0], gapless[name][1], d))
    for name in ("planar", "planar_tilted", "nearly_planar", "far_from_origin"):
        assert gapless[name] == (0, 256), name                      # the direction is compared for every query
    for name in ("collinear", "coincident", "extent_much_smaller_than_r"):
        assert gapless[name][0] == gapless[name][1] > 0, name       # ... and for none: the residual decides
    assert gapless["too_few"] == (0, 0)
    count = G.normals_reference_of("isotropic")[0]
    assert (count == 27).sum() == 64 and gapless["isotropic"][0] >= 64
    assert G.normals_reference_of("planar")[0].min() == 4 and G.normals_reference_of("planar")[0].max() == 9
    ext = fams["extent_much_larger_than_r"]["support"]
    assert (ext.max(axis=0) - ext.min(axis=0)).max() > 1000 * 0.01
    ext = fams["extent_much_smaller_than_r"]["support"]
    assert (ext.max(axis=0) - ext.min(axis=0)).max() < 0.25 / 4 and np.all(G.normals_reference_of("extent_much_smaller_than_r")[0] == 200)
    out = G.normals_reference_of("queries_outside_the_box")[0]
    q, sup = fams["queries_outside_the_box"]["queries"], fams["queries_outside_the_box"]["support"]
    assert np.all((q < sup.min(axis=0)).any(axis=1) | (q > sup.max(axis=0)).any(axis=1))
    assert np.all(out[18:] == 0) and (out[:18] >= 3).sum() >= 6
    xyz, offsets, queries, radius = G.packed_edge_sets()
    assert list(np.diff(offsets)) == [100, 0, 216, 1, 2] and queries.shape == (5, 216, 3)


def test_the_mutants_fail_the_cases_written_for_them():
    kT, kobj = G.procrustes_allowance()
    c = G.procrustes_table()["slab_mirrored"]
    good = R.compose(R.umeyama(c["P"][c["I"]], c["Q"][c["J"]]), c["T0"])
    bad = R.compose(G.umeyama_no_reflection(c["P"][c["I"]], c["Q"][c["J"]]), c["T0"])
    assert G.transform_error(good, c["ref"], c["trans0"]) <= kT * c["u"]
    assert G.objective_error(good, c["ref"], c["v"]) <= kobj
    assert abs(np.linalg.det(good[:3, :3]) - 1.0) <= 8.0 * 2.0 ** -52
    assert abs(np.linalg.det(bad[:3, :3]) + 1.0) < 1e-12            # a reflection: not proper, ...
    assert G.transform_error(bad, c["ref"], c["trans0"]) > 1e6 * kT * c["u"]        # ... not the maximiser, ...
    assert G.objective_error(bad, c["ref"], c["v"]) > 1e6 * kobj                    # ... and above the maximum over SO(3)
    # without the fix the blob, whose Sigma has a positive determinant, still passes: the slab is what catches it
    b = G.procrustes_table()["blob"]
    same = R.compose(G.umeyama_no_reflection(b["P"][b["I"]], b["Q"][b["J"]]), b["T0"])
    assert G.transform_error(same, b["ref"], b["trans0"]) <= kT * b["u"]
    # `<=` for `<` in the radius test
    cases = G.matching_cases()
    for name, strict, inclusive in (("exact_radius", 0, 64), ("around_zero", None, None)):
        P, Q, I, J, D = _stats(cases[name], G.MATCH_RADIUS)
        got = G.count_inclusive(P, Q, G.MATCH_RADIUS)
        assert got > len(I), name
        if strict is not None:
            assert (len(I), got) == (strict, inclusive)
    fam = G.normals_families()["too_few"]
    sup = fam["support"].astype(np.float64)
    d = sup[:, None] - sup[None]
    assert (((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2) <= 0.25 ** 2).sum(axis=1).max() == 7     # `<=`: 7, not 1
