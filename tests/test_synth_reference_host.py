"""CPU: the restatement of on-line synthesis alone (tests/synth_reference.py) -- every hull-vertex case that
tests/test_50_synth_paths_gpu.py runs lies inside the contract csrc/synth.hip states (no exact repeats, the viewpoint a hull
vertex, every non-vertex clearly below the hull; the lattices: exactly corners + viewpoint), the integer gather against a
plain loop, the occluder against hand-placed Philox words."""
import os

import numpy as np
import pytest

import pose_sampling_reference as P
import synth_reference as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(case):
    missed = S.conditions(case)
    hull = S.hull_of(case)
    print("SYNTHREF %-22s n1 %5d vertices %5d smallest non-vertex margin %.3g" % (case.name, len(case.points), len(hull.vertices),
                                                                                S.smallest_margin(case)))
    assert not missed, (case.name, missed)
    if case.kind != "lattice":
        assert S.smallest_margin(case) >= 1e-10


@pytest.mark.parametrize("name", S.HULL_CASE_NAMES)
def test_hull_case_is_inside_the_contract(name):
    cases = S.hull_cases()
    assert tuple(cases) == S.HULL_CASE_NAMES
    _check(cases[name])


def test_lattice_vertex_counts():
    """The cube lattice gives 9 vertices, the plane 5: corners + viewpoint, nothing from a face, an edge or the inside."""
    cube, plane = S.hull_cases()["lattice_5x5x5"], S.hull_cases()["lattice_7x7_plane"]
    assert len(S.hull_of(cube).vertices) == 9 and len(cube.corners) == 9 and cube.points.shape == (126, 3)
    assert len(S.hull_of(plane).vertices) == 5 and len(plane.corners) == 5 and plane.points.shape == (50, 3)
    assert np.array_equal(cube.points, np.round(cube.points)) and np.array_equal(plane.points, np.round(plane.points))
    assert (plane.points[:49, 2] == 4).all()
    assert S.visible_ids(cube).tolist() == sorted(cube.corners)[:-2] and S.visible_ids(plane).tolist() == sorted(plane.corners)[:-2]


@pytest.mark.parametrize("name", ["b513_n9", "b3_n9", "b3_n194", "b3_n4097", "golden_2449"])
def test_batch_cases_are_inside_the_contract(name):
    batch = S.golden_batch(GOLDEN) if name == "golden_2449" else S.batch_cases()[name]
    assert len({c.name for c in batch}) == len(batch) and len({c.points.shape for c in batch}) == 1
    for case in batch[:: 16 if len(batch) > 64 else 1]:         # (every cloud is checked; one in 16 of the 513 is printed)
        _check(case)
    for case in batch:
        assert not S.conditions(case), case.name


def test_conforming_seed_search_is_a_function_of_the_inputs():
    a, b = S.conforming_flipped_cloud(1025), S.conforming_flipped_cloud(1025)
    assert a.name == "flipped_1025_s0" and np.array_equal(a.points, b.points)
    assert np.array_equal(a.points, S.hull_cases()["flipped_1025_s0"].points)


def test_largest_cloud_case_is_inside_the_contract():
    """The GPU test makes its largest case at the size it finds there; 12 783 points is what the library built from this
    tree accepts (160 KB of LDS less the 16-wave hull kernel's static 10.2 KB, 12 bytes a point)."""
    case = S.conforming_flipped_cloud(12783)
    assert case.name == "flipped_12783_s0"
    _check(case)


def test_margin_signs():
    """A cube's corners and its centre: the centre lies half an edge below every face, the diagonal is sqrt(3)."""
    from scipy.spatial import ConvexHull
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)] + [[0.5, 0.5, 0.5], [0.5, 0.5, 1.0], [0.5, 0.5, 1.25]], float)
    hull = ConvexHull(p[:8])
    m = S.margin(p, hull, [8, 9, 10])
    assert np.allclose(m, np.array([0.5, 0.0, -0.25]) / np.linalg.norm([1, 1, 1.25]), atol=1e-12)
    assert S.margin(p, hull, []).shape == (0,)


def _gather_loop(ids, org, seed, h, rows):
    """hpr_gather_kernel as a plain loop over output rows."""
    ids = sorted(int(i) for i in ids)
    nv = max(0, len(ids) - 2)
    vis, vid, src = [], [], []
    for r in range(rows):
        if r < nv:
            row = r
        elif nv > 0:
            row = int(P.philox4x32(seed, [(h << 32) | r], 7)[0, 0]) % nv
        else:
            row = -1
        vis.append(org[ids[row]] if row >= 0 else np.zeros(3, np.float32))
        vid.append(ids[r] if r < nv else -1)
        src.append(row)
    return np.array(vis, np.float32).reshape(rows, 3), nv, np.array(vid, np.int32), np.array(src, np.int32)


@pytest.mark.parametrize("ids", [[], [4], [9, 2], [7, 0, 3], [11, 1, 5, 8, 2, 10, 6]])
def test_gather_equals_a_plain_loop(ids):
    org = np.random.default_rng(3).standard_normal((12, 3)).astype(np.float32)
    nv = max(0, len(ids) - 2)
    for seed in (0, 2 ** 40 + 3):
        for h in (0, 2):
            for rows in sorted({1, max(1, nv - 1), max(1, nv), nv + 1, 12, 36}):
                got, want = S.gather(ids, org, seed, h, rows), _gather_loop(ids, org, seed, h, rows)
                assert got[1] == want[1] == nv
                for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
                    assert g.dtype == w.dtype and np.array_equal(g, w), (seed, h, rows)
                if nv == 0:
                    assert (got[0] == 0).all() and (got[2] == -1).all() and (got[3] == -1).all()
                else:
                    assert np.array_equal(got[3][:min(nv, rows)], np.arange(min(nv, rows))) and got[3].max() < nv
    # the draw depends on the sample and on the seed
    if nv > 1:
        a = S.gather(ids, org, 0, 0, 400)[3]
        assert not np.array_equal(a, S.gather(ids, org, 0, 1, 400)[3]) and not np.array_equal(a, S.gather(ids, org, 1, 0, 400)[3])


def test_occluder_follows_the_philox_words():
    """spherical_occluder against the words of the known-vector-checked Philox, placed by hand: centre x from words 0 / 1 of
    stream 1, y from words 2 / 3, z from words 0 / 1 of stream 2; pair j's normals from streams 3 and 4 at (cloud << 32) | j;
    blob 0 on even rows, blob 1 on odd rows."""
    f = np.float32
    seed, b, per = 0x0123456789ABCDEF, 3, 5
    wnear, hnear, near, sigma = f(0.71901), f(0.55785), f(0.5), f(0.01)
    trans = np.array([[0.1, 0.2, 0.6], [0.0, 0.0, 1.1], [-0.3, 0.1, 1.6]], f)
    occ = S.spherical_occluder(trans, per, wnear, hnear, near, sigma, seed)
    assert occ.shape == (b, 2 * per, 3) and occ.dtype == f
    for cloud in range(b):
        z = trans[cloud, 2]
        w1, w2 = P.philox4x32(seed, [cloud], 1)[0], P.philox4x32(seed, [cloud], 2)[0]
        nx, ny, nz = P.normal2(w1[0], w1[1]), P.normal2(w1[2], w1[3]), P.normal2(w2[0], w2[1])
        for blob in range(2):
            c = [nx[blob] * (wnear / f(10)), ny[blob] * (hnear / f(10)), (near + z) / f(2) + nz[blob] * ((z - near) / f(6))]
            for j in range(per):
                w3, w4 = P.philox4x32(seed, [(cloud << 32) | j], 3)[0], P.philox4x32(seed, [(cloud << 32) | j], 4)[0]
                g = list(P.normal2(w3[0], w3[1])) + list(P.normal2(w3[2], w3[3])) + list(P.normal2(w4[0], w4[1]))
                want = np.array([c[a] + sigma * g[3 * blob + a] for a in range(3)], f)
                assert np.array_equal(occ[cloud, 2 * j + blob], want), (cloud, blob, j)
    # a sample's rows do not depend on the batch it is in; two seeds differ; double differs from single only by rounding
    assert np.array_equal(S.spherical_occluder(trans[:2], per, wnear, hnear, near, sigma, seed), occ[:2])
    other = S.spherical_occluder(trans, per, wnear, hnear, near, sigma, seed + 1)
    assert not np.array_equal(other, occ) and np.abs(other - occ).max() > 1e-3
    o32, tol = S.occluder_tolerance(trans, per, wnear, hnear, near, sigma, seed)
    assert np.array_equal(o32, occ) and 4 * np.spacing(f(np.abs(occ).max())) <= tol < 1e-4
    # the two blobs of a cloud are apart, each of spread sigma around its own centre
    big = S.spherical_occluder(trans, 200, wnear, hnear, near, sigma, seed)
    for blob in range(2):
        assert abs(big[:, blob::2].std(axis=1).mean() - 0.01) < 1e-3
    assert np.abs(big[:, 0::2].mean(1) - big[:, 1::2].mean(1)).max() > 0.01
    # z == near: no spread of the centres along z, both sit on the near plane
    flat = S.spherical_occluder(np.array([[0, 0, near]], f), 200, wnear, hnear, near, sigma, seed)
    assert abs(flat[0, :, 2].mean() - near) < 3e-3


def test_flip_subtracts_the_centre_first():
    from oracle import synth_oracle as SO
    rng = np.random.default_rng(9)
    a, b = (rng.standard_normal((7, 3)) + [0, 0, 5]).astype(np.float32), (rng.standard_normal((3, 3)) + [0, 0, 4]).astype(np.float32)
    c = np.array([0.02, -0.03, 0.01], np.float32)
    f, o = S.flip(a, b, c, 0.0)
    assert f.shape == o.shape == (11, 3) and np.array_equal(o[:-1], np.concatenate([a, b], 0) - c) and (o[-1] == 0).all() and (f[-1] == 0).all()
    far = int(np.argmax(np.linalg.norm(o, axis=1)))
    assert np.array_equal(f[far], o[far])                              # param = 0: R is the largest norm itself
    f2, o2 = S.flip(a, None, None, 0.8 * np.pi)
    f3, o3 = SO.spherical_flip(a)
    assert np.array_equal(f2, f3) and np.array_equal(o2, o3)
    f4, _ = S.flip(np.zeros((0, 3), np.float32), b, None, 0.8 * np.pi)
    assert np.array_equal(f4, SO.spherical_flip(b)[0])
