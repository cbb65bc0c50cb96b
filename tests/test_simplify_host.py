"""CPU: the NumPy restatement of DESIGN.md "Simplified meshes" (tests/simplify_reference.py) against closed forms on hand cases
with dyadic coordinates, the properties the definition promises, and the fused scenes of tests/fuse_reference.py.  What is
asserted of a scene was measured with this restatement and is listed in profiles/notes_simplify.md."""
import numpy as np
import pytest

import fuse_reference as FR
import simplify_reference as SR


def one_cell(case):
    """The sums and the placement of a hand case's cell (0, 0, 0)."""
    v, t = case['vertices'], case['triangles']
    keys = SR.cluster_keys(v, SR.HAND_ORIGIN, SR.HAND_CELL, SR.HAND_DIMS)
    assert np.all(keys == 0)
    _, rank, grid = SR.cells_of(keys, SR.HAND_DIMS)
    sums, counts = SR.cluster_sums(v, t, rank, grid, SR.HAND_ORIGIN, SR.HAND_CELL)
    pos, how, err = SR.cluster_place(sums, counts, grid, SR.HAND_ORIGIN, SR.HAND_CELL)
    return sums, counts, pos, how, err


# ---- hand cases -------------------------------------------------------------------------------------------------------------
def test_hand_cases_meet_their_closed_forms():
    for name, c in SR.hand_cases():
        sums, counts, pos, how, err = one_cell(c)
        print("%s: pos %s how %d E %.3g" % (name, pos[0], how[0], err[0]))
        assert counts.tolist() == [[len(c['vertices']), 3 * len(c['triangles'])]], name
        assert how[0] == c['how'], name
        assert np.array_equal(pos[0], c['pos']), name                                   # exact: dyadic numbers throughout
        if c['how'] < 4:
            assert err[0] == 0.0, name                                                  # the point lies on every plane
        else:
            assert err[0] > 0.0, name
    # the sheet alone, entry by entry: n = (0, 0, 0.25) three times, q_0 = (-0.25, -0.25, -0.25), d = 0.0625
    sums = one_cell(dict(SR.hand_cases())["a flat sheet: the mean moved onto the plane"])[0][0]
    want = np.zeros(16)
    want[SR.A0 + 5], want[SR.B0 + 2], want[SR.E0] = 3 * 0.0625, 3 * 0.25 * 0.0625, 3 * 0.0625 ** 2
    assert np.array_equal(sums, want)


def test_grid_boundaries_and_unused_vertices():
    nan, inf = np.float32('nan'), np.float32('inf')
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.5],        # exactly on a cell boundary: the upper cell
                  [2.0, 0.5, 0.5],                          # exactly on the grid's far plane: outside
                  [np.nextafter(np.float32(2.0), np.float32(0.0)), 1.0, 1.0], [-1e-30, 0.5, 0.5], [nan, 0.5, 0.5], [0.5, inf, 0.5],
                  [0.5, 0.5, -inf], [1.5, 1.5, 1.5]], np.float32)
    keys = SR.cluster_keys(v, [0.0, 0.0, 0.0], 1.0, (2, 2, 2))
    assert keys.tolist() == [0, 1, -1, 7, -1, -1, -1, -1, 7]
    cell_key, rank, grid = SR.cells_of(keys, (2, 2, 2))
    assert cell_key.tolist() == [0, 1, 7] and rank.tolist() == [0, 1, -1, 2, -1, -1, -1, -1, 2]
    assert grid.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1]]
    # a triangle with an index of -1, one with an index of V, one with an unused corner: dropped, no sums, nothing emitted
    t = np.array([[0, 1, 3], [0, 1, -1], [0, 9, 1], [0, 1, 2], [3, 1, 0]], np.int32)
    assert SR.dropped(t, rank).tolist() == [False, True, True, True, False]
    sums, counts = SR.cluster_sums(v, t, rank, grid, [0.0, 0.0, 0.0], 1.0)
    assert counts.tolist() == [[1, 2], [1, 2], [2, 2]]
    assert SR.triangle_keys(t, rank, 3).tolist() == [(0 << 42) + (1 << 21) + 2, -1, -1, -1, (0 << 42) + (2 << 21) + 1]
    # the default grid: the finite vertices' lower corner - c / 4, the smallest dims that hold the upper corner
    o, dims = SR.default_grid(v, 1.0)
    assert np.array_equal(o, [-0.25 - 1e-30, -0.25, -0.25]) and dims == (3, 2, 2)
    assert SR.default_grid(v[5:8], 1.0) is None
    assert SR.cluster_keys(v[:1], [0.0, 0.0, 0.0], 1.0, (1, 1, 1)).tolist() == [0]


def test_triangle_rules():
    rank = np.arange(6, dtype=np.int32)
    key = lambda a, b, c: (a << 42) + (b << 21) + c                                     # noqa: E731
    t = np.array([[1, 2, 3], [2, 3, 1], [3, 1, 2],       # the three rotations: one key
                  [1, 3, 2],                              # the mirror triple: another key, kept as well
                  [1, 2, 3],                              # a duplicate: the lower index stays
                  [4, 5, 1]], np.int32)
    k = SR.triangle_keys(t, rank, 6)
    assert k.tolist() == [key(1, 2, 3)] * 3 + [key(1, 3, 2), key(1, 2, 3), key(1, 4, 5)]
    pos = np.arange(18, dtype=np.float64).reshape(6, 3)
    v, out, cell_to_vertex = SR.assemble(k, pos)
    assert cell_to_vertex.tolist() == [-1, 0, 1, 2, 3, 4]                               # cell 0 is unreferenced: no vertex
    assert out.tolist() == [[0, 1, 2], [0, 2, 1], [0, 3, 4]]                            # kept in input order, renumbered
    assert np.array_equal(v, pos[1:].astype(np.float32))
    # two corners in one cell, all three in one cell
    two = np.array([0, 0, 1, 1, 1, 2], np.int32)
    assert SR.triangle_keys(np.array([[0, 1, 2], [2, 3, 4], [2, 0, 5], [0, 2, 5]], np.int32), two, 3).tolist() == \
        [-1, -1, key(0, 2, 1), key(0, 1, 2)]
    # the largest rank fits
    top = (1 << 21) - 1
    assert SR.triangle_keys(np.array([[0, 1, 2]], np.int32), np.array([top, top - 1, top - 2], np.int32), 1 << 21).tolist() == \
        [key(top - 2, top, top - 1)]
    assert SR.triangle_keys(np.array([[0, 1, 2]], np.int32), np.array([top, top - 1, top - 2], np.int32), top).tolist() == [-1]
    # an input that collapses entirely gives empty outputs
    v, out = SR.simplify(np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1]], np.float32), np.array([[0, 1, 2]], np.int32), 1.0)
    assert v.shape == (0, 3) and v.dtype == np.float32 and out.shape == (0, 3) and out.dtype == np.int32
    v, out = SR.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert v.shape == (0, 3) and out.shape == (0, 3)


def test_sums_that_give_no_quadric():
    grid, counts = np.zeros((4, 3), np.int32), np.full((4, 2), 2, np.int32)
    sums = np.zeros((4, 16))
    sums[:, :3] = [0.25, -0.5, 0.125]                                                   # the mean is (0.125, -0.25, 0.0625)
    sums[1, SR.A0] = np.nan
    sums[2, [SR.A0, SR.A0 + 3, SR.A0 + 5]] = -1.0, -2.0, -3.0                           # negative definite
    sums[3, [SR.A0, SR.A0 + 1]] = np.inf, 1.0
    pos, how, err = SR.cluster_place(sums, counts, grid, [0.0, 0.0, 0.0], 1.0)
    assert how.tolist() == [4, 4, 4, 4]
    assert np.array_equal(pos, np.tile([0.625, 0.25, 0.5625], (4, 1)))


# ---- properties -------------------------------------------------------------------------------------------------------------
def check_properties(v, t, cell, name):
    ov, ot, info = SR.simplify(v, t, cell, return_info=True)
    mv, mt, minfo = SR.simplify(v, t, cell, placement='mean', return_info=True)
    assert np.array_equal(ot, mt), name                                                 # placement='mean': the same triangles
    assert np.all(minfo['how'] == 4), name
    z = SR.cell_centres(info['cell_grid'], info['origin'], cell)
    # every vertex in its closed cell: |x| <= c / 2 is tested on x itself; z + x and the widened float32 vertices are then
    # within an ulp of float64 at the coordinates' magnitude
    slack = 4 * np.finfo(np.float64).eps * max(np.abs(z).max() + cell, 1e-300)
    assert np.all(np.abs(info['pos'] - z) <= cell / 2.0 + slack), name
    assert np.all(np.abs(minfo['pos'] - z) <= cell / 2.0 + slack), name
    used = info['cell_to_vertex'] >= 0
    assert np.array_equal(ov, info['pos'][used].astype(np.float32)), name
    # E(x) <= E(mean) whenever the quadric's point was taken, up to the rounding of E's terms
    took = info['how'] < 4
    scale = SR.error_scale(info['sums'], info['pos'] - z) + SR.error_scale(info['sums'], minfo['pos'] - z)
    assert np.all(info['err'][took] <= minfo['err'][took] + 64 * np.finfo(np.float64).eps * scale[took]), name
    assert np.all(info['err'][took] >= -64 * np.finfo(np.float64).eps * scale[took]), name
    return ov, ot, info


def test_properties_on_a_random_soup():
    v, t = SR.random_soup(seed=5)
    for cell in (0.07, 0.2, 0.45, 3.0):
        ov, ot, info = check_properties(v, t, cell, "soup, cell %g" % cell)
        print("soup, cell %g: %d -> %d triangles, how %s" % (cell, len(t), len(ot), np.bincount(info['how'], minlength=8).tolist()))
    assert len(SR.simplify(v, t, 3.0)[1]) == 0                                          # one cell: everything collapses


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def scene_mesh(name):
    if name == 'sphere':
        v, t = SR.sphere_mesh()
        return v, t, 1.0
    voxel = dict(cube=0.004, prism=0.0025)[name]
    s = FR.scene(name, voxel)
    return s['vertices'], s['triangles'], voxel


def surface_distance(name, points):
    if name == 'sphere':
        return np.abs(np.sqrt(((points - 12.0) ** 2).sum(axis=1)) - 8.3)
    return FR.surface_distance(points, FR.union_surface(FR.mesh_boxes(name)))


# (scene, cell in voxels, triangles, farthest sample from the true surface in voxels rounded up to a tenth): measured with
# this restatement (profiles/notes_simplify.md)
SCENES = [('cube', 3, 432, 0.8), ('cube', 4, 192, 0.7), ('prism', 4, 768, 0.8), ('sphere', 2, 618, 0.2), ('sphere', 3, 252, 0.3),
          ('sphere', 4, 156, 0.5)]


@pytest.mark.parametrize("name,cells,triangles,bound", SCENES)
def test_scenes_stay_closed_and_near_the_surface(name, cells, triangles, bound):
    v, t, voxel = scene_mesh(name)
    cell = cells * voxel
    ov, ot, info = check_properties(v, t, cell, name)
    before, m = FR.mesh_stats(v, t), FR.mesh_stats(ov, ot)
    far = surface_distance(name, SR.barycentric_samples(ov, ot, 7)).max() / voxel
    mv, mt = SR.simplify(v, t, cell, placement='mean')
    mean_m = FR.mesh_stats(mv, mt)
    mean_far = surface_distance(name, SR.barycentric_samples(mv, mt, 7)).max() / voxel
    share = SR.near_a_threshold(info['details'], cell).mean()
    print("%s, cell %d voxels: %d -> %d triangles, %d vertices, Euler %d, volume ratio %.4f (mean placement %.4f), farthest sample "
          "%.3f voxel (mean placement %.3f), how %s, near a threshold %.2f %%"
          % (name, cells, before['T'], m['T'], m['V'], m['euler'], m['volume'] / before['volume'], mean_m['volume'] / before['volume'], far,
             mean_far, np.bincount(info['how'], minlength=8).tolist(), 100 * share))
    assert m['T'] == triangles
    assert m['boundary'] == 0 and m['oriented'] and m['components'] == 1 and m['euler'] == 2
    assert far <= bound and bound < cells                                              # below one cell side
    assert share <= 0.01
    if name in ('cube', 'sphere'):
        assert abs(m['volume'] - before['volume']) < abs(mean_m['volume'] - before['volume'])


def test_grid_alignment_breaks_topology_reported():
    """Reported, not asserted: a face of the cube that coincides with a cell plane scatters its vertices over two layers of
    cells, and the result is no longer a sphere."""
    v, t, voxel = scene_mesh('cube')
    cell = 4 * voxel
    lo = v.astype(np.float64).min(axis=0)
    for name, offset in (("0", 0.0), ("c/2", cell / 2.0), ("c/4 (the default)", cell / 4.0)):
        ov, ot = SR.simplify(v, t, cell, origin=lo - offset)
        m = FR.mesh_stats(ov, ot)
        print("cube, cell 4 voxels, origin = lower corner - %s: %d triangles, Euler %d, %d boundary edges, %d components"
              % (name, m['T'], m['euler'], m['boundary'], m['components']))
        assert m['T'] > 0
