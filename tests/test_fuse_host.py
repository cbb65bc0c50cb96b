"""CPU: the NumPy restatement of DESIGN.md "Fused models" (tests/fuse_reference.py) anchored on its own -- the integration
against closed forms on inputs whose arithmetic is exact, the case table against the geometry, the extraction on fields
written straight into the state, and the two fused scenes whose figures profiles/notes_fuse.md quotes.  The GPU tests
(tests/test_44_fuse_gpu.py) then hold the kernels to this restatement bit for bit."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

import fuse_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1.0 / 64.0


@pytest.fixture(scope="module")
def hand():
    return dict(FR.hand_cases())


# ---- integration by hand ---------------------------------------------------------------------------------------------------
def test_plane_votes_in_closed_form(hand):
    st = FR.run_case(hand["plane at 1 m"])
    for k in range(16):
        sdf_voxels = 7.5 - k                                          # (1 - Z_k) / s
        q = int(min(sdf_voxels, 4.0) * 1024)
        want = [q, 1, 0, 0] if sdf_voxels >= -1.5 else [0, 0, q, 1] if sdf_voxels >= -4.0 else [0, 0, 0, 0]
        assert np.all(st[k] == want), k


def test_thresholds_on_either_side(hand):
    c = hand["thresholds"]
    got = {}
    for f in range(9):
        one = dict(c, depth=c['depth'][f:f + 1], intr=c['intr'][f:f + 1], poses=c['poses'][f:f + 1])
        st = FR.run_case(one)
        got[f] = [tuple(st[k, 0, 0]) for k in (3, 12, 14)]
    # voxel 3, the surface 4 voxels behind it: one depth unit (1/8192 m = 1/128 voxel) nearer, at, and beyond the truncation
    assert [got[f][0] for f in (0, 1, 2)] == [(4088, 1, 0, 0), (4096, 1, 0, 0), (4096, 1, 0, 0)]
    # voxel 12, the surface 1.5 voxels in front of it: just past -behind is the deep band, at it and inside the near band
    assert [got[f][1] for f in (3, 4, 5)] == [(0, 0, -1544, 1), (-1536, 1, 0, 0), (-1528, 1, 0, 0)]
    # voxel 14, the surface 4 voxels in front of it: past -front nothing, at it and inside the deep band
    assert [got[f][2] for f in (6, 7, 8)] == [(0, 0, 0, 0), (0, 0, -4096, 1), (0, 0, -4088, 1)]
    # the frames summed in one call are the sum of the frames alone
    assert np.array_equal(FR.run_case(c)[[3, 12, 14], 0, 0], sum(np.array(got[f]) for f in range(9)))


def test_a_tie_of_rint_goes_to_even(hand):
    st = FR.run_case(hand["rint tie"])
    for k in range(4, 10):                                            # (7.5 - k) 1024 + 0.5 exactly; the integer is even
        assert np.all(st[k, :, :, 0] == int((7.5 - k) * 1024)) and np.all(st[k, :, :, 1] == 1), k
    assert np.all(st[10, :, :, 2] == -2560)


def test_image_borders(hand):
    st = FR.run_case(hand["image borders"])
    cnt = st[0, :, :, 1]                                              # Z = 1: voxel i projects to u + 0.5 = i exactly
    assert np.all(cnt[:8, :8] == 1) and np.all(cnt[8:, :] == 0) and np.all(cnt[:, 8:] == 0)
    assert np.all(st[0, :8, :8, 0] == 0) and np.all(st[1, 2:7, 2:7, :2] == [-1024, 1])      # sdf = 0, and -s one voxel on


def test_z_near_is_exclusive(hand):
    st = FR.run_case(hand["z_near"])
    votes = st[..., 1] + st[..., 3]
    assert np.all(votes[0] == 0) and np.all(votes[1] == 0) and np.all(votes[2] == 1) and np.all(votes[3] == 1)


def test_depth_zero_and_labels(hand):
    st = FR.run_case(hand["depth 0"])
    votes = st[..., 1] + st[..., 3]
    assert np.all(votes[:, 1, 1] == 0) and np.all(votes[:, 6, 6] == 1) and np.all(votes[:, 1, 6] == 1)
    st = FR.run_case(hand["labels"])
    votes = st[..., 1] + st[..., 3]
    assert np.all(votes[:, 5, 1] == 2) and np.all(votes[:, 5, 6] == 1)           # want 0 and 2 on the left, want 0 alone on the right
    c = dict(hand["labels"])
    c.pop('label'), c.pop('want')
    assert np.all((lambda s: s[..., 1] + s[..., 3])(FR.run_case(c))[:, 5, [1, 6]] == 3)


def test_any_split_and_order_of_the_frames_gives_the_same_state():
    s = FR.scene('cube', 0.004)
    a = dict(origin=s['origin'], voxel=s['voxel'], front=4 * s['voxel'], behind=1.5 * s['voxel'])
    st = FR.new_state(s['dims'])
    for sel in (slice(9, 14), slice(0, 9)):
        FR.integrate(st, depth=s['depth'][sel][::-1], intr=s['intr'][sel][::-1], poses=s['poses'][sel][::-1], **a)
    assert np.array_equal(st, s['state'])


# ---- the case table --------------------------------------------------------------------------------------------------------
def test_generated_tables_are_the_ones_in_the_kernel_file_and_agree_with_the_geometry():
    sys.path.insert(0, ROOT)
    from tools import gen_tsdf_tables as G
    out = io.StringIO()
    with redirect_stdout(out):
        G.main()
    source = open(os.path.join(ROOT, "cloudaae_amd", "csrc", "tsdf.hip")).read()
    for line in out.getvalue().strip().splitlines():
        assert line in source, line
    table = FR.swap_table()
    for ti, tet in enumerate(G.tetrahedra()):
        assert tuple(tet) == tuple(FR.tetrahedra()[ti])
        for p in range(1, 15):
            assert G.swapped(tet, p) == bool(table[ti, p]), (ti, p)
            assert [list(t) for t in FR.pattern_triangles(p)] == [list(map(tuple, t)) for t in G.triangles(p)]


def _tet_gradient(values, point):
    """The gradient of the piecewise linear field of a unit cell (corner values [8]) at a point inside it."""
    order = sorted(range(3), key=lambda a: -point[a])                 # the tetrahedron: coordinate a1 >= a2 >= a3
    c1 = 1 << order[0]
    c2 = c1 | (1 << order[1])
    g = np.zeros(3)
    g[order[0]], g[order[1]], g[order[2]] = values[c1] - values[0], values[c2] - values[c1], values[7] - values[c2]
    return g


def test_all_256_patterns_face_outwards():
    rng = np.random.default_rng(11)
    per_tet = [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    for mask in range(256):
        mag = rng.uniform(0.1, 0.9, 8)
        st = FR.pattern_state(mask, mag)
        count, pos, key = FR.extract_triangles(st, [0.0, 0.0, 0.0], 1.0)
        want = sum(per_tet[sum(((mask >> c) & 1) << l for l, c in enumerate(tet))] for tet in FR.tetrahedra())
        assert count.tolist() == [want] and len(pos) == want
        values = FR.corner_values(st)[0].reshape(8)
        for tri in pos:
            n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            g = _tet_gradient(values, tri.mean(axis=0) - 0.5)
            assert n @ g > 0, (mask, tri)
        assert key.min(initial=1) >= 1 and np.all((key % 8 >= 1)) and key.max(initial=0) < 8 * 8


def test_random_field_is_closed_and_oriented():
    v, t = FR.extract_mesh(FR.random_field_state(), [0.0, 0.0, 0.0], 1.0)
    s = FR.mesh_stats(v, t)
    assert s['T'] > 1000 and s['boundary'] == 0 and s['oriented'] and s['volume'] > 0


# ---- extraction on a sphere ------------------------------------------------------------------------------------------------
def test_sphere():
    st = FR.sphere_state()
    v, t = FR.extract_mesh(st, [0.0, 0.0, 0.0], 1.0)
    s = FR.mesh_stats(v, t)
    assert s['boundary'] == 0 and s['oriented'] and s['components'] == 1 and s['euler'] == 2 and s['volume'] > 0
    L, r, front = np.sqrt(3.0), 8.3, 4.0
    bound = L * L / (8.0 * (r - L)) + front / 8192.0
    err = np.abs(np.sqrt(((v.astype(np.float64) - 12.0) ** 2).sum(axis=1)) - r).max()
    print("sphere: %d vertices, %d triangles, worst |radius error| %.4f voxel against %.4f" % (s['V'], s['T'], err, bound))
    assert err <= bound


def test_unknown_corners_min_count_and_an_empty_volume():
    st = FR.sphere_state()
    full = FR.extract_triangles(st, [0.0, 0.0, 0.0], 1.0)
    hole = st.copy()
    hole[12, 12, 20] = 0                                             # a voxel next to the surface (radius 8.3 around 12)
    count = FR.extract_triangles(hole, [0.0, 0.0, 0.0], 1.0)[0].reshape(23, 23, 23)
    assert full[0].reshape(23, 23, 23)[11:13, 11:13, 19:21].sum() > 0 and count[11:13, 11:13, 19:21].sum() == 0
    rest = np.ones((23, 23, 23), bool)
    rest[11:13, 11:13, 19:21] = False
    assert np.array_equal(count[rest], full[0].reshape(23, 23, 23)[rest])
    v, t = FR.extract_mesh(hole, [0.0, 0.0, 0.0], 1.0)
    assert FR.mesh_stats(v, t)['boundary'] > 0
    # min_count = 2: single votes do not count; two votes of the same value give the same mesh; the deep band fills in
    assert FR.extract_triangles(st, [0.0, 0.0, 0.0], 1.0, min_count=2)[0].sum() == 0
    twice = st.copy()
    twice[..., 0] *= 2
    twice[..., 1] = 2
    deep = st[..., [2, 3, 0, 1]].copy()
    for other in (twice, deep):
        got = FR.extract_triangles(other, [0.0, 0.0, 0.0], 1.0, min_count=2)
        assert all(np.array_equal(a, b) for a, b in zip(got, full))
    mixed = st.copy()
    mixed[..., 2], mixed[..., 3] = -st[..., 0], 1                    # the deep band says the opposite: used only where near is short
    assert all(np.array_equal(a, b) for a, b in zip(FR.extract_triangles(mixed, [0.0, 0.0, 0.0], 1.0), full))
    inverted = FR.extract_triangles(mixed, [0.0, 0.0, 0.0], 1.0, min_count=2)
    assert inverted[0].sum() == full[0].sum() and not np.array_equal(inverted[2], full[2])
    # all outside, and v == 0 counts as outside
    for field in (0.5, 0.0):
        count, pos, key = FR.extract_triangles(FR.state_from_field(np.full((5, 4, 3), field)), [0.0, 0.0, 0.0], 1.0)
        assert count.shape == (4 * 3 * 2,) and count.sum() == 0 and pos.shape == (0, 3, 3) and key.shape == (0, 3)
        v, t = FR.weld(pos, key)
        assert v.shape == (0, 3) and t.shape == (0, 3)


# ---- the scenes ------------------------------------------------------------------------------------------------------------
# measured with this restatement on the project's rasteriser (profiles/notes_fuse.md), rounded up to the next tenth of a voxel
SCENES = [('cube', 0.004, 0.8, 0.7), ('prism', 0.0025, 0.9, 0.8)]


@pytest.mark.parametrize("name, voxel, vertex_cap, sample_cap", SCENES, ids=[s[0] for s in SCENES])
def test_fused_scene(name, voxel, vertex_cap, sample_cap):
    s = FR.scene(name, voxel)
    m = FR.mesh_stats(s['vertices'], s['triangles'])
    to_surface, to_vertex = FR.scene_distances(s, name)
    print("%s at %g mm: %s voxels, V %d T %d, vertex -> surface %.3f voxel, surface sample -> vertex %.3f voxel"
          % (name, voxel * 1e3, s['dims'], m['V'], m['T'], to_surface, to_vertex))
    assert m['boundary'] == 0 and m['oriented'] and m['components'] == 1 and m['euler'] == 2 and m['volume'] > 0
    assert vertex_cap <= 1.0 and sample_cap <= 1.0
    assert to_surface <= vertex_cap and to_vertex <= sample_cap


def test_one_symmetric_band_bulges():
    s = FR.scene('cube', 0.004, FR.FRONT_VOXELS)                      # behind = front
    to_surface, _ = FR.scene_distances(s, 'cube')
    m = FR.mesh_stats(s['vertices'], s['triangles'])
    print("behind = front: vertex -> surface %.3f voxel, Euler %d, %d components" % (to_surface, m['euler'], m['components']))
    assert to_surface > 2.0


def test_union_surface_of_the_prism():
    rects = FR.union_surface(FR.mesh_boxes('prism'))
    area = sum(float(np.prod(hi - lo)) for _, _, lo, hi in rects)
    # two boxes of 16 x 4 x 4 and 4 x 10 x 4 cm that share a 4 x 4 x 4 cm block: an L of 16 + 6 cm by 4 x 4
    l_area = 2 * (0.16 * 0.04 + 0.04 * 0.06) + 0.04 * (0.16 + 0.10 + 0.04 + 0.06 + 0.12 + 0.04)
    # where faces of the two boxes coincide (x, y low over the shared block's 4 x 4 cm, z low and high likewise) both are listed:
    # twice the same surface, which changes no distance
    assert abs(area - (l_area + 4 * 0.04 * 0.04)) < 1e-7
    assert FR.surface_distance([[0.0, 0.0, 0.0]], rects)[0] == pytest.approx(0.01, abs=1e-7)
