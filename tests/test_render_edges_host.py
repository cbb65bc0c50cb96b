"""CPU: every family of tests/render_edge_cases.py has the property its GPU test (tests/test_40_render_edges_gpu.py)
rests on, measured with the restatement (tests/render_reference.py) and with edge values recomputed here -- so a scene
that silently misses its boundary fails in this file.  Then the restatement's neighbours (render_reference.VARIANTS:
exclusive edges, half-even rounding, the open ends of the depth range, of the near plane and of the guard band, the
owner search with < for <=): each changes the images of the family named for it."""
import numpy as np
import pytest

import render_edge_cases as C
import render_reference as R

S = C.RN_SMALL
KEYS = ('depth', 'label', 'tri', 'dropped', 'degenerate')


def drawn(family, case):
    """[(rank, setup)] of the ranks that reach the rasteriser."""
    return [(g, s) for g, s in enumerate(C.setups(family, case)) if s is not None]


def coverage(s):
    wa, wb, wc = C.edge_values(s)
    assert np.all(wa + wb + wc == s['area2'])
    zeros = (wa == 0).astype(int) + (wb == 0) + (wc == 0)
    return (wa >= 0) & (wb >= 0) & (wc >= 0), zeros


def test_constants_are_read_from_the_kernel():
    assert (C.RN_SMALL, C.RN_BLOCK, C.RN_QUEUE_BLOCKS, C.WAVES) == (16, 256, 1024, 4096)     # today's; the families scale


def test_setups_agree_with_the_restatement():
    """The helper's clamped boxes are the restatement's, rank by rank, in every scene."""
    for family, case in C.ALL:
        box = C.reference(family, case)['box']
        mine = C.setups(family, case)
        assert len(box) == len(mine), (family, case)
        for g, s in enumerate(mine):
            want = -1 if s is None else np.prod(C.box_dims(s))
            assert box[g] == want, (family, case, g)


# ---- on_edge ---------------------------------------------------------------------------------------------------------------
def test_on_edge_samples_sit_on_edges_and_vertices():
    on_edge, on_vertex = 0, 0
    for case in C.CASES['on_edge']:
        for g, s in drawn('on_edge', case):
            if min(C.box_dims(s)) == 0:
                continue
            cov, zeros = coverage(s)
            on_edge += int((cov & (zeros >= 1)).sum())
            on_vertex += int((cov & (zeros == 2)).sum())
    print("on_edge: %d covered samples with an edge value of 0, %d of them vertices" % (on_edge, on_vertex))
    assert on_edge >= 200 and on_vertex >= 20


def test_on_edge_shared_edge_goes_to_the_nearer_later_triangle():
    ref = C.reference('on_edge', 'shared')
    H, W = ref['tri'].shape[1:]
    owners = [[[] for _ in range(W)] for _ in range(H)]
    for g, s in drawn('on_edge', 'shared'):
        cov, zeros = coverage(s)
        u0, u1, v0, v1 = s['box']
        for v, u in zip(*np.nonzero(cov & (zeros >= 1))):
            owners[v0 + v][u0 + u].append(g)
    shared = [(v, u, o) for v in range(H) for u in range(W) for o in [owners[v][u]] if len(o) >= 2]
    later = [(v, u) for v, u, o in shared if ref['tri'][0, v, u] > min(o)]
    first = [(v, u) for v, u, o in shared if ref['tri'][0, v, u] == min(o)]
    print("shared: %d samples on an edge of two triangles or more; the later rank wins %d, the first %d"
          % (len(shared), len(later), len(first)))
    assert len(shared) >= 40 and len(later) >= 10 and len(first) >= 10
    # the first pair: ranks 0 (depth 1024) and 1 (512) meet on the anti-diagonal u + v = 16
    assert all(ref['tri'][0, v, 16 - v] == 1 and ref['depth'][0, v, 16 - v] == 512 for v in range(2, 15))
    # the pair at one depth: the lower rank (4) keeps it
    assert all(ref['tri'][0, v, 48 - v] == 4 for v in range(2, 15))


def test_on_edge_slivers_and_boxes_below_zero():
    sl = C.setups('on_edge', 'slivers')
    dims = [C.box_dims(s) for s in sl]
    assert dims[0] == (8, 8) and dims[1] == (3, 3) and dims[4] == (1, 21) and dims[5] == (15, 1)
    assert 0 in dims[2] and dims[3] == (0, 21)
    counts = [int(coverage(s)[0].sum()) if min(C.box_dims(s)) else 0 for s in sl]
    assert counts == [0, 0, 0, 0, 21, 1]
    ref = C.reference('on_edge', 'slivers')
    assert set(np.unique(ref['tri'])) == {-1, 4, 5} and list(ref['box']) == [64, 9, 0, 0, 21, 15]
    ng = C.setups('on_edge', 'negative')
    assert [min(s['xs']) for s in ng[:2]] == [-768, -767] and [max(s['xs']) for s in ng[2:4]] == [-1, 0]
    assert [C.box_dims(s) for s in ng] == [(6, 7), (5, 7), (0, 11), (1, 13), (21, 0), (21, 1), (7, 7)]
    ref = C.reference('on_edge', 'negative')
    assert (ref['tri'] == 3).sum() == 1 and ref['tri'][0, 32, 0] == 3 and ref['tri'][0, 0, 30] == 5
    assert not (ref['tri'] == 2).any() and not (ref['tri'] == 4).any()


def test_on_edge_exact_halves_exist_and_decide():
    meshes, frames, intr, H, W, z_near = C.scene('on_edge', 'half_vertex')
    x = float(meshes[0][0][0, 0])
    assert x * 256.0 == 2560.5                                       # an exact half above an even integer
    ix = R.project(meshes[0][0], C.EYE, intr[0], z_near)[0]
    even = R.project(meshes[0][0], C.EYE, intr[0], z_near, variant='half_even_vertex')[0]
    assert ix[0] == 2561 and even[0] == 2560 and np.array_equal(ix[1:], even[1:])
    up, ev = C.reference('on_edge', 'half_vertex'), C.reference('on_edge', 'half_vertex', 'half_even_vertex')
    assert up['tri'][0, 3, 10] == 0 and ev['tri'][0, 3, 10] == -1
    # (rounded to even the vertex itself lands on the sample (10, 2), which the definition leaves out)
    assert up['tri'][0, 2, 10] == -1 and ev['tri'][0, 2, 10] == 0 and int((up['tri'] != ev['tri']).sum()) == 2
    # the depth: z = 1 and 1 / 2 exactly, factor 1000.5: 1000.5 rounds up to 1001, to even 1000; 500.25 is no half
    assert float(np.float32(C.HALF_FACTOR)) == 1000.5
    up, ev = C.reference('on_edge', 'half_depth'), C.reference('on_edge', 'half_depth', 'half_even_depth')
    assert set(np.unique(up['depth'])) == {0, 500, 1001} and set(np.unique(ev['depth'])) == {0, 500, 1000}


# ---- box_threshold ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES['box_threshold'])
def test_box_threshold_sizes(case):
    w, h = C.BOXES[case] if case in C.BOXES else C.CORNERS[case]
    assert case.startswith('lane_') == (w * h <= S) or case.startswith('corner_')
    sl = C.setups('box_threshold', case)
    ref = C.reference('box_threshold', case)
    assert len(sl) == 2 and [C.box_dims(s) for s in sl] == [(w, h), (w, h)] and list(ref['box']) == [w * h, w * h]
    H, W = ref['tri'].shape[1:]
    if case.startswith('corner_'):
        xs, ys = sl[0]['xs'], sl[0]['ys']
        assert (max(xs) - min(xs)) // 256 >= 300 and sl[0]['box'][1] == W - 1 and sl[0]['box'][3] == H - 1
    # the mirrored triangle covers the last sample of its box: the tail of a partial 8 x 8 block decides
    u0, u1, v0, v1 = sl[1]['box']
    assert ref['tri'][1, v1, u1] == 1 and ref['tri'][0, v0, u0] == 0
    assert (ref['tri'] >= 0).sum() >= 2


def test_box_threshold_covers_the_sizes_around_the_switch():
    sizes = sorted(set(w * h for w, h in list(C.BOXES.values()) + list(C.CORNERS.values())))
    assert {S - 1, S, S + 1} <= set(sizes)
    assert {(1, S - 1), (1, S), (1, S + 1), (S - 1, 1), (S, 1), (S + 1, 1), (4, 4), (2, 8), (3, 6), (17, 1), (8, 8), (9, 9),
            (1, 65), (65, 1), (7, 64), (15, 17)} <= set(C.BOXES.values())


# ---- queue_stride ----------------------------------------------------------------------------------------------------------
def test_queue_stride_makes_a_third_trip_and_every_ballot():
    box = C.reference('queue_stride', 'grid_and_ballots')['box']
    large = box > S
    queued = int(large.sum())
    n = C._grid_cells()
    print("queue_stride: %d x %d cells, %d triangles, %d queued against %d waves; boxes %s"
          % (n, n, len(box), queued, C.WAVES, sorted(set(box.tolist()))))
    assert queued > 2 * C.WAVES and set(box[:2 * n * n].tolist()) == {16, 20, 25}
    # small and large lanes inside one wave wherever the wave lies in a row of cells 3 pixels high (the rows 4 pixels high
    # hold boxes of 20 and 25 samples only)
    grid = large[:2 * n * n // 64 * 64].reshape(-1, 64)
    mixed = grid.any(axis=1) & ~grid.all(axis=1)
    print("queue_stride: %d of the grid's %d whole waves hold small and large boxes" % (mixed.sum(), len(grid)))
    assert mixed.sum() >= len(grid) // 3 and grid.any(axis=1).all()
    start = C.ballot_start()
    assert start % 64 == 0 and len(box) == start + 256
    waves = large[start:].reshape(4, 64)
    assert waves[0].all() and not waves[1].any()
    assert waves[2][0] and not waves[2][1:].any() and waves[3][63] and not waves[3][:63].any()
    assert np.all(box[start:] > 0)


# ---- depth_range -----------------------------------------------------------------------------------------------------------
def test_depth_range_ends():
    for case, want in C.RANGE_VALUES.items():
        ref = C.reference('depth_range', case)
        assert set(np.unique(ref['depth'])) == want, case
        assert (ref['depth'] != 0).sum() == (0 if want == {0} else 17 * 17 + 6), case      # the square and half a 3 x 3 box
    f = C.RANGE_FACTORS
    assert f['du_0'] < 8.0 and f['du_65535'] < f['du_65535_high'] < f['du_65536']
    assert all(float(np.float32(x)) == x for x in f.values())
    d = C.reference('depth_range', 'tilted')['depth'][0]
    # covered, and cut at both ends inside one box: du = 0 at the near vertex, 65536 along the far edge
    # (1 / z is linear on the screen, so du stays below 1 for three quarters of the way)
    assert not d[4, 4:35].any() and d[4, 35:44].all() and not d[4:45, 44].any() and d[30, 42] > 0
    assert d[10, 4] == 0 and not d[46, 4:41].any() and d[44, 10] > 0
    far = C.reference('depth_range', 'tilted')['depth'][1]
    assert far[4, 4] == 32768 and far[4, 4:31].all() and not far[4, 31:].any() and 60000 < far.max() <= 65535
    assert d[2, 2] == 0 and d[2, 5] == 1 and d[5, 2] == 1 and d.max() <= 65535 and d[d > 0].min() == 1
    assert C.reference('depth_range', 'tilted')['box'][2] == S


# ---- near_and_guard --------------------------------------------------------------------------------------------------------
def test_near_plane_and_guard_band():
    a, b = C.reference('near_and_guard', 'near_equal'), C.reference('near_and_guard', 'near_above')
    assert a['dropped'][0] == 0 and b['dropped'][0] == 2
    assert (a['tri'] == 0).any() and (a['tri'] == 1).any() and set(np.unique(b['tri'])) == {-1, 2}
    assert C.scene('near_and_guard', 'near_above')[5] == np.nextafter(C.NEAR_Z, 1.0) > C.NEAR_Z
    on, past = C.reference('near_and_guard', 'guard_on'), C.reference('near_and_guard', 'guard_past')
    assert on['depth'].shape == (2, 64, 64) and np.all(on['depth'][0] == int(C.GUARD_FACTOR)) and on['box'][0] == 4096
    assert list(on['dropped']) == [0, 0] and list(past['dropped']) == [1, 0]
    assert not past['depth'][0].any() and past['depth'][1].any() and on['depth'][1].any()
    s = C.setups('near_and_guard', 'guard_on')[0]
    assert sorted(s['xs']) == [-(1 << 24), 0, 1 << 24] and sorted(s['ys']) == [-(1 << 24), -(1 << 24), 1 << 24]
    big = max(int(np.abs(w).max()) for w in C.edge_values(s))
    print("guard band: the largest edge value is 2^%.2f" % np.log2(big))
    assert (1 << 49) <= big < (1 << 52)
    meshes, _, intr, _, _, z_near = C.scene('near_and_guard', 'guard_past')
    assert R.project(meshes[0][0], C.EYE, intr[0], z_near)[3].tolist() == [True, False, True]


def test_unusable_vertices_drop_their_triangles_only():
    ref = C.reference('near_and_guard', 'bad_vertices')
    assert list(ref['dropped']) == [9, 0, 1, 0, 1, 1, 0] and not ref['degenerate'].any()
    assert sorted(set(np.unique(ref['tri'])) - {-1}) == [3, 4, 8, 9, 13, 14, 16, 19]
    assert set(np.unique(ref['label'])) == {0, 1, 2, 4, 7}


# ---- launch_bounds ---------------------------------------------------------------------------------------------------------
def test_launch_bounds_sums_and_images():
    for case, want in zip(C.SUMS, (255, 256, 257, 513)):
        meshes, frames = C.scene('launch_bounds', case)[:2]
        vb, tb = R.instance_bases(meshes, frames)[4:]
        assert vb[-1] == want and tb[-1] == want, case
        ref = C.reference('launch_bounds', case)
        assert len(set(np.unique(ref['label'])) - {0}) >= 2 and ref['tri'].max() >= want - 60
    assert C.reference('launch_bounds', 'sums_257')['degenerate'][0] == 1
    for case, want in zip(C.IMAGES, (1, 97, 97, 255, 256, 257)):
        _, frames, _, H, W, _ = C.scene('launch_bounds', case)
        assert len(frames) * H * W == want, case
        assert (C.reference('launch_bounds', case)['depth'] != 0).all(), case
    assert [C.IMAGES[k][1:] for k in ('image_1x1', 'image_1x97', 'image_97x1')] == [(1, 1), (1, 97), (97, 1)]


def test_launch_bounds_many_small_frames():
    meshes, frames, intr, H, W, _ = C.scene('launch_bounds', 'many_frames')
    assert (len(frames), H, W) == (300, 5, 7) and [f for f in range(300) if not frames[f]] == [0, 1, 150, 299]
    assert len(set(map(tuple, intr.tolist()))) == 300
    offs, mesh, lab, poses, vb, tb = R.instance_bases(meshes, frames)
    count = np.diff(tb)
    assert set(count.tolist()) == {0, 1, 2} and count[0] == 0 and count[-1] == 0
    assert np.any((count[:-1] == 0) & (count[1:] == 0))
    assert np.any((np.diff(vb) == 0)) and np.any((np.diff(vb) == 2) & (count == 0))
    owner = np.searchsorted(tb, np.arange(64), side='right') - 1           # the instances of the first wave's ranks
    assert len(set(np.searchsorted(offs, owner, side='right').tolist())) >= 40
    ref = C.reference('launch_bounds', 'many_frames')
    shown = [f for f in range(300) if ref['depth'][f].any()]
    assert len(shown) == int((count > 0).sum()) and not ref['depth'][[0, 1, 150, 299]].any()
    assert all(set(np.unique(ref['label'][f])) - {0} == {1 + f % 255} for f in shown)


def test_labels_keep_their_low_eight_bits():
    assert C.LABELS == (1, 255, 256, 263, 0)
    ref = C.reference('launch_bounds', 'labels')
    for i, want in enumerate((1, 255, 0, 7, 0)):
        patch = (slice(0, 1), slice(0, 9), slice(8 * i, 8 * i + 8))
        hit = ref['tri'][patch] == i
        assert hit.sum() == 28 and np.all(ref['depth'][patch][hit] == 1000) and np.all(ref['label'][patch][hit] == want), i


# ---- contention ------------------------------------------------------------------------------------------------------------
def test_contention_winners():
    ref = C.reference('contention', 'decreasing')
    hit = ref['tri'][0] >= 0
    assert hit[2:9, 2:9].all() and np.all(ref['tri'][0][hit] == 2900) and np.all(ref['depth'][0][hit] == 6400 - 2900)
    assert np.all(ref['label'][0][hit] == 1 + 2900 % 250) and (ref['box'] == 10 * 10).all() and len(ref['box']) == C.RACERS
    same = C.reference('contention', 'same_depth')
    assert np.array_equal(same['tri'][0] >= 0, hit) and np.all(same['tri'][0][hit] == 0) and len(same['box']) == C.RACERS
    mixed = C.reference('contention', 'lane_and_wave')
    assert set(mixed['box'].tolist()) == {S, 10 * 10} and set(np.unique(mixed['tri'])) == {-1, 2900, 2901}
    assert np.all(mixed['depth'][0][hit] == 3500)


# ---- the restatement's neighbours ------------------------------------------------------------------------------------------------
FAILS = {'exclusive_edges': [('on_edge', 'slopes'), ('on_edge', 'shared'), ('box_threshold', 'wave_1x65'), ('launch_bounds', 'image_1x1')],
         'half_even_vertex': [('on_edge', 'half_vertex')],
         'half_even_depth': [('on_edge', 'half_depth')],
         'du_gt_1': [('depth_range', 'du_1'), ('depth_range', 'tilted')],
         'du_lt_65535': [('depth_range', 'du_65535'), ('depth_range', 'du_65535_high')],
         'z_gt_near': [('near_and_guard', 'near_equal')],
         'guard_lt': [('near_and_guard', 'guard_on')],
         'owner_lt': [('launch_bounds', 'labels'), ('launch_bounds', 'many_frames'), ('contention', 'decreasing')]}


def test_every_variant_is_listed():
    assert set(FAILS) == set(R.VARIANTS)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_variant_of_the_restatement_fails_its_family(variant):
    for family, case in FAILS[variant]:
        want, got = C.reference(family, case), C.reference(family, case, variant)
        differ = {k: int((want[k] != got[k]).sum()) for k in KEYS}
        print("%s on %s/%s: %s" % (variant, family, case, differ))
        assert sum(differ.values()) > 0, (variant, family, case)


def test_no_variant_is_the_restatement():
    """The switches change nothing unless named."""
    meshes, frames, intr, H, W, z_near = C.scene('on_edge', 'shared')
    a, b = R.render(meshes, frames, intr, H, W, z_near), R.render(meshes, frames, intr, H, W, z_near, variant=())
    assert all(np.array_equal(a[k], b[k]) for k in KEYS + ('box',))
