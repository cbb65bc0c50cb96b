"""CPU: anchors of tests/depth_components_reference.py, the NumPy restatement of DESIGN.md "Depth components" that
tests/test_37_depth_components_gpu.py compares the kernels with: the rendered table scene and the facts measured on it,
the components against scipy.ndimage.label, and the input builders' own claims."""
import numpy as np
import pytest

import depth_components_reference as D


def test_the_table_scene_gives_the_pinned_facts():
    depth, label, intr = D.scene()
    assert depth.shape == (1, 60, 80) and sorted(np.unique(label).tolist()) == [0, 1, 2, 3, 4]
    r = D.scene_result(min_pixels=16)
    print("plane_hyp %d count %d tested %d fg %d" % (r['plane_hyp'], r['count'][max(r['plane_hyp'], 0)], r['tested'],
                                                    int(r['fg'].sum())))
    assert r['plane_hyp'] == 0 and int(r['count'][0]) == 954 and r['tested'] == 1040
    # the rendered table is an exact plane: many hypotheses tie at the largest count, and the lowest of them wins
    assert int(r['count'].max()) == 954 and int((r['count'] == 954).sum()) > 10
    objects = (label[0] >= 2) & (depth[0] != 0)
    assert int(objects.sum()) == 337 and np.array_equal(r['fg'] != 0, objects)       # every object pixel, no plane pixel
    assert list(zip(r['comp_root'][:3].tolist(), r['comp_size'][:3].tolist())) == [(1616, 192), (1731, 72), (2696, 56)]
    assert r['n_components'] == 3 and r['n_candidates'] == 3 and r['n_all'] == 13
    assert np.all(r['comp_root'][3:] == -1) and np.all(r['comp_size'][3:] == -1) and np.all(r['comp_box'][3:] == -1)
    ious = []
    for k, value in enumerate((2, 3, 4)):
        got, iou = D.match(r['label'], label[0], depth[0], value)
        assert got == k + 1
        ious.append(iou)
    print("iou", ious)
    assert [round(x, 3) for x in ious] == [0.950, 0.935, 0.966]
    assert min(ious) >= 0.9           # a condition on the scene: the method isolates the objects
    assert D.match(r['label'], label[0], depth[0], 5) == (0, 0.0)
    # the plane is the table: un-normalised, the camera on its non-negative side, the table's pixels within tol
    n, d = r['plane'][:3], r['plane'][3]
    assert d >= 0
    pts = D.backproject(depth[0], intr[0])
    dist = np.abs(D.signed(pts, n, d)) / np.sqrt(n @ n)
    assert np.median(dist[label[0] == 1]) < 0.005


def test_plane_sign_and_void_rules():
    depth, _, intr = D.scene()
    pts = D.backproject(depth[0], intr[0])
    n, d, q, void, pix = D.hypotheses(depth[0], pts, 1, 0, 64)
    assert void.any() and (~void).any()                     # the scene has pixels without depth: some hypotheses are void
    assert np.all(d[~void] >= 0) and np.all(q[~void] > 0) and np.all(n[void] == 0) and np.all(q[void] == 0)
    for h in np.nonzero(void)[0]:
        e = pts.reshape(-1, 3)[pix[h]]
        assert np.any(depth[0].reshape(-1)[pix[h]] == 0) or np.all(np.cross(e[1] - e[0], e[2] - e[0]) == 0)
    # another frame index draws other pixels
    assert not np.array_equal(pix, D.hypotheses(depth[0], pts, 1, 1, 64)[4])


@pytest.mark.parametrize("shape", [(37, 70), (48, 64), (1, 70), (37, 1), (1, 1)])
def test_components_equal_scipy_on_fully_joined_masks(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    masks = [rng.random((H, W)) < p for p in (0.3, 0.6, 0.9)] + [D.checkerboard(H, W), D.serpentine(H, W)[0], D.u_shape(H, W),
                                                                  D.combs(H, W)[0], np.zeros((H, W), bool), np.ones((H, W), bool)]
    depth = rng.integers(1, 65536, (H, W)).astype(np.uint16)
    for m in masks:
        root = D.components(depth, m.astype(np.uint8), 65535)
        lab, n = ndimage.label(m)                           # 4-connectivity is scipy's default structure
        assert np.array_equal(root >= 0, m)
        assert len(np.unique(root[m])) == n
        for k in range(1, n + 1):
            sel = lab == k
            assert np.all(root[sel] == np.flatnonzero(sel)[0])      # one root per component: its smallest pixel index


def test_jump_rule_is_inclusive():
    depth = np.array([[1000, 1020, 1041, 1041]], np.uint16)
    root = D.components(depth, np.ones((1, 4), np.uint8), 20)
    assert root.tolist() == [[0, 0, 2, 2]]
    assert D.jump_units(0.02, 1000.0) == 20 and D.jump_units(0.02, 10000.0) == 200 and D.jump_units(0.00149, 1000.0) == 1


def test_table_order_and_cap():
    root = np.full((4, 8), -1, np.int32)
    root[0, 0:3] = 0            # size 3
    root[1, 0:3] = 8            # size 3: the tie goes to the lower root
    root[2, 0:5] = 16           # size 5
    root[3, 0:2] = 24           # size 2
    t = D.table(root, min_pixels=3, max_components=2)
    assert t['n_candidates'] == 3 and t['n_components'] == 2
    assert t['comp_root'].tolist() == [16, 0] and t['comp_size'].tolist() == [5, 3]
    assert t['comp_box'].tolist() == [[0, 2, 4, 2], [0, 0, 2, 0]]
    assert t['label'][2, 0] == 1 and t['label'][0, 0] == 2 and t['label'][1, 0] == 0 and t['label'][3, 0] == 0


def test_builders_keep_their_claims():
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in ((37, 70), (48, 64), (480, 640)):
        m, length = D.serpentine(H, W)
        assert ndimage.label(m)[1] == 1 and m[0, 0] and length == int(m.sum())
        assert ndimage.label(D.u_shape(H, W))[1] == 1 and ndimage.label(D.u_shape(H, W)[:-1])[1] == 2
        both, first = D.combs(H, W)
        assert ndimage.label(both)[1] == 2 and ndimage.label(first)[1] == 1
