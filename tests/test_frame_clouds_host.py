"""CPU: the NumPy restatement of "Rendered training clouds" (tests/frame_clouds_reference.py) on cases worked by hand, the
properties of its strata, and the new C symbols in the header and in the Python host's table."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import frame_clouds_reference as R  # noqa: E402
from pose_sampling_reference import philox4x32  # noqa: E402

SEED, G = 77, 5
INTR = np.array([2.0, 4.0, 1.0, 1.0, 1000.0], np.float32)         # fx, fy, cx, cy, factor_depth


def _frame(pixels):
    """A 3 x 4 frame whose pixels (a list of p = 4 v + u) carry label 1 and depth 1000 + 100 p."""
    depth, label = np.zeros(12, np.uint16), np.zeros(12, np.uint8)
    for p in pixels:
        depth[p], label[p] = 1000 + 100 * p, 1
    return depth.reshape(3, 4), label.reshape(3, 4)


def _point(p):
    """The back-projection of pixel p of _frame, by hand in float32."""
    u, v = p % 4, p // 4
    dm = np.float32(1000 + 100 * p) / np.float32(1000.0)
    return np.array([(np.float32(u - 1.0) * dm) / np.float32(2.0), (np.float32(v - 1.0) * dm) / np.float32(4.0), dm],
                    np.float32)


def _q(j, stream):
    return int(philox4x32(SEED, np.array([(G << 24) + j], np.uint64), stream)[0, 0])


def test_empty_mask_gives_the_fallback():
    depth, label = _frame([])
    label[1, 1] = 1                                # a labelled pixel without depth is not in the mask
    depth[2, 2] = 700                              # nor is depth under another label
    cloud, n, distinct, src = R.frame_cloud(depth, label, INTR, 1, G, 5, SEED, fallback=[0.1, 0.2, 0.3])
    assert n == 0 and distinct == 1 and np.array_equal(src, np.zeros(5, np.int32))
    assert np.array_equal(cloud, np.tile(np.array([0.1, 0.2, 0.3], np.float32), (5, 1)))
    cloud, _, _, _ = R.frame_cloud(depth, label, INTR, 1, G, 2, SEED)
    assert np.array_equal(cloud, np.zeros((2, 3), np.float32))


def test_small_mask_is_filled_by_redraws():
    depth, label = _frame([3, 9])                  # n = 2 < rows = 5
    cloud, n, distinct, src = R.frame_cloud(depth, label, INTR, 1, G, 5, SEED)
    assert n == 2 and distinct == 2
    want_src = [0, 1] + [(_q(j, 24) * 2) >> 32 for j in (2, 3, 4)]     # floor(q 2 / 2^32): the top bit of q
    assert want_src[2:] == [_q(j, 24) >> 31 for j in (2, 3, 4)]
    assert src.tolist() == want_src
    pts = [_point(3), _point(9)]
    assert np.array_equal(cloud, np.stack([pts[s] for s in want_src]))
    # u = 3, v = 0, dm = 1.3: ((3 - 1) dm) / 2 = dm, ((0 - 1) dm) / 4
    assert np.array_equal(_point(3), np.array([np.float32(1.3), -np.float32(1.3) / np.float32(4.0), np.float32(1.3)]))


def test_mask_of_exactly_rows_keeps_every_pixel_in_order():
    pixels = [0, 2, 5, 6, 11]
    depth, label = _frame(pixels)
    cloud, n, distinct, src = R.frame_cloud(depth, label, INTR, 1, G, 5, SEED)
    assert n == 5 and distinct == 5 and src.tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(cloud, np.stack([_point(p) for p in pixels]))                 # strata of one pixel: no choice


def test_large_mask_is_one_pixel_per_stratum():
    pixels = [1, 2, 4, 6, 7, 9, 10]                # n = 7 > rows = 3: s = 0, 2, 4, 7
    depth, label = _frame(pixels)
    assert R.strata(7, 3).tolist() == [0, 2, 4, 7]
    cloud, n, distinct, src = R.frame_cloud(depth, label, INTR, 1, G, 3, SEED)
    assert n == 7 and distinct == 3 and src.tolist() == [0, 1, 2]
    ranks = [0 + ((_q(0, 23) * 2) >> 32), 2 + ((_q(1, 23) * 2) >> 32), 4 + ((_q(2, 23) * 3) >> 32)]
    assert np.array_equal(cloud, np.stack([_point(pixels[r]) for r in ranks]))
    # another label of the same frame selects other pixels
    label[0, 1] = 2
    cloud2, n2, _, _ = R.frame_cloud(depth, label, INTR, 2, G, 3, SEED)
    assert n2 == 1 and np.array_equal(cloud2, np.tile(_point(1), (3, 1)))


def test_strata_are_disjoint_cover_the_mask_and_match_the_hint():
    for n in range(1, 65):
        for rows in range(1, n + 1):
            s = R.strata(n, rows)
            assert s[0] == 0 and s[-1] == n and np.all(np.diff(s) >= 1), (n, rows)     # non-empty, disjoint, covering
            r = np.arange(n)
            owner = np.searchsorted(s, r, side='right') - 1
            assert np.array_equal(R.stratum_of(r, n, rows), owner), (n, rows)
            ranks, distinct, src = R.select(n, rows, SEED, n * 100 + rows)
            assert distinct == rows and np.all(ranks >= s[:-1]) and np.all(ranks < s[1:]), (n, rows)
            assert np.all(np.diff(ranks) > 0)      # order-keeping, without replacement


def test_row_src_points_into_the_distinct_rows():
    for n in range(1, 40):
        for rows in (1, 2, 5, 39, 64):
            ranks, distinct, src = R.select(n, rows, SEED + n, rows)
            assert distinct == min(n, rows)
            assert src.min() >= 0 and src.max() < distinct, (n, rows)
            assert np.array_equal(src[:distinct], np.arange(distinct))
            assert ranks.min() >= 0 and ranks.max() < n


def test_out_of_range_descriptions_are_the_empty_case():
    depth, label = _frame([0, 1, 2])
    out = R.frame_clouds(depth[None], label[None], INTR[None], [0, 1, -1, 0], [1, 1, 1, 1], [G, G, G, 1 << 39], 2, SEED,
                         fallback=np.arange(12, dtype=np.float32).reshape(4, 3))
    assert out['num_pixels'].tolist() == [3, 0, 0, 0] and out['num_distinct'].tolist() == [2, 1, 1, 1]
    for c in (1, 2, 3):
        assert np.array_equal(out['cloud'][c], np.tile(np.arange(3 * c, 3 * c + 3, dtype=np.float32), (2, 1)))


def test_scene_restatement_by_hand():
    rot = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0])])
    t = np.array([[0.1, 0.2, 0.7], [0.0, 0.0, 0.8]], np.float32)
    s = R.rendered_scene([2, 7], [5, 4, 3], rot, t, seed=3, first_index=10, max_v=6, max_t=8, classes=[0, 1, 2])
    assert s['inst_offsets'].tolist() == [0, 1, 3, 4, 6]
    assert s['inst_label'].tolist() == [1, 1, 2, 1, 1, 2]
    assert s['inst_mesh'][[0, 1]].tolist() == [3, 3] and s['inst_mesh'][[3, 4]].tolist() == [-1, -1]   # class 7: no mesh
    assert s['vert_base'].tolist() == [0, 6, 12, 18, 24, 30, 36] and s['tri_base'].tolist() == [0, 8, 16, 24, 32, 40, 48]
    pose = s['inst_pose'].reshape(6, 4, 4)
    assert np.array_equal(pose[0], pose[1]) and np.array_equal(pose[0, :3, 3], t[0].astype(np.float64))
    assert np.array_equal(pose[2, :3, :3], rot[0]) and np.array_equal(pose[5, :3, :3], rot[1])
    assert np.array_equal(pose[5, :3, 3], s['occluder_centre'][1].astype(np.float64))
    assert np.array_equal(pose[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (6, 1)))
    assert all(int(s['inst_mesh'][3 * i + 2]) == [5, 4, 3][int(s['occluder_class'][i])] for i in range(2))


def test_new_symbols_are_declared_and_in_the_signature_table():
    header = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    from cloudaae_amd import _lib
    for name, nargs in (("cloudaae_frame_clouds", 20), ("cloudaae_rendered_scene", 24)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib._SIGNATURES[name]) == nargs
    assert re.search(r"long long\s+cloudaae_frame_clouds_workspace_bytes\s*\(", header)
    assert int(re.search(r"#define\s+CLOUDAAE_ABI_VERSION\s+(\d+)", header).group(1)) == 602 == _lib.ABI_VERSION
    for word in ("cloudaae_frame_clouds", "cloudaae_rendered_scene"):
        assert word in header.split("#define CLOUDAAE_ABI_VERSION")[0], "the list of additions under 602 names %s" % word
