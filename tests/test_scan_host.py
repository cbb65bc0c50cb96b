"""CPU: the NumPy restatement of DESIGN.md "Scanning" (tests/scan_reference.py) anchored by hand, and the conditions of the
scenes asserted for the restatement alone.  tests/test_45_scan_gpu.py holds the kernel and utils/scan.py to it."""
import numpy as np
import pytest

import fuse_reference as FR
import render_reference as R
import scan_reference as S


@pytest.fixture(scope="module")
def hand():
    return {name: (c, S.run_case(c, details=True)) for name, c in S.hand_cases()}


# ---- the raycast by hand ---------------------------------------------------------------------------------------------------
def test_linear_field_in_closed_form(hand):
    """voxel 1/64, the first voxel centre at (0, 0, 1), the identity pose, fx = fy = 64, factor 8192: the central ray has
    g_z = 64 (z - 1), samples at g_z = k / 2, and the field 0.25 (5.25 - g_z) crosses zero at z* = 1 + 5.25 / 64 exactly."""
    c, (d, n) = hand["linear field"]
    g0, gd, z0, z1, live = S.ray_setup(c['origin'], c['voxel'], (4, 4, 16), np.eye(4), c['intr_win'][0], 1, 1)
    assert np.array_equal(g0, [0.0, 0.0, -64.0]) and np.array_equal(gd.ravel(), [0.0, 0.0, 64.0])
    assert live.all() and z0[0, 0] == 1.0 and z1[0, 0] == 1.0 + 15.0 / 64.0
    assert d[0, 0, 0] == int((1.0 + 5.25 / 64.0) * 8192.0) == 8864 and n[0, 0, 0] == 12       # the samples g_z = 0, 0.5, .. 5.5


def test_zero_on_a_sample_is_outside(hand):
    _, (d, n) = hand["zero on a sample"]
    assert d[0, 0, 0] == int((1.0 + 6.0 / 64.0) * 8192.0) and n[0, 0, 0] == 14               # closed by g_z = 6.5, t = 0


def test_parallel_rays_and_the_clamp(hand):
    assert hand["parallel outside"][1][0][0, 0, 0] == 0 and hand["parallel outside"][1][1][0, 0, 0] == 0
    assert hand["through the last centres"][1][0][0, 0, 0] == 8864                           # g_x = g_y = n - 1: cell n - 2, f = 1
    c = hand["through the last centres"][0]
    g0 = S.ray_setup(c['origin'], c['voxel'], (4, 4, 16), np.eye(4), c['intr_win'][0], 1, 1)[0]
    assert np.array_equal(g0[:2], [3.0, 3.0])


def test_unknown_samples(hand):
    assert hand["unknown beside the ray"][1][0][0, 0, 0] == 0 and hand["unknown beside the ray"][1][1][0, 0, 0] == 13
    assert hand["unknown then negative"][1][0][0, 0, 0] == 0                                 # a back face
    assert hand["min_count 2 takes the deep band"][1][0][0, 0, 0] == int((1.0 + 7.25 / 64.0) * 8192.0)
    assert hand["min_count 1 beside it"][1][0][0, 0, 0] == 8864


def test_quantisation_limits(hand):
    assert [int(hand["du %d" % k][1][0][0, 0, 0]) for k in (0, 1, 65535, 65536)] == [0, 1, 65535, 0]
    # 65536 is kept out by the interval's far end: the ray stops at z1 = 65535 / factor before the sample that would close it
    assert hand["du 65536"][1][1][0, 0, 0] == hand["du 65535"][1][1][0, 0, 0] == 16


def test_rays_that_see_nothing(hand):
    assert hand["surface in front of z_near"][1][0][0, 0, 0] == 0 and hand["surface in front of z_near"][1][1][0, 0, 0] == 1
    for name in ("volume behind the camera", "NaN pose"):
        assert hand[name][1][0][0, 0, 0] == 0 and hand[name][1][1][0, 0, 0] == 0, name
    assert hand["more than 4096 samples"][1][0][0, 0, 0] == 0 and hand["more than 4096 samples"][1][1][0, 0, 0] == 4096
    assert hand["fewer than 4096 samples"][1][0][0, 0, 0] == int((1.0 + 12.25 / 64.0) * 8192.0)
    assert hand["fewer than 4096 samples"][1][1][0, 0, 0] == 3138


def test_a_pose_with_any_nan_gives_an_empty_image():
    st, origin, voxel = S.big_wavy()
    poses, rows, wh, ww = S.batch_case()
    assert S.raycast(st, origin, voxel, poses[:1], rows[:1], wh, ww).any()
    for r in range(3):
        for c in range(4):
            T = poses[0].copy()
            T[r, c] = np.nan
            assert not S.raycast(st, origin, voxel, T[None], rows[:1], wh, ww).any(), (r, c)


# ---- the sphere ------------------------------------------------------------------------------------------------------------
def test_sphere_from_60_cm():
    """fuse_reference.sphere_state at 4 mm voxels: every hit pixel back-projects onto the sphere within the interpolation bound
    tests/test_fuse_host.py uses, L^2 / (8 (r - L)) + front / 8192 = 0.058 voxel (a depth unit is 0.025 voxel here)."""
    voxel, r = 0.004, 8.3
    d = np.array([0.3, -0.5, 1.0])
    T = FR.look_at(d / np.sqrt((d * d).sum()), np.full(3, 12.0 * voxel), 0.6)
    row = np.array([600.0, 600.0, 49.5, 49.5, 10000.0], np.float32)
    depth = S.raycast(FR.sphere_state(), [0.0, 0.0, 0.0], voxel, T[None], row[None], 100, 100)[0]
    p = S.backproject(depth, row, T)
    err = float((np.abs(np.sqrt(((p - 12.0 * voxel) ** 2).sum(axis=1)) - r * voxel) / voxel).max())
    bound = 3.0 / (8.0 * (r - np.sqrt(3.0))) + 4.0 / 8192.0
    print("sphere: %d pixels, worst |radius error| %.4f voxel against %.4f" % (len(p), err, bound))
    assert len(p) > 3000
    assert err <= 0.042 <= bound <= 0.1                               # measured 0.0413


# ---- consistency with the mesh ---------------------------------------------------------------------------------------------
def test_raycast_agrees_with_the_rendered_mesh():
    """The cube scene at 4 mm: the raycast of the fused state from each of the 14 views against render_reference of the
    restatement's own extracted mesh.  Marching tetrahedra and the trilinear march cut the same field differently, so a pixel
    may differ; more than one voxel along the ray is rare."""
    s = FR.scene('cube', 0.004)
    ray = S.raycast(s['state'], s['origin'], 0.004, s['poses'], s['intr'], FR.SCENE_H, FR.SCENE_W).astype(np.int64)
    ref = R.render([(s['vertices'], s['triangles'])], [[(0, 1, T)] for T in s['poses']], s['intr'], FR.SCENE_H, FR.SCENE_W)['depth']
    ref = ref.astype(np.int64)
    fx, fy, cx, cy, factor = (float(k) for k in FR.SCENE_INTR)
    y, x = np.mgrid[0:FR.SCENE_H, 0:FR.SCENE_W]
    along = np.sqrt(((x - cx) / fx) ** 2 + ((y - cy) / fy) ** 2 + 1.0)[None]
    both, either = (ray != 0) & (ref != 0), (ray != 0) | (ref != 0)
    far = both & (np.abs(ray - ref) / factor * along > 0.004)
    share = far.sum() / either.sum()
    print("raycast against the mesh: %d pixels set in either, %d in both, %d more than a voxel apart (%.5f), largest %d units"
          % (either.sum(), both.sum(), far.sum(), share, np.abs(ray - ref)[both].max()))
    assert both.sum() >= 0.99 * either.sum()
    assert share <= 1e-4 <= 2e-2                                       # measured 4 of 101 194: 4e-5; the cap is 2e-2


# ---- the orbit -------------------------------------------------------------------------------------------------------------
def test_orbit_is_tracked_within_a_voxel():
    o = S.orbit()
    r, truth = o['result'], o['truth']
    err = S.pose_errors(r['poses'], truth)
    hold = np.array([np.abs(truth[f - 1] - truth[f]).max() for f in range(1, len(truth))])
    print("orbit at 4 mm: pose error per frame %s" % np.array2string(err[1:], precision=5))
    print("holding the previous frame's true pose: %s" % np.array2string(hold, precision=4))
    print("pairs per step %d .. %d" % (min(s[1] for st in r['steps'] for s in st), max(s[1] for st in r['steps'] for s in st)))
    assert all(s[2] == 0 for st in r['steps'] for s in st) and not r['lost'].any()
    assert np.all(err[1:] < 4e-3)                                     # one voxel
    assert np.all(err[1:] < hold / 10.0)
    dist, components = S.mesh_distance(r, S.ORBIT_VOXEL)
    print("scanned mesh: largest vertex-to-surface distance %.3f voxel, %d component(s)" % (dist, components))
    assert components == 1 and dist <= 0.3 <= 1.0                     # measured 0.242


def test_a_removed_object_is_lost_and_found_again():
    o = S.orbit(8, S.ORBIT_VOXEL, S.STEP_VOXELS, (5,))
    r, truth = o['result'], o['truth']
    assert r['lost'].tolist() == [False] * 5 + [True, False, False]
    assert (r['num'][5], r['den'][5]) == (0, 1)
    assert np.array_equal(r['states'][5], r['states'][4]) and not np.array_equal(r['states'][6], r['states'][5])
    assert np.array_equal(r['poses'][5], r['poses'][4])
    assert np.array_equal(r['steps'][6][0][0], r['poses'][4])         # frame 6 starts from the last good pose
    err = S.pose_errors(r['poses'], truth)
    print("removed in frame 5: pose error per frame %s" % np.array2string(err, precision=5))
    assert err[6] < 4e-3 and err[7] < 4e-3
