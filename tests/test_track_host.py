"""CPU: the NumPy restatement of DESIGN.md "Tracking" (tests/track_reference.py) anchored on cases worked by hand, and the
conditions of the test scene that the GPU tests (tests/test_42_track_gpu.py) rest on: what the method must reach on the 384 x
512 scene of a table and a 7 cm cube is asserted HERE, for the restatement alone, and the GPU side is then held to the
restatement.

The bounds of the scene's conditions are conditions with about ten times the room a float64 prototype showed, not
measurements.  The motions are this file's: the slow one is 1.1 cm and 2 degrees per frame towards the table's middle; the
fast one is 2.2 cm and 5 degrees per frame across the table and starts from rest (its first interval is half a step), because
a constant-velocity start has no velocity in its first tracked frame and is there the constant start -- with a full first
step both starts lose the cube at once, which says nothing about either.  Figures of the restatement as written (max |T -
T_true| over the 4 x 4 entries): static refinement 2.5e-2 -> 1.1e-3, 1.8e-4, 8.1e-5, 4.6e-5; slow / constant 4.7e-5, 3.1e-5,
2.3e-5, 4.0e-5, 6.2e-5; fast / velocity 9.5e-5, 5.4e-5, 2.9e-5, 5.5e-5, 3.2e-5; fast / constant 9.5e-5, 7.1e-2 and lost from
frame 2 on; the cube's score 3340 / 3340 present, 184 / 3302 removed."""
import numpy as np
import pytest

import detect_reference as DR
import track_reference as TR


def _step1(**c):
    """One sample's step and its pairs."""
    args = {k: c[k] for k in ('depth_test', 'frame_of', 'origin', 'depth_hyp', 'intr_win', 'gate', 'jump', 'cos_min', 'pose_in')}
    pr = TR.pairs(c['depth_test'][int(c['frame_of'][0])], c['origin'][0], c['depth_hyp'][0], c['intr_win'][0], c['gate'][0],
                  c['jump'][0], c['cos_min'])
    return TR.step(**args), pr


# ---- hand anchors -----------------------------------------------------------------------------------------------------------
def test_plane_patch_sums_are_the_closed_forms_and_the_pose_stays():
    k, d0 = 50, 8000
    c = TR.plane_patch(k=k, d0=d0)
    r, pr = _step1(**c)
    xs, ys = c['xs'], c['ys']
    square = np.zeros((12, 16), bool)
    square[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = True
    assert np.array_equal(pr['pair'], square) and r['n_pairs'][0] == 64
    n = pr['n'][square]
    assert np.all(n[:, :2] == 0.0) and np.all(np.abs(n[:, 2]) == 1.0)
    fx, fy, cx, cy, factor = (float(v) for v in c['intr_win'][0])
    dm, res = d0 / factor, d0 / factor - (d0 - k) / factor
    assert abs(res - k / factor) < 1e-15
    px = np.array([(x - cx) * dm / fx for x in xs])
    py = np.array([(y - cy) * dm / fy for y in ys])
    N = len(xs)
    want = np.zeros(28)
    want[0] = N * N * res * res
    want[1], want[2], want[6] = N * (py * py).sum(), -px.sum() * py.sum(), N * py.sum()            # A00, A01, A05
    want[7], want[11], want[21] = N * (px * px).sum(), -N * px.sum(), N * N                         # A11, A15, A55
    want[22], want[23], want[27] = N * py.sum() * res, -N * px.sum() * res, N * N * res              # b0, b1, b5
    assert np.allclose(r['sums'][0], want, rtol=1e-12, atol=1e-18)
    assert np.all(r['sums'][0][[3, 4, 5, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 24, 25, 26]] == 0.0)
    assert r['status'][0] == 2                                                                     # rank 3: the third pivot is 0
    assert r['pose_out'][0].tobytes() == np.asarray(c['pose_in'][0], np.float64).tobytes()
    assert np.all(r['x'][0] == 0.0)


def test_gate_edges():
    c = TR.plane_patch(k=50)
    c['cos_min'] = 0.0
    c['depth_test'] = c['depth_test'].copy()
    c['depth_test'][0, 2 + 5, 3 + 6] -= 1                  # |d - t| = gate + 1 at window pixel (6, 5)
    c['depth_test'][0, 2 + 6, 3 + 7] += 3                  # nearer the hypothesis: still a pair
    r, pr = _step1(**c)
    assert not pr['pair'][5, 6] and pr['pair'][6, 7] and pr['pair'][5, 7] and r['n_pairs'][0] == 63
    c['gate'] = np.array([51], np.int32)
    r, pr = _step1(**c)
    assert pr['pair'][5, 6] and r['n_pairs'][0] == 64


@pytest.mark.parametrize("extra, pair", [(0, True), (1, False)])
def test_jump_edges(extra, pair):
    """A 2 x 2 hypothesis: pixel (0, 0) has its right neighbour alone along x.  At exactly `jump` that neighbour is valid; at
    jump + 1 the axis has no slope and the pixel is flat."""
    jump, d0 = 10, 8000
    hyp = np.zeros((1, 4, 4), np.uint16)
    hyp[0, 1:3, 1:3] = d0
    hyp[0, 1, 2] = d0 + jump + extra
    frame = np.full((1, 4, 4), d0, np.uint16)
    rows = np.array([[500.0, 500.0, 1.5, 1.5, 10000.0]], np.float32)
    pr = TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, jump, 0.0)
    assert bool(pr['pair'][1, 1]) == pair
    assert pr['pair'][2, 1]                                # its neighbours stay within the jump
    assert bool(pr['pair'][1, 2]) == pair and bool(pr['pair'][2, 2]) == pair       # the changed pixel is their one neighbour


def _tilted(h, w, d0, gu, gv):
    v, u = np.mgrid[0:h, 0:w]
    return (d0 + gu * u + gv * v).astype(np.uint16)


def test_cos_min_keeps_the_neighbour_above_and_drops_the_one_below():
    hyp, frame = _tilted(9, 9, 8000, 2, 1)[None], _tilted(9, 9, 8005, -6, 9)[None]
    rows = np.array([[500.0, 500.0, 4.0, 4.0, 10000.0]], np.float32)
    dot = TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, 50, 0.5)['dot'][4, 4]
    assert 0.5 < dot < 1.0
    for cos_min, kept in ((dot, True), (np.nextafter(dot, 0.0), True), (np.nextafter(dot, 1.0), False)):
        assert bool(TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, 50, cos_min)['pair'][4, 4]) == kept
    assert TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, 50, 0.0)['pair'][4, 4]
    frame[0, 4, 3] = frame[0, 4, 5] = 0                     # the observed pixel loses its slope along x
    assert not TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, 50, 0.5)['pair'][4, 4]
    assert TR.pairs(frame[0], (0, 0), hyp[0], rows[0], 100, 50, 0.0)['pair'][4, 4]       # cos_min <= 0 reads no observed neighbour


def test_a_hypothesis_pixel_on_the_windows_edge_takes_the_one_sided_slope():
    hyp = _tilted(5, 6, 8000, 3, -2)
    row = np.array([500.0, 450.0, 2.5, 1.5, 10000.0], np.float32)
    zb = np.zeros((7, 8), np.int64)
    zb[1:-1, 1:-1] = hyp
    unit, ok = TR.unit_normals(zb, row, 50)
    assert ok.all()

    def P(x, y):
        dm = float(hyp[y, x]) / 10000.0
        return np.array([((x - 2.5) * dm) / 500.0, ((y - 1.5) * dm) / 450.0, dm])
    for (x, y), gx, gy in (((0, 2), P(1, 2) - P(0, 2), P(0, 3) - P(0, 1)), ((5, 0), P(5, 0) - P(4, 0), P(5, 1) - P(5, 0)),
                           ((3, 4), P(4, 4) - P(2, 4), P(3, 4) - P(3, 3))):
        n = np.array([gx[1] * gy[2] - gx[2] * gy[1], gx[2] * gy[0] - gx[0] * gy[2], gx[0] * gy[1] - gx[1] * gy[0]])
        n = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        assert unit[y, x].tobytes() == n.tobytes(), (x, y)


def test_a_window_overhanging_the_frame_pairs_nothing_outside_it():
    frame = np.full((10, 12), 8000, np.uint16)
    hyp = np.full((8, 9), 8004, np.uint16)
    row = np.array([500.0, 500.0, 4.0, 4.0, 10000.0], np.float32)
    for (u0, v0) in ((-3, -2), (7, 5), (-3, 5), (20, 20)):
        pr = TR.pairs(frame, (u0, v0), hyp, row, 10, 10, 0.8)
        inside = np.array([[0 <= u0 + x < 12 and 0 <= v0 + y < 10 for x in range(9)] for y in range(8)])
        assert np.array_equal(pr['pair'], inside), (u0, v0)


def test_statuses():
    c = TR.plane_patch()
    assert TR.step(**{k: c[k] for k in c if k not in ('xs', 'ys')})['status'][0] == 2
    few = dict(c, depth_hyp=np.where(np.arange(16)[None, None, :] < 6, c['depth_hyp'], 0).astype(np.uint16))   # 2 x 8 pixels
    few['depth_hyp'][0, 3:] = 0                                                                                 # ... 1 row: flat
    r = TR.step(**{k: few[k] for k in few if k not in ('xs', 'ys')})
    assert r['n_pairs'][0] < 6 and r['status'][0] == 1
    for fo in (-1, 1):
        r = TR.step(**dict({k: c[k] for k in c if k not in ('xs', 'ys')}, frame_of=np.array([fo], np.int32)))
        assert r['status'][0] == 4 and r['n_pairs'][0] == 0 and np.all(r['sums'] == 0.0)
        assert r['pose_out'].tobytes() == np.asarray(c['pose_in'], np.float64).tobytes()
    assert TR.solve(np.full(28, np.inf))[0] == 2
    s = np.zeros(28)
    s[[1, 7, 12, 16, 19, 21]] = 1e-300                     # A = 1e-300 I
    s[22:] = 1e300
    assert TR.solve(s)[0] == 3


def test_pose_windows():
    meshes = DR.scene_meshes()
    aabb = TR.mesh_aabb(meshes)[[TR.CUBE, TR.CUBE, TR.CUBE]]
    T = TR.cube_pose(0)
    behind = T.copy()
    behind[2, 3] = 0.06                                    # a corner lies nearer than z_near
    beside = TR.at_pixel(T, -400.0, 100.0)                 # wholly left of the image
    origin, wh, ww, ok = TR.pose_windows([T, behind, beside], aabb, TR.SCENE_INTR[0], TR.SCENE_H, TR.SCENE_W)
    assert list(ok) == [True, False, False] and ww % 8 == 0
    depth = TR.reference_renderer([[T]])[0]
    vs, us = np.nonzero(depth)
    assert origin[0, 0] <= us.min() and us.max() < origin[0, 0] + ww and origin[0, 1] <= vs.min() and vs.max() < origin[0, 1] + wh
    assert ww <= 2 * (us.max() - us.min() + 1) + 16 and wh <= 2 * (vs.max() - vs.min() + 1) + 8


# ---- the scene's conditions -------------------------------------------------------------------------------------------------
def test_static_refinement_condition():
    depth, truth = TR.frames(TR.SLOW)
    start = TR.off_pose(truth[0], 2.0, 0.005)
    a = TR.align(depth[:1], TR.SCENE_INTR, DR.scene_meshes(), [TR.CUBE], [0], [start], iterations=4)
    err = [TR.pose_error(p[0], truth[0]) for p in a['poses']]
    print("static refinement", err, a['n_pairs'].ravel())
    assert err[4] <= 1e-3 and err[4] <= err[0] / 10.0 and np.all(a['status'] == 0)


def _errors(motion, start):
    r, truth = TR.sequence(motion, start)
    err = [TR.pose_error(r['poses'][f, 0], truth[f]) for f in range(TR.FRAMES)]
    print(motion, start, err, r['lost'].ravel())
    return r, truth, err


def test_slow_sequence_condition():
    r, truth, err = _errors(TR.SLOW, 'constant')
    assert max(err) <= 1e-3 and not r['lost'].any()
    assert all(TR.pose_error(truth[0], truth[f]) > 1e-2 for f in range(2, TR.FRAMES))      # the first pose, held


def test_fast_sequence_conditions():
    r, _, err = _errors(TR.FAST, 'velocity')
    assert max(err) <= 5e-3 and not r['lost'].any()
    _, _, err = _errors(TR.FAST, 'constant')
    assert max(err[:4]) > 1e-2


def test_score_conditions():
    depth, truth = TR.lost_sequence()
    meshes = DR.scene_meshes()
    origin, wh, ww, ok = TR.pose_windows(truth[2:3], TR.mesh_aabb(meshes)[[TR.CUBE]], TR.SCENE_INTR[0], TR.SCENE_H, TR.SCENE_W)
    for f, low, high in ((2, 0.9, 1.0), (3, 0.0, 0.2)):
        num, den, counts = TR.score(depth, np.tile(TR.SCENE_INTR, (5, 1)), meshes, [TR.CUBE], [f], truth[2:3], origin, wh, ww)
        print("score in frame", f, int(num[0]), int(den[0]), counts[0])
        assert low <= num[0] / den[0] <= high
    r = TR.track(depth, TR.SCENE_INTR, meshes, [TR.CUBE], truth[:1])
    assert list(r['lost'][:, 0]) == [False, False, False, True, False]
    assert r['poses'][3].tobytes() == r['poses'][2].tobytes()


# ---- the host side of utils/track.py ----------------------------------------------------------------------------------------
def test_the_packages_windows_and_starts_are_the_restatements():
    from cloudaae_amd.utils import track
    meshes = DR.scene_meshes()
    T = TR.cube_pose(0)
    behind = T.copy()
    behind[2, 3] = 0.06
    poses = np.array([T, behind, TR.at_pixel(T, -400.0, 100.0), TR.at_pixel(T, 3.0, 380.0), TR.cube_pose(3, TR.FAST)])
    aabb = TR.mesh_aabb(meshes)[[TR.CUBE, TR.CUBE, TR.CUBE, 0, 1]]
    for margin in (0.5, 0, 0.1):
        want = TR.pose_windows(poses, aabb, TR.SCENE_INTR[0], TR.SCENE_H, TR.SCENE_W, margin)
        got = track.pose_windows(poses, aabb, TR.SCENE_INTR[0], TR.SCENE_H, TR.SCENE_W, margin)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3] and np.array_equal(got[3], want[3])
        assert got[0].dtype == np.int32 and list(got[3]) == [True, False, False, True, True]
    a, b = TR.cube_pose(1, TR.FAST), TR.cube_pose(2, TR.FAST)
    assert track.predict(b, a, 'velocity').tobytes() == TR.predict(b, a, 'velocity').tobytes()
    # (a turn about the cube's own axis is not a constant left factor: the prediction is close, not exact)
    assert TR.pose_error(track.predict(b, a, 'velocity'), TR.cube_pose(3, TR.FAST)) < 5e-3 < 1e-2 < TR.pose_error(b, TR.cube_pose(3, TR.FAST))
    assert track.predict(b, a, 'constant').tobytes() == b.tobytes() == track.predict(b, None, 'velocity').tobytes()
    assert (track.ITERATIONS, track.GATE, track.JUMP, track.COS_MIN, track.MARGIN, track.MIN_SCORE) == (4, 0.03, 0.005, 0.8, 0.5, (1, 2))
