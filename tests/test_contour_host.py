"""CPU: the NumPy restatement of DESIGN.md "Contours" (tests/contour_reference.py) anchored on cases worked by hand, and the
conditions of the test scene that the GPU tests (tests/test_43_contour_gpu.py) rest on: what the contour term must reach on
the 384 x 512 table scene is asserted HERE, for the restatement alone, and the GPU side is then held to the restatement.

The bounds of the scene's conditions leave two to three times the room of what the restatement gives at the defaults (radius
16, step 2 cm, weight 1/16, 4 iterations; max |T - T_true| over the 4 x 4 entries, frames 0 to 5):
  prism slow constant  2.0e-5 9.2e-4 9.2e-4 1.0e-3 3.6e-4 2.3e-4   (without the term 0 5.9e-3 1.0e-2 1.3e-2 1.6e-2 1.7e-2)
  plate slow constant  6.3e-5 2.0e-3 2.2e-3 8.9e-4 4.3e-3 2.9e-3, status 0   (without: status 2, 3.5e-2 .. 1.7e-1)
  cube slow constant   5.8e-5 3.9e-5 8.1e-5 8.0e-5 7.0e-5 5.0e-5
  cube fast constant   5.8e-5 4.3e-5 3.5e-5 7.1e-5 1.4e-4 1.8e-4, nothing lost   (without: lost from frame 2)"""
import inspect

import numpy as np
import pytest

import contour_reference as CR
import track_reference as TR


# ---- edge masks -------------------------------------------------------------------------------------------------------------
def test_edge_masks_by_hand():
    z = np.array([[0, 0, 0, 0, 0],
                  [0, 500, 500, 700, 0],
                  [0, 500, 500, 701, 0],
                  [500, 500, 500, 500, 500]], np.uint16)
    m = CR.edge_masks(z, 200)
    assert m[0].tolist() == [0] * 5                         # z = 0: no mask
    assert m[1, 1] == (1 | 4) and m[1, 2] == 4              # 700 - 500 = step: no edge towards it
    assert m[2, 2] == 2 and m[2, 1] == 1                    # 701 - 500 > step: the nearer side is the edge ...
    assert m[2, 3] == 2 and m[1, 3] == (2 | 4)              # ... the farther side is not (500 - 701 < 0)
    assert m[3].tolist() == [4, 0, 0, 4, 4]                 # the frame's border sets no bit; an empty or far pixel above does


# ---- the nearest map --------------------------------------------------------------------------------------------------------
def _nearest_both(frame, origin, wh, ww, radius, step=200):
    mask = CR.edge_masks(frame, step)
    got = CR.nearest(mask, origin, wh, ww, radius)
    assert np.array_equal(got, CR.brute_nearest(mask, origin, wh, ww, radius))
    assert np.array_equal(got, CR.edge_nearest(frame[None], [0], [origin], wh, ww, [step], radius)[0])
    return got


def _decode(code, radius):
    return (int(code) & 255) - radius, ((int(code) >> 8) & 255) - radius, int(code) >> 16


def test_nearest_ties_go_to_the_smaller_j_then_the_smaller_i():
    R = 5
    got = _nearest_both(CR.dots(15, 15, [(4, 7), (10, 7)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (-3, 0, 15)            # left / right
    got = _nearest_both(CR.dots(15, 15, [(7, 4), (7, 10)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (0, -3, 15)            # up / down
    got = _nearest_both(CR.dots(15, 15, [(4, 7), (10, 7), (7, 4), (7, 10)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (0, -3, 15)            # four ways: (9, -3, 0) is the smallest key
    got = _nearest_both(CR.dots(15, 15, [(5, 5), (9, 5), (5, 9), (9, 9)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (-2, -2, 15)           # the diagonal four: the smaller j, then the smaller i


def test_nearest_at_exactly_the_radius_and_outside_the_disc():
    R = 5
    got = _nearest_both(CR.dots(15, 15, [(12, 7)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (5, 0, 15) and got[7, 6] == -1
    got = _nearest_both(CR.dots(15, 15, [(10, 11)]), (0, 0), 15, 15, R)
    assert _decode(got[7, 7], R) == (3, 4, 15)             # 9 + 16 = 25
    got = _nearest_both(CR.dots(15, 15, [(11, 11)]), (0, 0), 15, 15, R)
    assert got[7, 7] == -1                                  # (4, 4): inside the square, outside the disc
    assert _decode(got[8, 8], R) == (3, 3, 15)


def test_nearest_of_a_window_overhanging_the_frame_and_a_negative_origin():
    rng = np.random.RandomState(3)
    frame = np.where(rng.rand(12, 14) < 0.12, 8000, 0).astype(np.uint16)
    frame[0, 0] = frame[11, 13] = frame[0, 13] = 8000      # edge pixels in the frame's corners
    for origin, wh, ww, R in (((-4, -3), 10, 9, 3), ((8, 6), 11, 12, 4), ((-6, -6), 24, 26, 5), ((20, 3), 4, 4, 3),
                              ((13, 11), 1, 1, 1)):
        got = _nearest_both(frame, origin, wh, ww, R)
        y, x = np.mgrid[0:wh, 0:ww]
        ok = got >= 0
        i, j = (got & 255) - R, ((got >> 8) & 255) - R
        u, v = origin[0] + x + i, origin[1] + y + j
        assert np.all((u[ok] >= 0) & (u[ok] < 14) & (v[ok] >= 0) & (v[ok] < 12))       # an edge lies inside the frame
    assert np.all(CR.edge_nearest(frame[None], [-1, 1], [(0, 0), (0, 0)], 5, 6, [200, 200], 4) == -1)


def test_nearest_on_a_step_between_two_depths():
    """An edge of a depth step, not of empty pixels: the nearer side alone is the edge."""
    frame = np.full((9, 12), 9000, np.uint16)
    frame[2:7, 3:8] = 8000
    got = _nearest_both(frame, (0, 0), 9, 12, 4, step=200)
    assert _decode(got[4, 10], 4) == (-3, 0, 2)            # from the far side: the square's right column, facing +x
    assert _decode(got[4, 5], 4) == (0, -2, 4)             # from the square's middle, two pixels from all four sides: the top
    assert np.all(_nearest_both(frame, (0, 0), 9, 12, 4, step=1000) == -1)


# ---- the sums' hand anchor --------------------------------------------------------------------------------------------------
def test_each_vertical_side_pairs_with_its_own_side_and_the_sums_are_the_closed_forms():
    k, d0, R = 2, 8000, 5
    top, bottom, left, right = 3, 20, 8, 15
    c = CR.rectangle_pair(k=k, d0=d0, top=top, bottom=bottom, left=left, right=right)
    near = CR.edge_nearest(c['depth_test'], c['frame_of'], c['origin'], 24, 32, c['step'], R)
    pr = CR.pairs(c['depth_test'][0], c['origin'][0], c['depth_hyp'][0], c['gate'][0], c['step'][0], R, near[0])
    # the interior of the vertical sides: more than k rows from the observed top and bottom rows, which lie over the
    # hypothesis' right side and are nearer than its own side within k rows
    ys = np.arange(top + k + 1, bottom - k)
    for x, bit in ((left, 1), (right, 2)):
        assert np.all(pr['mask_hyp'][ys, x] == bit) and np.all(pr['pair'][ys, x])
        assert np.all(pr['i'][ys, x] == k) and np.all(pr['j'][ys, x] == 0)
        assert np.all(near[0][ys, x] >> 16 == bit)
    assert not pr['pair'][ys, left + 1:right].any() and np.all(pr['mask_hyp'][ys, left + 1:right] == 0)     # no edge inside
    sides = np.zeros_like(pr['pair'])
    sides[ys[0]:ys[-1] + 1, [left, right]] = True
    r, J = CR.rows_of(dict(pr, pair=pr['pair'] & sides), c['depth_hyp'][0], c['intr_win'][0])
    sums, abs_sums = CR.sums_of(r, J)
    assert len(r) == 4 * len(ys) and np.all(r[1::2] == 0.0)                      # the v rows: j = 0
    fx, fy, cx, cy, factor = (float(v) for v in c['intr_win'][0])
    dm = d0 / factor
    ru = -k * dm / fx
    px = np.repeat([(left - cx) * dm / fx, (right - cx) * dm / fx], len(ys))
    py = np.tile((ys - cy) * dm / fy, 2)
    gz = -px / dm
    want_b = ru * np.array([(py * gz).sum(), (dm - px * gz).sum(), (-py).sum(), 2.0 * len(ys), 0.0, gz.sum()])
    assert np.isclose(sums[0], 2 * len(ys) * ru * ru, rtol=1e-12, atol=0.0)
    assert np.allclose(sums[22:], want_b, rtol=1e-12, atol=1e-18)
    assert np.all(abs_sums >= np.abs(sums))
    # the whole window: the u rows of all pairs carry residuals 0 or -k pixels, and every pair gives two rows
    full = CR.contour_sums(near=near, radius=R, **c)
    assert full['n_rows'][0] == 2 * int(pr['pair'].sum()) >= 4 * len(ys)


def test_a_side_facing_the_wrong_way_pairs_with_nothing():
    R = 5
    c = CR.rectangle_pair(k=9, left=8, right=15)           # observed columns 17..24: its left side meets the hypothesis' right
    near = CR.edge_nearest(c['depth_test'], c['frame_of'], c['origin'], 24, 32, c['step'], R)
    pr = CR.pairs(c['depth_test'][0], c['origin'][0], c['depth_hyp'][0], c['gate'][0], c['step'][0], R, near[0])
    ys = np.arange(4, 20)
    assert np.all(near[0][ys, 15] >= 0) and np.all(pr['i'][ys, 15] == 2)        # an edge is found two pixels to the right ...
    assert np.all(near[0][ys, 15] >> 16 == 1) and np.all(pr['mask_hyp'][ys, 15] == 2)       # ... facing -x against +x
    assert np.all(near[0][ys, 8] == -1)                     # the left side is 9 pixels from any edge
    assert not pr['pair'].any()
    full = CR.contour_sums(near=near, radius=R, **c)
    assert full['n_rows'][0] == 0 and np.all(full['sums'] == 0.0)


def test_the_gate_is_on_the_depth_at_the_edge():
    R = 5
    c = CR.rectangle_pair(k=2, left=8, right=15)
    c['depth_test'] = (c['depth_test'].astype(np.int64) + np.where(c['depth_test'] != 0, 11, 0)).astype(np.uint16)
    near = CR.edge_nearest(c['depth_test'], c['frame_of'], c['origin'], 24, 32, c['step'], R)
    assert CR.contour_sums(near=near, radius=R, **c)['n_rows'][0] == 0           # |d - t_c| = gate + 1
    c['gate'] = np.array([11], np.int32)
    assert CR.contour_sums(near=near, radius=R, **c)['n_rows'][0] > 0


# ---- the combined solve -----------------------------------------------------------------------------------------------------
def test_combined_statuses_and_weight_zero():
    p = TR.plane_patch()
    args = {k: p[k] for k in p if k not in ('xs', 'ys')}
    plane = TR.step(**args)
    assert plane['status'][0] == 2
    zero, some = np.zeros((1, 28)), np.full((1, 28), 0.25)
    s = CR.solve_sums(plane['sums'], plane['n_pairs'], [4], some, [100], 1.0, p['pose_in'])
    assert s['status'][0] == 4 and s['pose_out'].tobytes() == np.asarray(p['pose_in'], np.float64).tobytes()
    s = CR.solve_sums(plane['sums'], [3], [0], some, [2], 1.0, p['pose_in'])
    assert s['status'][0] == 1                              # 3 + 2 < 6
    s = CR.solve_sums(plane['sums'], [3], [0], zero, [4], 0.0, p['pose_in'])
    assert s['status'][0] == 2 and np.all(s['x'] == 0.0)    # 3 + 4 >= 6: solved, and the plane patch has rank three
    assert s['pose_out'].tobytes() == np.asarray(p['pose_in'], np.float64).tobytes()
    name, c = TR.step_cases(TR.reference_renderer)[3]
    plane = TR.step(**c)
    s = CR.solve_sums(plane['sums'], plane['n_pairs'], plane['status'], some, [10], 0.0, c['pose_in'])
    assert plane['status'][0] == 0 and s['pose_out'].tobytes() == plane['pose_out'].tobytes(), name


# ---- the scene's conditions -------------------------------------------------------------------------------------------------
def _show(name, r, err):
    print(name, ' '.join('%.1e' % e for e in err), 'lost', r['lost'].ravel().astype(int))


def test_prism_condition():
    r, _, err = CR.sequence(CR.PRISM, TR.SLOW, 'constant')
    _show('prism slow constant', r, err)
    assert max(err) <= 3e-3 and not r['lost'].any()


def test_plate_condition():
    r, _, err = CR.sequence(CR.PLATE, TR.SLOW, 'constant')
    _show('plate slow constant', r, err)
    assert np.all(r['status_steps'] == 0) and max(err) <= 1e-2 and not r['lost'].any()


def test_cube_conditions():
    r, _, err = CR.sequence(CR.CUBE, TR.SLOW, 'constant')
    _show('cube slow constant', r, err)
    assert max(err) <= 1e-3 and not r['lost'].any()
    r, _, err = CR.sequence(CR.CUBE, TR.FAST, 'constant')
    _show('cube fast constant', r, err)
    assert max(err) <= 1e-3 and not r['lost'].any()


def test_the_parent_lets_the_prism_slide_and_never_moves_the_plate():
    r, _, err = CR.sequence(CR.PRISM, TR.SLOW, 'constant', contour=False)
    _show('prism slow constant, no contour', r, err)
    assert err[5] >= 1e-2 and not r['lost'].any()
    r, _, err = CR.sequence(CR.PLATE, TR.SLOW, 'constant', contour=False)
    _show('plate slow constant, no contour', r, err)
    assert np.all(r['status'] == 2) and err[1] >= 3e-2


# ---- the host side of utils/track.py ----------------------------------------------------------------------------------------
def test_the_package_has_the_bindings_and_the_restatements_defaults():
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import track
    for fn, n_args in (("cloudaae_depth_edge_nearest", 13), ("cloudaae_depth_contour_sums", 20), ("cloudaae_depth_align_solve", 12)):
        assert len(_lib._SIGNATURES[fn]) == n_args
    assert all(callable(getattr(track, f)) for f in ("edge_nearest", "contour_sums", "solve_sums"))
    assert track._contour_settings(None) is None
    assert track._contour_settings(True) == CR.DEFAULTS == dict(radius=16, step=0.02, weight=1.0 / 16.0)
    assert track._contour_settings(dict(radius=8)) == dict(CR.DEFAULTS, radius=8)
    for bad in (dict(radius=0), dict(radius=33), dict(weight=float('nan')), dict(reach=3), 7):
        with pytest.raises(Exception):
            track._contour_settings(bad)
    for fn in (track.align_poses, track.track_objects):
        assert inspect.signature(fn).parameters['contour'].default is None
