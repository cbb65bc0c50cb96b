"""CPU: the NumPy restatement of DESIGN.md "Creases" (tests/creases_reference.py) on folds written from a formula, on the
table scenes with spheres apart and touching, clean and through the sensor model, on the detection scene, and on a
detection across a touch; then the coverage of the random cases the GPU test compares.  Every assertion is on the
restatement alone: this file anchors what tests/test_41_creases_gpu.py holds the kernels to."""
import numpy as np
import pytest

import creases_reference as C
import depth_components_reference as D
import detect_reference as DR


def _fold(depth, step=2, smooth=0, angle=30.0, jump_units=C.FOLD_JUMP_UNITS):
    return C.creases(depth, np.ones(depth.shape, np.uint8), C.FOLD_INTR, jump_units, step, smooth, C.cos2_of(angle))


# ---- hand-made folds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 3])
def test_a_valley_is_flagged_on_one_side_of_the_angle_only(step):
    smooth = 0
    inner = slice(step, C.FOLD_H - step)
    # Across the fold a chord sees the whole deviation d; a diagonal chord runs sqrt(2) as far for the same rise and sees
    # 2 atan(tan(d / 2) / sqrt(2)): 36.5 degrees of 50, 52.7 of 70, 80.2 of 100.
    for deviation, angle, flagged, diagonals in ((50.0, 30.0, True, True), (20.0, 30.0, False, False), (50.0, 60.0, False, False),
                                                 (70.0, 60.0, True, False), (100.0, 60.0, True, True)):
        r = _fold(C.fold_depth(deviation), step, smooth, angle)
        print("valley of %g degrees at %g: %d crease pixels" % (deviation, angle, r['n_crease']))
        assert np.all(r['tested'][inner, 8:33] == 15)
        if not flagged:
            assert r['n_crease'] == 0
            continue
        # the fold's own column, in the direction across it and, where they see enough of it, in both diagonals; never along it
        assert np.all(r['crease'][inner, 20] & 1)
        assert np.all((r['crease'][inner, 20] & 12) == (12 if diagonals else 0))
        assert not np.any(r['crease'] & 2)
        # and nowhere farther from the fold than the chord (and the box) reaches
        far = np.abs(np.arange(C.FOLD_W) - 20) >= step + 1
        assert not r['crease'][:, far].any()
        assert np.array_equal(r['fg_cut'], (r['crease'] == 0).astype(np.uint8))


def test_the_smoothing_rounds_a_fold_off():
    """With the box of 3 x 3 the fold's own pixel is the mean of itself and two lower neighbours: at step 3 the rise to either
    end of the chord shrinks by 2 / 9, and a chord across a fold of d degrees sees 2 atan(7 / 9 tan(d / 2)): 39.9 of 50, 57.2
    of 70, 85.6 of 100."""
    inner = slice(4, C.FOLD_H - 4)
    for deviation, angle, flagged in ((50.0, 30.0, True), (20.0, 30.0, False), (70.0, 60.0, False), (100.0, 60.0, True)):
        r = _fold(C.fold_depth(deviation), 3, 1, angle)
        assert np.all(r['crease'][inner, 20] & 1) if flagged else r['n_crease'] == 0
        assert not r['crease'][:, np.abs(np.arange(C.FOLD_W) - 20) >= 5].any()


@pytest.mark.parametrize("step,smooth", [(1, 0), (2, 0), (3, 1)])
def test_a_roof_and_an_oblique_plane_are_never_flagged(step, smooth):
    for depth in (C.fold_depth(50.0, valley=False), C.fold_depth(20.0, valley=False), C.fold_depth(120.0, valley=False),
                  C.oblique_plane_depth(), C.oblique_plane_depth(-0.3, 1.1)):
        for angle in (5.0, 30.0):
            r = _fold(depth, step, smooth, angle)
            assert np.all(r['tested'][step:C.FOLD_H - step, step:C.FOLD_W - step] == 15)
            if smooth and angle < 30.0:
                # a box cut off by the frame's border is the mean of one side only: on a steep plane the chord that ends
                # there sees a fold of a few degrees.  Where both ends' boxes are whole there is none.
                m = step + smooth
                assert not r['crease'][m:C.FOLD_H - m, m:C.FOLD_W - m].any()
            else:
                assert r['n_crease'] == 0 and r['fg_cut'].all()


def test_a_depth_step_larger_than_the_reach_is_never_tested():
    step, ju = 2, 50
    for units, tested in ((step * ju, True), (step * ju + 1, False)):
        r = _fold(C.depth_step(units), step, 0, 30.0, ju)
        across = r['tested'][step:-step, 20 - step:20 + step]          # the pixels whose chord crosses the step
        assert np.all((across & 13) == (13 if tested else 0)) and np.all(across & 2)
        assert np.all(r['tested'][step:-step, step:20 - step] == 15)
        # at the reach the step is a fold like any other (a corner at the foot of the nearer plane); past it, nothing
        assert not r['crease'][:, :20 - step].any() and not r['crease'][:, 20 + step:].any()
        assert (r['n_crease'] > 0) == tested
    # the box does not reach across a step larger than jump_units either: three columns of one depth, not a mix
    smap = C.smooth_map(C.depth_step(ju + 1), np.ones((C.FOLD_H, C.FOLD_W), np.uint8), ju, 1)
    assert smap[5, 19] == ((6 * 10000) << 8) | 6 and smap[5, 20] == ((6 * (10001 + ju)) << 8) | 6
    assert smap[5, 10] == ((9 * 10000) << 8) | 9 and smap[0, 0] == ((4 * 10000) << 8) | 4


def test_what_is_no_foreground_or_has_no_jump_is_left_alone():
    depth = C.fold_depth(50.0)
    fg = np.ones(depth.shape, np.uint8)
    fg[:, 18] = 0
    r = C.creases(depth, fg, C.FOLD_INTR, C.FOLD_JUMP_UNITS, 2, 0, C.cos2_of(30.0))
    assert not r['smooth_map'][:, 18].any() and not r['tested'][:, 18].any() and not r['fg_cut'][:, 18].any()
    assert not (r['tested'][:, 20] & 13).any() and (r['tested'][2:-2, 20] & 2).all()      # its chord ends on column 18
    none = C.creases(depth, fg, C.FOLD_INTR, -1, 2, 0, C.cos2_of(30.0))
    assert not none['smooth_map'].any() and not none['tested'].any() and np.array_equal(none['fg_cut'], fg)


# ---- the clean scenes ----------------------------------------------------------------------------------------------------
def test_three_spheres_apart_have_no_crease():
    depth, _, intr = D.scene()
    plain = D.scene_result()
    for cut in (C.CLEAN_CUT, C.NOISY_CUT, dict(step=1, smooth=0, angle=30.0), dict(step=3, smooth=2, angle=45.0)):
        s = C.scene_segments(depth, intr, cut, 16, 'apart')
        assert s['n_crease'] == 0 and np.array_equal(s['fg_cut'], plain['fg'])
        assert np.array_equal(s['root'], plain['root']) and np.array_equal(s['label'], plain['label'])
        assert s['comp_size'][:4].tolist() == [192, 72, 56, -1]


def test_touching_spheres_are_cut_apart():
    depth, label = C.sphere_scene(C.TOUCHING_SPHERES, D.SCENE_INTR, D.SCENE_H, D.SCENE_W)
    plain = C.scene_segments(depth, D.SCENE_INTR, None, 16, 'touch')
    assert plain['n_components'] == 2 and plain['comp_size'][:2].tolist() == [274, 66]
    assert C.shares(plain, label[0]).tolist() == [[0, 190, 84, 0], [0, 0, 0, 66]]
    cut = C.scene_segments(depth, D.SCENE_INTR, C.CLEAN_CUT, 16, 'touch')
    print("crease pixels %d, components %s" % (cut['n_crease'], cut['comp_size'][:4].tolist()))
    assert cut['n_components'] == 3 and cut['n_crease'] == 14
    assert C.shares(cut, label[0]).tolist() == [[0, 186, 0, 0], [0, 0, 74, 0], [0, 0, 0, 66]]     # one sphere each, nothing else
    assert np.array_equal(cut['fg'], plain['fg']) and int(cut['fg'].sum()) - int(cut['fg_cut'].sum()) == 14


def test_the_noisy_frame_needs_the_smoothing():
    depth, _ = C.big_scene(noise=True)
    _, clean_label = C.big_scene(noise=False)
    plain = C.scene_segments(depth, C.BIG_INTR, None, C.BIG_MIN_PIXELS, 'bignoisy')
    assert plain['n_components'] == 2
    cut = C.scene_segments(depth, C.BIG_INTR, C.NOISY_CUT, C.BIG_MIN_PIXELS, 'bignoisy')
    sh = C.shares(cut, clean_label[0])
    print("crease pixels %d, components %s, pixels on (table, sphere 1, 2, 3) %s" % (cut['n_crease'], cut['comp_size'][:4].tolist(),
                                                                                   sh.tolist()))
    assert cut['n_components'] == 3
    for k in range(3):
        assert 10 * sh[k, 1 + k] >= 9 * cut['comp_size'][k], "component %d lies on sphere %d with under 90 %% of its pixels" % (k, k)
    # the spheres apart, through the same sensor, stay three components
    apart, _ = C.big_scene(tuple(D.SCENE_SPHERES), noise=True)
    assert C.scene_segments(apart, C.BIG_INTR, C.NOISY_CUT, C.BIG_MIN_PIXELS, 'bigapartnoisy')['n_components'] == 3


def test_the_detection_scene_has_no_crease_at_the_defaults():
    s, g = DR.scene(), DR.scene_segments()
    seg = C.segment(s['depth'], s['intr'], dict(C.DEFAULTS), **DR.SCENE_SEGMENT)[0]
    assert seg['n_crease'] == 0 and np.array_equal(seg['label'][None], g['label'])
    assert np.array_equal(seg['comp_size'][None], g['comp_size']) and np.array_equal(seg['comp_box'][None], g['comp_box'])


# ---- detection across a touch ------------------------------------------------------------------------------------------------
def test_detection_across_a_touch():
    plain, cut = C.detect_score(None), C.detect_score(C.CLEAN_CUT)
    print("without: n_det %s classes %s; with: n_det %s classes %s fractions %s / %s" % (
        plain['n_det'].tolist(), plain['det_class'].tolist(), cut['n_det'].tolist(), cut['det_class'].tolist(),
        cut['det_num'].tolist(), cut['det_den'].tolist()))
    assert int(plain['n_det'][0]) <= 2 and C.detect_scene(None)['seg']['n_components'] == 2
    assert C.detect_scene(C.CLEAN_CUT)['object_of'] == [0, 1, 2]
    assert cut['n_det'].tolist() == [3] and cut['det_class'][0].tolist() == [0, 1, 2]      # each component the sphere it shows
    assert np.all(cut['det_hyp'][0] == 0)                                                   # at the true pose, not the moved one


# ---- the random cases of the GPU test ---------------------------------------------------------------------------------------
def test_the_random_cases_cover_every_direction_both_ways():
    n_fg = 0
    tested, flagged = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for case in C.CASES:
        c, r = C.case_inputs(case[0]), C.case_result(case[0])
        n_fg += int((c['fg'] != 0).sum())
        for b in range(4):
            tested[b] += int(((r['tested'] >> b) & 1).sum())
            flagged[b] += int(((r['crease'] >> b) & 1).sum())
        assert not (r['crease'] & ~r['tested']).any()
    print("foreground %d, tested %s, set %s" % (n_fg, tested.tolist(), flagged.tolist()))
    for b in range(4):
        assert 20 * tested[b] >= n_fg, "direction %d is tested on under 5 %% of the foreground" % b
        assert 20 * flagged[b] >= tested[b] and 20 * (tested[b] - flagged[b]) >= tested[b], "direction %d is one-sided" % b
    # the ends of the packing occur: a full box of 225 members of 65535; boxes of one; whole boxes that miss members
    full = C.case_result("65535")['smooth_map']
    assert (full == np.uint32(((225 * 65535) << 8) | 225)).any()
    assert set(np.unique(C.case_result("31x65")['smooth_map'] & 255).tolist()) == {0, 1}
    n = C.case_result("33x33")['smooth_map'][0, 7:26, 7:26] & 255
    assert n.max() < 225 and n.max() > n[n > 0].min() > 1
    # and the frames no wider than the step test nothing
    assert not (C.case_result("40x3_step3")['tested'] & 13).any() and not (C.case_result("8x50_step8")['tested'] & 14).any()
    assert not C.case_result("1x1")['tested'].any()
