"""CPU: anchors of tests/detect_reference.py, the NumPy restatement of DESIGN.md "Detections" that
tests/test_38_detect_gpu.py compares the kernels with: the windowed counts against pose_verify_reference.fit_counts on
zero-padded crops, the greedy assignment against a brute-force statement of its properties on tiny tables, the windows at
the frame's corners, and the scene the GPU tests share, on which the restatement alone has to name every component."""
import itertools

import numpy as np
import pytest

import detect_reference as DR
import pose_verify_reference as V


# ---- windowed counts -------------------------------------------------------------------------------------------------------
def _padded_crop(image, u0, v0, wh, ww, fill):
    """The window cut out of the image padded by `fill` on every side."""
    H, W = image.shape
    pad = max(abs(u0), abs(v0), abs(u0 + ww - W), abs(v0 + wh - H), 0) + 1
    big = np.pad(image, pad, constant_values=fill)
    return big[v0 + pad:v0 + pad + wh, u0 + pad:u0 + pad + ww]


@pytest.mark.parametrize("wh,ww", [(9, 8), (5, 13), (7, 1), (30, 40)])
def test_windowed_counts_equal_full_counts_on_zero_padded_crops(wh, ww):
    rng = np.random.default_rng(wh * 100 + ww)
    F, H, W, P = 2, 20, 27, 3
    dt = np.where(rng.random((F, H, W)) < 0.2, 0, rng.integers(990, 1011, (F, H, W))).astype(np.uint16)
    label = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    origin = np.array([[0, 0], [-3, -2], [W - 4, 5], [6, H - 3], [-ww, 2], [W, H], [3, -wh - 1], [5, 4]], np.int32)
    B = len(origin)
    frame_of = np.array([0, 1, 0, 1, 0, 1, 0, 2], np.int32)               # the last one names no frame
    want = rng.integers(0, 3, B).astype(np.int32)
    tau = np.array([0, 3, 7, 65535, 2, 2, 2, 2], np.int32)
    dh = np.where(rng.random((B, P, wh, ww)) < 0.3, 0, rng.integers(985, 1016, (B, P, wh, ww))).astype(np.uint16)
    got = DR.fit_counts_window(dt, label, frame_of, want, origin, wh, ww, dh, tau)
    bare = DR.fit_counts_window(dt, None, frame_of, None, origin, wh, ww, dh, tau)
    for b in range(B):
        fr = int(frame_of[b])
        if fr >= F:
            assert not got[0][b].any() and got[1][b] == 0 and not got[2][b].any()
            continue
        # a padded label of 255 is nobody's segment: want is below 3, and the padded depth is 0 anyway
        t = _padded_crop(dt[fr], int(origin[b, 0]), int(origin[b, 1]), wh, ww, 0)[None]
        lab = _padded_crop(label[fr], int(origin[b, 0]), int(origin[b, 1]), wh, ww, 255)[None]
        ref = V.fit_counts(t, lab, [0], want[b:b + 1], dh[b:b + 1], tau[b:b + 1])
        for g, r in zip(got, ref):
            assert np.array_equal(g[b], r[0]), b
        ref = V.fit_counts(t, None, [0], None, dh[b:b + 1], tau[b:b + 1])
        for g, r in zip(bare, ref):
            assert np.array_equal(g[b], r[0]), b
    # a window wholly outside: what is rendered is unknown, and nothing else is counted
    for b in (4, 5, 6):
        c = got[0][b]
        assert np.array_equal(c[:, 0], c[:, 4]) and c[:, 0].min() > 0 and not c[:, [1, 2, 3, 5]].any() and got[1][b] == 0
    # the whole frame as the window is the full-frame definition itself
    dh_full = np.where(rng.random((2, P, H, W)) < 0.3, 0, rng.integers(985, 1016, (2, P, H, W))).astype(np.uint16)
    full = DR.fit_counts_window(dt, label, [1, 0], [1, 2], np.zeros((2, 2), np.int32), H, W, dh_full, [4, 0])
    for g, r in zip(full, V.fit_counts(dt, label, [1, 0], [1, 2], dh_full, [4, 0])):
        assert g.dtype == r.dtype and np.array_equal(g, r)


# ---- assignment ------------------------------------------------------------------------------------------------------------
def _tiny_tables(rng, F, K, C, P):
    counts = np.zeros((F, K, C, P, 6), np.int32)
    counts[..., 5] = rng.integers(0, 5, (F, K, C, P))          # explained
    counts[..., 1] = counts[..., 5] + rng.integers(0, 2, (F, K, C, P))
    counts[..., 2] = rng.integers(0, 3, (F, K, C, P))          # in_front
    counts[..., 3] = rng.integers(0, 2, (F, K, C, P))
    seg_total = rng.integers(1, 5, (F, K, C)).astype(np.int32)
    valid = (rng.random((F, K, C, P)) < 0.85).astype(np.int32)
    return counts, seg_total, valid


@pytest.mark.parametrize("mode,max_per_class,min_score", [(0, 1, (1, 2)), (0, 2, (0, 1)), (1, 1, (1, 1)), (1, 2, (2, 3)),
                                                          (0, 1, (3, 4))])
def test_assignment_has_the_greedy_rule_s_properties(mode, max_per_class, min_score):
    rng = np.random.default_rng(10 * mode + max_per_class)
    F, K, C, P = 40, 4, 3, 3
    counts, seg_total, valid = _tiny_tables(rng, F, K, C, P)
    n_components = rng.integers(0, K + 1, F).astype(np.int32)
    pose = rng.standard_normal((F, K, C, P, 4, 4))
    r = DR.assign(counts, seg_total, valid, pose, n_components, mode, min_score[0], min_score[1], max_per_class)
    ties = 0
    for f in range(F):
        nc = int(n_components[f])
        # step 1 against a brute-force maximum over the hypotheses with exact rationals
        frac = {}
        for k, c in itertools.product(range(K), range(C)):
            fr = [V.fraction(counts[f, k, c, j], seg_total[f, k, c], valid[f, k, c, j] and k < nc, mode) for j in range(P)]
            top = max(n * 1.0 / d for n, d in fr)                    # tiny integers: the quotients are distinct when the fractions are
            first = [j for j, (n, d) in enumerate(fr) if n * 1.0 / d == top][0]
            assert r['pair_hyp'][f, k, c] == first and (r['pair_num'][f, k, c], r['pair_den'][f, k, c]) == fr[first]
            assert r['pair_score'][f, k, c] == float(fr[first][0]) / float(fr[first][1])
            frac[k, c] = fr[first]
        det = r['det_class'][f]
        order = sorted((int(r['det_rank'][f, k]), k) for k in range(K) if det[k] >= 0)
        assert [o[0] for o in order] == list(range(len(order))) and r['n_det'][f] == len(order)
        assert all(det[k] < 0 and r['det_rank'][f, k] < 0 for k in range(nc, K))
        for c in range(C):
            assert int((det == c).sum()) <= max_per_class                                   # the cap
        used, taken = [0] * C, set()

        def eligible(k, c):
            n, d = frac[k, c]
            return k < nc and k not in taken and used[c] < max_per_class and n > 0 and n * min_score[1] >= min_score[0] * d
        for _, k in order:
            c = int(det[k])
            assert eligible(k, c)
            n, d = frac[k, c]
            for k2, c2 in itertools.product(range(K), range(C)):
                if not eligible(k2, c2) or (k2, c2) == (k, c):
                    continue
                n2, d2 = frac[k2, c2]
                assert n2 * d <= n * d2                              # no eligible pair beats the one taken
                if n2 * d == n * d2:
                    ties += 1
                    assert (k, c) < (k2, c2)                          # a tie goes to the lowest k, then c
            taken.add(k)
            used[c] += 1
            assert (r['det_num'][f, k], r['det_den'][f, k]) == (n, d) and r['det_hyp'][f, k] == r['pair_hyp'][f, k, c]
            assert np.array_equal(r['det_pose'][f, k], pose[f, k, c, r['pair_hyp'][f, k, c]])
        assert not any(eligible(k, c) for k, c in itertools.product(range(K), range(C)))   # it stopped for want of a pair
        for k in range(K):
            if det[k] < 0:
                assert not r['det_pose'][f, k].any() and (r['det_num'][f, k], r['det_den'][f, k], r['det_hyp'][f, k]) == (0, 1, -1)
            others = [c for c in range(C) if c != det[k]]
            a = int(r['alt_class'][f, k])
            assert a in others and (r['alt_num'][f, k], r['alt_den'][f, k]) == frac[k, a]
            for c in others:
                assert frac[k, c][0] * frac[k, a][1] <= frac[k, a][0] * frac[k, c][1]
                assert c >= a or frac[k, c][0] * frac[k, a][1] < frac[k, a][0] * frac[k, c][1]
    assert ties >= 5                                                 # the tables are small enough for ties at the top


def test_assignment_of_one_class_has_no_alternative():
    counts = np.zeros((1, 2, 1, 1, 6), np.int32)
    counts[0, :, 0, 0, 5] = (3, 4)
    r = DR.assign(counts, np.full((1, 2, 1), 4, np.int32), np.ones((1, 2, 1, 1), np.int32), np.tile(np.eye(4), (1, 2, 1, 1, 1, 1)),
                  [2], 0, 1, 2, 1)
    assert r['det_class'].tolist() == [[-1, 0]] and r['det_rank'].tolist() == [[-1, 0]] and r['n_det'].tolist() == [1]
    assert r['alt_class'].tolist() == [[0, -1]] and r['alt_num'].tolist() == [[3, 0]] and r['alt_den'].tolist() == [[4, 1]]


# ---- windows ---------------------------------------------------------------------------------------------------------------
def test_windows_at_the_corners_and_as_wide_as_the_frame():
    from cloudaae_amd.utils import detect
    H, W = 48, 70
    box = np.array([[[0, 0, 9, 5], [60, 40, 69, 47], [0, 42, 3, 47], [-1, -1, -1, -1]],
                    [[0, 10, 69, 12], [66, 0, 69, 1], [5, 5, 5, 5], [30, 30, 44, 40]]], np.int64)
    n = np.array([3, 4])
    for margin in (0.5, 0, 0.1, 2):
        origin, wh, ww = detect.windows(box, n, H, W, margin)
        ro, rh, rw = DR.windows(box, n, H, W, margin)
        assert (wh, ww) == (rh, rw) and np.array_equal(origin, ro) and origin.dtype == np.int32
        assert ww % 8 == 0 and wh <= H and ww <= (W + 7) // 8 * 8
        for f in range(2):
            for k in range(4):
                if k >= n[f]:
                    assert origin[f, k].tolist() == [0, 0]
                    continue
                u0, v0 = origin[f, k]
                bw, bh = box[f, k, 2] - box[f, k, 0] + 1, box[f, k, 3] - box[f, k, 1] + 1
                if bw <= ww and bh <= wh:                             # the window holds the box, centred to a pixel
                    assert u0 <= box[f, k, 0] and u0 + ww > box[f, k, 2] and v0 <= box[f, k, 1] and v0 + wh > box[f, k, 3]
                    assert 0 <= (u0 + ww - 1 - box[f, k, 2]) - (box[f, k, 0] - u0) <= 1
    origin, wh, ww = detect.windows(box, n, H, W, 0.5)
    # the box as wide as the frame asks for 140 columns: capped at 70, rounded up to 72; rows: 11 + 2 * 6 = 23
    assert (wh, ww) == (23, 72)
    assert origin[0, 0].tolist() == [0 - (72 - 10) // 2, 0 - (23 - 6) // 2] and origin[0, 1].tolist() == [60 - 31, 40 - 7]
    assert origin[1, 0].tolist() == [-1, 10 - 10] and origin[1, 1].tolist() == [66 - 34, 0 - 10]
    assert detect.windows(box, n, H, W, 0.1)[1:] == (11 + 2 * 2, 72)          # a tenth of 11 rows, rounded up: 2
    assert detect.windows(box, [0, 0], H, W)[1:] == (1, 8) and not detect.windows(box, [0, 0], H, W)[0].any()


# ---- the scene -------------------------------------------------------------------------------------------------------------
def test_the_restatement_names_the_scene_s_components():
    s, g = DR.scene(), DR.scene_segments()
    assert s['depth'].shape == (1, DR.SCENE_H, DR.SCENE_W) and sorted(np.unique(s['label']).tolist()) == [0, 1, 2, 3, 4]
    assert int(g['n_components'][0]) == 3 and sorted(g['object_of']) == [0, 1, 2]
    r = DR.scene_score()
    print("window %d x %d origin %s" % (r['wh'], r['ww'], r['origin'][0].tolist()))
    print("pair_score\n%s" % r['pair_score'][0])
    for k in ('det_class', 'det_hyp', 'det_num', 'det_den', 'det_rank', 'alt_class', 'alt_num', 'alt_den'):
        print(k, r[k][0].tolist())
    # all three named, hypothesis 0 (the true pose) chosen, nothing for the sphere that is not there
    assert r['det_class'][0].tolist() == g['object_of'] and r['det_hyp'][0].tolist() == [0, 0, 0] and r['n_det'].tolist() == [3]
    assert 3 not in r['det_class'] and not r['dropped'].any()
    # seg_total is the component's size: the window holds its box
    assert np.array_equal(r['seg_total'][0], np.repeat(g['comp_size'][0, :3, None], 4, axis=1))
    # a condition on the scene: no correct pair within 0.1 of the threshold or of its runner-up
    alt = r['alt_num'][0] / r['alt_den'][0]
    assert r['det_score'][0].min() >= 0.5 + 0.1 and (r['det_score'][0] - alt).min() >= 0.1
    # the right shape in the wrong place, and turned, scores less than in its place
    for k, c in enumerate(g['object_of']):
        sc = [V.fraction(r['counts'][0, k, c, j], r['seg_total'][0, k, c], 1, 0) for j in range(3)]
        assert sc[0][0] * sc[2][1] > sc[2][0] * sc[0][1] and sc[0][0] * sc[1][1] >= sc[1][0] * sc[0][1]
    # the correct pairs are explained entirely, so they meet the threshold 1 / 1 with equality, and only they do
    one = DR.assign(r['counts'], r['seg_total'], np.ones((1, 3, 4, 3), np.int32), DR.scene_hypotheses(), [3], 0, 1, 1, 1)
    assert one['det_class'][0].tolist() == g['object_of'] and (one['det_num'] == one['det_den']).all()
    # with the true poses declared invalid the turned or moved ones are all there is: the plate's turned pose still passes
    valid = np.ones((1, 3, 4, 3), np.int32)
    valid[..., 0] = 0
    rest = DR.assign(r['counts'], r['seg_total'], valid, DR.scene_hypotheses(), [3], 0, 1, 2, 1)
    print("without the true poses: class %s hyp %s score %s" % (rest['det_class'][0].tolist(), rest['det_hyp'][0].tolist(),
                                                               rest['det_score'][0].tolist()))
    assert (rest['det_hyp'][rest['det_class'] >= 0] > 0).all() and rest['n_det'][0] < 3
