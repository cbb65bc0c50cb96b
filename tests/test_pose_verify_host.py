"""CPU: the NumPy restatement of DESIGN.md "Pose verification" (tests/pose_verify_reference.py) on hand-written frames
whose counts are typed in by hand, the selection rule's corner cases, the flip hypotheses of a box, the packing of a
HypothesisTable, and the whole pipeline on the NumPy renderer: of the four flip candidates of an L-shaped prism behind an
occluding plate the ground truth wins by a wide margin."""
import numpy as np
import pytest

import pose_verify_reference as V


# ---- the six predicates on 3 x 5 frames -------------------------------------------------------------------------------------
T = np.array([[[100, 100, 0, 200, 200],
               [100, 0, 100, 300, 300],
               [0, 100, 100, 100, 65535]]], np.uint16)
LABEL = np.array([[[1, 1, 1, 2, 2],
                   [1, 2, 1, 1, 0],
                   [1, 1, 2, 1, 1]]], np.uint8)
D0 = np.array([[100, 103, 50, 0, 190],
               [104, 70, 96, 310, 289],
               [0, 0, 0, 97, 1]], np.uint16)
D1 = np.zeros((3, 5), np.uint16)


def test_reference_counts_on_hand_written_frames():
    """tau = 3, want = 1.  Pixel by pixel for D0 (t -> d):
    row 0: 100->100 consistent, seg; 100->103 consistent (|3| <= 3), seg; 0->50 unknown; 200->0 not rendered;
           200->190 in_front (t - d = 10).
    row 1: 100->104 behind (d - t = 4); 0->70 unknown; 100->96 in_front (4); 300->310 behind; 300->289 in_front.
    row 2: three not rendered; 100->97 consistent, seg; 65535->1 in_front.
    seg = label 1 with depth: row 0: 2 (the third has no depth), row 1: 3, row 2: 3 (the first has no depth): 8."""
    counts, seg_total, abs_sum = V.fit_counts(T, LABEL, [0], [1], np.stack([D0, D1])[None], [3])
    assert counts.shape == (1, 2, 6) and counts.dtype == np.int32
    #                            rendered consistent in_front behind unknown explained
    assert counts[0, 0].tolist() == [11, 3, 4, 2, 2, 3]
    assert counts[0, 1].tolist() == [0, 0, 0, 0, 0, 0]
    assert seg_total.tolist() == [8]
    assert abs_sum.tolist() == [[0 + 3 + 3, 0]]
    # rendered = consistent + in_front + behind + unknown
    assert counts[0, 0, 0] == counts[0, 0, 1:5].sum()
    # without a label nothing is explained and there is no segment; tau = 0 keeps the exact hit only
    counts, seg_total, abs_sum = V.fit_counts(T, None, [0], None, D0[None, None], [0])
    assert counts[0, 0].tolist() == [11, 1, 5, 3, 2, 0] and seg_total.tolist() == [0] and abs_sum.tolist() == [[0]]
    # a label value no pixel has; a frame outside the frames
    counts, seg_total, _ = V.fit_counts(T, LABEL, [0, 1, -1], [7, 1, 1], np.stack([D0[None]] * 3), [3, 3, 3])
    assert counts[0, 0].tolist() == [11, 3, 4, 2, 2, 0] and seg_total.tolist() == [0, 0, 0] and not counts[1:].any()
    # tau = 65535 makes every pixel with both depths consistent: 9, of which 7 lie in the segment
    counts, _, abs_sum = V.fit_counts(T, LABEL, [0], [1], D0[None, None], [65535])
    assert counts[0, 0].tolist() == [11, 9, 0, 0, 2, 7]
    assert abs_sum[0, 0] == 3 + 10 + 4 + 4 + 10 + 11 + 3 + 65534


def test_reference_reads_the_depths_unsigned():
    t = np.array([[[0, 1, 32767, 32768, 40000, 65535]]], np.uint16)
    d = np.array([[[[32768, 32768, 32768, 32767, 65535, 40000]]]], np.uint16)
    counts, _, abs_sum = V.fit_counts(t, None, [0], None, d, [1])
    # 0->32768 unknown; 1->32768 behind; 32767->32768 consistent; 32768->32767 consistent; 40000->65535 behind; 65535->40000 in front
    assert counts[0, 0].tolist() == [6, 2, 1, 2, 1, 0] and abs_sum[0, 0] == 2


# ---- the selection rule --------------------------------------------------------------------------------------------------
def _counts(rows):
    """rows: per hypothesis (consistent, in_front, behind, explained) -> [1,P,6]."""
    c = np.zeros((1, len(rows), 6), np.int32)
    for j, (cons, front, behind, expl) in enumerate(rows):
        c[0, j] = [cons + front + behind, cons, front, behind, 0, expl]
    return c


def test_selection_ties_zero_denominators_and_invalid_hypotheses():
    P = 4
    pose = np.arange(P * 16, dtype=np.float64).reshape(1, P, 4, 4)
    ones = np.ones((1, P), np.int32)
    # mode 0, seg_total 10: 5 / 10, 6 / 12, 1 / 2 are one number; the lowest index keeps it
    c = _counts([(0, 0, 0, 5), (0, 2, 0, 6), (0, 0, 0, 4), (0, 0, 0, 5)])
    best, score, pose_best, margin = V.select(c, [10], ones, pose, 0)
    assert best.tolist() == [0] and score[0].tolist() == [0.5, 0.5, 0.4, 0.5] and margin.tolist() == [0.0]
    assert np.array_equal(pose_best[0], pose[0, 0])
    # an invalid hypothesis scores 0 whatever it counts; then 1 and 3 tie and 1 wins
    valid = np.array([[0, 1, 1, 1]], np.int32)
    best, score, pose_best, margin = V.select(c, [10], valid, pose, 0)
    assert best.tolist() == [1] and score[0].tolist() == [0.0, 0.5, 0.4, 0.5] and margin.tolist() == [0.0]
    assert np.array_equal(pose_best[0], pose[0, 1])
    # den = 0 everywhere (no segment, nothing in front): every score is 0 and hypothesis 0 stays
    best, score, _, margin = V.select(_counts([(0, 0, 0, 0)] * P), [0], ones, pose, 0)
    assert best.tolist() == [0] and not score.any() and margin.tolist() == [0.0]
    # mode 1: consistent / (consistent + in_front + behind); den = 0 for hypothesis 2
    c = _counts([(3, 1, 0, 0), (6, 1, 1, 0), (0, 0, 0, 0), (1, 0, 3, 0)])
    best, score, _, margin = V.select(c, [0], ones, pose, 1)
    assert best.tolist() == [0] and score[0].tolist() == [0.75, 0.75, 0.0, 0.25] and margin.tolist() == [0.0]
    c = _counts([(3, 1, 0, 0), (7, 1, 0, 0), (0, 0, 0, 0), (1, 0, 3, 0)])
    best, score, _, margin = V.select(c, [0], ones, pose, 1)
    assert best.tolist() == [1] and margin.tolist() == [0.875 - 0.75]
    # one hypothesis: it wins with margin 0
    best, score, _, margin = V.select(_counts([(3, 1, 0, 0)]), [0], ones[:, :1], pose[:, :1], 1)
    assert best.tolist() == [0] and score.tolist() == [[0.75]] and margin.tolist() == [0.0]


def test_selection_orders_fractions_as_the_integers_do():
    """3333333 / 9999998 is above 1 / 3 by 1 / (3 * 9999998); (2^24 - 1) / (2^25 - 1) is above (2^24 - 2) / (2^25 - 3) by
    about 2^-50, a few units in the last place of a double, at the limits num < 2^24, den < 2^26 of the rule.  The integers
    order both."""
    ones = np.ones((1, 2), np.int32)
    pose = np.zeros((1, 2, 4, 4))
    c = _counts([(0, 0, 0, 1), (0, 9999998 - 3, 0, 3333333)])
    assert V.select(c, [3], ones, pose, 0)[0].tolist() == [1]
    c = _counts([(0, 0, 0, 3333333), (0, 0, 0, 1)])
    c[0, 0, 2] = 9999998 - 3
    assert V.select(c, [3], ones, pose, 0)[0].tolist() == [0]
    a, b = ((1 << 24) - 1, (1 << 25) - 1), ((1 << 24) - 2, (1 << 25) - 3)
    assert a[0] * b[1] > b[0] * a[1]
    c = _counts([(0, b[1] - 100, 0, b[0]), (0, a[1] - 100, 0, a[0])])
    best, score, _, margin = V.select(c, [100], ones, pose, 0)
    assert best.tolist() == [1] and margin[0] >= 0.0


# ---- flip hypotheses and their table ----------------------------------------------------------------------------------------
def _box_sample():
    g = np.linspace(-0.5, 0.5, 9)
    x, y, z = np.meshgrid(g * 1.0, g * 2.0, g * 3.0, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) + [0.3, -0.2, 0.7]


def test_flip_hypotheses_of_a_box():
    from cloudaae_amd.utils import pose_verify as PV
    pts = _box_sample()
    H = PV.flip_hypotheses(pts)
    assert H.shape == (4, 4, 4) and H.dtype == np.float64
    assert np.array_equal(H[0], np.eye(4))                        # the identity, exactly, first
    c = np.append(pts.mean(axis=0), 1.0)
    for k in range(1, 4):
        assert np.abs(H[k] @ H[k] - np.eye(4)).max() <= 1e-12      # a half turn
        assert np.abs(H[k] @ c - c).max() <= 1e-12                 # through the centroid
        assert abs(np.linalg.det(H[k][:3, :3]) - 1.0) <= 1e-12 and abs(np.trace(H[k][:3, :3]) + 1.0) <= 1e-12
        assert H[k][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    # by descending eigenvalue: the box's long side is z, then y, then x
    for k, axis in ((1, 2), (2, 1), (3, 0)):
        assert abs(H[k][axis, axis] - 1.0) <= 1e-12
    assert np.abs(H - V.flip_hypotheses(pts)).max() <= 1e-12
    assert np.array_equal(PV.flip_hypotheses(np.concatenate([pts, pts], axis=1).astype(np.float32))[0], np.eye(4))


def test_hypothesis_table_packing():
    from cloudaae_amd.utils import pose_verify as PV
    pts = _box_sample()
    flips = PV.flip_hypotheses(pts)
    table = PV.HypothesisTable.from_sets({1: flips, 3: flips[:2]}, num_class=5)
    assert table.index.tolist() == [0, 0, 4, 4, 6, 6] and table.index.dtype == np.int32
    assert table.hyp.shape == (6, 4, 4) and table.num_class == 5 and table.num_total == 6 and table.max_members == 4
    assert np.array_equal(table.members(1), flips) and np.array_equal(table.members(3), flips[:2]) and len(table.members(0)) == 0
    models = np.stack([pts, pts[:, [2, 0, 1]]]).astype(np.float32)
    both = PV.HypothesisTable.from_models(models)
    assert both.index.tolist() == [0, 4, 8]
    assert np.array_equal(both.members(1), PV.flip_hypotheses(models[1]))
    one = PV.HypothesisTable.from_models(models[1:], classes=[2], num_class=4)
    assert one.index.tolist() == [0, 0, 0, 4, 4] and np.array_equal(one.members(2), both.members(1))
    with pytest.raises(ValueError, match="identity"):
        PV.HypothesisTable.from_sets({0: flips[1:]})
    moved = PV.HypothesisTable.from_sets({0: flips[[1, 2, 0, 3]]}, identity_first=False)
    assert np.array_equal(moved.members(0)[2], np.eye(4))
    with pytest.raises(ValueError, match="class id"):
        PV.HypothesisTable.from_sets({4: flips}, num_class=4)
    with pytest.raises(_lib_error()):
        table.on("cpu")
    # the restatement's composition: a base times the identity is the base, times a half turn twice the base again
    base = np.eye(4)
    base[:3, :3] = flips[1][:3, :3] @ flips[2][:3, :3]
    base[:3, 3] = [0.1, -0.2, 0.9]
    pose, trans, valid = V.compose(base[None], [1, ], table.index, table.hyp, 5)
    assert valid.tolist() == [[1, 1, 1, 1, 0]] and np.array_equal(pose[0, 4], pose[0, 0])
    assert np.abs(pose[0, 0] - base).max() == 0.0 and np.abs(V.compose_one(pose[0, 2], flips[2]) - base).max() <= 1e-12
    assert trans.dtype == np.float32 and np.array_equal(trans[0, 1], pose[0, 1, :3, 3].astype(np.float32))
    pose, _, valid = V.compose(base[None], [0], table.index, table.hyp, 2)          # a class without a set
    assert valid.tolist() == [[0, 0]] and np.array_equal(pose[0, 0], pose[0, 1]) and np.abs(pose[0, 0] - base).max() == 0.0
    pose, _, valid = V.compose(base[None], [9], table.index, table.hyp, 2)          # a class outside the table
    assert valid.tolist() == [[0, 0]] and np.abs(pose[0, 1] - base).max() == 0.0


def _lib_error():
    from cloudaae_amd import _lib
    return _lib.HipLibraryError


def test_tau_units():
    from cloudaae_amd.utils import pose_verify as PV
    assert PV.tau_units([0.01, 0.00014999, 0.00015001, 0.0], [10000.0, 10000.0, 10000.0, 1000.0]).tolist() == [100, 1, 2, 0]
    assert np.array_equal(PV.tau_units([0.01, 0.02], [1000.0, 10000.0]), V.tau_units([0.01, 0.02], [1000.0, 10000.0]))
    assert PV.tau_units(1e9, 1e9).tolist() == 2147483647 and PV.tau_units(-1.0, 10.0).tolist() == 0


# ---- end to end on the NumPy renderer --------------------------------------------------------------------------------------
def test_the_ground_truth_wins_among_its_flips():
    """64 x 48: the L prism under the ground truth, a nearer plate over the end of its long leg.  The candidates are the
    ground truth times the four flips with the identity third."""
    s = V.scene()
    lab = s['label'][0]
    assert (lab == 1).sum() > 100 and (lab == 2).sum() > 100
    alone = V.verify(s['meshes'], [0], s['poses'][:, 2:3], s['depth'], s['label'], [1], s['intr'], [0])
    assert alone['counts'][0, 0, 3] > 10, "the plate hides nothing of the object"           # behind
    assert np.array_equal(s['poses'][0, 2], s['gt'])
    r = V.verify(s['meshes'], [0], s['poses'], s['depth'], s['label'], [1], s['intr'], [0])
    print("counts %s seg_total %s score %s best %s margin %s" % (r['counts'][0].tolist(), r['seg_total'].tolist(),
                                                                r['score'][0].tolist(), r['best'].tolist(), r['margin'].tolist()))
    assert r['best'].tolist() == [2] and r['score'][0, 2] == 1.0
    assert r['margin'][0] >= 0.1
    assert np.array_equal(r['pose_best'][0], s['gt']) and not r['dropped'].any()
    c = r['counts'][0]
    assert np.array_equal(c[:, 0], c[:, 1:5].sum(axis=1)) and c[2, 2] == 0 and c[2, 4] == 0 and r['abs_sum'][0, 2] == 0
    assert (c[[0, 1, 3], 2] > 0).all() and (c[[0, 1, 3], 4] > 0).all()                     # the flips stick out
    # the silhouette rule, without the label, picks it too
    r1 = V.verify(s['meshes'], [0], s['poses'], s['depth'], None, None, s['intr'], [0], mode=1)
    print("mode 1: score %s margin %s" % (r1['score'][0].tolist(), r1['margin'].tolist()))
    assert r1['best'].tolist() == [2] and np.array_equal(r1['counts'][:, :, :5], r['counts'][:, :, :5])
