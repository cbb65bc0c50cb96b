"""CPU: the NumPy restatement of DESIGN.md "BOP pose errors (VSD, MSSD, MSPD)" (tests/bop_score_reference.py) and the
host side of cloudaae_amd/utils/bop_score.py, anchored on cases worked by hand."""
import numpy as np
import torch

import bop_score_reference as BR
from cloudaae_amd.utils import bop_score as B

# a camera whose factor is a power of two, so D(d) = d / 1024 is exact at the pixel (u, v) = (cx, cy) where m = 1
INTR = np.array([[1024.0, 1024.0, 1.0, 0.0, 1024.0]], np.float32)
DELTA = 16.0 / 1024.0


def _six_pixels(dt_at_delta):
    """2 x 3, row-major pixels 0..5:
    0 no test depth, dg = de                         -> vis_g, vis_e; |Dg - De| = 0
    1 (m = 1) D(dg) - D(dt) = (2048 - dt) / 1024; de 32 units behind dg, visible only through vis_g
    2 an occluder a metre nearer than dg and de      -> neither
    3 de = 0                                         -> vis_g only
    4 dg = 0, de in front of the test depth          -> vis_e only
    5 nothing anywhere"""
    dt = np.array([[0, dt_at_delta, 1000], [2048, 2048, 0]], np.uint16)[None]
    dg = np.array([[2048, 2048, 2048], [2048, 0, 0]], np.uint16)[None]
    de = np.array([[2048, 2080, 2048], [0, 2040, 0]], np.uint16)[None, None]
    return dt, dg, de


def test_six_pixels_by_hand():
    tau = np.array([[32.0 / 1024.0, 33.0 / 1024.0]])
    dt, dg, de = _six_pixels(2032)                       # D(dg) - D(dt) = 16 / 1024 = delta exactly: visible (<=)
    assert BR.distance_image(dg[0], INTR[0])[0, 1] == 2.0 and BR.distance_image(dg[0], INTR[0])[0, 0] > 2.0
    c = BR.vsd_counts(dt, INTR, [0], dg, de, DELTA, tau)
    assert c['visib_gt'].tolist() == [3]                 # pixels 0, 1, 3
    assert c['inter'].tolist() == [[2]]                  # 0, 1
    assert c['union'].tolist() == [[4]]                  # 0, 1, 3, 4
    assert c['over'].tolist() == [[[1, 0]]]              # pixel 1: |Dg - De| = 32 / 1024 = tau_1 exactly (>=), below tau_2
    e = BR.vsd_errors(c['inter'], c['union'], c['over'])
    assert e.tolist() == [[[0.75, 0.5]]]                 # (1 + 4 - 2) / 4, (0 + 4 - 2) / 4
    assert np.array_equal(B.vsd_errors(c['inter'], c['union'], c['over']), e)
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    assert np.array_equal(B.vsd_errors(t['inter'], t['union'], t['over']).numpy(), e)
    # one depth unit more between dt and dg: pixel 1 is occluded, and de there, no longer carried by vis_g, too
    dt, dg, de = _six_pixels(2031)
    c = BR.vsd_counts(dt, INTR, [0], dg, de, DELTA, tau)
    assert (c['visib_gt'].tolist(), c['inter'].tolist(), c['union'].tolist(), c['over'].tolist()) == ([2], [[1]], [[3]], [[[0, 0]]])
    # a frame_of entry outside the frames: zeros
    c = BR.vsd_counts(dt, INTR, [1], dg, de, DELTA, tau)
    assert not c['union'].any() and not c['visib_gt'].any()


def test_empty_union_costs_one():
    z = np.zeros((1, 2, 3), np.uint16)
    c = BR.vsd_counts(z + 500, INTR, [0], z, z[None], DELTA, np.array([[0.01, 0.02, 0.03]]))
    assert c['union'].tolist() == [[0]]
    assert BR.vsd_errors(c['inter'], c['union'], c['over']).tolist() == [[[1.0, 1.0, 1.0]]]


def test_estimate_equal_to_ground_truth_has_no_error_whatever_the_test_depth():
    rng = np.random.default_rng(5)
    H, W = 9, 13
    intr = np.array([[20.0, 21.0, 6.3, 4.1, 1000.0]], np.float32)
    dg = np.where(rng.random((1, H, W)) < 0.3, 0, rng.integers(1, 65536, (1, H, W))).astype(np.uint16)
    for dt in (np.zeros((1, H, W), np.uint16), np.full((1, H, W), 1, np.uint16), dg.copy(),
               np.where(rng.random((1, H, W)) < 0.3, 0, rng.integers(1, 65536, (1, H, W))).astype(np.uint16)):
        c = BR.vsd_counts(dt, intr, [0], dg, dg[None], 0.015, np.array([[1e-300, 0.1]]))
        assert not c['over'].any() and np.array_equal(c['inter'], c['union']) and c['inter'][0, 0] == c['visib_gt'][0]


CUBE = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
RZ90 = np.array([[0.0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def test_mssd_of_a_turned_cube():
    gt = np.eye(4)
    gt[:3, 3] = [0.25, -0.5, 5.0]
    est = gt @ RZ90                                     # every vertex (x, y, z) goes to (-y, x, z): moved by 2
    mssd, mspd = BR.mssd_mspd(CUBE, est, gt)
    assert mssd == 2.0 and mspd is None
    four = np.stack([np.linalg.matrix_power(RZ90, k) for k in range(4)])      # exact entries
    assert BR.mssd_mspd(CUBE, est, gt, symmetries=four)[0] == 0.0
    assert BR.mssd_mspd(CUBE, est, gt, symmetries=four[[0, 2]])[0] == 2.0     # the half turn does not help
    made = B.symmetry_rotations((0, 0, 2.0), (0, 0, 0), 4)                    # sin and cos of pi / 2: entries to 1e-16
    assert made.shape == (4, 4, 4) and np.array_equal(made[0], np.eye(4)) and np.abs(made - four).max() < 1e-15
    assert BR.mssd_mspd(CUBE, est, gt, symmetries=made)[0] < 1e-15
    # an axis that does not pass through the origin keeps its own points fixed
    off = B.symmetry_rotations((0, 1, 0), (0.3, 0.0, -0.2), 3)
    for T in off:
        assert np.abs(T @ np.array([0.3, 7.0, -0.2, 1.0]) - np.array([0.3, 7.0, -0.2, 1.0])).max() < 1e-15
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-15
    sym, num = B.pack_symmetries([None, four, four[:2]], 3)
    assert sym.shape == (3, 4, 4, 4) and num.tolist() == [1, 4, 2] and np.array_equal(sym[0, 3], np.eye(4))


def test_mspd_of_an_image_plane_shift_and_behind_the_camera():
    plane = np.array([[x, y, 0.0] for x in (-0.1, 0.0, 0.07) for y in (-0.05, 0.02)], np.float32)
    intr = np.array([572.4, 573.6, 325.3, 242.0, 1000.0], np.float32)
    gt = np.eye(4)
    gt[:3, 3] = [0.02, -0.01, 0.8]
    est = gt.copy()
    est[0, 3] += 0.013
    mssd, mspd = BR.mssd_mspd(plane, est, gt, intr)
    want = float(np.float32(572.4)) * 0.013 / 0.8
    assert abs(mspd - want) <= 1e-12 * want and abs(mssd - 0.013) <= 1e-15
    behind = gt.copy()
    behind[2, 3] = -0.8
    assert BR.mssd_mspd(plane, behind, gt, intr)[1] == np.inf and BR.mssd_mspd(plane, gt, behind, intr)[1] == np.inf
    at_zero = gt.copy()
    at_zero[2, 3] = 0.0                                  # Z = 0 is not > 0
    assert BR.mssd_mspd(plane, at_zero, gt, intr)[1] == np.inf
    assert np.isfinite(BR.mssd_mspd(plane, behind, gt, intr)[0])


def test_recall_and_average_recall_of_a_table():
    th = B.THETAS
    assert np.allclose(th, [0.05 * j for j in range(1, 11)]) and B.VSD_TAUS == th and B.MSPD_PIXELS[0] == 5.0
    # one sample, two taus: e = 0.0 passes all ten thetas, e = 0.26 passes those above it: 0.3 .. 0.5 = 5 of 10
    e = np.array([[0.0, 0.26], [1.0, 1.0]])
    assert np.array_equal(B.recall(e, th), [15.0 / 20.0, 0.0]) and np.array_equal(BR.recall(e, th), B.recall(e, th))
    assert B.recall(np.array([0.05]), [0.05, 0.06]).tolist() == [0.5]         # strict
    # per-sample thresholds
    assert B.recall(np.array([0.1, 0.1]), np.array([[0.05, 0.2], [0.2, 0.3]])).tolist() == [0.5, 1.0]
    log = B.BopScoreLog(("pred",), diameters=[0.2, 0.4])
    cls = torch.tensor([0, 1, 1])
    vsd = torch.tensor([[[0.0] * 10], [[1.0] * 10], [[0.26] * 10]], dtype=torch.float64)        # recalls 1, 0, 0.5
    mssd = torch.tensor([[0.015], [0.07], [1.0]], dtype=torch.float64)    # thresholds 0.01 j and 0.02 j: 9/10, 7/10, 0
    mspd = torch.tensor([[12.0], [float('inf')], [2.0]], dtype=torch.float64)   # width 320: 2.5 j: 6/10, 0, 1
    log.append(cls, vsd, mssd, mspd, width=320, seq=[1, 1, 2], frame=[0, 1, 2])
    s = log.summary()
    a = s['all']['pred']
    assert a['n'] == 3 and abs(a['ar_vsd'] - 0.5) < 1e-15 and abs(a['ar_mssd'] - (0.9 + 0.7 + 0.0) / 3) < 1e-15
    assert abs(a['ar_mspd'] - (0.6 + 0.0 + 1.0) / 3) < 1e-15 and abs(a['ar'] - (a['ar_vsd'] + a['ar_mssd'] + a['ar_mspd']) / 3) < 1e-15
    c0, c1 = s['classes'][0]['pred'], s['classes'][1]['pred']
    assert (c0['n'], c0['ar_vsd'], c0['ar_mssd'], c0['ar_mspd']) == (1, 1.0, 0.9, 0.6)
    assert c1['n'] == 2 and c1['ar_vsd'] == 0.25 and c1['ar_mssd'] == 0.35 and c1['ar_mspd'] == 0.5
    lines = log.lines()
    assert len(lines) == 3 and lines[0].startswith("bop class 0 pred n 1 ar_vsd 1.000000") and lines[2].startswith("bop all pred n 3")
    assert log.rows()['seq'].tolist() == [1, 1, 2] and log.rows()['vsd'].shape == (3, 1, 10)
