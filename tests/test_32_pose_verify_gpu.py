"""GPU: cloudaae_depth_fit_counts, cloudaae_pose_compose and cloudaae_select_pose through the C ABI against the NumPy
restatement of DESIGN.md "Pose verification" (tests/pose_verify_reference.py), then utils/pose_verify.py through the
renderer, evaluate_batch(verify=...) and the evaluation's command line.

Every count is an integer and is compared for equality, no pixel left out; the composed matrices are fp64 products in a
stated order and are compared bit for bit; the winner is an exact integer comparison.  Outputs sit between guard rows
that are filled with a byte pattern, so every call starts on garbage."""
import os

import numpy as np
import pytest
import torch

import mesh_models_reference as MR
import pose_verify_reference as V
import render_reference as R

pytestmark = pytest.mark.gpu

GUARD = 4                  # rows kept before and after every output
FILL = 0xA5
SPECIAL = np.array([0, 1, 32767, 32768, 40000, 65535])


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_26_bop_score_gpu.py)."""

    def __init__(self, rows, cols, dtype, dev):
        item = torch.empty((), dtype=dtype).element_size()
        self.rb = cols * item
        self.full = torch.full(((rows + 2 * GUARD) * self.rb,), FILL, dtype=torch.uint8, device=dev)
        self.view = self.full[GUARD * self.rb:(GUARD + rows) * self.rb].view(dtype).view(rows, cols)
        self.rows = rows

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        full = self.full.cpu().numpy()
        edge = GUARD * self.rb
        assert np.all(full[:edge] == FILL) and np.all(full[edge + self.rows * self.rb:] == FILL), "guard rows were written"
        return self.view.cpu().numpy()


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _d(a, ty, dev):
    return torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)


def _shifted(a, ty, dev, shift):
    """The array on the device, its first element `shift` elements past an allocation's start (torch allocations are
    aligned to 256 bytes and more)."""
    flat = np.ascontiguousarray(a, ty).reshape(-1)
    buf = torch.zeros((len(flat) + shift,), dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    assert buf.data_ptr() % 256 == 0
    buf[shift:] = torch.from_numpy(flat).to(dev)
    return buf[shift:]


def launch_fit(hip, dev, dt, label, frame_of, want, dh, tau, shift=0):
    """cloudaae_depth_fit_counts on guarded outputs -> (counts [B,P,6], seg_total [B], abs_sum [B,P]) as the restatement's."""
    F, h, w = dt.shape
    B, P = dh.shape[:2]
    g = [_shifted(dt.view(np.int16), np.int16, dev, shift), _shifted(dh.view(np.int16), np.int16, dev, shift),
         None if label is None else _shifted(label, np.uint8, dev, shift), _d(frame_of, np.int32, dev),
         None if want is None else _d(want, np.int32, dev), _d(tau, np.int32, dev)]
    if shift:
        assert g[0].data_ptr() % 16 == 2 * shift and g[1].data_ptr() % 16 == 2 * shift
    counts, seg, asum = Guarded(B * P, 6, torch.int32, dev), Guarded(B, 1, torch.int32, dev), Guarded(B, P, torch.int64, dev)
    hip.check(hip.lib().cloudaae_depth_fit_counts(F, h, w, g[0].data_ptr(), None if label is None else g[2].data_ptr(), B, P,
                                                  g[3].data_ptr(), None if want is None else g[4].data_ptr(), g[1].data_ptr(),
                                                  g[5].data_ptr(), counts.ptr(), seg.ptr(), asum.ptr(), hip.stream()),
              "cloudaae_depth_fit_counts")
    torch.cuda.synchronize()
    return counts.numpy().reshape(B, P, 6).copy(), seg.numpy().ravel().copy(), asum.numpy().copy()


def assert_fit_equal(got, want, what):
    names = ("counts", "seg_total", "abs_sum")
    for k, g, w in zip(names, got, want):
        print("%s: %s differs in %d of %d entries" % (what, k, int((g != w).sum()), w.size))
    for k, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k)


def _case(h, w, P, seed):
    """F = 2 < B = 4 (frame_of 1, 0, 1, 1).  Depths around 1000 units with zeros and the values that a signed read of
    the bits would get wrong, on both sides; tau 0, 65535, 7 and 3; want 1, 2, 1 and 9, which no pixel has.  The last
    hypothesis of sample 0 is empty and the last of sample 1 is empty but for its final pixel."""
    rng = np.random.default_rng(seed)
    F, B = 2, 4

    def image(*shape):
        d = rng.integers(990, 1011, shape)
        d = np.where(rng.random(shape) < 0.25, 0, d)
        return np.where(rng.random(shape) < 0.2, SPECIAL[rng.integers(0, len(SPECIAL), shape)], d).astype(np.uint16)
    dt, dh = image(F, h, w), image(B, P, h, w)
    dh[0, P - 1] = 0
    dh[1, P - 1] = 0
    dh[1, P - 1, h - 1, w - 1] = dt[0, h - 1, w - 1]
    label = rng.integers(0, 3, (F, h, w)).astype(np.uint8)
    return (dt, label, np.array([1, 0, 1, 1], np.int32), np.array([1, 2, 1, 9], np.int32), dh,
            np.array([0, 65535, 7, 3], np.int32))


# ---- cloudaae_depth_fit_counts ------------------------------------------------------------------------------------------------
# 5 x 13: no lane has eight pixels, the tail path alone; 48 x 64: two aligned runs, the second half full; 45 x 70: an
# aligned run whose tail is no multiple of eight; 7 x 24 from a base 2 bytes past a 16-byte boundary: the scalar path.
# P = 8, 9 and 17: a full chunk of hypotheses, one more, and a third chunk of one.
@pytest.mark.parametrize("h,w,P,shift", [(5, 13, 1, 0), (5, 13, 3, 0), (48, 64, 3, 0), (48, 64, 5, 0), (45, 70, 5, 0),
                                         (7, 24, 3, 1), (7, 24, 1, 3), (48, 64, 1, 1), (7, 24, 8, 0), (7, 24, 9, 1),
                                         (45, 70, 17, 0)])
def test_counts_equal_the_restatement(hip, dev, h, w, P, shift):
    dt, label, frame_of, want, dh, tau = _case(h, w, P, 1000 * h + 10 * P + shift)
    ref = V.fit_counts(dt, label, frame_of, want, dh, tau)
    assert ref[0][2, 0].min() > 0 and ref[1][:3].min() > 0            # every counter is exercised
    assert ref[1][3] == 0 and not ref[0][0, P - 1].any()
    assert_fit_equal(launch_fit(hip, dev, dt, label, frame_of, want, dh, tau, shift), ref, "%d x %d P %d" % (h, w, P))
    # without a label: no segment, nothing explained, the other counters as before
    bare = launch_fit(hip, dev, dt, None, frame_of, None, dh, tau, shift)
    assert_fit_equal(bare, V.fit_counts(dt, None, frame_of, None, dh, tau), "no label")
    assert not bare[1].any() and not bare[0][:, :, 5].any() and np.array_equal(bare[0][:, :, :5], ref[0][:, :, :5])


def test_special_depth_values_on_both_sides(hip, dev):
    """Every pair of 0, 1, 32767, 32768, 40000 and 65535 as (test, hypothesis) depth, with tau = 0, 1 and 65535."""
    t, d = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    dt = t.astype(np.uint16)[None]
    dh = np.repeat(d.astype(np.uint16)[None, None], 3, axis=0)
    label = np.ones((1, 6, 6), np.uint8)
    tau = np.array([0, 1, 65535], np.int32)
    ref = V.fit_counts(dt, label, [0, 0, 0], [1, 1, 1], dh, tau)
    assert ref[0][:, 0].tolist() == [[30, 5, 10, 10, 5, 5], [30, 7, 9, 9, 5, 7], [30, 25, 0, 0, 5, 25]]
    assert_fit_equal(launch_fit(hip, dev, dt, label, np.zeros(3, np.int32), np.ones(3, np.int32), dh, tau), ref, "special")


def test_samples_do_not_depend_on_the_batch_or_the_run(hip, dev):
    dt, label, frame_of, want, dh, tau = _case(45, 70, 3, 7)
    full = launch_fit(hip, dev, dt, label, frame_of, want, dh, tau)
    for b in range(len(frame_of)):
        alone = launch_fit(hip, dev, dt, label, frame_of[b:b + 1], want[b:b + 1], dh[b:b + 1], tau[b:b + 1])
        for g, a in zip(full, alone):
            assert np.array_equal(a[0], g[b]), b
    again = launch_fit(hip, dev, dt, label, frame_of, want, dh, tau)
    for g, a in zip(full, again):
        assert np.array_equal(a.view(np.uint8), g.view(np.uint8))


def test_frame_outside_the_frames_gives_zero_counts(hip, dev):
    dt, label, frame_of, want, dh, tau = _case(45, 70, 3, 7)
    full = launch_fit(hip, dev, dt, label, frame_of, want, dh, tau)
    got = launch_fit(hip, dev, dt, label, np.array([1, 2, -1, 1], np.int32), want, dh, tau)      # (the guards are checked)
    for g, f in zip(got, full):
        assert np.array_equal(g[0], f[0]) and np.array_equal(g[3], f[3]) and not g[1:3].any()


def test_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    H, W, B, P = 45, 70, 2, 2
    dt, lab = _d(np.full((1, H, W), 1000), np.int16, dev), _d(np.ones((1, H, W)), np.uint8, dev)
    dh = _d(np.full((B, P, H, W), 1001), np.int16, dev)
    fo, want, tau = _d([0, 0], np.int32, dev), _d([1, 1], np.int32, dev), _d([1, 0], np.int32, dev)
    counts, seg, asum = Guarded(B * P, 6, torch.int32, dev), Guarded(B, 1, torch.int32, dev), Guarded(B, P, torch.int64, dev)

    def call(h=H, w=W, b=B, p=P, f=1, out=counts.ptr(), sg=seg.ptr(), sm=asum.ptr(), wn=want.data_ptr(), t=tau.data_ptr()):
        return L.cloudaae_depth_fit_counts(f, h, w, dt.data_ptr(), lab.data_ptr(), b, p, fo.data_ptr(), wn, dh.data_ptr(), t,
                                           out, sg, sm, hip.stream())
    assert call(f=0) != 0
    assert b"cloudaae_depth_fit_counts" in L.cloudaae_last_error()
    assert call(h=4097, w=4096) != 0                                          # h w above 2^24
    assert call(h=4096, w=4096, b=5, p=4) != 0 and call(b=1 << 20, p=1 << 20) != 0      # b p h w above 2^28
    assert call(out=None) != 0 and call(sg=None) != 0 and call(sm=None) != 0 and call(b=0) != 0 and call(p=0) != 0
    assert call(wn=None) != 0 and call(t=None) != 0 and call(h=0) != 0 and call(w=0) != 0
    torch.cuda.synchronize()
    for buf in (counts, seg, asum):
        assert np.all(buf.numpy().view(np.uint8) == FILL)              # nothing was written, guards included
    assert call() == 0
    torch.cuda.synchronize()
    n = H * W
    assert counts.numpy().tolist() == [[n, n, 0, 0, 0, n]] * 2 + [[n, 0, 0, n, 0, 0]] * 2
    assert seg.numpy().ravel().tolist() == [n, n] and asum.numpy().tolist() == [[n, n], [0, 0]]

    pose = _d(np.tile(np.eye(4).reshape(16), (B, P, 1)), np.float64, dev)
    valid = _d(np.ones((B, P)), np.int32, dev)
    best, score = Guarded(B, 1, torch.int32, dev), Guarded(B, P, torch.float64, dev)
    pb, margin = Guarded(B, 16, torch.float64, dev), Guarded(B, 1, torch.float64, dev)

    def sel(b=B, p=P, mode=0, c=counts.ptr(), out=best.ptr(), v=valid.data_ptr()):
        return L.cloudaae_select_pose(b, p, c, seg.ptr(), v, pose.data_ptr(), mode, out, score.ptr(), pb.ptr(), margin.ptr(),
                                      hip.stream())
    assert sel(mode=2) != 0
    assert b"cloudaae_select_pose" in L.cloudaae_last_error()
    assert sel(mode=-1) != 0 and sel(b=0) != 0 and sel(p=0) != 0 and sel(b=1 << 20, p=1 << 20) != 0
    assert sel(c=None) != 0 and sel(out=None) != 0 and sel(v=None) != 0
    cls, index = _d([0, 0], np.int64, dev), _d([0, 1], np.int32, dev)
    hyp = _d(np.eye(4).reshape(1, 16), np.float64, dev)
    rot, trans = Guarded(B * P, 3, torch.float64, dev), Guarded(B * P, 3, torch.float32, dev)
    ok, out = Guarded(B, P, torch.int32, dev), Guarded(B * P, 16, torch.float64, dev)

    def comp(b=B, p=P, nclass=1, n_total=1, h=hyp.data_ptr(), o=out.ptr(), v=ok.ptr()):
        return L.cloudaae_pose_compose(b, pose.data_ptr(), cls.data_ptr(), nclass, index.data_ptr(), n_total, h, p, o, rot.ptr(),
                                       trans.ptr(), v, hip.stream())
    assert comp(b=0) != 0
    assert b"cloudaae_pose_compose" in L.cloudaae_last_error()
    assert comp(p=0) != 0 and comp(nclass=0) != 0 and comp(n_total=-1) != 0 and comp(h=None) != 0 and comp(o=None) != 0
    assert comp(v=None) != 0 and comp(b=1 << 20, p=1 << 20) != 0
    torch.cuda.synchronize()
    for buf in (best, score, pb, margin, rot, trans, ok, out):
        assert np.all(buf.numpy().view(np.uint8) == FILL)
    assert sel() == 0 and comp() == 0
    torch.cuda.synchronize()
    assert best.numpy().ravel().tolist() == [0, 0] and score.numpy().tolist() == [[1.0, 1.0], [0.0, 0.0]]
    assert ok.numpy().tolist() == [[1, 0], [1, 0]] and not rot.numpy().any()


# ---- cloudaae_pose_compose ----------------------------------------------------------------------------------------------------
def test_compose_equals_the_restatement(hip, dev):
    """Classes 0 (the four flips of a box sample), 1 (two members), 2 (no set) of a table of three, and class ids 5 and -1
    outside it; P = 5 asks past every set's end.  A base of a quarter turn makes hypotheses whose angle is pi exactly."""
    from cloudaae_amd.utils import pose_verify as PV
    rng = np.random.default_rng(32)
    pts = rng.random((400, 3)) * [0.05, 0.11, 0.23] + [0.01, -0.02, 0.03]
    flips = PV.flip_hypotheses(pts)
    other = np.stack([np.eye(4), R.pose_matrix([0.3, -1.2, 0.4], [0.01, 0.02, -0.03])])
    table = PV.HypothesisTable.from_sets({0: flips, 1: other}, num_class=3)
    cls = np.array([0, 1, 2, 5, -1, 0, 0], np.int64)
    base = np.stack([R.pose_matrix(rng.standard_normal(3) * s, rng.standard_normal(3) * 0.3 + [0, 0, 0.8])
                     for s in (0.5, 1.0, 2.0, 0.1, 1.5, 0.0, 1.0)])
    base[6] = R.pose_matrix([0.0, 0.0, np.pi / 2], [0.1, 0.2, 0.9])
    B, P = len(cls), 5
    want_pose, want_trans, want_valid = V.compose(base, cls, table.index, table.hyp, P)
    assert want_valid.tolist() == [[1, 1, 1, 1, 0], [1, 1, 0, 0, 0]] + [[0] * 5] * 3 + [[1, 1, 1, 1, 0]] * 2
    got = PV.compose(_d(base, np.float64, dev), _d(cls, np.int64, dev), table, p=P)
    pose = got['pose'].cpu().numpy()
    assert pose.dtype == np.float64 and pose.shape == (B, P, 4, 4)
    assert np.array_equal(pose.view(np.uint64), want_pose.view(np.uint64))
    assert np.array_equal(got['valid'].cpu().numpy(), want_valid) and got['valid'].dtype == torch.int32
    trans = got['trans'].cpu().numpy()
    assert trans.dtype == np.float32 and np.array_equal(trans, want_trans)
    rot = got['rot_axag'].cpu().numpy()
    angle = np.sqrt((rot * rot).sum(axis=2))
    assert angle.max() <= np.pi + 1e-15
    worst = 0.0
    for b in range(B):
        for j in range(P):
            worst = max(worst, np.abs(R.pose_matrix(rot[b, j], [0, 0, 0])[:3, :3] - want_pose[b, j, :3, :3]).max())
    print("compose: rodrigues(rot_axag) against the composed rotation, worst %.3g; largest angle %.17g" % (worst, angle.max()))
    assert worst <= 1e-12
    # past the end and outside the table: hypothesis 0 again
    assert np.array_equal(pose[0, 4], pose[0, 0]) and np.array_equal(pose[1, 3], pose[1, 0]) and np.array_equal(pose[3, 2], pose[3, 0])
    assert np.abs(pose[3, 0] - base[3]).max() == 0.0
    # the default P is the largest set's
    assert tuple(PV.compose(_d(base, np.float64, dev), _d(cls, np.int64, dev), table)['pose'].shape) == (B, 4, 4, 4)


# ---- cloudaae_select_pose -----------------------------------------------------------------------------------------------------
def _counts(rows):
    """rows [B][P] of (consistent, in_front, behind, explained) -> [B,P,6]."""
    c = np.zeros((len(rows), len(rows[0]), 6), np.int32)
    for b, row in enumerate(rows):
        for j, (cons, front, behind, expl) in enumerate(row):
            c[b, j] = [cons + front + behind, cons, front, behind, 0, expl]
    return c


@pytest.mark.parametrize("mode", [0, 1])
def test_select_equals_the_restatement(hip, dev, mode):
    from cloudaae_amd.utils import pose_verify as PV
    big, a, b = 9999998, ((1 << 24) - 1, (1 << 25) - 1), ((1 << 24) - 2, (1 << 25) - 3)
    if mode == 0:
        # (consistent, in_front, behind, explained) with seg_total below: num = explained, den = seg_total + in_front
        rows = [[(0, 0, 0, 5), (0, 2, 0, 6), (0, 0, 0, 4), (0, 0, 0, 5)],              # 5/10 = 6/12 = 5/10: index 0
                [(0, 0, 0, 4), (0, 2, 0, 6), (0, 0, 0, 5), (0, 0, 0, 5)],              # 6/12 = 5/10 = 5/10: index 1
                [(0, 0, 0, 1), (0, big - 3, 0, 3333333), (0, 0, 0, 0), (0, 0, 0, 0)],   # 1/3 < 3333333/9999998
                [(0, big - 3, 0, 3333333), (0, 0, 0, 1), (0, 0, 0, 1), (0, 0, 0, 0)],
                [(0, b[1] - 100, 0, b[0]), (0, a[1] - 100, 0, a[0]), (0, 0, 0, 0), (0, b[1] - 100, 0, b[0])],
                [(0, 0, 0, 0)] * 4,                                                    # den = 0: all scores 0
                [(0, 0, 0, 9), (0, 0, 0, 3), (0, 0, 0, 8), (0, 0, 0, 1)],              # the best is invalid
                [(0, 5, 0, 0), (0, 0, 0, 0), (0, 1, 0, 1), (0, 3, 0, 1)]]              # 0/5, 0/0, 1/1, 1/3
        seg_total = np.array([10, 10, 3, 3, 100, 0, 10, 0], np.int32)
    else:
        rows = [[(3, 1, 0, 0), (6, 1, 1, 0), (0, 0, 0, 0), (1, 0, 3, 0)],              # 3/4 = 6/8: index 0
                [(1, 0, 3, 0), (0, 0, 0, 0), (6, 1, 1, 0), (3, 1, 0, 0)],              # index 2
                [(1, 1, 1, 7), (3333333, big - 3333333, 0, 0), (0, 9, 9, 0), (1, 2, 0, 0)],
                [(3333333, 3333332, 3333333, 0), (1, 1, 1, 0), (1, 0, 2, 0), (0, 0, 0, 0)],
                [(b[0], b[1] - b[0], 0, 0), (a[0], 0, a[1] - a[0], 0), (0, 0, 0, 0), (b[0], 0, b[1] - b[0], 0)],
                [(0, 0, 0, 0)] * 4,
                [(9, 0, 1, 0), (3, 3, 3, 0), (8, 1, 1, 0), (1, 5, 5, 0)],
                [(0, 5, 0, 0), (0, 0, 0, 0), (2, 0, 0, 0), (2, 1, 0, 0)]]
        seg_total = np.array([0, 5, 1, 0, 7, 0, 3, 0], np.int32)
    counts = _counts(rows)
    B, P = counts.shape[:2]
    valid = np.ones((B, P), np.int32)
    valid[6, 0] = 0
    pose = np.random.default_rng(5).standard_normal((B, P, 4, 4))
    want = V.select(counts, seg_total, valid, pose, mode)
    print("mode %d: best %s margin %s" % (mode, want[0].tolist(), want[3].tolist()))
    assert want[0].tolist() == [0, 1 if mode == 0 else 2, 1, 0, 1, 0, 2, 2]
    assert want[3][0] == 0.0 and want[3][5] == 0.0 and want[3][2] > 0.0 and want[3][4] >= 0.0
    got = PV.select(_d(counts, np.int32, dev), _d(seg_total, np.int32, dev), _d(valid, np.int32, dev), _d(pose, np.float64, dev), mode)
    assert got['best'].dtype == torch.int32 and np.array_equal(got['best'].cpu().numpy(), want[0])
    assert np.array_equal(got['score'].cpu().numpy().view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(got['pose_best'].cpu().numpy().view(np.uint64), want[2].view(np.uint64))
    assert np.array_equal(got['margin'].cpu().numpy().view(np.uint64), want[3].view(np.uint64))
    # one hypothesis: it wins, margin 0; valid=None means all valid
    one = PV.select(_d(counts[:, :1], np.int32, dev), _d(seg_total, np.int32, dev), None, _d(pose[:, :1], np.float64, dev), mode)
    w1 = V.select(counts[:, :1], seg_total, np.ones((B, 1), np.int32), pose[:, :1], mode)
    assert not one['best'].any() and not one['margin'].any() and np.array_equal(one['score'].cpu().numpy(), w1[1])
    assert np.array_equal(one['pose_best'].cpu().numpy(), pose[:, 0])


# ---- through the renderer ---------------------------------------------------------------------------------------------------------
def test_verify_poses_picks_the_ground_truth_as_the_restatement_does(hip, dev):
    from cloudaae_amd.utils import pose_verify as PV
    s = V.scene()
    want = V.verify(s['meshes'], [0], s['poses'], s['depth'], s['label'], [1], s['intr'], [0])
    depth, label = _d(s['depth'].view(np.int16), np.int16, dev), _d(s['label'], np.uint8, dev)
    got = PV.verify_poses(s['meshes'], [0], _d(s['poses'], np.float64, dev), depth, label, [1], s['intr'], [0])
    print("counts %s score %s margin %s" % (got['counts'].tolist(), got['score'].tolist(), got['margin'].tolist()))
    for k in ('counts', 'seg_total', 'abs_sum', 'best'):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert got['counts'].dtype == torch.int32 and got['abs_sum'].dtype == torch.int64
    for k in ('score', 'margin', 'pose_best'):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint64), want[k].view(np.uint64)), k
    assert got['best'].tolist() == [2] and float(got['margin'][0]) >= 0.1
    assert np.array_equal(got['dropped'], want['dropped']) and not got['dropped'].any()
    # the silhouette rule without a label; two samples in launches of one, the second with another order and tau
    w1 = V.verify(s['meshes'], [0, 0], np.concatenate([s['poses'], s['poses'][:, ::-1]]), np.repeat(s['depth'], 2, 0), None, None,
                  np.repeat(s['intr'], 2, 0), [1, 0], tau=[0.01, 0.002], mode=1)
    g1 = PV.verify_poses(s['meshes'], [0, 0], _d(np.concatenate([s['poses'], s['poses'][:, ::-1]]), np.float64, dev),
                         depth.repeat(2, 1, 1), None, None, np.repeat(s['intr'], 2, 0), [1, 0], tau=[0.01, 0.002], mode=1,
                         samples_per_launch=1)
    for k in ('counts', 'seg_total', 'abs_sum', 'best'):
        assert np.array_equal(g1[k].cpu().numpy(), w1[k]), k
    assert g1['best'].tolist() == [2, 1] and np.array_equal(g1['score'].cpu().numpy(), w1['score'])
    with pytest.raises(ValueError, match="label"):
        PV.verify_poses(s['meshes'], [0], _d(s['poses'], np.float64, dev), depth, None, None, s['intr'], [0])


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def records(hip, dev, tmp_path_factory):
    """Two made-up meshes in millimetres -- class 0 the L prism of the restatement's scene at one and a half times its
    size, class 1 a plate of 24 x 24 x 3 cm -- and four rendered frames of 160 x 120 with both, as
    tests/test_26_bop_score_gpu.py builds them; the element of class 0 with its frames and labels, and a randomly
    initialised graph."""
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import render
    tmp = tmp_path_factory.mktemp("verify")
    os.makedirs(str(tmp / "meshes"))
    lv, lt = V.l_prism()
    cv, ct, _ = MR.cube()
    _write_ply(str(tmp / "meshes" / "obj_000001.ply"), lv * np.float32(1500.0), lt)
    _write_ply(str(tmp / "meshes" / "obj_000002.ply"), (cv - np.float32(0.5)) * np.array([240.0, 240.0, 30.0], np.float32), ct)
    render.main(["--meshes", str(tmp / "meshes"), "--out", str(tmp / "data"), "--frames", "4", "--objects", "2", "--seq", "48",
                 "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    path = str(tmp / "data" / "0048_pcnn.tfrecord")
    files = mm.mesh_files(str(tmp / "meshes"))
    models = mm.models_from_meshes(files, scale=0.001, oversample=2, device=dev)
    packed = mm.pack_meshes(files, 0.001, dev)
    frames = tfrecord_io.read_frames(path, verify=True)
    N = 128
    el = E.element_from_frames(frames, 0, N, models, seed=4, device=dev, keep_frames=True, keep_labels=True)
    assert el is not None
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": len(el['class_id'])})
    return dict(tmp=tmp, path=path, models=models, packed=packed, frames=frames, el=el, graph=graph, N=N)


def test_keep_labels_adds_the_label_and_the_wanted_value(hip, dev, records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    frames, models, N, el = records['frames'], records['models'], records['N'], records['el']
    plain = E.element_from_frames(frames, 0, N, models, seed=4, device=dev)
    kept = E.element_from_frames(frames, 0, N, models, seed=4, device=dev, keep_frames=True)
    assert set(kept) - set(plain) == {"frame_depth", "frame_intrinsics"}           # keep_frames alone: its two keys
    assert set(el) - set(kept) == {"frame_label", "frame_want"}
    for k, v in kept.items():
        assert (torch.equal(v, el[k]) if isinstance(v, torch.Tensor) else np.array_equal(v, el[k])), k
    B = len(el['class_id'])
    assert el['frame_label'].dtype == torch.uint8 and tuple(el['frame_label'].shape) == (B, 120, 160)
    assert el['frame_want'].dtype == torch.int32 and el['frame_want'].tolist() == [1] * B
    for b, f in enumerate(el['frame_id']):
        assert np.array_equal(el['frame_label'][b].cpu().numpy(), frames[int(f)]['label'])
        assert (frames[int(f)]['label'] == 1).sum() >= N


def test_evaluate_batch_verifies_the_hypotheses(hip, dev, records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import pose_score
    from cloudaae_amd.utils import pose_verify as PV
    el, graph, packed, models = records['el'], records['graph'], records['packed'], records['models']
    tensors = {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}
    B = len(el['class_id'])
    flips = PV.flip_hypotheses(models[0])
    table = PV.HypothesisTable.from_models(models[:1], classes=[0], num_class=2)
    assert np.array_equal(table.members(0), flips) and not np.allclose(flips[1], flips[2])
    verify = dict(meshes=packed, mesh_index=None, hypotheses=table, tau=0.01, mode=0)
    base = E.evaluate_batch(graph, tensors, icp=True, score=True)
    out = E.evaluate_batch(graph, tensors, icp=True, score=True, verify=verify)
    new = set(out) - set(base)
    assert new == {"verify_best", "verify_score", "verify_margin", "verify_counts", "verify_candidates", "transformation_ver",
                   "rot_ver", "trans_ver", "trans_loss_ver", "trans_loss_perSample_ver", "axag_loss_ver",
                   "axag_loss_perSample_ver", "add_ver", "adds_ver"}, new
    for k, v in base.items():                                         # the other outputs are what they were
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, out[k]), k
    cand = out['verify_candidates']
    assert tuple(cand.shape) == (B, 4, 4, 4) and tuple(out['verify_counts'].shape) == (B, 4, 6)
    assert torch.equal(cand[:, 0], out['transformation_icp'])         # candidate 0 is the refined prediction, bit for bit
    best = out['verify_best'].to(torch.int64)
    print("icp: best %s margin %s score %s" % (best.tolist(), out['verify_margin'].tolist(), out['verify_score'].tolist()))
    assert torch.equal(out['transformation_ver'], cand[torch.arange(B, device=dev), best])
    assert tuple(out['rot_ver'].shape) == (B, 3) and out['rot_ver'].dtype == torch.float64 and out['trans_ver'].dtype == torch.float32
    for b in range(B):
        T = out['transformation_ver'][b].cpu().numpy()
        assert np.abs(R.pose_matrix(out['rot_ver'][b].cpu().numpy(), [0, 0, 0])[:3, :3] - T[:3, :3]).max() <= 1e-12
        assert np.array_equal(out['trans_ver'][b].cpu().numpy(), T[:3, 3].astype(np.float32))
    assert torch.isfinite(out['add_ver']).all() and tuple(out['add_ver'].shape) == (B,)
    sel = (best == 0)
    assert torch.equal(out['add_ver'][sel], out['add_icp'][sel]) and torch.equal(out['trans_loss_perSample_ver'][sel],
                                                                                  out['trans_loss_perSample_icp'][sel])
    # without an ICP the candidates are the composed poses; verify=None stays what it was
    plain = E.evaluate_batch(graph, tensors)
    ver = E.evaluate_batch(graph, tensors, verify=verify)
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, ver[k]), k
    pred = pose_score.pose_matrix(ver['rot_pred'].contiguous(), ver['trans_pred'].contiguous())
    want_pose, _, want_valid = V.compose(pred.cpu().numpy(), el['class_id'].cpu().numpy(), table.index, table.hyp, 4)
    assert np.array_equal(ver['verify_candidates'].cpu().numpy().view(np.uint64), want_pose.view(np.uint64)) and want_valid.all()
    assert 'add_ver' not in ver and 'transformation_icp' not in ver
    # the record's ground truth as the base, the identity third in the caller's set: it wins everywhere
    gt = pose_score.pose_matrix(el['axisangle'], el['translation'])
    moved = PV.HypothesisTable.from_sets({0: flips[[1, 3, 0, 2]]}, num_class=2, identity_first=False)
    for icp in (None, True):
        r = E.evaluate_batch(graph, tensors, icp=icp, verify=dict(verify, hypotheses=moved, base=gt))
        print("ground truth third (icp %s): best %s score %s margin %s" % (icp, r['verify_best'].tolist(),
                                                                           r['verify_score'].tolist(), r['verify_margin'].tolist()))
        assert r['verify_best'].tolist() == [2] * B
    assert (r['verify_margin'] > 0).all()
    # the silhouette rule needs no label
    bare = {k: v for k, v in tensors.items() if k not in ('frame_label', 'frame_want')}
    r1 = E.evaluate_batch(graph, bare, verify=dict(verify, hypotheses=moved, base=gt, mode=1))
    assert tuple(r1['verify_best'].shape) == (B,) and torch.equal(r1['verify_counts'][:, :, :5], E.evaluate_batch(
        graph, tensors, verify=dict(verify, hypotheses=moved, base=gt))['verify_counts'][:, :, :5])
    with pytest.raises(ValueError, match="frame_label"):
        E.evaluate_batch(graph, bare, verify=verify)
    with pytest.raises(ValueError, match="replay"):
        E.evaluate_batch(graph, tensors, replay=True, verify=verify)
    with pytest.raises(ValueError, match="hypotheses"):
        E.evaluate_batch(graph, tensors, verify=dict(meshes=packed))


def test_command_line_prints_the_verify_line(hip, dev, records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    tmp, path = records['tmp'], records['path']
    obj = str(tmp / "obj_models.tfrecords")
    mm.main(["--meshes", str(tmp / "meshes"), "--out", obj, "--scale", "0.001", "--oversample", "2"])
    graph = T.TrainGraph({"num_point": 128, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    common = ["--files", path, "--object_model", obj, "--trained_model", ckpt[:-len(".npz")], "--target_cls", "0",
              "--num_point", "128", "--batch_size", "1"]
    capsys.readouterr()
    assert E.main(common + ["--verify", "--icp", "--score", "--meshes", str(tmp / "meshes"), "--mesh_scale", "0.001"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    n = int([ln for ln in lines if ln.startswith("batch size ")][0].split()[-1])
    ver = [ln for ln in lines if ln.startswith("verify ")]
    assert n >= 1 and len(ver) == 1, lines[-8:]
    tok = ver[0].split()
    assert tok[:4] == ["verify", "class", "0", "n"] and int(tok[4]) == n
    assert [tok[i] for i in (5, 7, 9, 11, 13)] == ["kept0", "chose1", "chose2", "chose3", "mean_margin"]
    assert sum(int(tok[i]) for i in (6, 8, 10, 12)) == n and float(tok[14]) >= 0.0
    assert lines[-1] == ver[0]                                            # after the existing summaries
    assert any(" trans_loss_ver " in ln for ln in lines if ln.startswith("Validation batch "))
    assert [ln.split()[3] for ln in lines if ln.startswith("score class 0 ") and " add " in ln] == ["pred", "icp", "ver"]
    with pytest.raises(SystemExit) as err:
        E.main(common + ["--verify"])
    assert err.value.code == 2 and "--meshes" in capsys.readouterr().err
