"""GPU: cloudaae_depth_fit_counts_window and cloudaae_detect_assign through the C ABI against the NumPy restatement of
DESIGN.md "Detections" (tests/detect_reference.py), then utils/detect.py through the renderer, the proposals and the
evaluation.

Every count is an integer and is compared for equality, no pixel left out; the winner of every comparison is exact; the
doubles are single divisions or copies and are compared bit for bit.  Outputs sit between guard rows that are filled with a
byte pattern, so every call starts on garbage (as in tests/test_32_pose_verify_gpu.py)."""

import numpy as np
import pytest
import torch

import detect_reference as DR
import pose_verify_reference as V

pytestmark = pytest.mark.gpu

GUARD = 4                  # rows kept before and after every output
FILL = 0xA5
SPECIAL = np.array([0, 1, 32767, 32768, 65535])


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side."""

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
    """The array on the device, its first element `shift` elements past an allocation's start."""
    flat = np.ascontiguousarray(a, ty).reshape(-1)
    buf = torch.zeros((len(flat) + shift,), dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
    assert buf.data_ptr() % 256 == 0
    buf[shift:] = torch.from_numpy(flat).to(dev)
    return buf[shift:]


def _image(rng, *shape):
    """Depths around 1000 units with zeros and the values a signed or a narrow read would get wrong."""
    d = rng.integers(990, 1011, shape)
    d = np.where(rng.random(shape) < 0.25, 0, d)
    return np.where(rng.random(shape) < 0.2, SPECIAL[rng.integers(0, len(SPECIAL), shape)], d).astype(np.uint16)


# ---- cloudaae_depth_fit_counts_window -------------------------------------------------------------------------------------------
def launch_window(hip, dev, dt, label, frame_of, want, origin, dh, tau, shift=0):
    """On guarded outputs -> (counts [B,P,6], seg_total [B], abs_sum [B,P]) as the restatement's."""
    F, h, w = dt.shape
    B, P, wh, ww = dh.shape
    g = [_shifted(dt.view(np.int16), np.int16, dev, shift), _shifted(dh.view(np.int16), np.int16, dev, shift),
         None if label is None else _shifted(label, np.uint8, dev, shift), _d(frame_of, np.int32, dev),
         None if want is None else _d(want, np.int32, dev), _d(tau, np.int32, dev), _d(origin, np.int32, dev)]
    if shift:
        assert g[0].data_ptr() % 16 == 2 * shift and g[1].data_ptr() % 16 == 2 * shift
    counts, seg, asum = Guarded(B * P, 6, torch.int32, dev), Guarded(B, 1, torch.int32, dev), Guarded(B, P, torch.int64, dev)
    hip.check(hip.lib().cloudaae_depth_fit_counts_window(
        F, h, w, g[0].data_ptr(), None if label is None else g[2].data_ptr(), B, P, g[3].data_ptr(),
        None if want is None else g[4].data_ptr(), g[6].data_ptr(), wh, ww, g[1].data_ptr(), g[5].data_ptr(), counts.ptr(),
        seg.ptr(), asum.ptr(), hip.stream()), "cloudaae_depth_fit_counts_window")
    torch.cuda.synchronize()
    return counts.numpy().reshape(B, P, 6).copy(), seg.numpy().ravel().copy(), asum.numpy().copy()


def launch_full(hip, dev, dt, label, frame_of, want, dh, tau, shift=0):
    """The existing cloudaae_depth_fit_counts on the same data."""
    F, h, w = dt.shape
    B, P = dh.shape[:2]
    g = [_shifted(dt.view(np.int16), np.int16, dev, shift), _shifted(dh.view(np.int16), np.int16, dev, shift),
         None if label is None else _shifted(label, np.uint8, dev, shift), _d(frame_of, np.int32, dev),
         None if want is None else _d(want, np.int32, dev), _d(tau, np.int32, dev)]
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


# 48 x 64: aligned rows, every lane on the 16-byte path at shift 0; 45 x 70: rows of 140 bytes, so a lane's eight pixels
# straddle rows and few addresses are aligned; P = 1, 8, 9 and 17: a chunk of hypotheses, one more, a third chunk of one.
@pytest.mark.parametrize("h,w,P,shift", [(48, 64, 1, 0), (48, 64, 8, 1), (45, 70, 9, 0), (45, 70, 17, 3)])
def test_the_whole_frame_as_window_equals_the_full_frame_kernel(hip, dev, h, w, P, shift):
    rng = np.random.default_rng(1000 * h + 10 * P + shift)
    F, B = 2, 4
    dt, dh = _image(rng, F, h, w), _image(rng, B, P, h, w)
    dh[0, P - 1] = 0
    label = rng.integers(0, 3, (F, h, w)).astype(np.uint8)
    frame_of, want = np.array([1, 0, 1, 1], np.int32), np.array([1, 2, 1, 9], np.int32)
    tau, origin = np.array([0, 65535, 7, 3], np.int32), np.zeros((B, 2), np.int32)
    ref = V.fit_counts(dt, label, frame_of, want, dh, tau)
    assert ref[0][2, 0].min() > 0 and ref[1][:3].min() > 0 and ref[1][3] == 0          # every counter is exercised
    full = launch_full(hip, dev, dt, label, frame_of, want, dh, tau, shift)
    assert_fit_equal(full, ref, "full frame")
    assert_fit_equal(launch_window(hip, dev, dt, label, frame_of, want, origin, dh, tau, shift), full, "%d x %d P %d" % (h, w, P))
    bare = launch_window(hip, dev, dt, None, frame_of, None, origin, dh, tau, shift)
    assert_fit_equal(bare, launch_full(hip, dev, dt, None, frame_of, None, dh, tau, shift), "no label")
    assert not bare[1].any() and not bare[0][:, :, 5].any() and np.array_equal(bare[0][:, :, :5], full[0][:, :, :5])


# The origins: inside and aligned; inside and odd; over the left and the top border (negative, odd); over the right; over
# the bottom; over a corner; wholly outside on four sides; and a sample whose frame is none.
def _origins(H, W, wh, ww):
    return np.array([[8, 4], [3, 5], [-3, -1], [W - ww // 2 - 1, 7], [5, H - wh // 2 - 1], [W - 2, H - 1], [-ww, 3], [W, 0],
                     [2, -wh], [1, H], [-100000, 2000000000], [16, 8]], np.int32)


# ww = 8 and 24: whole lanes per row; 13: no multiple of 8, lanes straddle rows; 1: a column; 40 x 64 = 2560 pixels: more
# than one workgroup's run of 2048, the second one partly past the end.
@pytest.mark.parametrize("wh,ww,P,shift", [(9, 8, 3, 0), (7, 24, 9, 1), (5, 13, 8, 0), (11, 1, 1, 0), (40, 64, 17, 0),
                                           (6, 16, 2, 3)])
def test_windowed_counts_equal_the_restatement(hip, dev, wh, ww, P, shift):
    rng = np.random.default_rng(100 * wh + ww + shift)
    F, H, W = 2, 45, 72 if (wh, ww) == (6, 16) else 70
    dt = _image(rng, F, H, W)
    label = rng.integers(0, 3, (F, H, W)).astype(np.uint8)
    origin = _origins(H, W, wh, ww)
    B = len(origin)
    frame_of = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 2], np.int32)
    frame_of[-1] = [2, -1][shift % 2]
    want = np.array([1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 1], np.int32)
    tau = np.array([0, 65535, 7, 3, 1, 2, 5, 5, 5, 5, 5, 5], np.int32)
    dh = _image(rng, B, P, wh, ww)
    dh[1, P - 1] = 0
    ref = DR.fit_counts_window(dt, label, frame_of, want, origin, wh, ww, dh, tau)
    got = launch_window(hip, dev, dt, label, frame_of, want, origin, dh, tau, shift)
    assert_fit_equal(got, ref, "%d x %d P %d shift %d" % (wh, ww, P, shift))
    for b in (6, 7, 8, 9, 10):                     # wholly outside: what is rendered is unknown, nothing else
        c = got[0][b]
        assert np.array_equal(c[:, 0], c[:, 4]) and c[:, 0].min() > 0 and not c[:, [1, 2, 3, 5]].any() and got[1][b] == 0
    assert not got[0][11].any() and got[1][11] == 0 and not got[2][11].any()            # no frame: zero counts
    assert got[1][:5].min() > 0 or ww == 1                                                # the segments are not empty
    assert_fit_equal(launch_window(hip, dev, dt, None, frame_of, None, origin, dh, tau, shift),
                     DR.fit_counts_window(dt, None, frame_of, None, origin, wh, ww, dh, tau), "no label")
    # a sample does not depend on the batch it is in, nor on the run
    alone = launch_window(hip, dev, dt, label, frame_of[2:3], want[2:3], origin[2:3], dh[2:3], tau[2:3], shift)
    again = launch_window(hip, dev, dt, label, frame_of, want, origin, dh, tau, shift)
    for g, a, r in zip(got, alone, again):
        assert np.array_equal(a[0], g[2]) and np.array_equal(r.view(np.uint8), g.view(np.uint8))


def test_window_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    H, W, B, P, wh, ww = 45, 70, 2, 2, 6, 16
    dt, lab = _d(np.full((1, H, W), 1000), np.int16, dev), _d(np.ones((1, H, W)), np.uint8, dev)
    dh = _d(np.full((B, P, wh, ww), 1001), np.int16, dev)
    fo, want, tau = _d([0, 0], np.int32, dev), _d([1, 1], np.int32, dev), _d([1, 0], np.int32, dev)
    org = _d([[0, 0], [W - 8, H - 3]], np.int32, dev)
    counts, seg, asum = Guarded(B * P, 6, torch.int32, dev), Guarded(B, 1, torch.int32, dev), Guarded(B, P, torch.int64, dev)

    def call(h=H, w=W, b=B, p=P, f=1, y=wh, x=ww, out=counts.ptr(), sg=seg.ptr(), sm=asum.ptr(), wn=want.data_ptr(),
             t=tau.data_ptr(), o=org.data_ptr()):
        return L.cloudaae_depth_fit_counts_window(f, h, w, dt.data_ptr(), lab.data_ptr(), b, p, fo.data_ptr(), wn, o, y, x,
                                                  dh.data_ptr(), t, out, sg, sm, hip.stream())
    assert call(f=0) != 0
    assert b"cloudaae_depth_fit_counts_window" in L.cloudaae_last_error()
    assert call(h=4097, w=4096) != 0 and call(y=4097, x=4096) != 0                  # h w, wh ww above 2^24
    assert call(y=4096, x=4096, b=5, p=4) != 0 and call(b=1 << 20, p=1 << 20) != 0   # b p wh ww above 2^28
    assert call(out=None) != 0 and call(sg=None) != 0 and call(sm=None) != 0 and call(b=0) != 0 and call(p=0) != 0
    assert call(wn=None) != 0 and call(t=None) != 0 and call(o=None) != 0 and call(h=0) != 0 and call(w=0) != 0
    assert call(y=0) != 0 and call(x=0) != 0
    torch.cuda.synchronize()
    for buf in (counts, seg, asum):
        assert np.all(buf.numpy().view(np.uint8) == FILL)              # nothing was written, guards included
    assert call() == 0
    torch.cuda.synchronize()
    n, m = wh * ww, 3 * 8                                              # the second window keeps 3 rows of 8 columns
    assert counts.numpy().tolist() == [[n, n, 0, 0, 0, n]] * 2 + [[n, 0, 0, m, n - m, 0]] * 2
    assert seg.numpy().ravel().tolist() == [n, m] and asum.numpy().tolist() == [[n, n], [0, 0]]


# ---- cloudaae_detect_assign -------------------------------------------------------------------------------------------------------
ASSIGN_INT = ("pair_hyp", "pair_num", "pair_den", "det_class", "det_hyp", "det_num", "det_den", "det_rank", "alt_class",
              "alt_num", "alt_den", "n_det")
ASSIGN_F64 = ("pair_score", "det_score", "det_pose")


def launch_assign(hip, dev, counts, seg_total, valid, pose, n_components, mode, min_num, min_den, max_per_class):
    F, K, C, P = counts.shape[:4]
    rows = dict(pair_hyp=(F * K, C), pair_num=(F * K, C), pair_den=(F * K, C), pair_score=(F * K, C), det_pose=(F * K, 16),
                n_det=(F, 1))
    out = {k: Guarded(*rows.get(k, (F, K)), torch.float64 if k in ASSIGN_F64 else torch.int32, dev)
           for k in ASSIGN_INT + ASSIGN_F64}
    g = [_d(counts, np.int32, dev), _d(seg_total, np.int32, dev), _d(valid, np.int32, dev), _d(pose, np.float64, dev),
         _d(n_components, np.int32, dev)]
    hip.check(hip.lib().cloudaae_detect_assign(
        F, K, C, P, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), g[4].data_ptr(), mode, min_num, min_den,
        max_per_class, out["pair_hyp"].ptr(), out["pair_num"].ptr(), out["pair_den"].ptr(), out["pair_score"].ptr(),
        out["det_class"].ptr(), out["det_hyp"].ptr(), out["det_num"].ptr(), out["det_den"].ptr(), out["det_score"].ptr(),
        out["det_rank"].ptr(), out["det_pose"].ptr(), out["alt_class"].ptr(), out["alt_num"].ptr(), out["alt_den"].ptr(),
        out["n_det"].ptr(), hip.stream()), "cloudaae_detect_assign")
    torch.cuda.synchronize()
    return {k: v.numpy().copy() for k, v in out.items()}


def assert_assign_equal(got, want, what):
    bad = [k for k in ASSIGN_INT + ASSIGN_F64 if not np.array_equal(got[k].reshape(-1), want[k].reshape(-1))]
    print("%s: differing outputs %s" % (what, bad))
    for k in ASSIGN_INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k].reshape(want[k].shape), want[k]), (what, k)
    for k in ASSIGN_F64:
        assert np.array_equal(got[k].reshape(want[k].shape).view(np.uint64), want[k].view(np.uint64)), (what, k)


def _tiny_tables(rng, F, K, C, P):
    """explained 0..4, seg_total 1..4, in_front 0..2: fractions of tiny integers, so that ties occur at every level."""
    counts = np.zeros((F, K, C, P, 6), np.int32)
    counts[..., 5] = rng.integers(0, 5, (F, K, C, P))
    counts[..., 1] = counts[..., 5] + rng.integers(0, 2, (F, K, C, P))
    counts[..., 2] = rng.integers(0, 3, (F, K, C, P))
    counts[..., 3] = rng.integers(0, 2, (F, K, C, P))
    counts[..., 0] = counts[..., 1] + counts[..., 2] + counts[..., 3]
    return counts, rng.integers(1, 5, (F, K, C)).astype(np.int32), (rng.random((F, K, C, P)) < 0.85).astype(np.int32)


# thresholds 0 / 1 (everything with num > 0), 1 / 1 (met with equality or not at all) and 1 / 2, which 1 / 2 and 2 / 4 meet
# with equality; 200 tables of F = 3 frames in one launch
@pytest.mark.parametrize("mode,max_per_class,min_score", [(0, 1, (1, 2)), (0, 2, (0, 1)), (1, 1, (1, 1)), (1, 2, (1, 2)),
                                                          (0, 1, (1, 1)), (1, 1, (0, 1))])
def test_assignment_equals_the_restatement_on_tables_full_of_ties(hip, dev, mode, max_per_class, min_score):
    rng = np.random.default_rng(100 * mode + 10 * max_per_class + min_score[1])
    F, K, C, P = 3 * 200, 5, 4, 3
    counts, seg_total, valid = _tiny_tables(rng, F, K, C, P)
    n_components = rng.integers(0, K + 2, F).astype(np.int32) - (rng.random(F) < 0.05)      # -1 .. K + 1: clamped
    pose = rng.standard_normal((F, K, C, P, 4, 4))
    want = DR.assign(counts, seg_total, valid, pose, n_components, mode, min_score[0], min_score[1], max_per_class)
    num, den = want['pair_num'].astype(np.int64), want['pair_den'].astype(np.int64)
    if min_score[0] > 0:
        assert (num * min_score[1] == min_score[0] * den)[num > 0].any()         # a pair meets the threshold with equality
    assert (want['n_det'] == 0).any() and (want['n_det'] >= 2).any() and (n_components == 0).any() and (valid == 0).any()
    got = launch_assign(hip, dev, counts, seg_total, valid, pose, n_components, mode, min_score[0], min_score[1], max_per_class)
    assert_assign_equal(got, want, "mode %d cap %d threshold %s" % (mode, max_per_class, min_score))


def test_assignment_at_the_largest_table(hip, dev):
    rng = np.random.default_rng(254)
    F, K, C, P = 2, 254, 21, 4
    counts = np.zeros((F, K, C, P, 6), np.int32)
    counts[..., 5] = rng.integers(0, 40, (F, K, C, P))
    counts[..., 2] = rng.integers(0, 10, (F, K, C, P))
    seg_total = rng.integers(30, 50, (F, K, C)).astype(np.int32)
    valid = (rng.random((F, K, C, P)) < 0.9).astype(np.int32)
    pose = rng.standard_normal((F, K, C, P, 4, 4))
    n_components = np.array([254, 100], np.int32)
    want = DR.assign(counts, seg_total, valid, pose, n_components, 0, 1, 2, 12)
    print("n_det %s" % want['n_det'].tolist())
    assert want['n_det'][0] > 200 and want['n_det'][1] == 100
    assert_assign_equal(launch_assign(hip, dev, counts, seg_total, valid, pose, n_components, 0, 1, 2, 12), want, "254 x 21 x 4")


def test_assign_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    F, K, C, P = 1, 2, 2, 1
    counts = np.zeros((F, K, C, P, 6), np.int32)
    counts[0, :, :, 0, 5] = [[3, 1], [3, 2]]
    g = [_d(counts, np.int32, dev), _d(np.full((F, K, C), 4), np.int32, dev), _d(np.ones((F, K, C, P)), np.int32, dev),
         _d(np.tile(np.eye(4), (F, K, C, P, 1, 1)), np.float64, dev), _d([2], np.int32, dev)]
    rows = dict(pair_hyp=(F * K, C), pair_num=(F * K, C), pair_den=(F * K, C), pair_score=(F * K, C), det_pose=(F * K, 16),
                n_det=(F, 1))
    out = {k: Guarded(*rows.get(k, (F, K)), torch.float64 if k in ASSIGN_F64 else torch.int32, dev) for k in ASSIGN_INT + ASSIGN_F64}

    def call(f=F, k=K, c=C, p=P, mode=0, num=1, den=2, cap=1, first=g[0].data_ptr(), last=out["n_det"].ptr(), nc=g[4].data_ptr()):
        return L.cloudaae_detect_assign(f, k, c, p, first, g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), nc, mode, num, den,
                                        cap, out["pair_hyp"].ptr(), out["pair_num"].ptr(), out["pair_den"].ptr(),
                                        out["pair_score"].ptr(), out["det_class"].ptr(), out["det_hyp"].ptr(),
                                        out["det_num"].ptr(), out["det_den"].ptr(), out["det_score"].ptr(),
                                        out["det_rank"].ptr(), out["det_pose"].ptr(), out["alt_class"].ptr(),
                                        out["alt_num"].ptr(), out["alt_den"].ptr(), last, hip.stream())
    assert call(f=0) != 0
    assert b"cloudaae_detect_assign" in L.cloudaae_last_error()
    assert call(k=255) != 0 and call(c=257) != 0 and call(p=65) != 0 and call(k=0) != 0 and call(c=0) != 0 and call(p=0) != 0
    assert call(mode=2) != 0 and call(mode=-1) != 0 and call(num=-1) != 0 and call(num=3) != 0 and call(den=0) != 0
    assert call(num=0, den=(1 << 20) + 1) != 0 and call(cap=0) != 0 and call(f=1 << 16, k=254, c=256, p=64) != 0
    assert call(first=None) != 0 and call(last=None) != 0 and call(nc=None) != 0
    torch.cuda.synchronize()
    for buf in out.values():
        assert np.all(buf.numpy().view(np.uint8) == FILL)
    assert call() == 0
    torch.cuda.synchronize()
    # 3/4 ties between (0, 0) and (1, 0): component 0 takes class 0, component 1 is left with 2/4, which meets 1/2 exactly
    assert out["det_class"].numpy().tolist() == [[0, 1]] and out["det_rank"].numpy().tolist() == [[0, 1]]
    assert out["det_num"].numpy().tolist() == [[3, 2]] and out["alt_class"].numpy().tolist() == [[1, 0]]
    assert out["alt_num"].numpy().tolist() == [[1, 3]] and out["n_det"].numpy().tolist() == [[1 + 1]]


# ---- score_candidates on the host tests' scene ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(hip, dev):
    """The scene of tests/detect_reference.py, segmented on the GPU: the found label image and the table equal the
    restatement's (tests/test_37_depth_components_gpu.py checks the kernels; here it makes the two runs comparable)."""
    from cloudaae_amd.utils import depth_components as dc
    from cloudaae_amd.utils import mesh_models as mm
    s, g = DR.scene(), DR.scene_segments()
    seg = dc.segment_depth(s['depth'], s['intr'], device=dev, **DR.SCENE_SEGMENT)
    assert np.array_equal(seg.label.cpu().numpy(), g['label']) and seg.n_components.tolist() == [3]
    assert np.array_equal(seg.comp_box[0, :3], g['comp_box'][0, :3])
    depth = _d(s['depth'].view(np.int16), np.int16, dev)
    packed = mm.pack_meshes([m[:2] for m in s['meshes']], device=dev)
    return dict(s=s, g=g, seg=seg, depth=depth, packed=packed)


def test_score_candidates_equals_the_restatement_and_the_cpu_run(hip, dev, scene):
    from cloudaae_amd.utils import detect
    from cloudaae_amd.utils import pose_verify as PV
    s, g, seg = scene['s'], scene['g'], scene['seg']
    poses = DR.scene_hypotheses()
    F, K, C, P = poses.shape[:4]
    got = detect.score_candidates(seg, _d(poses, np.float64, dev), None, scene['packed'], [0, 1, 2, 3], s['intr'], scene['depth'],
                                  keep_depth=True)
    cpu = DR.scene_score()
    assert (got['wh'], got['ww']) == (cpu['wh'], cpu['ww']) and np.array_equal(got['origin'], cpu['origin'])
    # the counts equal the restatement's on the windows the GPU rendered
    dh = got['depth_hyp'].cpu().numpy().view(np.uint16)
    print("rendered windows differ from the NumPy renderer's in %d pixels" % int((dh != cpu['depth_hyp']).sum()))
    ref = DR.score(g['label'], g['comp_box'], g['n_components'], poses, None, None, None, s['intr'], s['depth'], depth_hyp=dh)
    for k in ('counts', 'seg_total', 'abs_sum'):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    assert_assign_equal({k: got[k].cpu().numpy() for k in ASSIGN_INT + ASSIGN_F64}, ref, "scene")
    # the table equals the CPU run's class for class, and is what the device tensors hold
    t = got['table']
    assert np.array_equal(t['det_class'], cpu['det_class']) and t['det_class'][0].tolist() == g['object_of']
    assert np.array_equal(t['det_hyp'], cpu['det_hyp']) and t['n_det'].tolist() == [3]
    for k in ("det_class", "det_hyp", "det_num", "det_den", "det_rank", "alt_class", "alt_num", "alt_den", "n_det"):
        assert t[k].dtype == np.int32 and np.array_equal(t[k], got[k].cpu().numpy()), k
    for k in ("det_score", "det_pose"):
        assert np.array_equal(t[k].view(np.uint64), got[k].cpu().numpy().view(np.uint64)), k
    assert np.array_equal(got['dropped'], np.zeros((F, K, C, P), np.int32))
    # seg_total is the component's size where the window holds its box
    assert np.array_equal(got['seg_total'].cpu().numpy()[0], np.repeat(seg.comp_size[0, :3, None], C, axis=1))
    # the result does not depend on the chunking
    one = detect.score_candidates(seg, _d(poses, np.float64, dev), None, scene['packed'], [0, 1, 2, 3], s['intr'], scene['depth'],
                                  samples_per_launch=5)
    for k in ('counts', 'seg_total', 'abs_sum', 'det_class', 'det_pose'):
        assert torch.equal(one[k], got[k]), k
    # a window as large as the frame: the counts are verify_poses's
    H, W = s['depth'].shape[1:]
    whole = detect.score_candidates(seg, _d(poses, np.float64, dev), None, scene['packed'], [0, 1, 2, 3], s['intr'], scene['depth'],
                                    window=(np.zeros((F, K, 2), np.int32), H, W))
    v = PV.verify_poses(scene['packed'], np.tile([0, 1, 2, 3], K), _d(poses.reshape(K * C, P, 4, 4), np.float64, dev),
                        scene['depth'], seg.label, np.repeat(np.arange(K) + 1, C), s['intr'], np.zeros(K * C, np.int64))
    for k in ('counts', 'seg_total', 'abs_sum'):
        assert torch.equal(whole[k].reshape(v[k].shape), v[k]), k
    assert np.array_equal(whole['table']['det_class'], t['det_class'])


# ---- detect_objects ---------------------------------------------------------------------------------------------------------------
def test_detect_objects_feeds_each_stage_to_the_next_as_the_restatement_does(hip, dev, scene):
    from cloudaae_amd.utils import detect
    from cloudaae_amd.utils import ppf
    s, g = scene['s'], scene['g']
    models = ppf.PPFModels.from_meshes([m[:2] for m in s['meshes'][:4]], num_point=96, device=dev)
    kw = dict(num_point=96, top=2, seed=DR.SCENE_SEGMENT['seed'],
              components={k: v for k, v in DR.SCENE_SEGMENT.items() if k != 'seed'})
    d = detect.detect_objects(s['depth'], s['intr'], scene['packed'], models, first_frame=1, **kw)
    assert d.segments.n_components.tolist() == [3]
    F, K, C, P = d.poses.shape[:4]
    assert (F, K, C, P) == (1, 3, 4, 2) and d.skipped == 0
    valid = d.valid.cpu().numpy()
    print("valid proposals per (component, class): %s" % valid.sum(axis=3)[0].tolist())
    assert valid.any()                                                # the clouds gave proposals
    # the proposals and the found segments, fed to the restatement with the NumPy renderer, give the same table
    seg = d.segments
    ref = DR.score(seg.label.cpu().numpy(), seg.comp_box, seg.n_components, d.poses.cpu().numpy(), valid, s['meshes'],
                   [0, 1, 2, 3], s['intr'], s['depth'])
    for k in ('counts', 'seg_total'):
        assert np.array_equal(d.scores[k].cpu().numpy(), ref[k]), k
    assert_assign_equal({k: d.scores[k].cpu().numpy() for k in ASSIGN_INT + ASSIGN_F64}, ref, "detect_objects")
    print("det_class %s score %s alt_class %s" % (d.table['det_class'].tolist(), d.table['det_score'].tolist(),
                                                   d.table['alt_class'].tolist()))
    assert np.array_equal(d.table['det_class'], ref['det_class']) and np.array_equal(d.dropped, ref['dropped'])
    # neither the chunking nor the batch the frame arrives in changes it: the frame as the second of two
    other = np.ascontiguousarray(s['depth'][:, :, ::-1])
    both = detect.detect_objects(np.concatenate([other, s['depth']]), np.repeat(s['intr'], 2, 0), scene['packed'], models,
                                 first_frame=0, samples_per_launch=3, **kw)
    k2 = both.poses.shape[1]
    assert both.segments.n_components[1] == 3 and k2 >= 3
    assert torch.equal(both.poses[1, :3], d.poses[0]) and torch.equal(both.valid[1, :3], d.valid[0])
    for k in ("det_class", "det_hyp", "det_num", "det_den", "det_rank", "alt_class", "alt_num", "alt_den"):
        assert np.array_equal(both.table[k][1, :3], d.table[k][0]), k
    assert np.array_equal(both.table['det_pose'][1, :3].view(np.uint64), d.table['det_pose'][0].view(np.uint64))
    # given segments are used as they are
    again = detect.detect_objects(s['depth'], s['intr'], scene['packed'], models, first_frame=1, segments=d.segments, **kw)
    assert torch.equal(again.poses, d.poses) and np.array_equal(again.table['det_class'], d.table['det_class'])


def test_detect_objects_refines_every_candidate_in_one_icp_call(hip, dev, scene, monkeypatch):
    from cloudaae_amd.utils import detect
    from cloudaae_amd.utils import icp as icp_util
    from cloudaae_amd.utils import ppf
    s = scene['s']
    models = ppf.PPFModels.from_meshes([m[:2] for m in s['meshes'][:4]], num_point=96, device=dev)
    kw = dict(num_point=96, top=2, seed=DR.SCENE_SEGMENT['seed'], components={k: v for k, v in DR.SCENE_SEGMENT.items() if k != 'seed'})
    plain = detect.detect_objects(s['depth'], s['intr'], scene['packed'], models, **kw)
    calls = []
    real = icp_util.refine_pose_icp

    def spy(model_xyz, scene_xyz, rot, trans, **params):
        r = real(model_xyz, scene_xyz, rot, trans, **params)
        calls.append((tuple(model_xyz.shape), tuple(scene_xyz.shape), rot.clone(), trans.clone(), r['transformation'].clone()))
        return r
    monkeypatch.setattr(icp_util, "refine_pose_icp", spy)
    d = detect.detect_objects(s['depth'], s['intr'], scene['packed'], models, icp=dict(rounds=3), **kw)
    F, K, C, P = d.poses.shape[:4]
    assert len(calls) == 1 and calls[0][0] == (K * C * P, 96, 3) and calls[0][1] == (K * C * P, 96, 3)
    # it started from the proposals and its result is what was scored
    assert torch.equal(calls[0][4].view(F, K, C, P, 4, 4), d.poses) and torch.equal(d.valid, plain.valid)
    assert np.array_equal(calls[0][3].view(K, C, P, 3).cpu().numpy(), plain.poses[0, :, :, :, :3, 3].cpu().numpy().astype(np.float32))
    seg = d.segments
    ref = DR.score(seg.label.cpu().numpy(), seg.comp_box, seg.n_components, d.poses.cpu().numpy(), d.valid.cpu().numpy(), s['meshes'],
                   [0, 1, 2, 3], s['intr'], s['depth'])
    assert_assign_equal({k: d.scores[k].cpu().numpy() for k in ASSIGN_INT + ASSIGN_F64}, ref, "detect_objects with icp")
    print("with icp: det_class %s score %s; without: %s %s" % (d.table['det_class'].tolist(), d.table['det_score'].tolist(),
                                                              plain.table['det_class'].tolist(), plain.table['det_score'].tolist()))


# ---- the evaluation ---------------------------------------------------------------------------------------------------------------
N_POINT = 64
DETECT_CLASSES = [1, 2, 3, 4]   # the record's classes: 0 the table, 1 .. 3 the objects, 4 the sphere that no frame shows


def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def records(hip, dev, scene, tmp_path_factory):
    """The scene as a frame record file, its meshes as *.ply files in the record's class order (the table first), the
    detector built from those files as the command line builds it, and what detect_objects says about the frame."""
    import os
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import detect, mesh_models as mm, ppf, render
    s = scene['s']
    tmp = tmp_path_factory.mktemp("detect")
    os.makedirs(str(tmp / "meshes"))
    for i, m in enumerate([s['meshes'][4]] + s['meshes'][:4]):
        _write_ply(str(tmp / "meshes" / ("obj_%06d.ply" % (i + 1))), m[0], m[1])
    poses = [np.eye(4)] + [s['gt'][c] for c in range(3)]
    payloads = render.frame_records(s['depth'], s['label'], s['intr'], [poses], [[0, 1, 2, 3]], 48, [0])
    path = str(tmp / "0048_pcnn.tfrecord")
    tfrecord_io.write_records(path, payloads)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    one, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(root, "tests", "golden", "obj_model_first1.tfrecords"))
    files = mm.mesh_files(str(tmp / "meshes"))
    detector = dict(meshes=mm.pack_meshes(files, 1.0), classes=DETECT_CLASSES, top=2, min_score=(1, 2), margin=0.5, num_point=N_POINT,
                    ppf_models=ppf.PPFModels.from_meshes([files[c] for c in DETECT_CLASSES], num_point=256, scale=1.0,
                                                         classes=DETECT_CLASSES, num_class=len(files)))
    params = {k: v for k, v in DR.SCENE_SEGMENT.items()}
    det = detect.detect_objects(s['depth'], s['intr'], first_frame=0, components={k: v for k, v in params.items() if k != 'seed'},
                                seed=params['seed'], **detector)
    print("detected classes %s scores %s" % (det.table['det_class'].tolist(), det.table['det_score'].tolist()))
    return dict(tmp=tmp, path=path, frames=tfrecord_io.read_frames(path, verify=True), models=np.repeat(one, 21, axis=0),
                detector=detector, params=params, det=det)


def _expected_choice(records, scene, target):
    """(k + 1 of the component detect_objects gave `target`, or 0; its IoU with the record's pixels; the record's choice)."""
    s, det = scene['s'], records['det']
    found = det.segments.label.cpu().numpy()[0]
    mine = [k for k in range(det.table['det_class'].shape[1]) if det.table['det_class'][0, k] == target]
    k = min(mine, key=lambda j: det.table['det_rank'][0, j]) + 1 if mine else 0
    want = (s['label'][0] == target + 1) & (s['depth'][0] != 0)
    iou = float(((found == k) & want).sum()) / float(((found == k) | want).sum()) if k else 0.0
    import depth_components_reference as D
    return k, iou, D.match(found, s['label'][0], s['depth'][0], target + 1)[0]


def test_element_from_frames_takes_the_detected_component(hip, dev, scene, records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import segment as S
    s, frames, models = scene['s'], records['frames'], records['models']
    det = records['det']
    assigned = [int(c) for c in det.table['det_class'][0] if c in (1, 2, 3)]
    assert assigned, "the detector named no component of the scene"
    target = assigned[0]
    k, iou, k_record = _expected_choice(records, scene, target)
    counts = {}
    el = E.element_from_frames(frames, target, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True,
                               labels="components", components=records['params'], counts=counts, choose="detect",
                               detector=records['detector'])
    assert el is not None and counts == dict(frames=1, detected=1, agree=int(k == k_record))
    found = det.segments.label.cpu().numpy()
    relabelled = np.where(found == k, target + 1, 0).astype(np.uint8)
    assert el['segment_iou'].tolist() == [iou] and el['detect_agree'].tolist() == [k == k_record]
    assert np.array_equal(el['frame_label'].cpu().numpy(), relabelled) and el['frame_want'].tolist() == [target + 1]
    # extract_segments fed the relabelled image of the detected component
    r = S.extract_segments(s['depth'], relabelled, s['intr'], classes=[[target]], num_point=N_POINT, device=dev)
    smp = S.sample_segments(r, N_POINT, seed=4)
    assert r.kept.tolist() == [True]
    assert torch.equal(el['xyz'], smp['xyz']) and torch.equal(el['xyz_inlier'], smp['xyz_inlier'])
    # choose="record" is the call without the argument, bit for bit
    base = E.element_from_frames(frames, target, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True,
                                 labels="components", components=records['params'])
    same = E.element_from_frames(frames, target, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True,
                                 labels="components", components=records['params'], choose="record")
    assert set(base) == set(same) and "detect_agree" not in base
    for key, v in base.items():
        assert torch.equal(v, same[key]) if isinstance(v, torch.Tensor) else np.array_equal(v, same[key]), key
    # a class the detector gave to no component: the frame is dropped and counted
    unassigned = [c for c in (1, 2, 3) if c not in assigned]
    if unassigned:
        counts = {}
        assert E.element_from_frames(frames, unassigned[0], N_POINT, models, seed=4, device=dev, labels="components",
                                     components=records['params'], counts=counts, choose="detect",
                                     detector=records['detector']) is None
        assert counts == dict(frames=1, detected=0, agree=0)
    with pytest.raises(ValueError):
        E.element_from_frames(frames, target, N_POINT, models, choose="detect", detector=records['detector'])
    with pytest.raises(ValueError):
        E.element_from_frames(frames, target, N_POINT, models, labels="components", choose="detect")
    with pytest.raises(ValueError):
        E.element_from_frames(frames, target, N_POINT, models, labels="components", detector=records['detector'])


def test_command_line_prints_the_detect_line(hip, dev, scene, records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    tmp, models, det = records['tmp'], records['models'], records['det']
    assigned = [int(c) for c in det.table['det_class'][0] if c in (1, 2, 3)]
    target = assigned[0]
    k, iou, k_record = _expected_choice(records, scene, target)
    obj = str(tmp / "obj_models.tfrecords")
    tfrecord_io.write_records(obj, [tfrecord_io.encode_example({"label": np.array([c]), "model": models[c].reshape(-1)})
                                    for c in range(target + 1)])
    graph = T.TrainGraph({"num_point": N_POINT, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    p = records['params']
    common = ["--files", records['path'], "--object_model", obj, "--trained_model", ckpt[:-len(".npz")], "--target_cls", str(target),
              "--num_point", str(N_POINT), "--batch_size", "1", "--seed", str(p['seed']), "--components_n_hyp", str(p['n_hyp']),
              "--components_stride", str(p['stride']), "--components_min_pixels", str(p['min_pixels']), "--components_max",
              str(p['max_components'])]
    capsys.readouterr()
    assert E.main(common + ["--labels", "components", "--choose", "detect", "--meshes", str(tmp / "meshes"), "--detect_classes",
                            "1,2,3,4", "--detect_top", "2", "--detect_min_score", "1/2", "--detect_margin", "0.5"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln for ln in lines if ln.startswith("batch size ")] == ["batch size 1"], lines
    assert lines[-1] == "detect class %d frames 1 detected 1 agree %d mean_iou %f" % (target, int(k == k_record), iou), lines[-3:]
    for bad in (["--choose", "detect", "--meshes", str(tmp / "meshes")], ["--labels", "components", "--choose", "detect"]):
        with pytest.raises(SystemExit) as err:
            E.main(common + bad)
        assert err.value.code == 2 and "--choose detect" in capsys.readouterr().err
