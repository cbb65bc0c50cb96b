"""GPU: every path of cloudaae_frame_segments, cloudaae_radius_outlier and cloudaae_ragged_fps (csrc/segment.hip) at the
block, grid and register boundaries that tests/test_15_frame_segments_gpu.py, with its one operating point, leaves out,
against the NumPy restatement of DESIGN.md "Frame segments" (tests/segment_reference.py).  Every comparison is bit for
bit; the shapes are the smallest at which each path exists.

The three entry points are called through the C ABI.  The workspace has exactly the size the query returns and lies,
like every output, between two guards that hold a byte pattern, as does the workspace itself before the call (it need
not be initialised).  After a call the guards must be intact and the rows of xyz, in_index and in_xyz past the
device-side total must still hold the pattern.  A workspace one byte short must be refused with nothing written."""
import numpy as np
import pytest
import torch

import segment_reference as R

pytestmark = pytest.mark.gpu

GUARD = 1024               # bytes in front of and behind every output and workspace
FILL = 0xA5
SEG_BLOCK = 256            # the constants of csrc/segment.hip the cases are placed by
SCAN_THREADS = 1024
FPS_THREADS = 512
FPS_REG_POINTS = 12288
RO_GRID_MAX = 32
INF = np.float32(np.inf)


class Guarded(object):
    """A buffer of `shape` elements between two guards of GUARD bytes; guards and buffer hold FILL."""

    def __init__(self, shape, dtype):
        self.shape = tuple(int(v) for v in shape)
        self.dtype = dtype
        self.nbytes = int(np.prod(self.shape)) * torch.empty((), dtype=dtype).element_size()
        self.full = torch.full((self.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.full.data_ptr() + GUARD

    def bytes(self):
        """the buffer's bytes on the host, after the guards were found intact"""
        full = self.full.cpu().numpy()
        assert np.all(full[:GUARD] == FILL) and np.all(full[GUARD + self.nbytes:] == FILL), "a guard was overwritten"
        return full[GUARD:GUARD + self.nbytes]

    def numpy(self):
        return self.bytes().view(torch.empty((), dtype=self.dtype).numpy().dtype).reshape(self.shape).copy()

    def untouched(self, from_byte=0):
        return bool(np.all(self.bytes()[from_byte:] == FILL))


def _dev(a, ty):
    return torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. frame segments -------------------------------------------------------------------------------------------------------

def _fs_call(hip, depth, label, intr, seg_frame, seg_class, threshold, short=0):
    F, H, W = depth.shape
    S, M = len(seg_frame), F * H * W
    L = hip.lib()
    nbytes = int(L.cloudaae_frame_segments_workspace_bytes(F, H, W, S))
    assert nbytes > 0
    ins = [_dev(depth.view(np.int16), np.int16), _dev(label, np.uint8), _dev(intr, np.float32),
           _dev(seg_frame, np.int32), _dev(seg_class, np.int32)]
    off, xyz, mean = Guarded((S + 1,), torch.int32), Guarded((M, 3), torch.float32), Guarded((S, 3), torch.float32)
    ws = Guarded((nbytes - short,), torch.uint8)
    rc = L.cloudaae_frame_segments(F, H, W, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), S, ins[3].data_ptr(),
                                   ins[4].data_ptr(), float(threshold), off.ptr(), xyz.ptr(), mean.ptr(), ws.ptr(),
                                   nbytes - short, hip.stream())
    torch.cuda.synchronize()
    return rc, off, xyz, mean, ws


def _fs_gpu(hip, depth, label, intr, seg_frame, seg_class, threshold):
    """-> offsets [S+1], xyz [total, 3], mean [S, 3]; the guards and the rows of xyz past the total were checked"""
    rc, off, xyz, mean, ws = _fs_call(hip, depth, label, intr, seg_frame, seg_class, threshold)
    hip.check(rc, "cloudaae_frame_segments")
    ws.bytes()
    o = off.numpy()
    total = int(o[-1])
    assert 0 <= total <= xyz.shape[0]
    assert xyz.untouched(12 * total), "rows of xyz past the total were written"
    return o, xyz.numpy()[:total], mean.numpy()


def _fs_check(got, ref):
    o, xyz, mean = got
    sizes = [s["num_point_after_filter"] for s in ref]
    print("segments %d, masked %d, kept %d (gpu %d)" % (len(ref), sum(len(s["mask_xyz"]) for s in ref), sum(sizes), o[-1]))
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(sizes)]))
    for i, s in enumerate(ref):
        assert np.array_equal(_bits(mean[i]), _bits(s["mean"])), i
        assert np.array_equal(_bits(xyz[o[i]:o[i + 1]]), _bits(s["xyz"])), i


LABELS = np.array([0, 3, 6, 9, 10, 255], np.uint8)    # classes 2, 5, 8, 9 and 254; class 8 is in the image, never listed
LISTED = (2, 5, 9, 254, 40)                          # class 40 is listed and has no pixel


def _frames(seed, F, H, W, labels=LABELS, zeros=0.3):
    """F frames, each with its own fx, fy, cx, cy, factor_depth 1000 and 10000 in turn; depth 0.5 .. 0.9 m with `zeros`
    of it 0 and up to two values of 65535 per frame."""
    rng = np.random.default_rng(seed)
    depth = np.empty((F, H, W), np.uint16)
    intr = np.empty((F, 5), np.float32)
    for f in range(F):
        factor = 1000.0 if f % 2 == 0 else 10000.0
        d = np.round(rng.uniform(0.5, 0.9, (H, W)) * factor).astype(np.uint16)
        d[rng.random((H, W)) < zeros] = 0
        if H * W >= 35:
            d.reshape(-1)[rng.integers(0, H * W, 2)] = 65535
        depth[f] = d
        intr[f] = [40.0 + 7.0 * f, 43.0 + 5.0 * f, W / 2 + 0.37 * f, H / 2 - 0.21 * f, factor]
    label = rng.choice(labels, (F, H, W)).astype(np.uint8)
    return depth, label, intr


def _hard_list(seed, F):
    """Shuffled, not frame-major: every (frame, class of LISTED), the pair (0, 2) twice with entries between, frames -1
    and F, classes -1, 255 and 300."""
    rng = np.random.default_rng(seed)
    pairs = [(f, c) for f in range(F) for c in LISTED if (f, c) != (0, 2)]
    pairs += [(-1, 2), (F, 5), (0, -1), (0, 255), (F - 1, 300)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    pairs = pairs[:1] + [(0, 2)] + pairs[1:] + [(0, 2)]
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def _as_frames(depth, label, intr):
    return [(depth[f], label[f], intr[f]) for f in range(len(depth))]


def _ref(case):
    depth, label, intr, sf, sc, thr = case
    return R.extract_listed(_as_frames(depth, label, intr), sf, sc, threshold=thr, nb_points=0, min_keep=0)


TINY = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (2, 1, 257), (2, 23, 45), (4, 32, 24)]


def _case_tiny(shape):
    F, H, W = shape
    depth, label, intr = _frames(100 + H * W, F, H, W)
    if H * W == 1:
        depth[0, 0, 0], label[0, 0, 0] = 700, 3
    sf, sc = _hard_list(F, F)
    case = (depth, label, intr, sf, sc, R.THRESHOLD)
    ref = _ref(case)
    first, last = [i for i in range(len(sf)) if (sf[i], sc[i]) == (0, 2)]
    assert last - first > 1 and ref[first]["num_point_after_filter"] == 0           # the duplicate: its last entry owns
    if H * W > 1:
        assert len(ref[last]["mask_xyz"]) > 0 and (label == 9).any() and len(set(intr[:, 4])) == 2
    if H * W >= 256:
        assert any(0 < s["num_point_after_filter"] < len(s["mask_xyz"]) for s in ref)   # the filter cuts
    return case, ref


def _case_single_segment():
    depth, label, intr = _frames(7, 2, 5, 7)
    case = (depth, label, intr, np.array([1], np.int32), np.array([5], np.int32), R.THRESHOLD)
    ref = _ref(case)
    assert len(ref) == 1 and len(ref[0]["mask_xyz"]) > 0
    return case, ref


def _case_many_segments():
    """More valid segments than SCAN_THREADS: scan_kernel over S takes more than one element per thread, fs_table_kernel and
    compact_offsets_kernel more than one block."""
    F, H, W = 5, 23, 45
    depth, label, intr = _frames(8, F, H, W, labels=np.arange(1, 256, dtype=np.uint8))
    rng = np.random.default_rng(9)
    pairs = [(f, c) for f in range(F) for c in range(255)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    sf, sc = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    case = (depth, label, intr, sf, sc, R.THRESHOLD)
    ref = _ref(case)
    assert len(ref) == 1275 > SCAN_THREADS and sum(len(s["mask_xyz"]) > 0 for s in ref) > SCAN_THREADS
    return case, ref


def _case_block_contents():
    """Frame 0: the first 256 pixels are one segment (ranks 0..255 across four waves); frame 1: the pixels alternate between
    two segments."""
    depth, label, intr = _frames(10, 2, 23, 45)
    label[0].reshape(-1)[:SEG_BLOCK] = 3
    d0 = depth[0].reshape(-1)
    d0[:SEG_BLOCK] = np.where((d0[:SEG_BLOCK] == 0) | (d0[:SEG_BLOCK] == 65535), 640, d0[:SEG_BLOCK])
    label[1].reshape(-1)[:] = np.where(np.arange(23 * 45) % 2 == 0, 3, 6)
    depth[1] = np.where(depth[1] == 0, 7000, depth[1])
    sf, sc = np.array([1, 0, 1, 0], np.int32), np.array([5, 2, 2, 5], np.int32)
    case = (depth, label, intr, sf, sc, INF)
    ref = _ref(case)
    assert len(ref[1]["mask_xyz"]) >= SEG_BLOCK and len(ref[0]["mask_xyz"]) == 517 and len(ref[2]["mask_xyz"]) == 518
    return case, ref


def _case_no_match():
    depth, label, intr = _frames(11, 2, 23, 45)
    case = (depth, label, intr, np.array([0, 1, 1], np.int32), np.array([40, 41, 0], np.int32), R.THRESHOLD)
    ref = _ref(case)
    assert sum(len(s["mask_xyz"]) for s in ref) == 0
    return case, ref


def _case_all_match(shape):
    """Every pixel of every frame is in a listed segment and the threshold keeps all: both totals are m, and
    compact_offsets_kernel reads blk_off[gblk] when m is a multiple of 256."""
    F, H, W = shape
    depth, label, intr = _frames(12, F, H, W, labels=np.array([3, 6], np.uint8), zeros=0.0)
    pairs = [(f, c) for c in (5, 2) for f in range(F)]
    case = (depth, label, intr, np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32), INF)
    ref = _ref(case)
    assert sum(s["num_point_after_filter"] for s in ref) == F * H * W
    assert (F * H * W % SEG_BLOCK == 0) == (shape == (4, 32, 24))
    return case, ref


def _case_masked_multiple_of_256():
    F, H, W = 4, 32, 24
    depth, label, intr = _frames(13, F, H, W, labels=np.array([0, 3, 6, 9], np.uint8), zeros=0.0)
    rng = np.random.default_rng(14)
    listed = np.nonzero((label.reshape(-1) == 3) | (label.reshape(-1) == 6))[0]
    drop = np.ones(F * H * W, bool)
    drop[rng.choice(listed, 2 * SEG_BLOCK, replace=False)] = False
    depth.reshape(-1)[drop] = 0
    pairs = [(f, c) for f in (2, 0, 3, 1) for c in (2, 5)]
    case = (depth, label, intr, np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32),
            R.THRESHOLD)
    ref = _ref(case)
    assert sum(len(s["mask_xyz"]) for s in ref) == 2 * SEG_BLOCK
    assert 0 < sum(s["num_point_after_filter"] for s in ref) < 2 * SEG_BLOCK
    return case, ref


def _threshold_frames():
    depth, label, intr = _frames(15, 2, 23, 45)
    label[0, 11, 20], depth[0, 11, 20] = 77, 777                     # class 76: one point
    sf, sc = _hard_list(16, 2)
    return depth, label, intr, np.append(sf, 0).astype(np.int32), np.append(sc, 76).astype(np.int32)


def _case_threshold(which):
    """+inf keeps all; 0 keeps a one-point segment's point (its mean is the point); a negative threshold keeps nothing, so
    every offset is equal; at the boundary, threshold = d, the reference's fp32 distance of one point, keeps that point and
    the float below d does not."""
    base = _threshold_frames()
    everything = _ref(base + (INF,))
    if which in ("at-distance", "below-distance"):
        seg = max(everything, key=lambda s: len(s["mask_xyz"]))
        pts, m = seg["mask_xyz"], seg["mean"]
        d = (pts - m).astype(np.float32)
        dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32))
        at = np.float32(np.sort(dist)[len(dist) // 2])
        below = np.nextafter(at, np.float32(0))
        n_at = int(R.distance_filter(pts, m, at).sum())
        n_below = int(R.distance_filter(pts, m, below).sum())
        assert 0 < n_below < n_at < len(pts) and n_at - n_below == int((dist == at).sum())
        thr = at if which == "at-distance" else below
    else:
        thr = {"inf": INF, "zero": np.float32(0.0), "negative": np.float32(-1.0)}[which]
    case = base + (thr,)
    ref = everything if which == "inf" else _ref(case)
    sizes = [s["num_point_after_filter"] for s in ref]
    if which == "inf":
        assert sizes == [len(s["mask_xyz"]) for s in ref] and sum(sizes) > 500
    elif which == "zero":
        assert len(ref[-1]["mask_xyz"]) == 1 and sizes[-1] == 1
    elif which == "negative":
        assert sum(sizes) == 0 and sum(len(s["mask_xyz"]) for s in ref) > 500
    return case, ref


def _case_mean():
    """1200 points near depth 65535 / 10000: an fp32 running sum gives another fp32 mean than the definition's fp64 sum."""
    rng = np.random.default_rng(17)
    depth = rng.integers(65000, 65536, (1, 30, 40)).astype(np.uint16)
    label = np.ones((1, 30, 40), np.uint8)
    intr = np.array([[41.5, 43.25, 19.3, 15.6, 10000.0]], np.float32)
    case = (depth, label, intr, np.array([0], np.int32), np.array([0], np.int32), R.THRESHOLD)
    ref = _ref(case)
    pts = ref[0]["mask_xyz"]
    assert len(pts) == 1200
    running = np.cumsum(pts, axis=0, dtype=np.float32)[-1] / np.float32(1200)
    assert running.dtype == np.float32 and running[2] != ref[0]["mean"][2]
    assert 0 < ref[0]["num_point_after_filter"] < 1200
    return case, ref


FS_CASES = dict([("tiny-%dx%dx%d" % s, (_case_tiny, s)) for s in TINY] + [
    ("single-segment", (_case_single_segment,)), ("many-segments", (_case_many_segments,)),
    ("block-contents", (_case_block_contents,)), ("no-match", (_case_no_match,)),
    ("all-match-4x32x24", (_case_all_match, (4, 32, 24))), ("all-match-2x23x45", (_case_all_match, (2, 23, 45))),
    ("masked-multiple-of-256", (_case_masked_multiple_of_256,))] + [
    ("threshold-" + w, (_case_threshold, w)) for w in ("inf", "zero", "negative", "at-distance", "below-distance")] + [
    ("mean", (_case_mean,))])


@pytest.mark.parametrize("name", list(FS_CASES))
def test_frame_segments(hip, name):
    build = FS_CASES[name]
    case, ref = build[0](*build[1:])
    _fs_check(_fs_gpu(hip, *case), ref)


def test_frame_segments_refuses_a_short_workspace(hip):
    case, _ = _case_single_segment()
    rc, off, xyz, mean, ws = _fs_call(hip, *case, short=1)
    assert rc != 0
    assert off.untouched() and xyz.untouched() and mean.untouched() and ws.untouched()


# ---- 2. radius outlier ---------------------------------------------------------------------------------------------------------

def _ro_call(hip, sets, nb_points, radius, min_keep, max_points=None, short=0):
    from test_15_frame_segments_gpu import _packed
    off, xyz = _packed(sets)
    total, S = len(xyz), len(sets)
    M = max(total, 1) if max_points is None else int(max_points)
    assert M >= total
    rows = np.full((M, 3), 1e30, np.float32)                      # rows past the total: never read
    rows[:total] = xyz
    d_off, d_xyz = _dev(off, np.int32), _dev(rows, np.float32)
    L = hip.lib()
    nbytes = int(L.cloudaae_radius_outlier_workspace_bytes(S, M))
    assert nbytes > 0
    in_off, in_idx = Guarded((S + 1,), torch.int32), Guarded((M,), torch.int32)
    in_xyz, nv = Guarded((M, 3), torch.float32), Guarded((S,), torch.int32)
    ws = Guarded((nbytes - short,), torch.uint8)
    rc = L.cloudaae_radius_outlier(S, d_off.data_ptr(), d_xyz.data_ptr(), M, int(nb_points), float(radius), int(min_keep),
                                   in_off.ptr(), in_idx.ptr(), in_xyz.ptr(), nv.ptr(), ws.ptr(), nbytes - short,
                                   hip.stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_xyz.cpu().numpy().view(np.uint32), rows.view(np.uint32))
    return rc, in_off, in_idx, in_xyz, nv, ws


def _ro_gpu(hip, sets, nb_points, radius, min_keep, max_points=None):
    """-> per set: inlier indices and inlier points; num_valid [S]"""
    rc, in_off, in_idx, in_xyz, nv, ws = _ro_call(hip, sets, nb_points, radius, min_keep, max_points)
    hip.check(rc, "cloudaae_radius_outlier")
    ws.bytes()
    io = in_off.numpy()
    total = int(io[-1])
    assert io[0] == 0 and 0 <= total <= in_idx.shape[0]
    assert in_idx.untouched(4 * total) and in_xyz.untouched(12 * total), "rows past the total were written"
    idx, pts = in_idx.numpy(), in_xyz.numpy()
    S = len(sets)
    return ([idx[io[i]:io[i + 1]].astype(np.int64) for i in range(S)], [pts[io[i]:io[i + 1]] for i in range(S)],
            nv.numpy())


def _counts(pts, radius):
    if len(pts) == 0:
        return np.zeros(0, np.int64)
    return R.neighbour_counts_brute(pts, radius) if len(pts) <= 700 else R.neighbour_counts(pts, radius)


def _ro_check(got, sets, nb_points, radius, min_keep, counts=None):
    idx, pts, nv = got
    kept = 0
    for i, s in enumerate(sets):
        c = _counts(s, radius) if counts is None else counts[i]
        want, want_nv = R.radius_outlier(s, nb_points, radius, min_keep, counts=c)
        assert np.array_equal(idx[i], want), i
        assert nv[i] == want_nv, i
        assert np.array_equal(_bits(pts[i]), _bits(s[want])), i
        kept += len(want)
    print("sets %d, points %d, kept %d" % (len(sets), sum(len(s) for s in sets), kept))


def _clouds():
    """Gaussian clouds at four scales, a dense core and a thin tail each: at every radius below, some cloud has points on
    both sides of the count."""
    rng = np.random.default_rng(20)
    return [(c + rng.standard_normal((n, 3)) * sigma).astype(np.float32)
            for n, sigma, c in ((3000, 0.002, [0.1, 0.2, 0.7]), (1000, 0.01, [-0.3, 0.1, 0.9]),
                                (3000, 0.05, [0.0, 0.0, 1.2]), (300, 0.3, [0.4, -0.5, 2.0]))]


_CLOUD_COUNTS = {}


def _cloud_counts(radius):
    """the reference's counts of _clouds() at a radius, computed once"""
    key = float(np.float32(radius))
    if key not in _CLOUD_COUNTS:
        _CLOUD_COUNTS[key] = [R.neighbour_counts(s, radius) for s in _clouds()]
    return _CLOUD_COUNTS[key]


RO_PARAMS = [(0, 0.02, 0), (1, 0.005, 1), (7, 0.05, 10), (3, 1e-3, 0), (R.NB_POINTS, R.RADIUS, R.MIN_KEEP)]


@pytest.mark.parametrize("nb_points, radius, min_keep", RO_PARAMS)
def test_radius_parameters(hip, nb_points, radius, min_keep):
    sets, counts = _clouds(), _cloud_counts(radius)
    if nb_points == 0:
        assert all((c > 0).all() for c in counts)                    # every point counts itself: all are kept
    else:
        assert any(0 < (c > nb_points).sum() < len(c) for c in counts)
    _ro_check(_ro_gpu(hip, sets, nb_points, radius, min_keep), sets, nb_points, radius, min_keep, counts)


@pytest.mark.parametrize("which", ["at-count", "above-count", "no-inlier"])
def test_radius_min_keep(hip, which):
    """seg_count < min_keep: min_keep = the inlier count keeps the inliers, one above keeps every point (num_valid = n - 1);
    min_keep = 0 on a set with no inlier leaves an empty set."""
    sets, counts = _clouds(), _cloud_counts(R.RADIUS)
    inliers = int((counts[1] > R.NB_POINTS).sum())
    assert 0 < inliers < len(sets[1]) and (counts[3] <= R.NB_POINTS).all()
    first = int(counts[1][0] > R.NB_POINTS)                           # count_nonzero leaves index 0 out
    min_keep = dict([("at-count", inliers), ("above-count", inliers + 1), ("no-inlier", 0)])[which]
    pick = [3, 1] if which == "no-inlier" else [1]
    sets, counts = [sets[i] for i in pick], [counts[i] for i in pick]
    idx, pts, nv = got = _ro_gpu(hip, sets, R.NB_POINTS, R.RADIUS, min_keep)
    _ro_check(got, sets, R.NB_POINTS, R.RADIUS, min_keep, counts)
    if which == "at-count":
        assert len(idx[0]) == inliers and nv[0] == inliers - first
    elif which == "above-count":
        assert len(idx[0]) == len(sets[0]) and nv[0] == len(sets[0]) - 1
    else:
        assert len(idx[0]) == 0 and nv[0] == 0 and len(idx[1]) == inliers


def _cell_edge(pts, radius=R.RADIUS):
    """the cell edge of ro_grid_kernel, in its arithmetic: max(r (1 + 2^-10), extent / 31), and the bounding box's minimum"""
    p = pts.astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    return max(float(np.float32(radius)) * (1.0 + 1.0 / 1024.0), ext / (RO_GRID_MAX - 1)), p.min(axis=0)


def _geometry_sets(origin):
    """Degenerate and cell-boundary geometry at `origin` (fp32): generic sets are shifted in fp32, the crafted pair is built
    in the shifted coordinates."""
    rng = np.random.default_rng(21)
    o = np.asarray(origin, np.float32)
    r = float(R.RADIUS)
    h0 = r * (1.0 + 1.0 / 1024.0)
    at_origin = not o.any()

    def shifted(p):
        return (np.asarray(p, np.float32) + o).astype(np.float32)
    sets = [shifted([[0.25, 0.5, 0.75]]),                                            # one point
            np.repeat(shifted([[0.125, 0.25, 0.5]]), 200, axis=0)]                  # 200 duplicates: extent 0
    for axis in range(3):                                                            # collinear along each axis
        p = np.zeros((500, 3))
        p[:, axis] = rng.uniform(0, 0.5, 500)
        sets.append(shifted(p))
    p = rng.uniform(0, 0.3, (2000, 3))                                               # coplanar
    p[:, 2] = 0.125
    sets.append(shifted(p))
    for side in (-1, 1):                                                             # either side of the cell-edge switch
        ext = 31 * h0 * (1 + side * 1e-4)
        p = rng.uniform(0, 1, (3000, 3)) * [ext, 0.02, 0.02]
        p[0], p[1] = [0, 0, 0], [ext, 0.02, 0.02]
        s = shifted(p)
        h, _ = _cell_edge(s)
        assert (h == h0) if side < 0 else (h0 < h < h0 * 1.001)
        sets.append(s)
    # a lattice of spacing 1/32 = the cell edge: points on cell boundaries and at the box's maximum; further points 0.01
    # below in x (the cell before) and 0.01 above in y (the same cell)
    g = np.arange(32) / 32.0
    lat = np.stack(np.meshgrid(g, g, g[:2], indexing="ij"), -1).reshape(-1, 3)
    lo = lat[rng.choice(np.nonzero(lat[:, 0] > 0)[0], 450, replace=False)] - [0.01, 0, 0]
    hi = lat[rng.choice(np.nonzero(lat[:, 1] < 0.9)[0], 450, replace=False)] + [0, 0.01, 0]
    s = shifted(np.concatenate([lat, lo, hi]))
    if at_origin:
        h, mn = _cell_edge(s)
        assert h == 1.0 / 32 and not mn.any() and np.array_equal(s[:2048] * 32, np.round(s[:2048] * 32))
        assert s[:, 0].max() * 32 == 31
    sets.append(s)
    # a pair at d^2 just below r^2 across the boundary of cells 0 and 1 (cells 0 and 2 were the edge 0.9 r), and a pair at
    # the next float, d^2 >= r^2; the box's corners keep the extent below 31 r, so the edge is r (1 + 2^-10)
    r2 = R.radius_sq()
    xa = np.float32(o[0] + np.float32(0.0179))
    xb = np.float32(xa + np.float32(0.02001))
    while (float(xb) - float(xa)) ** 2 >= r2:
        xb = np.nextafter(xb, np.float32(-np.inf))
    xc = np.nextafter(xb, np.float32(np.inf))
    y0, y1, z = np.float32(o[1] + np.float32(0.01)), np.float32(o[1] + np.float32(0.3)), np.float32(o[2] + np.float32(0.01))
    s = np.array([[o[0], o[1], o[2]], [xa, y0, z], [xb, y0, z], [xa, y1, z], [xc, y1, z],
                  [o[0] + np.float32(0.5), o[1] + np.float32(0.5), o[2] + np.float32(0.02)]], np.float32)
    h, mn = _cell_edge(s)
    cells = np.floor((s[:, 0].astype(np.float64) - mn[0]) / h).astype(int)
    assert h == h0 and list(cells[1:5]) == [0, 1, 0, 1]
    assert list(np.floor((s[1:3, 0].astype(np.float64) - mn[0]) / (0.9 * r)).astype(int)) == [0, 2]
    assert (float(xb) - float(xa)) ** 2 < r2 <= (float(xc) - float(xa)) ** 2
    assert list(R.neighbour_counts_brute(s)) == [1, 2, 2, 1, 1, 1]
    sets.append(s)
    return sets


_GEOMETRY = {}


def _geometry(origin):
    """the sets and the reference's counts at an origin, computed once"""
    if origin not in _GEOMETRY:
        sets = _geometry_sets(origin)
        _GEOMETRY[origin] = (sets, [_counts(s, R.RADIUS) for s in sets])
    return _GEOMETRY[origin]


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.3, -0.2, 6.5)])
@pytest.mark.parametrize("nb_points", [1, 30])
def test_radius_geometry(hip, nb_points, origin):
    sets, counts = _geometry(origin)
    idx, pts, nv = got = _ro_gpu(hip, sets, nb_points, R.RADIUS, 0)
    _ro_check(got, sets, nb_points, R.RADIUS, 0, counts)
    if nb_points == 1:
        assert list(idx[-1]) == [1, 2] and len(idx[0]) == 0 and len(idx[1]) == 200


def _layout_sets():
    """300 sets, most of them empty; boundaries in the middle of a wave and of a block; a set of 64 points at a multiple of
    64 and one of 256 at a multiple of 256; the total is a multiple of 256."""
    from test_15_frame_segments_gpu import _ball
    rng = np.random.default_rng(22)
    sizes = [37, 0, 0, 27, 64, 1, 0, 127, 256, 100, 0, 3]
    sizes += [int(rng.integers(1, 40)) if rng.random() < 0.3 else 0 for _ in range(300 - len(sizes) - 1)]
    sizes.append(SEG_BLOCK - sum(sizes) % SEG_BLOCK)
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert len(sizes) == 300 and sizes.count(0) > 150 and off[-1] % SEG_BLOCK == 0 and off[-1] <= 3000
    assert sizes[4] == 64 and off[4] % 64 == 0 and sizes[8] == 256 and off[8] % SEG_BLOCK == 0
    assert off[10] % 64 != 0 and off[12] % 64 != 0
    return [_ball(rng, n, rng.uniform(-1, 1, 3), 0.03) for n in sizes]


@pytest.mark.parametrize("slack", [0, 777])
def test_radius_layout(hip, slack):
    """max_points equal to the total and above it"""
    from test_15_frame_segments_gpu import _radius_gpu
    sets = _layout_sets()
    total = sum(len(s) for s in sets)
    nb_points, radius, min_keep = 5, R.RADIUS, 20
    counts = [_counts(s, radius) for s in sets]
    kept = [int((c > nb_points).sum()) for c in counts]
    assert any(0 < k < min_keep for k in kept) and any(min_keep <= k < len(c) for k, c in zip(kept, counts))
    idx, pts, nv = got = _ro_gpu(hip, sets, nb_points, radius, min_keep, max_points=total + slack)
    _ro_check(got, sets, nb_points, radius, min_keep, counts)
    if slack == 0:                                                  # the unguarded helper of test_15 sees the same
        idx15, nv15 = _radius_gpu(sets, nb_points, radius, min_keep)
        assert all(np.array_equal(a, b) for a, b in zip(idx, idx15)) and np.array_equal(nv, nv15)


def test_radius_outlier_refuses_a_short_workspace(hip):
    sets = _clouds()[3:]
    rc, in_off, in_idx, in_xyz, nv, ws = _ro_call(hip, sets, R.NB_POINTS, R.RADIUS, R.MIN_KEEP, short=1)
    assert rc != 0
    assert in_off.untouched() and in_idx.untouched() and in_xyz.untouched() and nv.untouched() and ws.untouched()


# ---- 3. ragged FPS -------------------------------------------------------------------------------------------------------------

def _fps_call(hip, sets, K, starts, max_points=None, short=0):
    from test_15_frame_segments_gpu import _packed
    off, xyz = _packed(sets)
    total, S = len(xyz), len(sets)
    M = max(total, 1) if max_points is None else int(max_points)
    rows = np.full((M, 3), 1e30, np.float32)
    rows[:total] = xyz
    d_off, d_xyz, d_st = _dev(off, np.int32), _dev(rows, np.float32), _dev(starts, np.int32)
    L = hip.lib()
    nbytes = int(L.cloudaae_ragged_fps_workspace_bytes(M))
    assert nbytes >= 8 * M
    idx, out = Guarded((S, K), torch.int32), Guarded((S, K, 3), torch.float32)
    ws = Guarded((nbytes - short,), torch.uint8)
    rc = L.cloudaae_ragged_fps(S, d_off.data_ptr(), d_xyz.data_ptr(), M, K, d_st.data_ptr(), idx.ptr(), out.ptr(), ws.ptr(),
                               nbytes - short, hip.stream())
    torch.cuda.synchronize()
    return rc, idx, out, ws


def _fps_gpu(hip, sets, K, starts, max_points=None):
    rc, idx, out, ws = _fps_call(hip, sets, K, starts, max_points)
    hip.check(rc, "cloudaae_ragged_fps")
    ws.bytes()
    return idx.numpy(), out.numpy()


def _fps_check(got, sets, K, starts):
    """-> the reference's indices per set (None where there is no set or no valid start: idx -1 and zeros)"""
    idx, pts = got
    wants = []
    for i, s in enumerate(sets):
        st = int(starts[i])
        if len(s) == 0 or st < 0 or st >= len(s):
            assert (idx[i] == -1).all() and not pts[i].view(np.uint32).any(), i
            wants.append(None)
            continue
        want = R.fps(s, K, st)
        assert np.array_equal(idx[i], want), i
        assert np.array_equal(_bits(pts[i]), _bits(s[want])), i
        wants.append(want)
    return wants


def _tie_set(n, start, a, b, seed):
    """Points with small integer coordinates (every distance is exact in fp64), the start at the origin, and two points at
    the same, largest distance from it: (8, 0, 0) at index a and (0, 8, 0) at index b."""
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, (n, 3)).astype(np.float32)
    s[start], s[a], s[b] = [0, 0, 0], [8, 0, 0], [0, 8, 0]
    p = s.astype(np.float64)
    d = ((p - p[start]) ** 2).sum(axis=1)
    assert d[a] == d[b] == 64.0 and np.sort(d)[-3] < 64.0
    return s


def test_fps_around_the_register_bound(hip):
    """Set sizes on both sides of FPS_REG_POINTS = 12288 and of the next multiple of 512; the farthest point in the last
    register slot, in the first slot in memory and at n - 1; ties across the split, within a lane, across lanes and waves;
    starts in memory and outside the set."""
    rng = np.random.default_rng(30)
    R0 = FPS_REG_POINTS
    sets, starts = [], []
    for n, st in ((R0 - 1, 5), (R0, R0 - 1), (R0 + 1, R0), (R0 + 511, 7000), (R0 + 512, R0 + 300), (R0 + 513, R0 + 512)):
        sets.append((rng.standard_normal((n, 3)) * 0.1).astype(np.float32))
        starts.append(st)
    far = []
    for n, at in ((R0, R0 - 1), (R0 + 1, R0), (R0 + 513, R0 + 512)):          # at == n - 1 in each; the slot differs
        s = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
        s[at] = [3, 3, 3]
        far.append((len(sets), at))
        sets.append(s)
        starts.append(0)
    s = (rng.standard_normal((R0 + 513, 3)) * 0.1).astype(np.float32)            # the last register slot of a longer set
    s[R0 - 1] = [3, 3, 3]
    far.append((len(sets), R0 - 1))
    sets.append(s)
    starts.append(R0 + 100)
    s = (rng.standard_normal((R0 + 513, 3)) * 0.1).astype(np.float32)            # the first slot in memory of a longer set
    s[R0] = [-3, 3, 3]
    far.append((len(sets), R0))
    sets.append(s)
    starts.append(3)
    ties = []
    T = FPS_THREADS
    for n, st, a, b in ((R0 + 700, 40, R0 - 288, R0 + 212),       # below and above the split
                        (2000, 3, 700, 700 + T),                   # one lane: t and t + 512
                        (2000, 3, 70, 200),                        # lanes of different waves
                        (2000, 3, 5, 9),                           # lanes of one wave
                        (2000, 3, T - 1, T),                       # the lower index in the last wave, the higher in lane 0
                        (R0 + 700, 40, R0 - 1, R0)):               # the same across the split
        ties.append((len(sets), a, b))
        sets.append(_tie_set(n, st, a, b, n + a))
        starts.append(st)
    sets += [(rng.standard_normal((100, 3)) * 0.1).astype(np.float32) for _ in range(3)] + [np.zeros((0, 3), np.float32)]
    starts += [-1, 100, 105, 0]
    K = 32
    wants = _fps_check(_fps_gpu(hip, sets, K, starts), sets, K, starts)
    for i, at in far:
        assert wants[i][1] == at, i
    for i, a, b in ties:
        assert a < b and wants[i][1] == a and wants[i][2] == b, i     # the lower index wins, then the other
    assert wants[-4] is None and wants[-3] is None and wants[-2] is None and wants[-1] is None


def test_fps_one_sample(hip):
    rng = np.random.default_rng(31)
    sets = [(rng.standard_normal((n, 3)) * 0.1).astype(np.float32) for n in (1, 700, FPS_REG_POINTS + 5, 9)]
    starts = [0, 699, FPS_REG_POINTS + 4, 9]
    wants = _fps_check(_fps_gpu(hip, sets, 1, starts, max_points=sum(len(s) for s in sets) + 100), sets, 1, starts)
    assert wants[3] is None and list(wants[2]) == [FPS_REG_POINTS + 4]


def test_fps_more_samples_than_points(hip):
    rng = np.random.default_rng(32)
    sizes = (1, 2, 63, 64, 65, 511, 512, 513)
    sets = [(rng.standard_normal((n, 3)) * 0.1).astype(np.float32) for n in sizes]
    starts = [int(rng.integers(n)) for n in sizes]
    K = 520
    wants = _fps_check(_fps_gpu(hip, sets, K, starts), sets, K, starts)
    for n, w in zip(sizes, wants):
        assert len(set(w[:n])) == n and (w[n:] == 0).all()             # every point once, then all-zero distances: index 0


def test_ragged_fps_refuses_a_short_workspace(hip):
    rng = np.random.default_rng(33)
    sets = [(rng.standard_normal((300, 3)) * 0.1).astype(np.float32)]
    rc, idx, out, ws = _fps_call(hip, sets, 8, [0], short=1)
    assert rc != 0
    assert idx.untouched() and out.untouched() and ws.untouched()


# ---- 4. the Python wrapper with parameters of its own --------------------------------------------------------------------------

def test_wrapper_forwards_its_parameters(hip):
    from cloudaae_amd.utils import segment as S
    depth, label, intr = _frames(40, 2, 48, 64, labels=np.array([0, 3, 6, 6, 10], np.uint8), zeros=0.1)
    classes = [[5, 2], [9, 5, 2]]
    params = dict(threshold=np.float32(0.3), nb_points=2, radius=np.float32(0.07), min_keep=25)
    frames = _as_frames(depth, label, intr)
    ordered = [sorted(c) for c in classes]                             # the wrapper lists classes ascending
    ref = R.extract(frames, ordered, **params)
    for k, v in (("threshold", R.THRESHOLD), ("nb_points", 0), ("radius", R.RADIUS), ("min_keep", 3000)):
        other = R.extract(frames, ordered, **dict(params, **{k: v}))   # each parameter matters to the reference
        assert any(len(a["inlier_idx"]) != len(b["inlier_idx"]) for a, b in zip(ref, other)), k
    r = S.extract_segments(depth, label, intr, classes=classes, **params)
    torch.cuda.synchronize()
    assert len(ref) == len(r.cls) == 5
    for i, seg in enumerate(ref):
        assert (int(r.frame[i]), int(r.cls[i])) == (seg["frame"], seg["cls"])
        assert r.num_point_after_filter[i] == seg["num_point_after_filter"], i
        xyz, idx, xin = r.segment(i)
        assert np.array_equal(_bits(xyz), _bits(seg["xyz"])), i
        assert np.array_equal(_bits(r.mean[i].cpu().numpy()), _bits(seg["mean"])), i
        assert np.array_equal(idx, seg["inlier_idx"]), i
        assert np.array_equal(_bits(xin), _bits(seg["xyz_inlier_full"])), i
        assert r.num_valid_points_in_segment[i] == seg["num_valid_points_in_segment"], i
