"""CPU: frame records (tfrecord_io.decode_frame / encode_example / write_records), the NumPy restatement of DESIGN.md
"Frame segments" (tests/segment_reference.py) against plain brute force, the float32 radius, and the argument checks
of the segment entry points of the C ABI (revision 602), which must fail before they touch memory."""
import ctypes
import os

import numpy as np
import pytest

import segment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")


def _frame(rng, channels, H=6, W=5):
    return dict(image=rng.integers(0, 255, (H, W, channels), dtype=np.uint8), depth=rng.integers(0, 65535, (H, W)).astype(np.uint16),
                label=rng.integers(0, 22, (H, W)).astype(np.uint8), quaternions=rng.standard_normal((21, 4)).astype(np.float32),
                translations=rng.standard_normal((21, 3)).astype(np.float32),
                class_one_hot=(rng.random(21) < 0.3).astype(np.int64), seq_id=np.int64(48), frame_id=np.int64(1234567),
                fx=np.float32(1066.778), fy=np.float32(1067.487), cx=np.float32(312.9869), cy=np.float32(241.3109),
                factor_depth=np.float32(10000.0))


def _encode(f):
    from cloudaae_amd import tfrecord_io as io
    d = {k: v for k, v in f.items() if k not in ("image", "depth", "label")}
    for k in ("image", "depth", "label"):
        d[k] = f[k].astype("<u2").tobytes() if k == "depth" else f[k].tobytes()
        d[k + "_shape"] = np.array(f[k].shape, np.int64)
    return io.encode_example(d)


@pytest.mark.parametrize("channels", [3, 4])
def test_frame_record_round_trip(tmp_path, channels):
    from cloudaae_amd import tfrecord_io as io
    rng = np.random.default_rng(channels)
    frames = [_frame(rng, channels), _frame(rng, channels, 4, 7)]
    path = str(tmp_path / "0048_pcnn.tfrecord")
    io.write_records(path, [_encode(f) for f in frames])
    got = io.read_frames(path, verify=True)               # the masked CRCs check out
    assert len(got) == 2
    for f, g in zip(frames, got):
        assert np.array_equal(g["image"], f["image"][:, :, :3]) and g["image"].shape[2] == 3
        for k in ("depth", "label", "quaternions", "translations", "class_one_hot"):
            assert g[k].dtype == f[k].dtype and np.array_equal(g[k], f[k]), k
        for k in ("seq_id", "frame_id", "fx", "fy", "cx", "cy", "factor_depth"):
            assert g[k] == f[k] and g[k].dtype == f[k].dtype, k
    # the generic parser sees the reference's schema (:128-145)
    ex = io.parse_example(_encode(frames[0]))
    assert set(ex) == {"image", "image_shape", "depth", "depth_shape", "label", "label_shape", "quaternions",
                       "translations", "class_one_hot", "seq_id", "frame_id", "fx", "fy", "cx", "cy", "factor_depth"}


def test_radius_is_float32():
    """tf.py_func hands 0.02 over as float32: r = (double)(float)0.02, not the double 0.02."""
    from cloudaae_amd import _lib
    from cloudaae_amd.utils import segment as S
    r = float(np.float32(0.02))
    assert r != 0.02 and R.radius_sq() == r * r and R.radius_sq(0.02) == r * r
    assert _lib._SIGNATURES["cloudaae_radius_outlier"][5] is ctypes.c_float
    assert np.float32(S.RADIUS) == R.RADIUS and np.float32(S.THRESHOLD) == R.THRESHOLD


def test_neighbour_counts_match_brute_force():
    rng = np.random.default_rng(0)
    base = np.array([0.5, -0.25, 0.75], np.float32)
    x = np.float32(base[0] + np.float32(0.02))
    edge = np.array([[e, base[1], base[2]] for e in (np.nextafter(x, np.float32(-1)), x,
                                                     np.nextafter(x, np.float32(2)))], np.float32)
    for n in (1, 7, 300):
        pts = (rng.standard_normal((n, 3)) * 0.02).astype(np.float32)
        pts = np.concatenate([pts, pts[:3], base[None], edge])          # duplicates and the r^2 boundary
        assert np.array_equal(R.neighbour_counts(pts), R.neighbour_counts_brute(pts))
    for s in (0, 1, 2):
        c = R.neighbour_counts_brute(np.concatenate([base[None], edge[s:s + 1]]))
        d = float(edge[s, 0]) - float(base[0])
        assert c[0] == (2 if d * d < R.radius_sq() else 1)


def test_radius_outlier_rules():
    idx, nv = R.radius_outlier(np.zeros((5, 3), np.float32), counts=np.array([101, 5, 101, 101, 3]))
    assert np.array_equal(idx, np.arange(5)) and nv == 4                  # fewer than 512 keepers: all, index 0 not counted
    counts = np.full(600, 101)
    counts[0] = 100
    idx, nv = R.radius_outlier(np.zeros((600, 3), np.float32), counts=counts)
    assert len(idx) == 599 and idx[0] == 1 and nv == 599
    counts[0] = 101
    idx, nv = R.radius_outlier(np.zeros((600, 3), np.float32), counts=counts)
    assert len(idx) == 600 and nv == 599


def test_fps_and_mean_match_plain_loops():
    rng = np.random.default_rng(1)
    for n, k in ((1, 4), (5, 9), (50, 20), (9, 9)):
        pts = (rng.standard_normal((n, 3))).astype(np.float32)
        if n == 9:
            pts[:] = pts[0]                                                 # all duplicates: index 0 after the start
        start = int(rng.integers(n))
        dist = [sum((float(pts[start][d]) - float(p[d])) ** 2 for d in range(3)) for p in pts]
        want = [start]
        for _ in range(1, k):
            j = max(range(n), key=lambda i: (dist[i], -i))
            want.append(j)
            dist = [min(dist[i], sum((float(pts[j][d]) - float(pts[i][d])) ** 2 for d in range(3))) for i in range(n)]
        assert list(R.fps(pts, k, start)) == want
    pts = (rng.standard_normal((1000, 3)) * 0.3 + 0.7).astype(np.float32)
    acc = [0.0, 0.0, 0.0]
    for p in pts:
        for d in range(3):
            acc[d] += float(p[d])
    assert np.array_equal(R.segment_mean(pts), np.array([a / 1000 for a in acc], np.float32))


def _same_segment(a, b):
    for k in ("frame", "cls", "num_point_after_filter", "num_valid_points_in_segment"):
        assert a[k] == b[k], k
    for k in ("xyz", "mean", "xyz_inlier_full"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.array_equal(a["inlier_idx"], b["inlier_idx"])


def test_extract_listed_equals_extract_on_frame_major_lists():
    rng = np.random.default_rng(4)
    frames = []
    for f in range(3):
        depth = rng.integers(4000, 9000, (9, 11)).astype(np.uint16)
        depth[rng.random(depth.shape) < 0.3] = 0
        label = rng.choice(np.array([0, 1, 4, 8, 255], np.uint8), depth.shape)
        frames.append((depth, label, np.array([50.0 + f, 52.0, 5.0, 4.0 + f, 10000.0], np.float32)))
    classes = [[0, 3, 7, 254], [3], [0, 5, 254]]                      # class 5 has no pixel
    params = dict(threshold=np.float32(0.15), nb_points=2, radius=np.float32(0.05), min_keep=3)
    want = R.extract(frames, classes, **params)
    seg_frame = [f for f, cl in enumerate(classes) for _ in cl]
    seg_class = [c for cl in classes for c in cl]
    got = R.extract_listed(frames, seg_frame, seg_class, **params)
    assert len(got) == len(want) == 8
    for a, b in zip(got, want):
        _same_segment(a, b)
    assert sum(s["num_point_after_filter"] for s in want) > 20
    assert any(0 < len(s["inlier_idx"]) < s["num_point_after_filter"] for s in want)


def test_extract_listed_duplicate_and_invalid_rules():
    depth = np.arange(1, 17, dtype=np.uint16).reshape(4, 4) * 500
    depth[1, 2] = 0
    label = np.array([[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 255, 255], [3, 3, 0, 0]], np.uint8)
    intr = np.array([4.0, 4.0, 1.5, 1.5, 1000.0], np.float32)
    frames = [(depth, label, intr), (depth[::-1].copy(), label, intr)]
    params = dict(threshold=np.float32(np.inf), nb_points=0, min_keep=0)
    #            0  1   2  3  4    5    6    7  8   9
    seg_frame = [1, 0, -1, 0, 2,   0,   0,   0, 0,  1]
    seg_class = [0, 1,  1, 0, 0, 255, 300,  -1, 1, 254]
    got = R.extract_listed(frames, seg_frame, seg_class, **params)
    assert [s["num_point_after_filter"] for s in got] == [4, 0, 0, 4, 0, 0, 0, 0, 3, 1]   # class 2 (label 3): not listed
    for i, s in enumerate(got):
        assert (s["frame"], s["cls"]) == (seg_frame[i], seg_class[i])                        # list order
    alone = R.extract(frames, [[0, 1], [0, 254]], **params)                                 # 0/0, 0/1, 1/0, 1/254
    for i, j in ((3, 0), (8, 1), (0, 2), (9, 3)):
        _same_segment(got[i], alone[j])
    for i in (1, 2, 4, 5, 6, 7):                      # the earlier of two entries, and every invalid pair: empty
        s = got[i]
        assert s["xyz"].shape == (0, 3) and s["mask_xyz"].shape == (0, 3) and not s["mean"].any()
        assert len(s["inlier_idx"]) == 0 and s["num_valid_points_in_segment"] == 0
    assert len(got[8]["mask_xyz"]) == 3                # depth 0 at (1, 2) is masked out of class 1


def test_quat2axangle_matches_the_rotation():
    from cloudaae_amd.utils import segment as S
    rng = np.random.default_rng(2)
    for _ in range(20):
        q = rng.standard_normal(4)
        ax, ang = S.quat2axangle(q)
        rax, rang = R.quat2axangle(q)
        assert np.allclose(ax, rax, atol=1e-15) and abs(ang - rang) < 1e-15
        w = q / np.linalg.norm(q)
        assert abs(np.cos(ang / 2) - w[0]) < 1e-12 and np.allclose(np.sin(ang / 2) * ax, w[1:], atol=1e-12)
    assert S.quat2axangle([1.0, 0.0, 0.0, 0.0])[1] == 0.0


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


_X = 0x1000          # a fake, never dereferenced address: every call below must fail in validation


def _fs(**kw):
    a = dict(f=1, h=480, w=640, depth=_X, label=_X, intr=_X, s=1, seg_frame=_X, seg_class=_X, thr=0.2, offsets=_X,
             xyz=_X, mean=_X, ws=_X, wsb=1 << 40)
    a.update(kw)
    return list(a.values()) + [None]


def _ro(**kw):
    a = dict(s=1, offsets=_X, xyz=_X, m=1000, nb=100, r=0.02, keep=512, in_off=_X, in_idx=_X, in_xyz=_X, nv=_X, ws=_X,
             wsb=1 << 40)
    a.update(kw)
    return list(a.values()) + [None]


def _fps(**kw):
    a = dict(s=1, offsets=_X, xyz=_X, m=1000, k=256, starts=_X, idx=_X, out=_X, ws=_X, wsb=1 << 40)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("fn, args, needle", [
    ("cloudaae_frame_segments", _fs(f=0), "f, h and w"), ("cloudaae_frame_segments", _fs(h=-1), "f, h and w"),
    ("cloudaae_frame_segments", _fs(w=-640), "f, h and w"), ("cloudaae_frame_segments", _fs(s=0), "s must"),
    ("cloudaae_frame_segments", _fs(s=-3), "s must"), ("cloudaae_frame_segments", _fs(f=1 << 20), "limit"),
    ("cloudaae_frame_segments", _fs(thr=float("nan")), "threshold"),
    ("cloudaae_frame_segments", _fs(wsb=16), "workspace"),
] + [("cloudaae_frame_segments", _fs(**{k: None}), "null") for k in
     ("depth", "label", "intr", "seg_frame", "seg_class", "offsets", "xyz", "mean", "ws")] + [
    ("cloudaae_radius_outlier", _ro(s=0), "s must"), ("cloudaae_radius_outlier", _ro(m=-1), "max_points"),
    ("cloudaae_radius_outlier", _ro(nb=-1), "nb_points"), ("cloudaae_radius_outlier", _ro(keep=-1), "min_keep"),
    ("cloudaae_radius_outlier", _ro(r=0.0), "radius"), ("cloudaae_radius_outlier", _ro(r=-0.02), "radius"),
    ("cloudaae_radius_outlier", _ro(wsb=16), "workspace"),
] + [("cloudaae_radius_outlier", _ro(**{k: None}), "null") for k in
     ("offsets", "xyz", "in_off", "in_idx", "in_xyz", "nv", "ws")] + [
    ("cloudaae_ragged_fps", _fps(s=0), "s must"), ("cloudaae_ragged_fps", _fps(s=-1), "s must"),
    ("cloudaae_ragged_fps", _fps(k=0), "k must"), ("cloudaae_ragged_fps", _fps(k=-5), "k must"),
    ("cloudaae_ragged_fps", _fps(m=-1), "max_points"), ("cloudaae_ragged_fps", _fps(wsb=16), "workspace"),
] + [("cloudaae_ragged_fps", _fps(**{k: None}), "null") for k in ("offsets", "xyz", "starts", "idx", "out", "ws")])
def test_invalid_arguments_are_rejected(cdll, fn, args, needle):
    from cloudaae_amd import _lib
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert fn in msg and needle in msg, msg


def test_workspace_queries(cdll):
    from cloudaae_amd import _lib
    L = _lib.lib()
    assert L.cloudaae_frame_segments_workspace_bytes(8, 480, 640, 21) > 8 * 480 * 640 * 16
    assert L.cloudaae_frame_segments_workspace_bytes(0, 480, 640, 21) == -1
    assert L.cloudaae_radius_outlier_workspace_bytes(21, 307200) > 307200 * 16
    assert L.cloudaae_radius_outlier_workspace_bytes(0, 10) == -1
    assert L.cloudaae_ragged_fps_workspace_bytes(1000) >= 8000 and L.cloudaae_ragged_fps_workspace_bytes(-1) == -1
    assert _lib.ABI_VERSION == 602 and cdll.cloudaae_version() == 602
