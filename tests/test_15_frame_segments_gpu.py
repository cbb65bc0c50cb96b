"""GPU: evaluation inputs from RGB-D frames (cloudaae_frame_segments, cloudaae_radius_outlier, cloudaae_ragged_fps;
utils/segment.py; evaluate_cloudAAE_ycbv.element_from_frames and main) against the NumPy restatement of DESIGN.md
"Frame segments" (tests/segment_reference.py).  Every comparison is exact."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segment_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640
INTR = np.array([1066.778, 1067.487, 312.9869, 241.3109, 10000.0], np.float32)     # YCB-Video camera, factor_depth


def synthetic_frame(seed, classes=(0, 3, 7), absent=(), holes=0.05, flying=0.01):
    """640x480: a background plane (label 0) and one analytic surface per class (a sphere cap, a tilted plane, a
    cylinder), each in a box of pixels; random depth holes and flying pixels (far depth inside a class's label).
    Classes in `absent` are listed in class_one_hot but have no pixel."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = np.full((H, W), 1.3, np.float64) + 0.0002 * (u - W / 2)
    label = np.zeros((H, W), np.uint8)
    for k, c in enumerate(classes):
        u0, v0 = rng.integers(40, W - 200), rng.integers(40, H - 200)
        du, dv = rng.integers(60, 160), rng.integers(60, 160)
        box = (u >= u0) & (u < u0 + du) & (v >= v0) & (v < v0 + dv)
        z0 = rng.uniform(0.6, 1.0)
        cu, cv = u0 + du / 2, v0 + dv / 2
        if k % 3 == 0:
            z = z0 - 0.05 * np.sqrt(np.clip(1 - ((u - cu) / du) ** 2 - ((v - cv) / dv) ** 2, 0, 1))
        elif k % 3 == 1:
            z = z0 + 0.0004 * (u - cu) - 0.0003 * (v - cv)
        else:
            z = z0 - 0.04 * np.sqrt(np.clip(1 - ((u - cu) / (du / 2)) ** 2, 0, 1))
        depth[box] = z[box]
        if c not in absent:
            label[box] = c + 1
    fly = rng.random((H, W)) < flying
    depth[fly & (label > 0)] = rng.uniform(1.5, 3.0, (fly & (label > 0)).sum())
    d16 = np.round(depth * INTR[4]).astype(np.uint16)
    d16[rng.random((H, W)) < holes] = 0
    onehot = np.zeros(21, np.int64)
    onehot[list(classes)] = 1
    quat = rng.standard_normal((21, 4)).astype(np.float32)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    trans = (rng.standard_normal((21, 3)) * 0.1 + [0, 0, 0.8]).astype(np.float32)
    return dict(depth=d16, label=label, class_one_hot=onehot, quaternions=quat, translations=trans,
                image=rng.integers(0, 255, (H, W, 4), dtype=np.uint8), seq_id=np.int64(48), frame_id=np.int64(seed),
                fx=INTR[0], fy=INTR[1], cx=INTR[2], cy=INTR[3], factor_depth=INTR[4])


def _extract(frames, **kw):
    from cloudaae_amd.utils import segment as S
    depth = np.stack([f["depth"] for f in frames])
    label = np.stack([f["label"] for f in frames])
    intr = np.stack([INTR] * len(frames))
    classes = [list(np.nonzero(f["class_one_hot"])[0]) for f in frames]
    r = S.extract_segments(depth, label, intr, classes=classes, **kw)
    torch.cuda.synchronize()
    return r, classes


def _check_against_reference(r, frames, classes):
    ref = R.extract([(f["depth"], f["label"], INTR) for f in frames], classes)
    assert len(ref) == len(r.cls)
    for i, seg in enumerate(ref):
        assert (int(r.frame[i]), int(r.cls[i])) == (seg["frame"], seg["cls"])
        assert r.num_point_after_filter[i] == seg["num_point_after_filter"], i
        xyz, idx, xin = r.segment(i)
        assert np.array_equal(xyz.view(np.uint32), seg["xyz"].view(np.uint32)), i
        assert np.array_equal(r.mean[i].cpu().numpy().view(np.uint32), seg["mean"].view(np.uint32)), i
        assert np.array_equal(idx, seg["inlier_idx"]), i
        assert np.array_equal(xin.view(np.uint32), seg["xyz_inlier_full"].view(np.uint32)), i
        assert r.num_valid_points_in_segment[i] == seg["num_valid_points_in_segment"], i
    return ref


def test_frames_against_restatement(hip):
    frames = [synthetic_frame(1), synthetic_frame(2, classes=(1, 4, 5, 20), absent=(5,)),
              synthetic_frame(3, classes=(2,), holes=0.3, flying=0.05)]
    r, classes = _extract(frames)
    ref = _check_against_reference(r, frames, classes)
    sizes = [s["num_point_after_filter"] for s in ref]
    assert 0 in sizes and max(sizes) > 5000                         # the absent class, and real segments


def test_batch_independence_and_determinism(hip):
    frames = [synthetic_frame(11), synthetic_frame(12, classes=(6, 9)), synthetic_frame(13)]
    alone, _ = _extract(frames[1:2])
    batch, _ = _extract(frames)
    again, _ = _extract(frames)
    for k in range(len(alone.cls)):
        j = 3 + k
        for a, b in zip(alone.segment(k), batch.segment(j)):
            assert np.array_equal(a, b)
    for name in ("offsets", "inlier_offsets", "num_valid_points_in_segment"):
        assert np.array_equal(getattr(batch, name), getattr(again, name))
    for i in range(len(batch.cls)):
        for a, b in zip(batch.segment(i), again.segment(i)):
            assert np.array_equal(a, b)
    from cloudaae_amd.utils import segment as S
    s1 = S.sample_segments(batch, 256, seed=5)
    s2 = S.sample_segments(batch, 256, seed=5)
    for k in ("xyz_inlier", "xyz", "idx_inlier", "idx"):
        assert torch.equal(s1[k], s2[k]), k


def _packed(sets):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    xyz = np.concatenate([s for s in sets if len(s)] or [np.zeros((0, 3), np.float32)]).astype(np.float32)
    return off, xyz


def _radius_gpu(sets, nb_points=100, radius=np.float32(0.02), min_keep=512):
    from cloudaae_amd import _lib
    off, xyz = _packed(sets)
    M = max(len(xyz), 1)
    S = len(sets)
    d_off = torch.from_numpy(off).cuda()
    d_xyz = torch.zeros((M, 3), dtype=torch.float32, device="cuda")
    d_xyz[:len(xyz)] = torch.from_numpy(xyz).cuda()
    in_off = torch.empty(S + 1, dtype=torch.int32, device="cuda")
    in_idx = torch.empty(M, dtype=torch.int32, device="cuda")
    in_xyz = torch.empty((M, 3), dtype=torch.float32, device="cuda")
    nv = torch.empty(S, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    nbytes = int(L.cloudaae_radius_outlier_workspace_bytes(S, M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.cloudaae_radius_outlier(S, d_off.data_ptr(), d_xyz.data_ptr(), M, nb_points, float(radius), min_keep,
                                         in_off.data_ptr(), in_idx.data_ptr(), in_xyz.data_ptr(), nv.data_ptr(),
                                         ws.data_ptr(), nbytes, _lib.stream()), "cloudaae_radius_outlier")
    torch.cuda.synchronize()
    io = in_off.cpu().numpy()
    idx = in_idx.cpu().numpy()
    return [idx[io[i]:io[i + 1]].astype(np.int64) for i in range(S)], nv.cpu().numpy()


def _ball(rng, n, centre, spread):
    return (centre + rng.uniform(-spread, spread, (n, 3))).astype(np.float32)


def test_radius_edges(hip):
    rng = np.random.default_rng(7)
    r2 = R.radius_sq()
    base = np.array([0.5, -0.25, 0.75], np.float32)
    # three points on the x axis around d^2 = r^2: the float below, at and above base + r
    x = np.float32(base[0] + np.float32(0.02))
    edge = [np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))]
    ring = np.array([[e, base[1], base[2]] for e in edge], np.float32)
    d2 = [(float(e) - float(base[0])) ** 2 for e in edge]
    assert min(d2) < r2 <= max(d2)
    big = _ball(rng, 600, np.array([2.0, 2.0, 2.0]), 0.005)                  # every point: > 100 neighbours
    c101 = _ball(rng, 101, np.array([3.0, 0.0, 0.0]), 0.004)                 # exactly 101, the query included
    c100 = _ball(rng, 100, np.array([4.0, 0.0, 0.0]), 0.004)                 # exactly 100: not kept
    dup = np.repeat(_ball(rng, 1, np.array([5.0, 0.0, 0.0]), 0.0), 101, axis=0)   # 101 duplicates: kept
    near = _ball(rng, 99, base, 1e-4)                                        # base + 99: the edge point decides
    sets = [
        np.concatenate([c101, big, c100, base[None]]),                   # point 0 inside the inliers
        np.concatenate([c100, big, c101, dup]),                          # point 0 outside
        np.concatenate([c101, c100]),                                    # fewer than 512 keepers: all kept
        np.zeros((0, 3), np.float32),                                    # empty
        big[:1],
    ] + [np.concatenate([base[None], near, ring[None, e], big]) for e in range(3)]   # d^2 below, at / above r^2
    counts0 = [R.neighbour_counts_brute(s)[0] for s in sets[-3:]]
    assert counts0[0] == 101 and counts0[2] == 100                           # the base point: 101, then 100
    got, nv = _radius_gpu(sets)
    for i, s in enumerate(sets):
        counts = R.neighbour_counts_brute(s) if len(s) else np.zeros(0, np.int64)
        want, want_nv = R.radius_outlier(s, counts=counts)
        assert np.array_equal(got[i], want), i
        assert nv[i] == want_nv, i
    assert 0 in got[0] and 0 not in got[1] and len(got[2]) == len(sets[2])
    assert nv[0] == len(got[0]) - 1 and nv[1] == len(got[1])


def test_ragged_fps_mixed_sizes(hip):
    from cloudaae_amd.utils import segment as S
    rng = np.random.default_rng(3)
    grid = np.stack(np.meshgrid(*[np.arange(6, dtype=np.float32) * 0.01] * 3), -1).reshape(-1, 3)   # ties
    sets = [rng.standard_normal((1, 3)), rng.standard_normal((5, 3)), grid,
            np.repeat(rng.standard_normal((3, 3)), 40, axis=0),                                           # duplicates
            rng.standard_normal((3000, 3)) * 0.1, rng.standard_normal((20000, 3)) * 0.1,
            rng.standard_normal((120000, 3)) * 0.1, np.zeros((0, 3))]
    sets = [np.asarray(s, np.float32) for s in sets]
    off, xyz = _packed(sets)
    K = 256
    starts = np.array([0, 4, 17, 1, 2999, 12345, 110000, 0], np.int32)
    idx, pts = S.ragged_fps(torch.from_numpy(off).cuda(), torch.from_numpy(xyz).cuda(), K, starts)
    idx, pts = idx.cpu().numpy(), pts.cpu().numpy()
    for i, s in enumerate(sets):
        if len(s) == 0:
            assert (idx[i] == -1).all()
            continue
        want = R.fps(s, K, int(starts[i]))
        assert np.array_equal(idx[i], want), i
        assert np.array_equal(pts[i], s[want]), i


def _write_records(tmp, frames, seq=48):
    from cloudaae_amd import tfrecord_io as io
    keys = ("quaternions", "translations", "class_one_hot", "seq_id", "frame_id", "fx", "fy", "cx", "cy",
            "factor_depth")
    payloads = []
    for f in frames:
        d = {k: f[k] for k in keys}
        d.update(image=f["image"].tobytes(), image_shape=np.array(f["image"].shape), depth=f["depth"].astype("<u2").tobytes(),
                 depth_shape=np.array(f["depth"].shape), label=f["label"].tobytes(), label_shape=np.array(f["label"].shape))
        payloads.append(io.encode_example(d))
    path = os.path.join(str(tmp), "%04d_pcnn.tfrecord" % seq)
    io.write_records(path, payloads)
    return path


@pytest.fixture(scope="module")
def models():
    from cloudaae_amd import tfrecord_io
    m, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    return m


def test_element_from_frames_end_to_end(hip, tmp_path, models):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import hidden_point_removal as hpr
    from cloudaae_amd.utils import segment as S
    frames = [synthetic_frame(21, classes=(0, 4)), synthetic_frame(22, classes=(3,)),
              synthetic_frame(23, classes=(0, 2), holes=0.995), synthetic_frame(24, classes=(0, 5))]
    path = _write_records(tmp_path, frames)
    read = tfrecord_io.read_frames(path, verify=True)
    N, seed = 256, 9
    el = E.element_from_frames(read, 0, N, models, seed=seed)
    torch.cuda.synchronize()
    # the restatement: frames holding class 0, its segment, the two rules, FPS from the same seeded starts
    with0 = [f for f in read if f["class_one_hot"][0] == 1]
    ref = R.extract([(f["depth"], f["label"], INTR) for f in with0], [[0]] * len(with0))
    sizes = np.array([[len(s["inlier_idx"]), s["num_point_after_filter"]] for s in ref]).reshape(-1)
    starts = S.random_starts(sizes, np.random.default_rng(seed)).reshape(-1, 2)
    kept = [i for i, s in enumerate(ref) if s["num_point_after_filter"] > 100 and s["num_valid_points_in_segment"] >= N]
    assert len(kept) == 2 and el["class_id"].shape == (2,)             # the frame with 99.5 % holes is dropped
    for b, i in enumerate(kept):
        s = ref[i]
        want = s["xyz_inlier_full"][R.fps(s["xyz_inlier_full"], N, int(starts[i, 0]))]
        assert np.array_equal(el["xyz_inlier"][b].cpu().numpy(), want), b
        want = s["xyz"][R.fps(s["xyz"], N, int(starts[i, 1]))]
        assert np.array_equal(el["xyz"][b].cpu().numpy(), want), b
        f = with0[i]
        assert np.array_equal(el["translation"][b].cpu().numpy(), f["translations"][0])
        np.testing.assert_allclose(el["axisangle"][b].cpu().numpy(), R.quat2axag(f["quaternions"][0]), atol=1e-6)
    assert (el["class_id"] == 0).all()
    # visiblePoints_org: the existing HPR path on the same poses
    mt = torch.from_numpy(models).cuda()
    x = dict(class_id=el["class_id"], translation=el["translation"], axisangle=el["axisangle"].clone())
    x = T.transform_object_model(T.get_rotation_matrix(T.get_object_model(x, mt)))
    x = hpr.hidden_point_removal_org(hpr.sphericalFlip_org(x, None, 0.8 * math.pi), seed=seed)
    assert torch.equal(el["visiblePoints_org"], x["visiblePoints_org"])
    assert torch.equal(el["obj_batch"], mt[el["class_id"]])
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": 2})
    out = E.evaluate_batch(graph, {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}, icp=True)
    for k in ("trans_loss", "axag_loss", "xyz_loss", "trans_loss_icp", "axag_loss_icp"):
        assert torch.isfinite(out[k]).all(), k


def test_cli_on_written_records(hip, tmp_path, models):
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    data = tmp_path / "data"
    data.mkdir()
    _write_records(data, [synthetic_frame(31, classes=(0, 4)), synthetic_frame(32, classes=(0,))])
    obj = tmp_path / "obj_models.tfrecords"
    rec = tfrecord_io.encode_example({"label": np.array([0]), "model": models[0].reshape(-1)})
    tfrecord_io.write_records(str(obj), [rec])
    graph = T.TrainGraph({"num_point": 256, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp_path / "model.ckpt"))
    cmd = [sys.executable, "-c", "import sys; from cloudaae_amd.evaluate_cloudAAE_ycbv import main; sys.exit(main())",
           "--data_dir", str(data), "--object_model", str(obj), "--trained_model", ckpt[:-len(".npz")],
           "--target_cls", "0", "--num_point", "256", "--batch_size", "1", "--icp", "--seed", "3"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert sum(line.startswith("Validation batch") for line in lines) == 2, p.stdout
    assert lines[-2] == "batch size 2" and lines[-1].startswith("trans_loss "), p.stdout
