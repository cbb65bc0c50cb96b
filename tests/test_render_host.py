"""CPU: the NumPy restatement of DESIGN.md "Rendered frames" (tests/render_reference.py) on cases whose answers are known
without it, and the frame records of cloudaae_amd/utils/render.py read back by tfrecord_io.  The GPU test
(tests/test_25_render_gpu.py) then holds the kernel to the restatement bit for bit."""
import numpy as np
import pytest

import render_reference as R
from cloudaae_amd import tfrecord_io
from cloudaae_amd.utils import render as RD
from cloudaae_amd.utils import segment as S

EYE = np.eye(4)


def square(z=1.0, half=0.25):
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_fronto_parallel_square():
    """fx = fy = 64, cx = cy = 16: the square's corners project to 0 and 32 exactly, both edges inclusive."""
    intr = np.array([[64, 64, 16, 16, 1000]], np.float32)
    out = R.render([square()], [[(0, 1, EYE)]], intr, 40, 48)
    v, u = np.mgrid[0:40, 0:48]
    inside = (u <= 32) & (v <= 32)
    assert np.array_equal(out['depth'][0] != 0, inside)
    assert np.all(out['depth'][0][inside] == 1000) and np.all(out['label'][0][inside] == 1)
    assert np.all(out['label'][0][~inside] == 0) and np.all(out['tri'][0][~inside] == -1)
    # triangle 0 holds the corner (32, 0), triangle 1 the corner (0, 32); the diagonal u = v belongs to both: rank 0
    assert np.all(out['tri'][0][inside & (u >= v)] == 0) and np.all(out['tri'][0][inside & (u < v)] == 1)
    assert out['dropped'][0] == 0 and out['degenerate'][0] == 0
    assert list(out['box']) == [33 * 33, 33 * 33]


def test_tilted_plane_has_the_ray_plane_depth():
    intr = np.array([[300, 310, 79.5, 60.25, 10000]], np.float32)
    # one steep triangle, 0.5 .. 1.6 m deep, that reaches past three image borders
    v = np.array([[-0.3, -0.25, 0.5], [0.5, -0.2, 1.6], [-0.1, 0.45, 0.9]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    out = R.render([(v, t)], [[(0, 9, EYE)]], intr, 120, 160)
    covered = out['depth'][0] != 0
    assert covered.sum() > 5000
    p = v.astype(np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    vv, uu = np.mgrid[0:120, 0:160]
    d = np.stack([(uu - float(intr[0, 2])) / float(intr[0, 0]), (vv - float(intr[0, 3])) / float(intr[0, 1]), np.ones((120, 160))], -1)
    z_plane = (n @ p[0]) / (d @ n)                    # the ray t d meets the plane at t = z
    want = np.floor(10000.0 * z_plane + 0.5)
    err = np.abs(out['depth'][0].astype(np.float64) - want)[covered]
    print("tilted plane: %d pixels, depth %d .. %d units, largest difference %g" % (covered.sum(), out['depth'][0][covered].min(),
                                                                                 out['depth'][0].max(), err.max()))
    assert err.max() <= 1
    assert out['depth'][0].max() - out['depth'][0][covered].min() > 3000


def test_draw_order_breaks_ties_and_sets_the_label():
    intr = np.array([[64, 64, 16, 16, 1000]], np.float32)
    a = R.render([square()], [[(0, 3, EYE), (0, 7, EYE)]], intr, 40, 48)
    b = R.render([square()], [[(0, 7, EYE), (0, 3, EYE)]], intr, 40, 48)
    hit = a['depth'][0] != 0
    assert hit.sum() == 33 * 33 and np.array_equal(a['depth'], b['depth'])
    assert np.all(a['label'][0][hit] == 3) and np.all(b['label'][0][hit] == 7)
    assert a['tri'][0][hit].max() <= 1 and np.array_equal(a['tri'], b['tri'])
    # the nearer one wins whatever its rank
    near = R.render([square(), square(z=0.5, half=0.125)], [[(0, 3, EYE), (1, 7, EYE)]], intr, 40, 48)
    assert np.all(near['label'][0][hit] == 7) and np.all(near['depth'][0][hit] == 500) and near['tri'][0][hit].min() == 2


def test_near_plane_and_zero_area():
    intr = np.array([[64, 64, 16, 16, 1000]], np.float32)
    v = np.array([[0, 0, 1], [0.2, 0, 1], [0, 0.2, 0.04],           # one vertex behind z_near = 0.05
                  [0, 0, 1], [0.1, 0.1, 1], [0.2, 0.2, 1],          # collinear
                  [0, 0, 1], [0.2, 0, 1], [0, 0.2, 1]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 9]], np.int32)      # the last names a vertex outside the mesh
    out = R.render([(v, t)], [[(0, 1, EYE)]], intr, 40, 48)
    assert not out['depth'].any() and not out['label'].any() and np.all(out['tri'] == -1)
    assert out['dropped'][0] == 2 and out['degenerate'][0] == 1
    ok = R.render([(v, np.array([[6, 7, 8]], np.int32))], [[(0, 1, EYE)]], intr, 40, 48, z_near=0.05)
    assert ok['depth'].any() and ok['dropped'][0] == 0
    gone = R.render([(v, np.array([[6, 7, 8]], np.int32))], [[(0, 1, EYE)]], intr, 40, 48, z_near=1.5)
    assert not gone['depth'].any() and gone['dropped'][0] == 1
    # a vertex outside the guard band of 2^24 / 256 = 65536 pixels
    far = np.array([[0, 0, 1], [0.2, 0, 1], [1100.0, 0, 1]], np.float32)
    out = R.render([(far, np.array([[0, 1, 2]], np.int32))], [[(0, 1, EYE)]], intr, 40, 48)
    assert not out['depth'].any() and out['dropped'][0] == 1


def test_image_edge_is_a_crop():
    """Coordinates and intrinsics are dyadic, so moving the principal point by whole pixels moves every fixed-point
    vertex by exactly that many pixels."""
    v = np.array([[-0.5, -0.25, 1.0], [1.0, 0.125, 2.0], [0.0, 0.75, 0.5], [-1.0, 0.5, 1.0]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    small = R.render([(v, t)], [[(0, 5, EYE)]], np.array([[64, 64, 16.5, 12.25, 4096]], np.float32), 24, 32)
    big = R.render([(v, t)], [[(0, 5, EYE)]], np.array([[64, 64, 16.5 + 40, 12.25 + 56, 4096]], np.float32), 24 + 100, 32 + 100)
    d = small['depth'][0]
    assert d[-1].all() and d[:, 0].any() and d[:, -1].any() and not d[0].any()      # it leaves through three borders
    assert big['depth'][0].sum() > small['depth'][0].sum()
    for k in ('depth', 'label', 'tri'):
        assert np.array_equal(small[k][0], big[k][0][56:56 + 24, 40:40 + 32]), k


def _rodrigues(r):
    return R.pose_matrix(r, [0, 0, 0])[:3, :3]


def test_mat2quat():
    rng = np.random.default_rng(5)
    for r in list(rng.standard_normal((20, 3))) + [[np.pi, 0, 0], [0, np.pi - 1e-9, 0], [0, 0, 3.0], [0, 0, 0], [1e-9, 0, 0]]:
        Rm = _rodrigues(r)
        w, x, y, z = RD.mat2quat(Rm)
        back = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert w >= 0 and abs(w * w + x * x + y * y + z * z - 1) < 1e-14 and np.abs(back - Rm).max() < 1e-14


def test_record_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    F, H, W = 3, 12, 20
    depth = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    label = rng.integers(0, 22, (F, H, W)).astype(np.uint8)
    intr = np.array([[1066.778, 1067.487, 312.9869, 241.3109, 10000.0]] * F, np.float32) + np.arange(F, dtype=np.float32)[:, None]
    classes = [[0, 20], [], [7, 3, 12]]
    rots = {c: rng.standard_normal(3) * 0.9 for c in (0, 3, 7, 12, 20)}
    poses = [[R.pose_matrix(rots[c], rng.uniform(-0.3, 0.9, 3).astype(np.float32)) for c in cl] for cl in classes]
    recs = RD.frame_records(depth.view(np.int16), label, intr, poses, classes, 48, [5, 6, 9])
    path = str(tmp_path / "0048_pcnn.tfrecord")
    tfrecord_io.write_records(path, recs)
    back = tfrecord_io.read_frames(path, verify=True)
    assert len(back) == F
    worst = 0.0
    for f, fr in enumerate(back):
        assert np.array_equal(fr['depth'], depth[f]) and np.array_equal(fr['label'], label[f])
        assert fr['image'].shape == (H, W, 3) and not fr['image'].any()
        assert [float(fr[k]) for k in ('fx', 'fy', 'cx', 'cy', 'factor_depth')] == [float(x) for x in intr[f]]
        assert int(fr['seq_id']) == 48 and int(fr['frame_id']) == [5, 6, 9][f]
        hot = np.zeros(21, np.int64)
        hot[classes[f]] = 1
        assert np.array_equal(fr['class_one_hot'], hot)
        for c, pose in zip(classes[f], poses[f]):
            assert np.array_equal(fr['translations'][c], pose[:3, 3].astype(np.float32))
            got = _rodrigues(S.quat2axag(fr['quaternions'][c]).astype(np.float64))
            worst = max(worst, float(np.abs(got - pose[:3, :3]).max()))
        absent = [c for c in range(21) if c not in classes[f]]
        assert not fr['translations'][absent].any() and not fr['quaternions'][absent].any()
    print("rotation through float32 quaternion and float32 axis-angle: largest entry difference %g" % worst)
    assert worst <= 1e-6
    with pytest.raises(Exception):
        RD.frame_records(depth, label, intr, [[EYE, EYE], [], []], [[4, 4], [], []], 48, [0, 1, 2])
    with pytest.raises(Exception):
        RD.frame_records(depth, label, intr, [[EYE], [], []], [[21], [], []], 48, [0, 1, 2])
