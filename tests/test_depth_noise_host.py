"""CPU: the NumPy restatement of DESIGN.md "Sensor noise" (tests/depth_noise_reference.py) tied to the definition by
cases worked by hand, the argument checks of cloudaae_depth_normals / cloudaae_depth_sensor_noise (C ABI revision 602,
which must fail before they touch memory), and the comparison rule of tests/test_27_depth_noise_gpu.py, fixed here before
any GPU run: the margin around a decision point is measured (10 x the largest change that the float32 normal2 makes
against the float64 one, floored at 1e-6), printed, compared with profiles/notes_depth_noise.md, and the share of
unsettled pixels is asserted to stay within 2 % on every input of the GPU tests."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import depth_noise_reference as D
import pose_sampling_reference as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")
NOTES = os.path.join(ROOT, "profiles", "notes_depth_noise.md")
KINECT_INTR = np.array([1066.778, 1067.487, 312.9869, 241.3109, 10000.0], np.float32)


# ---- anchors -----------------------------------------------------------------------------------------------------------
def test_preset_none_is_the_identity():
    from cloudaae_amd.utils import depth_noise
    assert depth_noise.sensor_params('none') == D.NONE and depth_noise.sensor_params('kinect1') == D.KINECT1
    assert depth_noise.PARAMS == D.PARAMS
    for name in D.scenes():
        depth, label, intr = D.rendered(name)
        r = D.apply(depth, label, intr, D.NONE, seed=5, first_frame=3)
        assert np.array_equal(r['depth'], depth) and np.array_equal(r['label'], label)
        assert np.array_equal(r['counts'][:, 0], (depth != 0).reshape(len(depth), -1).sum(axis=1))
        assert not r['counts'][:, 1:].any()
        assert np.array_equal(r['z_noisy'], depth / np.float64(1.0) / intr[:, 4].astype(np.float64)[:, None, None])


def test_constant_depth_faces_the_camera():
    """Depth 8000 units everywhere: gx = (2 dm / fx, 0, 0), gy = (0, 2 dm / fy, 0), so the normal is (0, 0, -1) and
    theta is the angle of the viewing ray to the optical axis, acos(z / |P|)."""
    H, W = 9, 11
    depth, label = np.full((H, W), 8000, np.uint16), np.ones((H, W), np.uint8)
    normal, theta, flat = D.slope(depth, label, KINECT_INTR)
    assert not flat.any()
    assert np.array_equal(normal, np.broadcast_to([0.0, 0.0, -1.0], (H, W, 3)))
    fx, fy, cx, cy = (float(k) for k in KINECT_INTR[:4])
    v, u = np.mgrid[0:H, 0:W]
    want = np.arccos(1.0 / np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0))
    assert np.abs(theta - want).max() < 1e-12
    # a single pixel and a single row have no slope: flat
    one = np.zeros((H, W), np.uint16)
    one[4, 5] = 8000
    assert D.slope(one, label, KINECT_INTR)[2].sum() == 1
    row = np.zeros((H, W), np.uint16)
    row[4] = 8000
    n, t, fl = D.slope(row, label, KINECT_INTR)
    assert fl.sum() == W and not n.any() and not t.any()
    # a neighbour of another label does not count: two columns of label 2 inside label 1 keep their one-sided slope
    lab = label.copy()
    lab[:, 5:7] = 2
    n2, _, fl2 = D.slope(depth, lab, KINECT_INTR)
    assert not fl2.any() and np.array_equal(n2, normal)


def test_tilted_plane_has_the_analytic_normal():
    """The plane z = zc + alpha x sampled by the camera: z(u) = zc / (1 - alpha (u - cx) / fx).  From the metric depths
    the central differences lie in the plane, so the normal is (alpha, 0, -1) / sqrt(1 + alpha^2) to rounding.  From the
    depth values (rounded to the unit) each difference moves by at most one unit 1 / factor along z against a length of
    at least 2 z / fx (2 z / fy), so the normal turns by at most sqrt((fx / (2 z factor))^2 + (fy / (2 z factor))^2)."""
    H, W, zc, alpha = 24, 32, 0.75, 0.6
    fx, fy, cx, cy, factor = (np.float64(k) for k in KINECT_INTR)
    v, u = np.mgrid[0:H, 0:W]
    dm = zc / (1.0 - alpha * (u - cx) / fx)
    label = np.ones((H, W), np.uint8)
    want = np.array([alpha, 0.0, -1.0]) / math.sqrt(1.0 + alpha * alpha)
    exact = D.slope_dm(dm, np.ones((H, W), bool), label, KINECT_INTR)[0]
    assert np.abs(exact - want).max() < 1e-9
    depth = np.floor(dm * factor + 0.5).astype(np.uint16)
    got = D.slope(depth, label, KINECT_INTR)[0]
    turn = np.arccos(np.clip((got * want).sum(axis=-1), -1.0, 1.0)).max()
    bound = math.hypot(fx / (2.0 * dm.min() * factor), fy / (2.0 * dm.min() * factor))
    print("plane: the depth unit turns a normal by at most %.3e rad (bound %.3e)" % (turn, bound))
    assert 0.0 < turn <= bound


def test_one_pixel_through_the_five_stages_by_hand():
    """Pixel (u, v) = (3, 2) of a 6 x 5 frame on a tilted plane, every stage in scalar arithmetic."""
    H, W, seed, g = 5, 6, 77, 9
    intr = np.array([60.0, 61.0, 2.6, 2.2, 1000.0], np.float32)
    fx, fy, cx, cy, factor = (float(k) for k in intr)
    v, u = np.mgrid[0:H, 0:W]
    depth = (900 + 40 * u + 15 * v).astype(np.uint16)
    label = np.full((H, W), 7, np.uint8)
    label[0, :] = 3
    p = dict(D.KINECT1, sigma_l=1.3, p_drop=0.25)
    r = D.apply(depth[None], label[None], intr[None], p, seed=seed, first_frame=g)
    flats = 0
    for (pu, pv) in ((3, 2), (0, 0), (5, 4), (2, 1), (4, 0), (1, 3)):
        ctr = (g << 24) + pv * W + pu
        w = PS.philox4x32(seed, [ctr], D.STREAM_NORMALS)[0]
        q = PS.philox4x32(seed, [ctr], D.STREAM_DROP)[0]
        n_u, n_v = (float(x[0]) for x in PS.normal2(w[0:1], w[1:2]))
        n_z = float(PS.normal2(w[2:3], w[3:4])[0][0])
        su = min(max(pu + round(n_u * 1.3), 0), W - 1)          # (Python rounds halves to even, like rint)
        sv = min(max(pv + round(n_v * 1.3), 0), H - 1)
        assert r['label'][0, pv, pu] == label[sv, su]

        def P(a, b):
            dm = float(depth[b, a]) / factor
            return np.array([((a - cx) * dm) / fx, ((b - cy) * dm) / fy, dm])

        def ok(a, b):
            return 0 <= a < W and 0 <= b < H and label[b, a] == label[sv, su]
        ends, flat = [], False
        for da, db in ((1, 0), (0, 1)):
            flat = flat or not (ok(su + da, sv + db) or ok(su - da, sv - db))      # an axis without a neighbour
            hi = P(su + da, sv + db) if ok(su + da, sv + db) else P(su, sv)
            lo = P(su - da, sv - db) if ok(su - da, sv - db) else P(su, sv)
            ends.append(hi - lo)
        gx, gy = ends
        n = np.array([gx[1] * gy[2] - gx[2] * gy[1], gx[2] * gy[0] - gx[0] * gy[2], gx[0] * gy[1] - gx[1] * gy[0]])
        ray = P(su, sv)
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]      # noqa: E731
        theta_raw = 0.0 if flat else \
            math.acos(min(abs(dot(n, ray)) / (math.sqrt(dot(n, n)) * math.sqrt(dot(ray, ray))), 1.0))
        flats += flat
        z = float(depth[sv, su]) / factor
        theta = min(theta_raw, p['theta_max'])
        sigma = (p['a0'] + p['a1'] * ((z - p['z0']) * (z - p['z0']))) + \
            ((p['a2'] / math.sqrt(z)) * (theta * theta)) / ((D.HALF_PI - theta) * (D.HALF_PI - theta))
        zn = z + n_z * sigma
        assert r['z_noisy'][0, pv, pu] == zn
        if theta_raw > p['theta_drop'] or int(q[0]) < math.floor(0.25 * 2 ** 32):
            want = 0
        else:
            fb = fx * p['baseline']
            k = round((fb / zn) / p['disparity_step'])
            zq = fb / (k * p['disparity_step'])
            du = math.floor(zq * factor + 0.5)
            want = du if k >= 1 and 1 <= du <= 65535 else 0
        assert r['depth'][0, pv, pu] == want, (pu, pv)
    print("flat sources among the six pixels: %d" % flats)
    c = r['counts'][0]
    assert c[0] == H * W and c[2] > 0 and c[0] - c[1] - c[2] - c[3] == (r['depth'] != 0).sum()


def test_frames_do_not_depend_on_the_launch_split():
    depth, label, intr = D.rendered('planes_48x64')
    whole = D.apply(depth, label, intr, D.KINECT1, seed=4, first_frame=0)
    alone = D.apply(depth[1:2], label[1:2], intr[1:2], D.KINECT1, seed=4, first_frame=1)
    for k in ('depth', 'label', 'z_noisy', 'counts'):
        assert np.array_equal(whole[k][1], alone[k][0]), k
    other = D.apply(depth[1:2], label[1:2], intr[1:2], D.KINECT1, seed=4, first_frame=0)
    assert not np.array_equal(other['depth'], alone['depth'])


def test_range_and_disparity_losses_are_counted():
    depth, label, intr = D.rendered('sphere_37x70')
    far = D.apply(depth, label, intr, dict(D.NONE, baseline=0.0005, disparity_step=0.125))     # disparities below half a step
    assert far['counts'][0, 3] == far['counts'][0, 0] and not far['depth'].any()
    k = intr.copy()
    k[:, 4] = 60000.0                                                                             # 1 m -> 60000 units
    deep = D.apply((depth.astype(np.int64) * 60).clip(0, 65535).astype(np.uint16), label, k, dict(D.NONE, a0=0.05), seed=2)
    assert 0 < deep['counts'][0, 3] < deep['counts'][0, 0]


# ---- the comparison rule of the GPU tests ------------------------------------------------------------------------------------
def test_margin_is_measured_and_the_unsettled_share_stays_within_the_cap():
    margin = D.measured_margin()
    print("margin around a decision point: %.4e" % margin)
    assert D.MARGIN_FLOOR <= margin < 1e-2
    for case in D.CASES:
        r32, r64 = D.case_results(case)
        un = D.unsettled(r64, D.STAGES[case[1]], margin)
        with_depth = int((D.rendered(case[0])[0] != 0).sum())
        share = un.sum() / with_depth
        outside = (r32['depth'] != r64['depth']) | (r32['label'] != r64['label'])
        print("%-13s %-9s unsettled %3d of %d (%.2f %%)" % (case[0], case[1], un.sum(), with_depth, 100.0 * share))
        assert share <= D.UNSETTLED_CAP, case
        # the rule holds inside the restatement: float32 and float64 draws agree at every settled pixel
        assert not (outside & ~un).any(), case
        assert np.abs(r32['counts'].astype(np.int64) - r64['counts']).sum() <= un.sum()
    # the notes quote the margin (two digits: the last ones follow the host's libm)
    text = open(NOTES).read()
    quoted = float(re.search(r"margin = ([0-9.e+-]+)", text).group(1))
    assert abs(quoted - margin) <= 0.05 * margin, (quoted, margin)


def test_slope_tolerance_is_measured():
    tn, tt = D.slope_tolerance()
    print("tolerance of normals %.3e, of theta %.3e" % (tn, tt))
    assert 4 * 2.0 ** -23 <= tn < 1e-5 and 4 * 2.0 ** -23 <= tt < 1e-5


# ---- argument checks, through the C entry ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_symbols_and_signatures(cdll):
    from cloudaae_amd import _lib
    I, U, P, Dd = ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_double
    want = {"cloudaae_depth_normals": [I, I, I] + [P] * 7,
            "cloudaae_depth_sensor_noise": [I, I, I, P, P, P, U, U] + [Dd] * 10 + [P] * 5}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read(), flags=re.S)
    for fn, sig in want.items():
        assert _lib._SIGNATURES[fn] == sig
        f = getattr(cdll, fn)
        assert list(f.argtypes) == sig and f.restype is ctypes.c_int
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % fn, header).group(1)
        assert len(decl.split(",")) == len(sig), decl
    assert _lib.ABI_VERSION == 602 and cdll.cloudaae_version() == 602


_X = 0x1000          # a fake, never dereferenced address: every call below must fail in validation
_N, _S = "cloudaae_depth_normals", "cloudaae_depth_sensor_noise"


def _dn(**kw):
    a = dict(f=2, h=48, w=64, depth=_X, label=_X, intr=_X, normals=_X, theta=None, flat=_X)
    a.update(kw)
    return list(a.values()) + [None]


def _sn(**kw):
    a = dict(f=2, h=48, w=64, depth=_X, label=_X, intr=_X, seed=1, first=0)
    a.update(D.KINECT1)
    a.update(depth_out=_X, label_out=_X, counts=_X, z=None)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("fn, args, needle", [
    (_N, _dn(f=0), "limits"), (_N, _dn(h=-1), "limits"), (_N, _dn(w=0), "limits"),
    (_N, _dn(h=4097, w=4096), "limits"), (_N, _dn(f=17, h=4096, w=4096), "limits"),
] + [(_N, _dn(**{k: None}), "null") for k in ("depth", "label", "intr", "normals", "flat")] + [
    (_S, _sn(f=0), "limits"), (_S, _sn(w=-5), "limits"), (_S, _sn(h=4097, w=4096), "limits"),
    (_S, _sn(f=65, h=2048, w=2048), "limits"),
    (_S, _sn(first=1 << 40), "2^40"), (_S, _sn(first=(1 << 40) - 1), "2^40"),
    (_S, _sn(sigma_l=-0.1), "sigma_l"), (_S, _sn(sigma_l=float("nan")), "sigma_l"),
    (_S, _sn(theta_max=math.pi / 2), "theta_max"), (_S, _sn(theta_max=2.0), "theta_max"), (_S, _sn(theta_max=-0.1), "theta_max"),
    (_S, _sn(p_drop=-0.01), "p_drop"), (_S, _sn(p_drop=1.01), "p_drop"), (_S, _sn(p_drop=float("nan")), "p_drop"),
    (_S, _sn(disparity_step=-1.0), "disparity_step"), (_S, _sn(a1=float("inf")), "finite"),
] + [(_S, _sn(**{k: None}), "null") for k in ("depth", "label", "intr", "depth_out", "label_out", "counts")])
def test_invalid_arguments_are_rejected(cdll, fn, args, needle):
    from cloudaae_amd import _lib
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert fn in msg and needle in msg, msg


def test_wrapper_argument_checks():
    from cloudaae_amd.utils import depth_noise as DN
    for bad in (dict(sigma_l=-1.0), dict(theta_max=math.pi / 2), dict(p_drop=1.5), dict(disparity_step=-0.1),
                dict(a0=float("nan")), dict(gain=1.0)):
        with pytest.raises(ValueError):
            DN.sensor_params('kinect1', **bad)
    with pytest.raises(ValueError):
        DN.sensor_params('kinect2')
    assert DN.sensor_params('kinect1', p_drop=0.1)['p_drop'] == 0.1
    d, lab = np.zeros((1, 4, 4), np.uint16), np.zeros((1, 4, 4), np.uint8)
    with pytest.raises(ValueError, match="factor_depth"):
        DN._frames(d, lab, np.array([[60, 60, 2, 2, 0]], np.float32))
    with pytest.raises(ValueError, match="intrinsics"):
        DN._frames(d, lab, np.zeros((2, 5), np.float32))
