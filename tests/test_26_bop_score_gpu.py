"""GPU: cloudaae_vsd_counts and cloudaae_pose_max_dist through the C ABI against the NumPy restatement of DESIGN.md "BOP
pose errors (VSD, MSSD, MSPD)" (tests/bop_score_reference.py), then utils/bop_score.py through the renderer and the
evaluation's command line.

Every output of cloudaae_vsd_counts is an integer and is compared for equality, no pixel left out; mssd and mspd are
maxima and minima of fp64 expressions written in the definition's order and are compared bit for bit.  Outputs sit
between guard rows."""
import os

import numpy as np
import pytest
import torch

import bop_score_reference as BR
import mesh_models_reference as MR
import render_reference as R

pytestmark = pytest.mark.gpu

GUARD = 4                  # rows kept before and after every output
FILL = 0xA5
H, W = 45, 70              # no multiple of 8 or 64


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_25_render_gpu.py)."""

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


def launch_counts(hip, dev, dt, intr, frame_of, dg, de, delta, tau):
    """cloudaae_vsd_counts on guarded outputs -> dict like bop_score_reference.vsd_counts's."""
    F, h, w = dt.shape
    B, P = de.shape[:2]
    K = tau.shape[1]
    g = [_d(dt.view(np.int16), np.int16, dev), _d(intr, np.float32, dev), _d(frame_of, np.int32, dev),
         _d(dg.view(np.int16), np.int16, dev), _d(de.view(np.int16), np.int16, dev), _d(tau, np.float64, dev)]
    inter, uni = Guarded(B, P, torch.int32, dev), Guarded(B, P, torch.int32, dev)
    over, visib = Guarded(B * P, K, torch.int32, dev), Guarded(B, 1, torch.int32, dev)
    hip.check(hip.lib().cloudaae_vsd_counts(F, h, w, g[0].data_ptr(), g[1].data_ptr(), B, P, g[2].data_ptr(), g[3].data_ptr(),
                                            g[4].data_ptr(), float(delta), K, g[5].data_ptr(), inter.ptr(), uni.ptr(),
                                            over.ptr(), visib.ptr(), hip.stream()), "cloudaae_vsd_counts")
    torch.cuda.synchronize()
    return dict(inter=inter.numpy().copy(), union=uni.numpy().copy(), over=over.numpy().reshape(B, P, K).copy(),
                visib_gt=visib.numpy().ravel().copy())


def assert_counts_equal(got, want, what):
    for k in ('inter', 'union', 'over', 'visib_gt'):
        print("%s: %s differs in %d of %d entries" % (what, k, int((got[k] != want[k]).sum()), want[k].size))
    for k in ('inter', 'union', 'over', 'visib_gt'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


# ---- (a) counts on crafted images --------------------------------------------------------------------------------------------
DELTA_A = 16.0 / 1024.0


def _crafted(K):
    """F = 2, B = 3 (frame_of 1, 0, 1), P = 2.  Depths lie around 1000 units with about 30 % zeros, so that differences fall
    on both sides of delta and of every tau.  Frame 1 has fx = fy = 2^100 and factor 1024: xn xn + yn yn vanishes against
    1, so m = 1 everywhere and D(d) = d / 1024 exactly.  Rows 0 and 1 of sample 0 hit D(dg) - D(dt) = delta exactly, row 0
    with |D(dg) - D(de)| = tau_k exactly (k = 1 + column mod K) and row 1 one depth unit below it; row 2 misses delta by one
    unit, so it is visible only under pose 1, whose depths lie in front."""
    rng = np.random.default_rng(26)
    F, B, P = 2, 3, 2

    def image(*shape):
        d = rng.integers(960, 1041, shape)
        return np.where(rng.random(shape) < 0.3, 0, d).astype(np.uint16)
    dt, dg, de = image(F, H, W), image(B, H, W), image(B, P, H, W)
    intr = np.array([[60.0, 61.0, 34.6, 22.3, 1000.0], [2.0 ** 100, 2.0 ** 100, 35.0, 22.0, 1024.0]], np.float32)
    frame_of = np.array([1, 0, 1], np.int32)
    tau = np.stack([np.arange(1, K + 1) * 8.0 / 1024.0, np.linspace(0.004, 0.05, K), np.arange(1, K + 1) * 3.0 / 1024.0])
    k = 1 + np.arange(W) % K
    dg[0, 0:3] = 2048
    dt[1, 0:2], dt[1, 2] = 2032, 2031                    # D(dg) - D(dt) = 16 / 1024 = delta; 17 / 1024 in row 2
    de[0, 0, 0], de[0, 0, 1], de[0, 0, 2] = 2048 + 8 * k, 2048 + 8 * k - 1, 2048 + 8 * k       # |D(dg) - D(de)| = tau_k; a unit less
    de[0, 1, 0], de[0, 1, 1], de[0, 1, 2] = 2048 - 8 * k, 2048 - 8 * k + 1, 2048 - 8 * k       # the same in front
    return dt, intr, frame_of, dg, de, tau


@pytest.fixture(scope="module")
def crafted():
    return _crafted(10)


@pytest.fixture(scope="module")
def crafted_ref(crafted):
    dt, intr, frame_of, dg, de, tau = crafted
    return BR.vsd_counts(dt, intr, frame_of, dg, de, DELTA_A, tau)


@pytest.fixture(scope="module")
def crafted_got(hip, dev, crafted):
    dt, intr, frame_of, dg, de, tau = crafted
    return launch_counts(hip, dev, dt, intr, frame_of, dg, de, DELTA_A, tau)


def test_counts_on_crafted_images(crafted, crafted_got, crafted_ref):
    dt, intr, frame_of, dg, de, tau = crafted
    assert BR.distance_image(dg[0], intr[1])[0, 0] == 2.0            # m = 1 in frame 1
    # the crafted rows decide what they were built for: the exact hits count, the near misses do not.  Each k owns 7 columns.
    rows = BR.vsd_counts(dt[:, 0:3], intr, frame_of[:1], dg[:1, 0:3], de[:1, :, 0:3], DELTA_A, tau[:1])
    assert rows['visib_gt'][0] == 2 * W and rows['inter'][0].tolist() == [2 * W, 2 * W] and rows['union'][0].tolist() == [2 * W, 3 * W]
    hits = [7 * (11 - j) + 7 * (10 - j) for j in range(1, 11)]       # row 0: k >= j; row 1: k >= j + 1
    assert rows['over'][0].tolist() == [hits, hits]
    assert_counts_equal(crafted_got, crafted_ref, "crafted K = 10")
    assert crafted_ref['inter'].min() > 100 and (crafted_ref['union'] > crafted_ref['inter']).all()
    assert (np.diff(crafted_ref['over'], axis=2) <= 0).all() and crafted_ref['over'][:, :, 0].min() > 0


@pytest.mark.parametrize("K", [1, 16])
def test_counts_with_one_and_sixteen_thresholds(hip, dev, K):
    dt, intr, frame_of, dg, de, tau = _crafted(K)
    got = launch_counts(hip, dev, dt, intr, frame_of, dg, de, DELTA_A, tau)
    assert_counts_equal(got, BR.vsd_counts(dt, intr, frame_of, dg, de, DELTA_A, tau), "crafted K = %d" % K)


# ---- (c) independence of the batch and of the run -------------------------------------------------------------------------------
def test_samples_do_not_depend_on_the_batch(hip, dev, crafted, crafted_got):
    dt, intr, frame_of, dg, de, tau = crafted
    for b in range(3):
        alone = launch_counts(hip, dev, dt, intr, frame_of[b:b + 1], dg[b:b + 1], de[b:b + 1], DELTA_A, tau[b:b + 1])
        for k in ('inter', 'union', 'over', 'visib_gt'):
            assert np.array_equal(alone[k][0], crafted_got[k][b]), (b, k)
    again = launch_counts(hip, dev, dt, intr, frame_of, dg, de, DELTA_A, tau)
    for k in ('inter', 'union', 'over', 'visib_gt'):
        assert np.array_equal(again[k].view(np.uint8), crafted_got[k].view(np.uint8)), k


def test_frame_outside_the_frames_gives_zero_counts(hip, dev, crafted, crafted_got):
    dt, intr, frame_of, dg, de, tau = crafted
    got = launch_counts(hip, dev, dt, intr, np.array([1, 2, -1], np.int32), dg, de, DELTA_A, tau)
    for k in ('inter', 'union', 'over', 'visib_gt'):
        assert np.array_equal(got[k][0], crafted_got[k][0]) and not got[k][1:].any(), k


# ---- (b) through the renderer --------------------------------------------------------------------------------------------------
def test_vsd_of_a_partly_hidden_sphere(hip, dev):
    """A sphere of diameter 0.2 m behind a nearer cube that hides part of it in the test frame.  Pose 0 is the ground truth;
    pose 1 stands a diameter to the side; pose 2 lies 0.07 diameter farther along the ray: every point is moved along its
    own ray (the top three rows of the pose times 1 + 0.07 d / |t|), so the silhouette stays what it is -- a translation
    alone shrinks it by a sixth of a pixel, and union - inter = 10 of 135 pixels then keeps e_10 at 0.074 in the
    restatement -- while every distance grows by
    0.0175 D >= 0.0175 * 0.7 m = 0.01225 m: above tau_1 = 0.01 m by far more than the depth unit of 1e-4 m, below tau_2 =
    0.02 m and below delta = 0.015 m."""
    from cloudaae_amd.utils import bop_score as B
    iv, it = MR.icosphere(2)
    cv, ct, _ = MR.cube()
    meshes = [((iv.astype(np.float64) * 0.1).astype(np.float32), it), (cv, ct)]
    h, w, d = 64, 96, 0.2
    intr = np.array([[80.0, 81.0, 47.3, 30.6, 10000.0]], np.float32)
    gt = R.pose_matrix([0.1, 0.2, 0.3], [-0.05, 0.01, 0.8])
    cube = R.pose_matrix([0.4, 0.6, 0.1], [-0.09, -0.02, 0.6])
    cube[:3, :3] *= 0.08
    test = R.render(meshes, [[(0, 1, gt), (1, 2, cube)]], intr, h, w)
    side = gt.copy()
    side[0, 3] += d
    far = gt.copy()
    far[:3] *= 1.0 + 0.07 * d / np.linalg.norm(gt[:3, 3])
    est = np.stack([gt, side, far])[None]
    want = BR.vsd(meshes, [0], est, gt[None], test['depth'], intr, [0], d)
    full = int((want['depth_gt'][0] != 0).sum())
    print("sphere: %d pixels alone, %d visible; errors %s" % (full, want['visib_gt'][0], want['errors'][0].tolist()))
    assert 0 < want['visib_gt'][0] < full and (test['label'][0] == 2).sum() > 20
    got = B.vsd(meshes, [0], _d(est, np.float64, dev), _d(gt[None], np.float64, dev),
                _d(test['depth'].view(np.int16), np.int16, dev), intr, [0], d)
    for k in ('inter', 'union', 'over', 'visib_gt'):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    e = got['errors'].cpu().numpy()
    assert e.dtype == np.float64 and e.shape == (1, 3, 10) and np.array_equal(e, want['errors'])
    assert np.array_equal(got['dropped'], want['dropped']) and not got['dropped'].any()
    assert np.all(e[0, 0] == 0.0)                                    # est = gt
    assert np.all(e[0, 1] == 1.0)                                    # a diameter to the side
    assert e[0, 2, 0] >= 0.99 and e[0, 2, 9] == 0.0                  # along the ray
    # more samples than one launch takes, in another order of frames: the rows of each sample stay what they were
    three = B.vsd(meshes, [0, 0, 0], _d(np.repeat(est, 3, 0), np.float64, dev), _d(np.repeat(gt[None], 3, 0), np.float64, dev),
                  _d(np.repeat(test['depth'], 2, 0).view(np.int16), np.int16, dev), np.repeat(intr, 2, 0), [1, 0, 1], d,
                  samples_per_launch=2)
    assert np.array_equal(three['errors'].cpu().numpy(), np.repeat(want['errors'], 3, 0))


# ---- (d) cloudaae_pose_max_dist ------------------------------------------------------------------------------------------------
def launch_max_dist(hip, dev, model, est, gt, sym, num_sym, intr):
    L = hip.lib()
    B, M = model.shape[:2]
    P, smax = est.shape[1], sym.shape[1]
    g = [_d(model, np.float32, dev), _d(est, np.float64, dev), _d(gt, np.float64, dev), _d(num_sym, np.int32, dev),
         _d(sym, np.float64, dev), None if intr is None else _d(intr, np.float32, dev)]
    mssd, mspd = Guarded(B, P, torch.float64, dev), Guarded(B, P, torch.float64, dev)
    nbytes = int(L.cloudaae_pose_max_dist_workspace_bytes(B, P, smax))
    assert nbytes == 16 * B * P * smax
    ws = Guarded(nbytes // 8, 1, torch.int64, dev)
    hip.check(L.cloudaae_pose_max_dist(B, P, M, g[0].data_ptr(), model.shape[2], M * model.shape[2], g[1].data_ptr(),
                                       g[2].data_ptr(), smax, g[3].data_ptr(), g[4].data_ptr(),
                                       None if intr is None else g[5].data_ptr(), mssd.ptr(),
                                       None if intr is None else mspd.ptr(), ws.ptr(), hip.stream()), "cloudaae_pose_max_dist")
    torch.cuda.synchronize()
    ws.numpy()
    out = mspd.numpy()
    if intr is None:
        assert np.all(out.view(np.uint8) == FILL)
    return mssd.numpy().copy(), out.copy()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 129, 2048])
def test_max_dist_equals_the_restatement(hip, dev, M):
    """Rows of 6 floats, P = 2, num_sym = 1, 4, 2 of smax = 4 (the unused slots hold a transform that would change the
    result), with and without intrinsics; pose 1 of sample 2 puts the model across the camera plane."""
    from cloudaae_amd.utils import bop_score as BS
    rng = np.random.default_rng(100 + M)
    B, P, smax = 3, 2, 4
    model = (rng.standard_normal((B, M, 6)) * 0.05).astype(np.float32)
    gt = np.stack([R.pose_matrix(rng.standard_normal(3), [0.1 * b - 0.1, 0.05, 0.7 + 0.1 * b]) for b in range(B)])
    est = np.stack([[R.pose_matrix(rng.standard_normal(3) * (0.2 + p), gt[b][:3, 3] + rng.standard_normal(3) * 0.01)
                     for p in range(P)] for b in range(B)])
    est[2, 1, 2, 3] = 0.0 if M > 1 else -0.5
    num_sym = np.array([1, 4, 2], np.int32)
    # the unused slots hold the transform under which pose 0 has no error: a kernel that read them would return 0
    sym = np.stack([np.tile(np.linalg.inv(gt[b]) @ est[b, 0], (smax, 1, 1)) for b in range(B)])
    sets = [None, BS.symmetry_rotations((0.2, 0.1, 1.0), (0.01, 0.0, 0.0), 4), BS.symmetry_rotations((1, 0, 0), (0, 0, 0), 2)]
    packed, num = BS.pack_symmetries(sets, B)
    assert num.tolist() == num_sym.tolist()
    for b in range(B):
        sym[b, :num_sym[b]] = packed[b, :num_sym[b]]
    intr = np.array([[572.4, 573.6, 325.3, 242.0, 10000.0], [60, 61, 34.6, 22.3, 1000], [1066.8, 1067.5, 312.9, 241.3, 10000]],
                    np.float32)
    want = np.array([[BR.mssd_mspd(model[b], est[b, p], gt[b], intr[b], sym[b, :num_sym[b]]) for p in range(P)]
                     for b in range(B)], np.float64)
    mssd, mspd = launch_max_dist(hip, dev, model, est.reshape(B, P, 16), gt.reshape(B, 16), sym.reshape(B, smax, 16), num_sym, intr)
    print("M = %d: mssd %s mspd %s" % (M, mssd.tolist(), mspd.tolist()))
    assert np.array_equal(mssd.view(np.uint64), want[:, :, 0].copy().view(np.uint64))
    assert np.array_equal(mspd.view(np.uint64), want[:, :, 1].copy().view(np.uint64))
    assert mspd[2, 1] == np.inf and np.isfinite(mspd[:2]).all() and np.isfinite(mssd).all() and mssd.min() > 0
    bare, _ = launch_max_dist(hip, dev, model, est.reshape(B, P, 16), gt.reshape(B, 16), sym.reshape(B, smax, 16), num_sym, None)
    assert np.array_equal(bare.view(np.uint64), mssd.view(np.uint64))
    if M == 65:
        # the wrapper: strided rows, the symmetry sets packed by the host
        got = BS.mssd_mspd(_d(model, np.float32, dev), _d(est, np.float64, dev), _d(gt, np.float64, dev),
                           _d(intr, np.float32, dev), sets)
        assert np.array_equal(got['mssd'].cpu().numpy().view(np.uint64), mssd.view(np.uint64))
        assert np.array_equal(got['mspd'].cpu().numpy().view(np.uint64), mspd.view(np.uint64))
        assert 'mspd' not in BS.mssd_mspd(_d(model, np.float32, dev), _d(est, np.float64, dev), _d(gt, np.float64, dev))


# ---- (e) the limits ------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    B, P, K = 2, 2, 16
    dt, intr = _d(np.full((1, H, W), 1000), np.int16, dev), _d([[60, 61, 34.6, 22.3, 1000]], np.float32, dev)
    dg, de = _d(np.full((B, H, W), 1000), np.int16, dev), _d(np.full((B, P, H, W), 1001), np.int16, dev)
    fo, tau = _d([0, 0], np.int32, dev), _d(np.full((B, K), 0.01), np.float64, dev)
    inter, uni = Guarded(B, P, torch.int32, dev), Guarded(B, P, torch.int32, dev)
    over, visib = Guarded(B * P, K, torch.int32, dev), Guarded(B, 1, torch.int32, dev)

    def call(h=H, w=W, b=B, p=P, k=K, out=inter.ptr(), vis=visib.ptr()):
        return L.cloudaae_vsd_counts(1, h, w, dt.data_ptr(), intr.data_ptr(), b, p, fo.data_ptr(), dg.data_ptr(), de.data_ptr(),
                                     0.015, k, tau.data_ptr(), out, uni.ptr(), over.ptr(), vis, hip.stream())
    assert call(k=0) != 0
    assert b"cloudaae_vsd_counts" in L.cloudaae_last_error()
    assert call(k=17) != 0 and call(h=4097, w=4096) != 0                      # h w above 2^24
    assert call(h=4096, w=4096, b=5, p=4) != 0 and call(b=1 << 20, p=1 << 20) != 0      # b p h w above 2^28
    assert call(out=None) != 0 and call(vis=None) != 0 and call(b=0) != 0 and call(p=0) != 0
    torch.cuda.synchronize()
    for buf in (inter, uni, over, visib):
        assert np.all(buf.numpy().view(np.uint8) == FILL)              # nothing was written, guards included
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(inter.numpy() == H * W) and np.all(visib.numpy() == H * W) and not over.numpy().any()

    model, pose = _d(np.zeros((1, 8, 3)), np.float32, dev), _d(np.eye(4).reshape(1, 16), np.float64, dev)
    num = _d([1], np.int32, dev)
    mssd, mspd, ws = Guarded(1, 1, torch.float64, dev), Guarded(1, 1, torch.float64, dev), Guarded(2, 1, torch.int64, dev)
    q = L.cloudaae_pose_max_dist_workspace_bytes
    assert q(1, 1, 1) == 16 and q(0, 1, 1) == -1 and q(1, 0, 1) == -1 and q(1, 1, 0) == -1

    def dist(b=1, m=8, stride=3, smax=1, out=mssd.ptr(), k=intr.data_ptr(), out2=mspd.ptr()):
        return L.cloudaae_pose_max_dist(b, 1, m, model.data_ptr(), stride, 24, pose.data_ptr(), pose.data_ptr(), smax,
                                        num.data_ptr(), pose.data_ptr(), k, out, out2, ws.ptr(), hip.stream())
    assert dist(m=0) != 0
    assert b"cloudaae_pose_max_dist" in L.cloudaae_last_error()
    assert dist(b=0) != 0 and dist(stride=2) != 0 and dist(smax=0) != 0 and dist(out=None) != 0
    assert dist(k=None) != 0 and dist(out2=None) != 0                         # intrinsics and mspd go together
    torch.cuda.synchronize()
    for buf in (mssd, mspd, ws):
        assert np.all(buf.numpy().view(np.uint8) == FILL)
    assert dist() == 0
    torch.cuda.synchronize()
    assert mssd.numpy()[0, 0] == 0.0 and mspd.numpy()[0, 0] == np.inf         # every point at the camera centre: Z = 0


# ---- (f) end to end ------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def rendered_records(hip, dev, tmp_path_factory):
    """Two made-up meshes in millimetres (a ball of 6 cm radius, a plate of 24 x 24 x 3 cm) and four rendered frames of
    160 x 120 with both, as in tests/test_25_render_gpu.py."""
    from cloudaae_amd.utils import render
    tmp = tmp_path_factory.mktemp("bop")
    os.makedirs(str(tmp / "meshes"))
    iv, it = MR.icosphere(3)
    cv, ct, _ = MR.cube()
    _write_ply(str(tmp / "meshes" / "obj_000001.ply"), iv * np.float32(60.0), it)
    _write_ply(str(tmp / "meshes" / "obj_000002.ply"), (cv - np.float32(0.5)) * np.array([240.0, 240.0, 30.0], np.float32), ct)
    render.main(["--meshes", str(tmp / "meshes"), "--out", str(tmp / "data"), "--frames", "4", "--objects", "2", "--seq", "48",
                 "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    return tmp, str(tmp / "data" / "0048_pcnn.tfrecord")


def test_rendered_records_score_end_to_end(hip, dev, rendered_records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import bop_score as BS
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import pose_score
    tmp, path = rendered_records
    files = mm.mesh_files(str(tmp / "meshes"))
    models = mm.models_from_meshes(files, scale=0.001, oversample=2, device=dev)
    packed = mm.pack_meshes(files, 0.001, dev)
    frames = tfrecord_io.read_frames(path, verify=True)
    N = 128
    plain = E.element_from_frames(frames, 0, N, models, seed=4, device=dev)
    el = E.element_from_frames(frames, 0, N, models, seed=4, device=dev, keep_frames=True)
    assert el is not None and set(el) - set(plain) == {"frame_depth", "frame_intrinsics"}
    for k, v in plain.items():                                        # the default output is what it was
        assert (torch.equal(v, el[k]) if isinstance(v, torch.Tensor) else np.array_equal(v, el[k])), k
    B = len(el['class_id'])
    assert el['frame_depth'].dtype == torch.int16 and tuple(el['frame_depth'].shape) == (B, 120, 160)
    assert tuple(el['frame_intrinsics'].shape) == (B, 5) and el['frame_intrinsics'].dtype == torch.float32
    for b, f in enumerate(el['frame_id']):
        assert np.array_equal(el['frame_depth'][b].cpu().numpy().view(np.uint16), frames[int(f)]['depth'])
    diam = pose_score.model_diameter(models[:, :, :3].contiguous())
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    tensors = {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}
    bop = dict(meshes=packed, mesh_index=None, diameters=diam, symmetries={0: BS.symmetry_rotations((0, 0, 1), (0, 0, 0), 2)})
    out = E.evaluate_batch(graph, tensors, bop=bop)
    assert tuple(out['vsd_pred'].shape) == (B, 10) and tuple(out['mssd_pred'].shape) == (B,) == tuple(out['mspd_pred'].shape)
    assert torch.isfinite(out['mssd_pred']).all() and torch.isfinite(out['mspd_pred']).all()
    assert (out['vsd_pred'] >= 0).all() and (out['vsd_pred'] <= 1).all()
    base = E.evaluate_batch(graph, tensors)
    assert 'vsd_pred' not in base and torch.equal(base['trans_pred'], out['trans_pred'])
    with pytest.raises(ValueError, match="replay"):
        E.evaluate_batch(graph, tensors, replay=True, bop=bop)
    # the record's own ground-truth pose as the estimate
    gt = pose_score.pose_matrix(el['axisangle'], el['translation'])
    r = BS.vsd(packed, el['class_id'].cpu().numpy(), gt, gt, el['frame_depth'], el['frame_intrinsics'], np.arange(B), diam[0])
    print("visib_gt %s union %s" % (r['visib_gt'].tolist(), r['union'].tolist()))
    assert (r['union'] > 0).all() and torch.equal(r['union'], r['inter']) and (r['errors'] == 0).all()
    assert (r['visib_gt'] > 0).all() and not r['dropped'].any()


def test_command_line_prints_the_average_recalls(hip, dev, rendered_records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    tmp, path = rendered_records
    obj = str(tmp / "obj_models.tfrecords")
    mm.main(["--meshes", str(tmp / "meshes"), "--out", obj, "--scale", "0.001", "--oversample", "2"])
    graph = T.TrainGraph({"num_point": 128, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    common = ["--files", path, "--object_model", obj, "--trained_model", ckpt[:-len(".npz")], "--target_cls", "0",
              "--num_point", "128", "--batch_size", "1"]
    capsys.readouterr()
    assert E.main(common + ["--bop", "--meshes", str(tmp / "meshes"), "--mesh_scale", "0.001"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    n = int([ln for ln in lines if ln.startswith("batch size ")][0].split()[-1])
    bop = [ln for ln in lines if ln.startswith("bop ")]
    assert n >= 1 and len(bop) == 2, lines[-6:]
    assert bop[0].startswith("bop class 0 pred n %d ar_vsd " % n) and bop[1].startswith("bop all pred n %d ar_vsd " % n)
    for ln in bop:
        tok = ln.split()
        vals = [float(tok[tok.index(k) + 1]) for k in ("ar_vsd", "ar_mssd", "ar_mspd", "ar")]
        assert len(vals) == 4 and all(0.0 <= v <= 1.0 for v in vals) and abs(vals[3] - sum(vals[:3]) / 3) < 1e-5, ln
    with pytest.raises(SystemExit) as err:
        E.main(common + ["--bop"])
    assert err.value.code == 2 and "--meshes" in capsys.readouterr().err
