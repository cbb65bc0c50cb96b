"""GPU: kernels whose dynamic LDS passes 48 KiB are allowed their MAXIMUM once per kernel and device
(csrc/common.h: allow_dynamic_lds), not the size of the launch that happened to come first.  Each case below makes a
first launch above 48 KiB and then, in the same process, a larger launch of the same kernel: a helper that remembered the
first launch's size would fail the second one.  Results are compared exactly with the references the kernels' own tests
use.  (profiles/notes_lds_limit.md lists, per launch site, the existing test that takes it past 64 KiB; these three
kernels are the ones whose request used to follow the launch.)  The two ICP cases are what that audit found missing: no
other test gives icp_kernel more than 2048 target points, where its hash table doubles and its launch passes 64 KiB."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import edgeconv_reference as R
import icp_plane_reference as PL
import icp_reference as IR
import normals_reference as NR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(golden_dir):
    import os
    from cloudaae_amd import tfrecord_io as T
    models, _ = T.read_and_decode_obj_model(os.path.join(golden_dir, "obj_model_first1.tfrecords"))
    return models[0]                                  # [2048, 6] float32: xyz | rgb


def test_fps_larger_cloud_after_first_large_launch(hip, oracle):
    """fps_kernel<PPT, true>, 12 bytes a point: n = 5500 asks for 66 000 B, n = 9000 for 108 000 B.  Those two are served by
    different instantiations (PPT = 16 up to 8192 points, 32 above), so each is followed by a larger cloud of its own
    instantiation: 8000 points (96 000 B) and 12 000 (144 000 B)."""
    from cloudaae_amd.tf_ops.sampling import tf_sampling
    for n in (5500, 8000, 9000, 12000):
        rng = np.random.default_rng(n)
        p = rng.standard_normal((1, n, 3)).astype(np.float32)
        p[:, n // 2:n // 2 + 100] = p[:, :100]
        want = oracle.farthest_point_sample(8, p, threads=8)
        got = tf_sampling.farthest_point_sample(8, torch.from_numpy(p).cuda()).cpu().numpy()
        assert np.array_equal(want, got), n


def test_revlists_larger_cloud_after_first_large_launch(hip):
    """ec_revlist_kernel, 4 bytes a point: n = 16 400 asks for 65 600 B, n = 30 000 for 120 000 B.  Constructed lists (a
    hub 200 points name, planted in-degrees, a point nobody names); offsets exactly, every list's sources as a set (their
    order inside a list is the atomics')."""
    L = hip.lib()
    k = 2
    for n in (16400, 30000):
        idx = R.neighbour_lists(np.random.default_rng(n), SimpleNamespace(B=1, N=n, k=k, hub=200))
        assert np.bincount(idx.ravel(), minlength=n)[R.NOBODY] == 0 and (idx[0, :, 0] == R.HUB).sum() >= 200
        idx_d = torch.from_numpy(idx).cuda()
        rev_d = torch.full((n + 1 + n * k,), -1, dtype=torch.int32, device="cuda")
        idxs, revs = (ctypes.c_void_p * 1)(idx_d.data_ptr()), (ctypes.c_void_p * 1)(rev_d.data_ptr())
        hip.check(L.cloudaae_edgeconv_revlists(1, 1, n, k, idxs, revs, hip.stream()), "cloudaae_edgeconv_revlists")
        torch.cuda.synchronize()
        rev = rev_d.cpu().numpy()
        order, off, _, deg = R._lists(idx.reshape(n, k), n)
        assert np.array_equal(rev[:n + 1], off), n
        got, want = rev[n + 1:], order // k
        key = lambda s: np.lexsort((s, np.repeat(np.arange(n), deg)))
        assert np.array_equal(got[key(got)], want[key(want)]), n


def test_hidden_point_removal_larger_cloud_after_first_large_launch(hip, model):
    """hull_vertex_kernel, 12 bytes a point (viewpoint row included).  The 8-wave form serves clouds up to 6058 points, the
    16-wave form the larger ones, so each gets its own pair: 4101 points (49 212 B) then 5601 (67 212 B); 6401 points
    (76 812 B) then 8593 (103 116 B: the size of tests/test_04_synth_gpu.py's large hull).  hpr_gather_kernel behind them
    keeps an int per point: only clouds near the launcher's limit of 12 783 points take it past 48 KiB, 12 401 points
    (49 604 B) then 12 701 (50 804 B; the hull test has 152 412 B there).  Visible ids = qhull's."""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    from oracle import synth_oracle as SO
    base = model[:, :3]
    rng = np.random.default_rng(24)
    for n1 in (4101, 5601, 6401, 8593, 12401, 12701):
        n = n1 - 401
        ax = rng.standard_normal(3)
        ax = (ax / np.linalg.norm(ax) * rng.uniform(0, np.pi)).astype(np.float32)
        t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)], np.float32)
        pts = SO.transform_object_model(base[rng.integers(0, len(base), n)] + rng.standard_normal((n, 3)).astype(np.float32) * 1e-3,
                                        ax, t)
        occ = (rng.standard_normal((400, 3)) * 0.02 + [t[0], t[1], t[2] * 0.7]).astype(np.float32)
        fl, org = SO.spherical_flip(np.concatenate([pts, occ], 0))
        assert fl.shape == (n1, 3)
        _, num, ids = hpr.convexHull(torch.from_numpy(fl[None]).cuda(), torch.from_numpy(org[None]).cuda(), return_ids=True)
        want, _ = SO.convex_hull_visible(fl)
        assert np.array_equal(ids[0, :int(num[0])].cpu().numpy(), want), n1


ICP_KW = dict(rounds=3, max_iteration=10)


def _icp_agree(got, T, fit, rmse, its, m):
    """the checks of tests/test_14_icp_gpu.py and tests/test_19_icp_plane_gpu.py, for cloud 0 of a call"""
    print("updates %d, max |T - T_ref| %.3e, rmse %.6e vs %.6e"
          % (its.sum(), np.abs(got["transformation"][0] - T).max(), got["inlier_rmse"][0], rmse))
    assert np.array_equal(got["iterations"][0], its), (got["iterations"][0], its)
    assert round(got["fitness"][0] * m) == round(fit * m) and fit > 0.5
    assert np.abs(got["transformation"][0] - T).max() <= 1e-9
    assert abs(got["inlier_rmse"][0] - rmse) <= 1e-9 * rmse


def _icp_gpu(src, dst, rot, trans, **kw):
    from cloudaae_amd.utils.icp import refine_pose_icp
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[None])).cuda()
    if "normals" in kw:
        kw["normals"] = dev(kw["normals"])
    out = refine_pose_icp(dev(src), dev(dst), dev(rot), dev(trans), **dict(ICP_KW, **kw))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n", [2049, 3048, 4096])
def test_icp_point_to_point_more_than_2048_target_points(hip, model, n):
    """icp_kernel<false>: 1600 + 16 n + 4 (H + 9) bytes, H = 8192 buckets from n = 2049: 67 188 B there (n = 2048: 50 788 B),
    83 172 B at n = 3048, 99 940 B at the limit of 4096.  The target is a noisy view of the whole posed model followed by
    a second, independently noisy view of its first n - 2048 points; the model is the source.  Smallest first."""
    rng = np.random.default_rng(n)
    rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
    trans = np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)
    sc, rot0, trans0 = IR.scene(model[:, :3], rot, trans, 2048, 1e-3, rng, 3.0, 4e-3)
    posed = model[:n - 2048, :3].astype(np.float64) @ IR.rodrigues(rot).T + trans
    scene = np.concatenate([sc, (posed + rng.standard_normal(posed.shape) * 1e-3).astype(np.float32)], 0)
    assert scene.shape == (n, 3)
    got = _icp_gpu(model, scene, rot0, trans0)
    _icp_agree(got, *IR.refine(model, scene, rot0, trans0, **ICP_KW), m=2048)


@pytest.mark.parametrize("n", [2049, 3048, 4096])
def test_icp_point_to_plane_more_than_2048_target_points(hip, model, n):
    """icp_kernel<true>: 2368 + 16 n + 4 (H + 9) bytes: 67 956 B at n = 2049, 83 940 B at 3048, 100 708 B at 4096.  As in
    test_19 the scene (a half-space cut of 512 points) is the source and the model the target, here followed by a copy
    of its first n - 2048 points moved by 0.1 mm of noise, with the restatement's normals of the whole target."""
    rng = np.random.default_rng(100 + n)
    rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
    trans = np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)
    sc, rot0, trans0 = IR.scene(model[:, :3], rot, trans, 512, 1e-3, rng, 3.0, 4e-3)
    extra = model[:n - 2048, :3] + (rng.standard_normal((n - 2048, 3)) * 1e-4).astype(np.float32)
    target = np.concatenate([model[:, :3], extra], 0)
    assert target.shape == (n, 3)
    nrm = NR.estimate_normals(target, 0.015)[0]
    got = _icp_gpu(sc, target, rot0, trans0, estimation="point_to_plane", normals=nrm, pose_maps_target_to_source=True)
    _icp_agree(got, *PL.refine(sc, target, nrm, rot0, trans0, pose_maps_target_to_source=True, **ICP_KW), m=512)
