"""GPU: batched point-to-point ICP (cloudaae_icp_point_to_point, utils/icp.py) against the float64 NumPy
restatement of its definition (tests/icp_reference.py), and the refinement inside evaluate_batch."""
import os
import warnings

import numpy as np
import pytest
import torch

import icp_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    from cloudaae_amd import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    return models[0]                                  # [2048, 6] float32: xyz | rgb


def _batch(model, B, N, seed, noise=1e-3, deg=(2.0, 4.0), mm=(3.0, 5.0)):
    """B scenes of the model: seeded true pose near (0, 0, 0.8) m, a half-space cut of N points, Gaussian noise,
    initial pose perturbed by deg degrees and mm millimetres.  Returns numpy (obj [B,2048,6], scene [B,N,3], rot0,
    trans0 [B,3] f32, true transforms [B,4,4])."""
    rng = np.random.default_rng(seed)
    scenes, rots, transs, truth = [], [], [], []
    for _ in range(B):
        rot = R.log_map(R.rodrigues(rng.standard_normal(3)))
        trans = np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)
        sc, r0, t0 = R.scene(model[:, :3], rot, trans, N, noise, rng, rng.uniform(*deg), rng.uniform(*mm) * 1e-3)
        scenes.append(sc)
        rots.append(r0)
        transs.append(t0)
        truth.append(R.initial_transform(rot, trans))
    obj = np.repeat(model[None], B, axis=0)
    return obj, np.stack(scenes), np.stack(rots), np.stack(transs), np.stack(truth)


def _gpu(obj, scene, rot, trans, **kw):
    from cloudaae_amd.utils.icp import refine_pose_icp
    out = refine_pose_icp(torch.from_numpy(obj).cuda(), torch.from_numpy(scene).cuda(), torch.from_numpy(rot).cuda(),
                          torch.from_numpy(trans).cuda(), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_rotations(out):
    """R orthonormal to 1e-14 and Rodrigues(rot_axag) = R to 1e-12, angle in [0, pi]; trans = T's translation."""
    for c in range(len(out["transformation"])):
        T = out["transformation"][c]
        Rm = T[:3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(Rm) - 1.0) < 1e-14
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        assert np.abs(R.rodrigues(out["rot_axag"][c]) - Rm).max() < 1e-12
        assert np.linalg.norm(out["rot_axag"][c]) <= np.pi + 1e-12
        assert np.array_equal(out["trans"][c], T[:3, 3].astype(np.float32))


@pytest.mark.parametrize("B,N,max_iteration,rounds", [
    (1, 256, 30, 10), (1, 1024, 30, 10), (1, 2048, 30, 10), (7, 1024, 30, 10), (7, 256, 1, 10),
    (1, 2048, 1, 1), (7, 1024, 0, 10), (1, 1024, 30, 1), (1, 1024, 30, 0),
])
def test_icp_vs_restatement(hip, model, B, N, max_iteration, rounds):
    obj, scene, rot, trans, _ = _batch(model, B, N, seed=1000 * B + N + max_iteration + rounds)
    kw = dict(rounds=rounds, max_iteration=max_iteration)
    got = _gpu(obj, scene, rot, trans, **kw)
    assert got["iterations"].shape == (B, rounds) and got["iterations"].dtype == np.int32
    for c in range(B):
        T, fit, rmse, its = R.refine(obj[c], scene[c], rot[c], trans[c], **kw)
        assert np.array_equal(got["iterations"][c], its), (c, got["iterations"][c], its)
        assert round(got["fitness"][c] * 2048) == round(fit * 2048), c
        assert np.abs(got["transformation"][c] - T).max() <= 1e-9, c
        assert abs(got["inlier_rmse"][c] - rmse) <= 1e-9 * rmse, c
        if max_iteration == 0 or rounds == 0:
            assert np.abs(got["transformation"][c] - R.initial_transform(rot[c], trans[c])).max() <= 1e-15
    _check_rotations(got)


def test_icp_recovers_the_true_pose(hip, model):
    """The whole posed model as the scene, noise-free, 2 deg / 3 mm off: the truth up to the fp32 rounding of the
    scene (6e-8 m at 0.8 m), and the restatement's answer to 1e-9."""
    obj, scene, rot, trans, truth = _batch(model, 2, 2048, seed=77, noise=0.0, deg=(2.0, 2.0), mm=(3.0, 3.0))
    got = _gpu(obj, scene, rot, trans)
    for c in range(2):
        T, fit, rmse, its = R.refine(obj[c], scene[c], rot[c], trans[c])
        assert np.abs(got["transformation"][c] - truth[c]).max() < 1e-7
        assert np.abs(got["transformation"][c] - T).max() <= 1e-9
        assert got["fitness"][c] == 1.0 and got["inlier_rmse"][c] < 1e-7
        assert np.array_equal(got["iterations"][c], its)
    _check_rotations(got)


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1.0, np.pi - 1e-6, float(np.float32(np.pi))])
def test_icp_without_correspondences_keeps_the_initial_pose(hip, model, angle):
    obj, scene, rot, trans, _ = _batch(model, 3, 1024, seed=5)
    scene = scene + np.float32(1.0)                          # every target 1 m away from every source point
    axis = np.array([[0.3, -0.5, 0.8], [1.0, 0.0, 0.0], [-0.2, -0.1, 0.4]])
    rot = (axis / np.linalg.norm(axis, axis=1, keepdims=True) * angle).astype(np.float32)
    got = _gpu(obj, scene, rot, trans)
    t0 = _gpu(obj, scene, rot, trans, rounds=0)
    assert np.array_equal(got["transformation"].view(np.int64), t0["transformation"].view(np.int64))
    assert np.all(got["fitness"] == 0.0) and np.all(got["inlier_rmse"] == 0.0)
    assert np.all(got["iterations"] == 1)
    for c in range(3):
        R0 = R.rodrigues(rot[c])
        assert np.abs(got["transformation"][c][:3, :3] - R0).max() <= 1e-15
        assert np.abs(R.rodrigues(got["rot_axag"][c]) - R0).max() < 1e-12
    _check_rotations(got)


def test_icp_is_deterministic_and_batch_independent(hip, model):
    obj, scene, rot, trans, _ = _batch(model, 7, 1024, seed=11)
    a = _gpu(obj, scene, rot, trans)
    b = _gpu(obj, scene, rot, trans)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for c in (0, 3, 6):
        one = _gpu(obj[c:c + 1], scene[c:c + 1], rot[c:c + 1], trans[c:c + 1])
        for k in a:
            assert one[k][0].tobytes() == a[k][c].tobytes(), (c, k)


def test_icp_reads_strided_inputs_in_place(hip, model):
    """obj_batch [B,2048,6] (point stride 6) and a prefix of a wider scene buffer give the results of packed copies."""
    from cloudaae_amd.utils.icp import refine_pose_icp
    obj, scene, rot, trans, _ = _batch(model, 2, 256, seed=21)
    wide = np.concatenate([scene, np.zeros((2, 40, 3), np.float32)], axis=1)
    o, w, r, t = (torch.from_numpy(x).cuda() for x in (obj, wide, rot, trans))
    a = refine_pose_icp(o, w[:, :256], r, t)
    b = refine_pose_icp(o[:, :, :3].contiguous(), w[:, :256].contiguous(), r, t)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _graph_and_element(model, B, N):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    obj, scene, rot, trans, truth = _batch(model, B, N + 37, seed=31)
    el = dict(xyz_inlier=torch.from_numpy(scene), visiblePoints_org=torch.from_numpy(scene[:, :N]).clone(),
              class_id=torch.zeros(B, dtype=torch.int64), translation=torch.from_numpy(truth[:, :3, 3]).float(),
              axisangle=torch.from_numpy(np.stack([R.log_map(x[:3, :3]) for x in truth])),
              obj_batch=torch.from_numpy(obj))
    return graph, {k: v.cuda() for k, v in el.items()}


def test_evaluate_batch_icp(hip, model):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.losses import angular_distance_taylor, trans_distance
    from cloudaae_amd.utils.icp import refine_pose_icp
    B, N = 4, 256
    graph, el = _graph_and_element(model, B, N)
    plain = E.evaluate_batch(graph, el)
    out = E.evaluate_batch(graph, el, icp=True)
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(out[k], v), k
    direct = refine_pose_icp(el["obj_batch"], el["xyz_inlier"][:, :N], out["rot_pred"], out["trans_pred"])
    names = dict(transformation="transformation_icp", rot_axag="rot_icp", trans="trans_icp", fitness="fitness_icp",
                 inlier_rmse="inlier_rmse_icp", iterations="iterations_icp")
    for k, name in names.items():
        assert torch.equal(out[name], direct[k]), name
    tl, tper = trans_distance.get_translation_error(direct["trans"], el["translation"])
    al, aper = angular_distance_taylor.get_rotation_error(direct["rot_axag"].float(), el["axisangle"])
    assert torch.equal(out["trans_loss_icp"], tl) and torch.equal(out["trans_loss_perSample_icp"], tper)
    assert torch.equal(out["axag_loss_icp"], al) and torch.equal(out["axag_loss_perSample_icp"], aper)
    # recorded and replayed: the same bits, no torch kernel inside the plan
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r1 = E.evaluate_batch(graph, el, replay=True, icp=True)
        r2 = E.evaluate_batch(graph, el, replay=True, icp=True)
    plans = graph.__dict__["_eval_plans"]
    assert any(p[0] is not None and not p[0].foreign_ops for p in plans.values())
    for r in (r1, r2):
        for k, v in out.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(r[k], v), k
    with pytest.raises(ValueError):
        E.evaluate_batch(graph, {k: v for k, v in el.items() if k != "obj_batch"}, icp=True)
