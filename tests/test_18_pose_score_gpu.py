"""GPU: pose scores (cloudaae_pose_score, cloudaae_pose_matrix, cloudaae_cloud_diameter; utils/pose_score.py;
evaluate_batch(score=True) and main --score) against the float64 NumPy restatement of DESIGN.md "Pose scores"
(tests/pose_score_reference.py).  nn_d2 and the diameter are compared bit for bit; ADD and ADD-S within 1e-12 relative
(2048 non-negative terms, each rounding <= 2^-53 relative: any summation order stays below 2048 * 2^-53 = 2.3e-13)."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import icp_reference as IR
import pose_score_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-12


@pytest.fixture(scope="module")
def model():
    from cloudaae_amd import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    return models[0]                                  # [2048, 6] float32: xyz | rgb


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _poses(B, P, seed):
    """Ground truth near (0, 0, 0.8) m; estimate k of sample s: a few degrees / millimetres off (the operating point),
    far off, or equal to the ground truth, in turn."""
    rng = np.random.default_rng(seed)
    gt, est = np.empty((B, 4, 4)), np.empty((B, P, 4, 4))
    for s in range(B):
        rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
        trans = (np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)).astype(np.float32)
        gt[s] = R.pose_matrix(rot, trans)
        for k in range(P):
            kind = (s + k) % 3
            if kind == 2:
                est[s, k] = gt[s]
                continue
            deg, mm = (rng.uniform(1, 4), rng.uniform(1, 5)) if kind == 0 else (rng.uniform(60, 170), rng.uniform(50, 300))
            axis = rng.standard_normal(3)
            dR = IR.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(deg))
            step = rng.standard_normal(3)
            est[s, k] = gt[s]
            est[s, k, :3, :3] = dR @ gt[s, :3, :3]
            est[s, k, :3, 3] = gt[s, :3, 3] + step / np.linalg.norm(step) * mm * 1e-3
    return est, gt


def _gpu(models, est, gt, nn=True):
    from cloudaae_amd.utils import pose_score as S
    out = S.score_poses(torch.from_numpy(models).cuda(), torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda(),
                        return_nn_d2=nn)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(models, est, gt, out):
    B, P = est.shape[:2]
    worst = 0.0
    for s in range(B):
        for k in range(P):
            add, adds, nn = R.score(models[s], est[s, k], gt[s])
            assert np.array_equal(_bits(out["nn_d2"][s, k]), _bits(nn)), (s, k)
            for name, got, want in (("add", out["add"][s, k], add), ("adds", out["adds"][s, k], adds)):
                err = abs(got - want) / want if want else abs(got)
                worst = max(worst, err)
                assert err <= REL, (name, s, k, got, want)
    print("worst relative error of add / adds against the restatement: %.3g" % worst)


CASES = [(M, B, P) for M in (1, 63, 64, 65) for B in (1, 3, 32) for P in (1, 2)] + \
        [(2048, 1, 1), (2048, 1, 2), (2048, 3, 1), (2048, 32, 2), (5000, 1, 1), (5000, 1, 2), (5000, 3, 2), (5000, 32, 1)]


@pytest.mark.parametrize("M,B,P", CASES)
def test_random_clouds_vs_restatement(hip, M, B, P):
    rng = np.random.default_rng(1000 * M + 10 * B + P)
    models = (rng.standard_normal((B, M, 3)) * 0.05).astype(np.float32)
    est, gt = _poses(B, P, seed=M + B + P)
    out = _gpu(models, est, gt)
    _check(models, est, gt, out)
    same = [(s, k) for s in range(B) for k in range(P) if np.array_equal(est[s, k], gt[s])]
    for s, k in same:                                              # E = G: exact zeros
        assert out["add"][s, k] == 0.0 and out["adds"][s, k] == 0.0 and not out["nn_d2"][s, k].any()


@pytest.mark.parametrize("B,P", [(1, 1), (3, 2)])
def test_golden_model_in_place(hip, model, B, P):
    """obj_batch [B,2048,6] (point stride 6) goes in unsliced; a packed copy gives the same bits; and the C ABI called
    directly, without nn_d2, gives the wrapper's add / adds."""
    models = np.repeat(model[None], B, axis=0)
    est, gt = _poses(B, P, seed=77)
    out = _gpu(models, est, gt)
    _check(models, est, gt, out)
    packed = _gpu(np.ascontiguousarray(models[:, :, :3]), est, gt)
    for k in out:
        assert np.array_equal(_bits(out[k]), _bits(packed[k])), k
    m, e, g = (torch.from_numpy(x).cuda() for x in (models, est, gt))
    add, adds = torch.empty(B, P, dtype=torch.float64).cuda(), torch.empty(B, P, dtype=torch.float64).cuda()
    L = hip.lib()
    ws = torch.empty(int(L.cloudaae_pose_score_workspace_bytes(B, P, 2048)), dtype=torch.uint8).cuda()
    rc = L._cdll.cloudaae_pose_score(B, P, 2048, m.data_ptr(), 6, 2048 * 6, e.data_ptr(), g.data_ptr(), add.data_ptr(),
                                     adds.data_ptr(), None, ws.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(_bits(add.cpu().numpy()), _bits(out["add"]))
    assert np.array_equal(_bits(adds.cpu().numpy()), _bits(out["adds"]))


def test_duplicated_model_points(hip):
    rng = np.random.default_rng(5)
    base = (rng.standard_normal((40, 3)) * 0.05).astype(np.float32)
    models = base[rng.integers(0, 40, (2, 700))]                    # every point many times over
    est, gt = _poses(2, 2, seed=6)
    _check(models, est, gt, _gpu(models, est, gt))


def test_adversarial_lattice(hip):
    """A lattice of spacing 1e-4 m carried to t = (0.3, -0.2, 2.5), estimates shifted by fractions of the spacing: the
    squared distances that decide the minimum are ~1e-9 beside |a|^2 ~ 6.4, below fp32's resolution of the expansion
    |a|^2 + |b|^2 - 2 a.b.  Exact fp64 on the differences: still bit for bit."""
    lat = R.lattice(8, 1e-4)
    gt = np.eye(4)[None].copy()
    gt[0, :3, 3] = np.array([0.3, -0.2, 2.5], np.float32).astype(np.float64)
    est = np.repeat(gt[:, None], 2, axis=1)
    est[0, 0, :3, 3] += np.array([0.37, -0.21, 0.45]) * 1e-4
    est[0, 1, :3, :3] = IR.rodrigues(np.array([0.002, -0.001, 0.003]))
    est[0, 1, :3, 3] += np.array([-0.49, 0.51, 1.02]) * 1e-4
    out = _gpu(lat[None], est, gt)
    _check(lat[None], est, gt, out)
    assert 0.0 < out["nn_d2"].max() < (2e-4) ** 2


def test_batch_and_pose_independence_and_determinism(hip, model):
    B, P = 32, 2
    rng = np.random.default_rng(9)
    models = (rng.standard_normal((B, 2048, 3)) * 0.05).astype(np.float32)
    models[0] = model[:, :3]
    est, gt = _poses(B, P, seed=10)
    full = _gpu(models, est, gt)
    for s in (0, 1, 17, 31):
        for k in range(P):
            one = _gpu(models[s:s + 1], est[s:s + 1, k:k + 1], gt[s:s + 1])
            for name in ("add", "adds", "nn_d2"):
                assert np.array_equal(_bits(one[name][0, 0]), _bits(full[name][s, k])), (name, s, k)
    for _ in range(10):
        again = _gpu(models, est, gt)
        for name in full:
            assert np.array_equal(_bits(again[name]), _bits(full[name])), name


def test_pose_matrix(hip):
    from cloudaae_amd.utils import pose_score as S
    rng = np.random.default_rng(11)
    rot = rng.standard_normal((40, 3)) * rng.uniform(0.01, 2.0, (40, 1))
    rot[0] = 0.0                                                    # theta = 0: exactly I
    rot[1] = [np.pi, 0.0, 0.0]                                      # theta = pi
    rot[2] = np.array([0.0, -np.pi, 0.0])
    rot[3] = [1e-9, 0.0, -1e-9]
    trans = rng.standard_normal((40, 3)).astype(np.float32)
    for dtype in (np.float32, np.float64):
        r = rot.astype(dtype)
        T = S.pose_matrix(torch.from_numpy(r).cuda(), torch.from_numpy(trans).cuda())
        torch.cuda.synchronize()
        assert T.dtype == torch.float64 and tuple(T.shape) == (40, 4, 4)
        T = T.cpu().numpy()
        want = np.stack([R.pose_matrix(r[i], trans[i]) for i in range(40)])
        err = np.abs(T - want).max()
        print("pose_matrix %s: max abs error %.3g" % (np.dtype(dtype).name, err))
        assert np.abs(T[:, :3, :3] - want[:, :3, :3]).max() <= 1e-14
        assert np.array_equal(T[:, :3, 3], trans.astype(np.float64)) and np.array_equal(T[:, 3], want[:, 3])
        assert np.array_equal(T[0, :3, :3], np.eye(3))
    a, b = torch.from_numpy(want).cuda(), torch.from_numpy(want[::-1].copy()).cuda()
    st = S.stack_poses(a, b)
    assert torch.equal(st[:, 0], a) and torch.equal(st[:, 1], b)


def test_model_diameter(hip, model):
    from cloudaae_amd.utils import pose_score as S
    lat = R.lattice(8, 0.0078125)
    rng = np.random.default_rng(12)
    clouds = (rng.standard_normal((3, 2048, 6)) * 0.05).astype(np.float32)
    clouds[1] = model
    for x in (model[None], lat[None], clouds, clouds[:, :1], clouds[:, :65]):
        d = S.model_diameter(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        torch.cuda.synchronize()
        want = np.array([R.diameter(c) for c in x])
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(want)), (d.cpu().numpy(), want)
    assert R.diameter(lat) == np.sqrt(3 * (7 * 0.0078125) ** 2)


def _graph_and_element(model, B, N):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    rng = np.random.default_rng(31)
    scenes, truth = [], []
    for _ in range(B):
        rot = IR.log_map(IR.rodrigues(rng.standard_normal(3)))
        trans = np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.05, 0.05, 3)
        sc, _, _ = IR.scene(model[:, :3], rot, trans, N + 37, 1e-3, rng, 3.0, 0.004)
        scenes.append(sc)
        truth.append(IR.initial_transform(rot, trans))
    scene, truth = np.stack(scenes), np.stack(truth)
    el = dict(xyz_inlier=torch.from_numpy(scene), visiblePoints_org=torch.from_numpy(scene[:, :N]).clone(),
              class_id=torch.zeros(B, dtype=torch.int64), translation=torch.from_numpy(truth[:, :3, 3]).float(),
              axisangle=torch.from_numpy(np.stack([IR.log_map(x[:3, :3]) for x in truth])),
              obj_batch=torch.from_numpy(np.repeat(model[None], B, axis=0)))
    return graph, {k: v.cuda() for k, v in el.items()}


@pytest.mark.parametrize("icp", [None, True])
def test_evaluate_batch_score(hip, model, icp):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import pose_score as S
    B, N = 4, 256
    graph, el = _graph_and_element(model, B, N)
    base = E.evaluate_batch(graph, el, icp=icp)
    out = E.evaluate_batch(graph, el, icp=icp, score=True)
    new = {"add_pred", "adds_pred"} | ({"add_icp", "adds_icp"} if icp else set())
    assert set(out) - set(base) == new and set(base) <= set(out)
    for k, v in base.items():                                       # every other key: the bits of score=None
        if isinstance(v, torch.Tensor):
            assert torch.equal(out[k], v), k
    gt = S.pose_matrix(el["axisangle"], el["translation"])
    by_hand = S.score_poses(el["obj_batch"], S.pose_matrix(out["rot_pred"].contiguous(), out["trans_pred"].contiguous()), gt)
    assert torch.equal(out["add_pred"], by_hand["add"][:, 0]) and torch.equal(out["adds_pred"], by_hand["adds"][:, 0])
    assert out["add_pred"].dtype == torch.float64 and tuple(out["add_pred"].shape) == (B,)
    if icp:
        by_hand = S.score_poses(el["obj_batch"], out["transformation_icp"], gt)
        assert torch.equal(out["add_icp"], by_hand["add"][:, 0]) and torch.equal(out["adds_icp"], by_hand["adds"][:, 0])
    assert bool((out["adds_pred"] <= out["add_pred"]).all()) and bool(torch.isfinite(out["add_pred"]).all())
    # recorded and replayed: the same bits, no torch kernel inside the plan; the unscored plan keeps its key
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r1 = E.evaluate_batch(graph, el, replay=True, icp=icp, score=True)
        r2 = E.evaluate_batch(graph, el, replay=True, icp=icp, score=True)
        for r in (r1, r2):
            for k, v in out.items():
                if isinstance(v, torch.Tensor):
                    assert torch.equal(r[k], v), k
        E.evaluate_batch(graph, el, replay=True, icp=icp)
    plans = graph.__dict__["_eval_plans"]
    assert len(plans) == 2 and all(p[0] is not None and not p[0].foreign_ops for p in plans.values())
    scored = [k for k in plans if ("score",) in k]
    plain = [k for k in plans if ("score",) not in k]
    assert len(scored) == 1 and len(plain) == 1
    names = ["xyz_inlier", "visiblePoints_org", "class_id", "translation", "axisangle"] + (["obj_batch"] if icp else [])
    want = tuple((n, tuple(el[n][:, 0:N, :].shape if n == "visiblePoints_org" else el[n].shape)) for n in names)
    assert plain[0] == want + (((("icp", ()),)) if icp else ())
    with pytest.raises(ValueError):
        E.evaluate_batch(graph, {k: v for k, v in el.items() if k != "obj_batch"}, icp=icp, score=True)


def test_cli_score_on_written_records(hip, tmp_path, model):
    """main --icp --score on the records test_15 writes for its CLI test: the lines of a run without --score are there
    byte for byte, and the summary lines after them equal a PoseScoreLog fed by hand."""
    from test_15_frame_segments_gpu import _write_records, synthetic_frame
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import pose_score as S
    models = model[None]
    data = tmp_path / "data"
    data.mkdir()
    path = _write_records(data, [synthetic_frame(31, classes=(0, 4)), synthetic_frame(32, classes=(0,))])
    obj = tmp_path / "obj_models.tfrecords"
    rec = tfrecord_io.encode_example({"label": np.array([0]), "model": models[0].reshape(-1)})
    tfrecord_io.write_records(str(obj), [rec])
    graph = T.TrainGraph({"num_point": 256, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp_path / "model.ckpt"))
    cmd = [sys.executable, "-c", "import sys; from cloudaae_amd.evaluate_cloudAAE_ycbv import main; sys.exit(main())",
           "--data_dir", str(data), "--object_model", str(obj), "--trained_model", ckpt[:-len(".npz")],
           "--target_cls", "0", "--num_point", "256", "--batch_size", "1", "--icp", "--seed", "3"]
    runs = []
    for extra in ([], ["--score"]):
        p = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        runs.append(p.stdout.strip().splitlines())
    old, new = runs
    assert sum(line.startswith("Validation batch") for line in old) == 2 and old[-2] == "batch size 2"
    assert new[:len(old)] == old                                   # the existing lines, byte for byte
    summary = new[len(old):]
    assert summary and all(line.startswith("score ") for line in summary)
    # by hand: the same frames, seed and checkpoint through evaluate_batch, one sample per batch
    read_models, _ = tfrecord_io.read_and_decode_obj_model(str(obj))
    el = E.element_from_frames(tfrecord_io.read_frames(path, verify=True), 0, 256, read_models, seed=3)
    graph.restore(ckpt[:-len(".npz")])
    log = S.PoseScoreLog(("pred", "icp"), diameters=S.model_diameter(torch.from_numpy(read_models).cuda()))
    for i in range(2):
        b = {k: v[i:i + 1] for k, v in el.items() if isinstance(v, torch.Tensor)}
        out = E.evaluate_batch(graph, b, icp=True, score=True)
        log.append(b["class_id"], torch.stack([out["add_pred"], out["add_icp"]], dim=1),
                   torch.stack([out["adds_pred"], out["adds_icp"]], dim=1))
    assert summary == log.lines()
    assert len(summary) == 2 * 2 * 3 and summary[-1].startswith("score all icp add(-s) n 2 ")
