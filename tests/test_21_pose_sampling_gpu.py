"""GPU: cloudaae_sample_poses and cloudaae_random_object_occluder against the NumPy restatement of DESIGN.md "Pose
sampling" (tests/pose_sampling_reference.py), the batch built from drawn poses, and a short training run fed by them.

The tolerances are measured, not chosen: 10 x the largest change that evaluating the restatement in float64 instead of
float32 makes, floored at 4 ulp of fp32 (axisangle 1.1e-4 -- sqrt(1 - u^2) near the poles is that sensitive in fp32 --,
translation 9.6e-6 / 1.5e-5 ycbv / linemod, occluder points 3.7e-6 / 4.2e-6).  Measured on MI355X
(profiles/notes_pose_sampling.md): integer outputs and keep / replace equal with no sample excluded; axisangle within
2.4e-7, translation within 1.2e-7, occluder points within 2.4e-7.  Every test prints its figures before it asserts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_sampling_reference as R
from test_pose_sampling_host import ALL, GPU_CASES, WRAPPER_CTR, WRAPPER_SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('class_id', 'axisangle', 'rot_mat64', 'translation', 'in_fov', 'rot_gen_mat')


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    return T.synthetic_object_models(device=dev)


@pytest.fixture(scope="module")
def tolerances(models):
    m = models.cpu().numpy()
    tol = {d: R.float_tolerances(21, 65536, d, m, ALL) for d in ("ycbv", "linemod")}
    print("measured tolerances: %r" % (tol,))
    return tol


def _np(t):
    return t.detach().cpu().numpy()


def _raw(t):
    return _np(t).view(np.uint32)


def _draw(dataset, seed, first, n, dev, classes=None):
    from cloudaae_amd.utils import sample_pose_in_frustum as S
    return S.sample_poses(n, seed, first, classes=classes, dataset=dataset, device=dev, debug=True)


@pytest.mark.parametrize("dataset, seed, first, n", GPU_CASES)
def test_integer_outputs_and_keep_replace(dev, dataset, seed, first, n):
    got = _draw(dataset, seed, first, n, dev)
    want = R.sample_poses(n, seed, first, ALL, dataset)
    assert np.array_equal(_raw(got['raw']), want['raw'])                      # the bits behind every draw
    assert np.array_equal(_np(got['class_id']), want['class_id'])
    # keep / replace: a sample may be left out only when its restated pixel is within 1e-4 px of an image edge, and at
    # most 0.1 % of the samples (the host file shows that these seeds leave out none)
    near_edge = R.edge_distance(want['drawn'], dataset) < 1e-4
    assert near_edge.sum() <= n // 1000
    fov = _np(got['in_fov']).astype(bool)
    differ = fov != want['in_fov']
    print("%s: in_fov differs for %d samples, %d near an edge; kept share %.4f" % (dataset, differ.sum(), near_edge.sum(), fov.mean()))
    assert not np.any(differ & ~near_edge)
    # the replaced ones are the frustum middle exactly; the kept ones are the draw
    t, d = _np(got['translation']), _np(got['drawn'])
    assert np.all(t[~fov] == want['frustum_middle'][None, :]) and np.array_equal(t[fov], d[fov][:, :3])
    # a restricted class list
    sub = _draw(dataset, seed, first, 512, dev, classes=[3, 7, 20])
    assert np.array_equal(_np(sub['class_id']), R.sample_poses(512, seed, first, [3, 7, 20], dataset)['class_id'])


def test_philox_known_vector_on_the_device(dev):
    """The vector of the host file, from two uses of philox4x32 on the device: the raw words of the pose kernel, and an
    existing integer path -- the padding rows of cloudaae_hidden_point_removal, row = r0 % num_vis with stream 7 and
    counter (cloud << 32 | row), here for a fresh seed (the host file checks the stored batch of seed 5)."""
    got = _raw(_draw('ycbv', WRAPPER_SEED, WRAPPER_CTR, 1, dev)['raw'])[0]
    assert np.array_equal(got[:4], R.philox4x32(WRAPPER_SEED, [WRAPPER_CTR], 16)[0])
    assert np.array_equal(got[4:], R.philox4x32(WRAPPER_SEED, [WRAPPER_CTR], 17)[0])
    from test_pose_sampling_host import padding_rows_follow_philox
    from cloudaae_amd import tfrecord_io as io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    g = os.path.join(ROOT, "tests", "golden")
    m1, _ = io.read_and_decode_obj_model(os.path.join(g, "obj_model_first1.tfrecords"))
    rec = next(io.PoseRecords([os.path.join(g, "pose_records_cls0_first4.tfrecords")]).epoch(4, shuffle=False))
    x = T.get_small_data({k: torch.as_tensor(v).to(dev) for k, v in rec.items()}, torch.as_tensor(m1).to(dev), seed=41)
    padding_rows_follow_philox(_np(x['visiblePoints_org_src']), _np(x['num_vis_point_org']), 41 + 1)


@pytest.mark.parametrize("dataset, seed, first, n", GPU_CASES)
def test_floating_outputs(dev, tolerances, dataset, seed, first, n):
    from cloudaae_amd.losses import angular_distance_taylor
    got = _draw(dataset, seed, first, n, dev)
    want = R.sample_poses(n, seed, first, ALL, dataset)
    tol = tolerances[dataset]
    err_a = np.abs(_np(got['axisangle']) - want['axisangle']).max()
    both = _np(got['in_fov']).astype(bool) & want['in_fov']
    err_t = np.abs(_np(got['translation'])[both].astype(np.float64) - want['translation'][both]).max()
    print("%s: axisangle err %.3e (tol %.3e), translation err %.3e (tol %.3e)" % (dataset, err_a, tol['axisangle'], err_t, tol['translation']))
    assert err_a <= tol['axisangle'] and err_t <= tol['translation']
    # the axis-angle is an fp32 value widened; its matrix has the bits of the existing exponential map
    a = got['axisangle']
    assert torch.equal(a, a.float().double())
    assert torch.equal(got['rot_mat64'], angular_distance_taylor.exponential_map(a))
    assert torch.equal(got['rot_gen_mat'], got['rot_mat64'].float())
    assert got['rot_gen_axag'] is got['axisangle'] and got['trans_gen'] is got['translation']


def test_invariance_to_batch_split_and_replay(dev, hip):
    from cloudaae_amd.utils import generate_occluder as G, sample_pose_in_frustum as S
    from cloudaae_amd import train_cloudAAE_ycbv as T
    seed = 77
    one = S.sample_poses(256, seed, 0, device=dev)
    eight = [S.sample_poses(32, seed, 32 * s, device=dev) for s in range(8)]
    ranks = []
    for s in range(2):
        for r in range(4):
            sp = T.SampledPoses(10 ** 6, 128, r, 4, seed=seed, device=dev)
            ranks.append((sp.first_index(0, s), S.sample_poses(32, seed, sp.first_index(0, s), device=dev)))
    ranks = [p for _, p in sorted(ranks, key=lambda x: x[0])]
    for k in KEYS:
        assert torch.equal(one[k], torch.cat([p[k] for p in eight])), k
        assert torch.equal(one[k], torch.cat([p[k] for p in ranks])), k
    # two ranks of one step draw disjoint index ranges: other words, and together the one-rank batch
    a, b = (T.SampledPoses(10 ** 6, 64, r, 2, seed=seed, device=dev) for r in (0, 1))
    assert (a.first_index(0, 3), b.first_index(0, 3)) == (192, 224)
    ra, rb = (_raw(S.sample_poses(32, seed, x.first_index(0, 3), device=dev, debug=True)['raw']) for x in (a, b))
    assert not {tuple(w) for w in ra} & {tuple(w) for w in rb}
    assert np.array_equal(np.concatenate([ra, rb]), R.sample_poses(64, seed, 192, ALL)['raw'])
    # recorded and replayed: the same bits as the eager launch, pose and occluder
    x = dict(one, obj_model=T.synthetic_object_models(device=dev))
    eager = G.get_random_object_occluder(dict(x), 21, seed=seed, first_index=0)['occluder']
    plan = hip.StepPlan(dev)
    with hip.record(plan):
        rec = S.sample_poses(256, seed, 0, device=dev)
        rec = G.get_random_object_occluder(dict(rec, obj_model=x['obj_model']), 21, seed=seed, first_index=0)
    assert not plan.foreign_ops, plan.foreign_ops
    torch.cuda.synchronize()
    for k in KEYS + ('occluder',):
        assert torch.equal(rec[k], eager if k == 'occluder' else one[k]), k
    for k in KEYS + ('occluder',):
        rec[k].zero_()
    plan.replay()
    torch.cuda.synchronize()
    for k in KEYS + ('occluder',):
        assert torch.equal(rec[k], eager if k == 'occluder' else one[k]), k


@pytest.mark.parametrize("dataset, seed, first, n", GPU_CASES)
def test_object_occluder(dev, models, tolerances, dataset, seed, first, n):
    from cloudaae_amd.utils import generate_occluder as G
    n = 2048
    classes = [1, 4, 9, 16, 20]
    x = _draw(dataset, seed, first, n, dev)
    x['obj_model'] = models
    x = G.get_random_object_occluder(x, 21, seed=seed, dataset=dataset, first_index=first, classes=classes)
    occ = _np(x['occluder'])
    assert occ.shape == (n, 512, 3)
    want = R.object_occluder(models.cpu().numpy(), n, seed, first, classes, _np(x['rot_mat64']), _np(x['translation']),
                             dataset=dataset)
    assert np.array_equal(_np(x['occluder_class']), want['occ_class']) and set(want['occ_class']) <= set(classes)
    err = np.abs(occ.astype(np.float64) - want['occluder']).max()
    print("%s: occluder err %.3e (tol %.3e)" % (dataset, err, tolerances[dataset]['occluder']))
    assert err <= tolerances[dataset]['occluder']
    # between the near plane and the object in the mean: centre z ~ N((near + z)/2, (z - near)/6) per sample
    c = R.camera_constants(dataset)
    z = _np(x['translation'])[:, 2].astype(np.float64)
    centre_z = (occ[:, :, 2].astype(np.float64) - (want['occluder'][:, :, 2] - want['centre'][:, None, 2])).mean(1)
    dev_z = centre_z - (float(c['near']) + z) / 2
    se = np.sqrt((((z - float(c['near'])) / 6) ** 2).sum()) / n
    print("%s: centre z - (near + z)/2: mean %.3e, standard error %.3e" % (dataset, dev_z.mean(), se))
    assert abs(dev_z.mean()) < 5 * se
    # the default list is every model
    y = G.get_random_object_occluder(dict(x), 21, seed=seed, dataset=dataset, first_index=first)
    assert np.array_equal(_np(y['occluder_class']), R.object_occluder(models.cpu().numpy(), n, seed, first, ALL, _np(x['rot_mat64']),
                                                                        _np(x['translation']), dataset=dataset)['occ_class'])


def _rows(a):
    a = np.ascontiguousarray(a, np.float32)
    return {r.tobytes() for r in a.reshape(-1, 3)}


def test_get_small_data(dev, golden_dir, models):
    from cloudaae_amd import tfrecord_io as io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import sample_pose_in_frustum as S
    # the record path with default arguments: the batch the parent commit built from the same four records
    gold = np.load(os.path.join(golden_dir, "small_data_records_b4.npz"))
    m1, _ = io.read_and_decode_obj_model(os.path.join(golden_dir, "obj_model_first1.tfrecords"))
    rec = next(io.PoseRecords([os.path.join(golden_dir, "pose_records_cls0_first4.tfrecords")]).epoch(4, shuffle=False))
    x = T.get_small_data({k: torch.as_tensor(v).to(dev) for k, v in rec.items()}, torch.as_tensor(m1).to(dev),
                         seed=int(gold['seed']))
    for k in ("visiblePoints", "visiblePoints_org", "num_vis_point", "num_vis_point_org", "visiblePoints_org_src", "occluder"):
        assert np.array_equal(_np(x[k]), gold[k]), k
    # drawn poses, both occluders
    B = 8
    poses = S.sample_poses(B, 5, 1000, device=dev)
    sph = T.get_small_data(dict(poses), models, seed=3, first_index=1000, occluder_seed=5)
    obj = T.get_small_data(dict(poses), models, seed=3, occluder='object', first_index=1000, occluder_seed=5)
    assert tuple(sph['visiblePoints'].shape) == (B, 2449, 3) and tuple(obj['visiblePoints'].shape) == (B, 2561, 3)
    assert tuple(obj['occluder'].shape) == (B, 512, 3)
    assert torch.equal(sph['visiblePoints_org'], obj['visiblePoints_org'])
    assert torch.equal(sph['num_vis_point_org'], obj['num_vis_point_org'])
    for b in range(B):
        allowed = _rows(_np(obj['model_xyz_rot_trans'][b])) | _rows(_np(obj['occluder'][b]))
        nv = int(obj['num_vis_point'][b])
        assert 0 < nv < 2561
        assert _rows(_np(obj['visiblePoints'][b])) <= allowed
    # the transformed model is the drawn pose applied to the drawn class
    want = R.sample_poses(B, 5, 1000, ALL)
    assert np.array_equal(_np(obj['class_id']), want['class_id'])
    Rm = _np(poses['rot_mat64']).astype(np.float32)
    pts = models.cpu().numpy()[want['class_id'], :, :3]
    ref = np.einsum('bnk,brk->bnr', pts.astype(np.float64), Rm.astype(np.float64)) + _np(poses['translation'])[:, None, :]
    assert np.abs(_np(obj['model_xyz_rot_trans']) - ref).max() < 1e-6


def _train(extra, tmp):
    cmd = [sys.executable, "-m", "cloudaae_amd.train_cloudAAE_ycbv", "--poses", "sampled", "--num_point", "256", "--batch_size",
           "32", "--steps", "30", "--max_epoch", "1", "--log_dir", str(tmp), "--deterministic"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rows = re.findall(r"epoch 0 batch (\d+) xyz_loss (\S+) trans_loss (\S+) axag_loss (\S+)", out.stdout)
    assert [int(r[0]) for r in rows] == list(range(30)), out.stdout[-2000:]
    return np.array([[float(v) for v in r[1:]] for r in rows])


@pytest.mark.parametrize("occluder", ["spherical", "object"])
def test_training_on_sampled_poses(tmp_path, occluder):
    """main(--poses sampled) without --data_dir: 30 steps of B = 32, N = 256 on made-up object models, one process per
    run under its own time limit."""
    first = _train(["--occluder", occluder], tmp_path / "a")
    print("%s: chamfer first 10 %.6f last 10 %.6f" % (occluder, first[:10, 0].mean(), first[-10:, 0].mean()))
    assert np.all(np.isfinite(first))
    assert first[-10:, 0].mean() < first[:10, 0].mean()
    again = _train(["--occluder", occluder], tmp_path / "b")
    assert np.array_equal(first, again)                       # the same seed: the same poses, the same losses
    if occluder == "spherical":
        other = _train(["--occluder", occluder, "--pose_seed", "5"], tmp_path / "c")
        assert not np.array_equal(first, other)


@pytest.mark.parametrize("dataset", ["ycbv", "linemod"])
def test_reference_named_helpers(dev, dataset):
    """The reference's own chain -- in_frustum_translation -> get_proj_matrix -> get_final_translation -- against what
    sample_poses gives in one launch for the same (seed, index), and the rotation / translation helpers."""
    from cloudaae_amd.utils import sample_pose_in_frustum as S
    n, seed, first = 4096, 31, 700
    cam = S.camera_parameters(dataset)
    _, _, Wnear, _, Wfar = S.get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    want = S.sample_poses(n, seed, first, dataset=dataset, device=dev, debug=True)
    pts, middle = S.in_frustum_translation(n, Wnear, Wfar, cam['farDist'], cam['nearDist'], seed, first, dev)
    assert pts.device == middle.device == want['drawn'].device
    assert torch.equal(pts[:, :3], want['drawn'][:, :3]) and bool((pts[:, 3] == 1).all())
    proj = S.get_proj_matrix(S.camera_matrix(dataset), torch.eye(3), torch.zeros((3, 1)))
    assert tuple(proj.shape) == (3, 4)
    final, pts_2d = S.get_final_translation(proj, pts, cam['width'], cam['height'], middle)
    # the chain's pixel comes from a matrix product, the kernel's from (fx x + cx z) / z: the same number up to fp32
    # rounding, so the two may disagree on keeping a draw only where the pixel is within 1e-3 px of an image edge
    px = _np(want['drawn'])[:, 3:5].astype(np.float64)
    ok = np.isfinite(px).all(1) & (np.abs(px) < 2000).all(1)        # (1e-3 px is below fp32's step further out)
    assert np.abs(_np(pts_2d).T[ok] - px[ok]).max() < 1e-3
    edge = R.edge_distance(_np(want['drawn']), dataset) < 1e-3
    kept = _np(S.check_pts_in_image_fov(pts_2d, cam['width'], cam['height']))
    assert edge.sum() <= n // 1000 and np.array_equal(kept[~edge], _np(want['in_fov']).astype(bool)[~edge])
    assert np.array_equal(_np(final)[~edge][:, :3], _np(want['translation'])[~edge])
    # the rotation and translation helpers are the sampler's own outputs
    axag, rot = S.sample_rot(n, seed, first, dev)
    assert torch.equal(axag, want['axisangle']) and torch.equal(rot, want['rot_mat64'])
    x = S.rotation_generation(dict(class_id=want['class_id']), seed, first)
    assert torch.equal(x['rot_gen_mat'], want['rot_gen_mat']) and torch.equal(x['rot_gen_axag'], want['axisangle'])
    x = S.translation_generation(x, seed, first, dataset=dataset)
    assert torch.equal(x['trans_gen'], want['translation']) and torch.equal(x['in_fov'], want['in_fov'])
    assert tuple(x['frustum_corners'].shape) == (3, 8)
