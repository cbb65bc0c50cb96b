"""GPU: training on rendered, sensor-noised depth segments (--visibility rendered): the command line end to end in fresh
processes, the target's prefix form through the Chamfer loss, the refusal without meshes, and the untouched default
path of get_small_data."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_models_reference as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT = 240                   # seconds: a child imports torch, builds the graph and takes three small steps


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    """Two small PLY meshes in millimetres, as BOP meshes are: a ball of 5 cm radius (class 0) and a 10 cm box (class 1)."""
    d = tmp_path_factory.mktemp("meshes")
    cv, ct, _ = M.cube()
    iv, it = M.icosphere(2)
    _write_ply(d / "obj_000001.ply", np.asarray(iv, np.float32) * np.float32(50.0), it)
    _write_ply(d / "obj_000002.ply", (cv - np.float32(0.5)) * np.float32(100.0), ct)
    return str(d)


def _train(mesh_dir, log_dir):
    cmd = [sys.executable, "-m", "cloudaae_amd.train_cloudAAE_ycbv", "--poses", "sampled", "--meshes", mesh_dir, "--mesh_scale",
           "0.001", "--classes", "0,1", "--visibility", "rendered", "--sensor", "kinect1", "--sensor_seed", "3",
           "--deterministic", "--steps", "3", "--batch_size", "4", "--num_point", "64", "--max_epoch", "1", "--log_dir", log_dir]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = re.findall(r"epoch 0 batch (\d+) xyz_loss (\S+) trans_loss (\S+) axag_loss (\S+)", r.stdout)
    assert [int(x[0]) for x in rows] == [0, 1, 2], r.stdout[-2000:]
    return rows


def test_command_line_trains_and_repeats(hip, mesh_dir, tmp_path):
    first = _train(mesh_dir, str(tmp_path / "a"))
    print(first)
    assert np.all(np.isfinite(np.array([[float(x) for x in r[1:]] for r in first])))
    assert _train(mesh_dir, str(tmp_path / "b")) == first


def test_rendered_needs_meshes_and_sampled_poses(hip, mesh_dir, capsys):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    launches = []
    real = T.TrainGraph
    T.TrainGraph = lambda *a, **k: launches.append(1) or real(*a, **k)
    try:
        for argv in (['--poses', 'sampled', '--visibility', 'rendered'],
                     ['--visibility', 'rendered', '--meshes', mesh_dir],
                     ['--poses', 'sampled', '--meshes', mesh_dir, '--sensor', 'kinect1']):
            with pytest.raises(SystemExit) as e:
                T.main(argv + ['--steps', '1'])
            assert e.value.code == 2
            err = capsys.readouterr().err
            assert "--visibility rendered" in err or "--meshes needs" in err, err
    finally:
        T.TrainGraph = real
    assert not launches, "the refusal came after the graph was built"
    with pytest.raises(ValueError):
        T.get_small_data(dict(translation=torch.zeros(1, 3)), None, visibility='rendered')
    with pytest.raises(ValueError):
        T.get_small_data(dict(translation=torch.zeros(1, 3)), None, visibility='drawn')


def test_target_keys_describe_the_prefix_form(hip, dev, mesh_dir):
    """One step's Chamfer loss with num_vis_point_org / visiblePoints_org_src equals the loss with the keys dropped: the
    rows past the count are copies of the rows the keys name, so the search over the distinct rows finds the same
    neighbours as the search over all of them."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models, sample_pose_in_frustum as spf
    B, N = 4, 64
    packed = mesh_models.pack_meshes(mesh_models.mesh_files(mesh_dir), 0.001, dev)
    rec = spf.sample_poses(B, 7, 100, num_models=2, device=dev)
    # 48 x 64: an object covers some 150 to 350 pixels, so targets with fewer than 4N = 256 distinct rows (the fill rule)
    # and with more (the strata) both occur
    rendered = dict(packed_meshes=packed, num_point=N, sensor='kinect1', height=48, width=64)
    el = T.get_small_data(rec, None, seed=1, first_index=100, occluder_seed=7, visibility='rendered', rendered=rendered)
    n = el['num_pixels_org'].cpu().numpy()
    print("target pixels:", n.tolist(), "distinct:", el['num_vis_point_org'].cpu().tolist())
    assert (n < 4 * N).any() and (n >= 4 * N).any() and n.min() > 0
    assert tuple(el['visiblePoints'].shape) == (B, N, 3) and tuple(el['visiblePoints_org'].shape) == (B, 4 * N, 3)
    graph = T.TrainGraph({'num_point': N, 'gpu': 0}, {}, {'batch_size': B}, deterministic=True)
    with_keys = graph.eval_step(el)
    bare = {k: v for k, v in el.items() if k not in ('num_vis_point_org', 'visiblePoints_org_src')}
    without = graph.eval_step(bare)
    assert torch.isfinite(with_keys['xyz_loss']) and float(with_keys['xyz_loss']) > 0
    assert torch.equal(with_keys['xyz_loss'], without['xyz_loss'])
    assert torch.equal(with_keys['xyz_loss_per_sample'], without['xyz_loss_per_sample'])


def test_default_path_of_get_small_data_is_untouched(hip, dev, golden_dir):
    from cloudaae_amd import tfrecord_io as io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    gold = np.load(os.path.join(golden_dir, "small_data_records_b4.npz"))
    m1, _ = io.read_and_decode_obj_model(os.path.join(golden_dir, "obj_model_first1.tfrecords"))
    rec = next(io.PoseRecords([os.path.join(golden_dir, "pose_records_cls0_first4.tfrecords")]).epoch(4, shuffle=False))
    models = torch.as_tensor(m1).to(dev)

    def element(**kw):
        return T.get_small_data({k: torch.as_tensor(v).to(dev) for k, v in rec.items()}, models, seed=int(gold['seed']), **kw)
    a, b = element(), element(visibility='hpr')
    keys = ("visiblePoints", "visiblePoints_org", "num_vis_point", "num_vis_point_org", "visiblePoints_org_src", "occluder")
    assert set(a) == set(b)
    for k in keys:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
        assert np.array_equal(a[k].cpu().numpy(), gold[k]), k          # and what the path gave when it was recorded
