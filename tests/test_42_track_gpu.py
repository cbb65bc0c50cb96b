"""GPU: cloudaae_depth_align_step against the NumPy restatement of DESIGN.md "Tracking" (tests/track_reference.py) from
identical inputs, then utils/track.py -- the loop, the sequences and the lost tracks -- on the scene whose conditions
tests/test_track_host.py asserts for the restatement alone.

n_pairs and status are integers and must be equal.  A sum may differ from the restatement's by what two orders of summation
may differ by: 2 wh ww 2^-53 times its sum of |terms|.  pose_out is held to 1e-9, the bound of tests/test_14_icp_gpu.py.  A
pose that the definition leaves unchanged is compared bit for bit."""
import numpy as np
import pytest
import torch

import detect_reference as DR
import track_reference as TR

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def track(hip):
    from cloudaae_amd.utils import track
    return track


@pytest.fixture(scope="module")
def packed(dev):
    from cloudaae_amd.utils import mesh_models
    return mesh_models.pack_meshes(DR.scene_meshes(), device=dev)


@pytest.fixture(scope="module")
def cases(packed):
    """step_cases with the hypothesis windows cut from the GPU renderer's own output, and the restatement's result of each."""
    from cloudaae_amd.utils import render

    def gpu_renderer(cubes):
        inst = [[(TR.CUBE, 1, np.asarray(c, np.float64)) for c in cs] for cs in cubes]
        out = render.render_frames(packed, inst, np.tile(TR.SCENE_INTR, (len(inst), 1)), TR.SCENE_H, TR.SCENE_W)
        return out['depth'].cpu().numpy().view(np.uint16)
    return [(name, c, TR.step(**c)) for name, c in TR.step_cases(gpu_renderer)]


def _bits(t):
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int16))


def launch(track, dev, c, only=None):
    """align_step on the case's arrays (sample `only` alone when given) -> dict of numpy arrays."""
    sel = slice(None) if only is None else slice(only, only + 1)
    r = track.align_step(_bits(c['depth_test']).to(dev), torch.from_numpy(c['frame_of'][sel].astype(np.int32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(c['origin'][sel], np.int32)).to(dev),
                         _bits(c['depth_hyp'][sel]).to(dev), torch.from_numpy(np.ascontiguousarray(c['intr_win'][sel], np.float32)).to(dev),
                         torch.from_numpy(c['gate'][sel].astype(np.int32)).to(dev), torch.from_numpy(c['jump'][sel].astype(np.int32)).to(dev),
                         c['cos_min'], torch.from_numpy(np.ascontiguousarray(c['pose_in'][sel], np.float64)).to(dev))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_the_renderers_agree_on_the_case_images(cases):
    for (name, c, _), (_, ref) in zip(cases, TR.step_cases(TR.reference_renderer)):
        assert np.array_equal(c['depth_hyp'], ref['depth_hyp']), name


def test_one_step_equals_the_restatement(track, dev, cases):
    seen = set()
    for name, c, want in cases:
        got = launch(track, dev, c)
        B, wh, ww = c['depth_hyp'].shape
        bound = 2.0 * wh * ww * 2.0 ** -53 * want['abs_sums']
        diff = np.abs(got['sums'] - want['sums'])
        worst = float((diff / np.where(bound > 0, bound, 1.0)).max())
        print("%s: n_pairs %s status %s; worst sum at %.3g of its bound; pose within %.3g"
              % (name, got['n_pairs'], got['status'], worst, float(np.abs(got['pose_out'] - want['pose_out']).max())))
        assert np.array_equal(got['n_pairs'], want['n_pairs']), name
        assert np.array_equal(got['status'], want['status']), name
        assert np.all(diff <= bound), name
        assert np.abs(got['pose_out'] - want['pose_out']).max() <= POSE_TOL, name
        assert np.abs(got['x'] - want['x']).max() <= POSE_TOL, name
        for b in range(B):
            seen.add(int(got['status'][b]))
            if got['status'][b] != 0:
                assert got['pose_out'][b].tobytes() == np.asarray(c['pose_in'][b], np.float64).tobytes(), (name, b)
                assert np.all(got['x'][b] == 0.0)
            else:
                assert got['n_pairs'][b] >= 6 and np.all(got['pose_out'][b, 3] == [0.0, 0.0, 0.0, 1.0])
            if got['status'][b] == 4:
                assert got['n_pairs'][b] == 0 and np.all(got['sums'][b] == 0.0)
    assert seen == {0, 1, 2, 4}


def test_two_runs_and_the_batch_give_the_same_bits(track, dev, cases):
    c = dict((name, c) for name, c, _ in cases)['seven over two frames']
    a, b = launch(track, dev, c), launch(track, dev, c)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for i in range(len(c['frame_of'])):
        alone = launch(track, dev, c, only=i)
        for k in a:
            assert alone[k][0].tobytes() == a[k][i].tobytes(), (k, i)


def test_errors_launch_nothing(hip, dev):
    L = hip.lib()
    d = torch.zeros(64, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    assert L.cloudaae_depth_align_step_workspace_bytes(1, 8, 8) == 232 and L.cloudaae_depth_align_step_workspace_bytes(0, 8, 8) == 0
    assert L.cloudaae_depth_align_step_workspace_bytes(3, 33, 67) == 3 * 2 * 28 * 8 + 24

    def call(f=1, h=4, w=4, b=1, wh=2, ww=2, cos_min=0.5, ws=p, ws_bytes=232, hyp=p):
        return L.cloudaae_depth_align_step(f, h, w, p, b, p, p, wh, ww, hyp, p, p, p, cos_min, p, p, p, p, p, p, ws, ws_bytes,
                                           hip.stream())
    for kw in (dict(f=0), dict(b=0), dict(wh=0), dict(h=1 << 13, w=(1 << 11) + 1), dict(cos_min=float('nan')), dict(hyp=None),
               dict(ws=None), dict(ws_bytes=231), dict(ws=p + 4)):
        assert call(**kw) != 0, kw
        assert b"cloudaae_depth_align_step" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0


def test_loop_follows_the_restatement_step_by_step(track, dev, packed):
    depth, truth = TR.frames(TR.SLOW)
    start = TR.off_pose(truth[0])
    a = track.align_poses(depth[:1], TR.SCENE_INTR, packed, [TR.CUBE], [0], start[None], return_trajectory=True)
    traj = a['trajectory'].cpu().numpy()
    n_pairs, status = a['n_pairs_steps'].cpu().numpy(), a['status_steps'].cpu().numpy()
    ref = TR.align(depth[:1], TR.SCENE_INTR, DR.scene_meshes(), [TR.CUBE], [0], start[None], iterations=0)
    assert np.array_equal(a['origin'], ref['origin']) and (a['wh'], a['ww']) == (ref['wh'], ref['ww']) and a['ok'].all()
    assert traj.shape == (5, 1, 4, 4) and traj[0].tobytes() == start[None].tobytes()
    factor = float(TR.SCENE_INTR[0, 4])
    gate, jump = TR.V.tau_units([0.03], [factor]), TR.V.tau_units([0.005], [factor])
    for i in range(4):
        hyp = TR.render_windows(DR.scene_meshes(), [TR.CUBE], traj[i], ref['rows'], ref['wh'], ref['ww'])
        want = TR.step(depth[:1], [0], ref['origin'], hyp, ref['rows'], gate, jump, 0.8, traj[i])
        print("step %d: n_pairs %d, pose within %.3g of the restatement's step, %.3g of the truth"
              % (i, n_pairs[i, 0], np.abs(traj[i + 1] - want['pose_out']).max(), TR.pose_error(traj[i + 1, 0], truth[0])))
        assert n_pairs[i, 0] == want['n_pairs'][0] and status[i, 0] == want['status'][0] == 0
        assert np.abs(traj[i + 1] - want['pose_out']).max() <= POSE_TOL
    assert a['poses'].cpu().numpy().tobytes() == traj[4].tobytes()
    assert TR.pose_error(traj[4, 0], truth[0]) <= 1e-3


@pytest.mark.parametrize("motion, start", [(TR.SLOW, 'constant'), (TR.FAST, 'velocity')], ids=["slow-constant", "fast-velocity"])
def test_sequences(track, packed, motion, start):
    want, truth = TR.sequence(motion, start)
    depth, _ = TR.frames(motion)
    t = track.track_objects(depth, TR.SCENE_INTR, packed, ([TR.CUBE], truth[:1]), motion=start)
    for f in range(TR.FRAMES):
        got, ref = TR.pose_error(t.poses[f, 0], truth[f]), TR.pose_error(want['poses'][f, 0], truth[f])
        print("frame %d: error %.3g (restatement %.3g), score %d / %d, pairs %d" % (f, got, ref, t.num[f, 0], t.den[f, 0], t.n_pairs[f, 0]))
        assert got <= ref + 1e-6
    assert not t.lost.any() and np.all(t.status == 0)
    assert t.poses.shape == (TR.FRAMES, 1, 4, 4) and t.num.shape == t.den.shape == t.lost.shape == (TR.FRAMES, 1)


def test_a_removed_cube_is_lost_and_found_again(track, packed):
    depth, truth = TR.lost_sequence()
    t = track.track_objects(depth, TR.SCENE_INTR, packed, ([TR.CUBE], truth[:1]))
    print("lost", t.lost[:, 0], "score", t.num[:, 0], t.den[:, 0])
    assert list(t.lost[:, 0]) == [False, False, False, True, False]
    assert t.poses[3].tobytes() == t.poses[2].tobytes()
    assert TR.pose_error(t.poses[4, 0], truth[4]) <= 1e-3


def test_on_lost_poses_are_taken_up_in_the_same_frame(track, packed):
    depth, truth = TR.moved_sequence()
    asked = []
    t = track.track_objects(depth, TR.SCENE_INTR, packed, ([TR.CUBE], truth[:1]))
    assert list(t.lost[:, 0]) == [False, False, True] and t.poses[2].tobytes() == t.poses[1].tobytes()

    def hook(f, idx):
        asked.append((f, list(idx)))
        return TR.off_pose(truth[f])[None]
    t = track.track_objects(depth, TR.SCENE_INTR, packed, ([TR.CUBE], truth[:1]), on_lost=hook)
    assert asked == [(2, [0])] and not t.lost.any()
    assert TR.pose_error(t.poses[2, 0], truth[2]) <= 1e-3


def test_tracks_from_detections_and_a_track_without_a_window(track, packed):
    from cloudaae_amd.utils import detect
    depth, truth = TR.frames(TR.SLOW)
    d = detect.Detections()
    pose = np.zeros((1, 3, 4, 4))
    pose[0, 1] = truth[0]
    d.table = dict(det_class=np.array([[-1, TR.CUBE, -1]], np.int32), det_pose=pose)
    t = track.track_objects(depth[:2], TR.SCENE_INTR, packed, d)
    assert list(t.mesh_of) == [TR.CUBE] and not t.lost.any() and TR.pose_error(t.poses[1, 0], truth[1]) <= 1e-3
    behind = truth[0].copy()
    behind[2, 3] = 0.06
    t = track.track_objects(depth[:1], TR.SCENE_INTR, packed, ([TR.CUBE, TR.CUBE], np.array([truth[0], behind])))
    assert list(t.lost[0]) == [False, True] and list(t.status[0]) == [0, 4] and t.poses[0, 1].tobytes() == behind.tobytes()


def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


def test_command_line_follows_a_record_file(track, tmp_path, capsys):
    import os
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import render
    depth, truth = TR.frames(TR.SLOW)
    meshes = DR.scene_meshes()
    os.makedirs(str(tmp_path / "meshes"))
    for i, m in enumerate((meshes[TR.TABLE], meshes[TR.CUBE])):                 # class 0 the table, class 1 the cube
        _write_ply(str(tmp_path / "meshes" / ("obj_%06d.ply" % (i + 1))), m[0], m[1])
    n = 3
    label = (depth[:n] != 0).astype(np.uint8)
    payloads = render.frame_records(depth[:n], label, np.tile(TR.SCENE_INTR, (n, 1)), [[truth[f]] for f in range(n)], [[1]] * n, 48,
                                    list(range(n)))
    path = str(tmp_path / "0048_pcnn.tfrecord")
    tfrecord_io.write_records(path, payloads)
    assert track.main(["--files", path, "--meshes", str(tmp_path / "meshes"), "--motion", "velocity"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    assert len(lines) == n + 1 and lines[-1] == "3 frames, 1 tracks, 0 lost track-frames"
    for f, line in enumerate(lines[:n]):
        w = line.split()
        assert w[:4] == ["frame", str(f), "class", "1"] and w[6:8] == ["lost", "0"]
        assert float(w[9]) < 0.05 and float(w[11]) < 1e-3                       # degrees, metres (the record's poses are float32)
