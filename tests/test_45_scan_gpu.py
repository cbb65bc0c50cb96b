"""GPU: cloudaae_tsdf_raycast against the NumPy restatement of DESIGN.md "Scanning" (tests/scan_reference.py) from identical
inputs, for equality of every uint16; then utils/scan.py: step by step against the restatement from the GPU's own poses and
states, and end to end on the scenes whose conditions tests/test_scan_host.py asserts for the restatement alone."""
import numpy as np
import pytest
import torch

import fuse_reference as FR
import pose_verify_reference as V
import scan_reference as S
import track_reference as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scan(hip):
    from cloudaae_amd.utils import scan
    return scan


def gpu_renderer(meshes, frames, intr, H, W):
    from cloudaae_amd.utils import render
    return render.render_frames(meshes, frames, intr, H, W)['depth'].cpu().numpy().view(np.uint16)


def volume_of(dev, state, origin, voxel):
    from cloudaae_amd.utils import fuse
    nz, ny, nx, _ = state.shape
    vol = fuse.Volume(origin, voxel, (nx, ny, nz), dev)
    vol.state.copy_(torch.from_numpy(np.ascontiguousarray(state)))
    return vol


def cast(scan, vol, poses, rows, wh, ww, **kw):
    d = scan.raycast(vol, np.asarray(poses, np.float64).reshape(-1, 4, 4), np.asarray(rows, np.float32).reshape(-1, 5), wh, ww, **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.int16 and tuple(d.shape) == (len(np.asarray(poses).reshape(-1, 4, 4)), wh, ww)
    return d.cpu().numpy().view(np.uint16)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), \
        "%s: %d of %d pixels differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1, want.size)


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def test_hand_cases_equal_the_restatement(scan, dev):
    for name, c in S.hand_cases():
        vol = volume_of(dev, c['state'], c['origin'], c['voxel'])
        got = cast(scan, vol, c['poses'], c['intr_win'], c['wh'], c['ww'], step=c['step'], min_count=c['min_count'], z_near=c['z_near'])
        want = S.run_case(c)
        print("%s: %d" % (name, int(want[0, 0, 0])))
        same(got, want, name)


def test_small_volumes_steps_and_min_count(scan, dev):
    for name, st, origin, voxel, min_count in S.volume_cases():
        nz, ny, nx, _ = st.shape
        vol = volume_of(dev, st, origin, voxel)
        poses = np.array([S.view_of((nx, ny, nz), origin, voxel, d, 0.5) for d in ([0.2, 0.3, 1.0], [1.0, -0.4, 0.1], [-0.5, 1.0, -0.7])])
        extent = max(nx, ny, nz) * voxel
        rows = np.tile(S.window_row(33, 67, 0.5 * 60.0 / extent), (3, 1))
        hits = 0
        for step_voxels in (0.25, 0.5, 1.0):
            for mc in sorted({1, min_count}):
                want = S.raycast(st, origin, voxel, poses, rows, 33, 67, step_voxels * voxel, mc)
                same(cast(scan, vol, poses, rows, 33, 67, step=step_voxels * voxel, min_count=mc), want, (name, step_voxels, mc))
                hits += int((want != 0).sum())
        print("%s: %d hit pixels over the steps" % (name, hits))
        assert hits > 0, name


def test_windows(scan, dev):
    st, origin, voxel = S.big_wavy()
    vol = volume_of(dev, st, origin, voxel)
    for name, wh, ww, pose, row in S.window_cases():
        want = S.raycast(st, origin, voxel, pose[None], row[None], wh, ww)
        same(cast(scan, vol, pose[None], row[None], wh, ww), want, name)
        print("%s: %d of %d pixels hit" % (name, int((want != 0).sum()), want.size))
        if name == "all rays miss":
            assert not want.any()
        elif name == "half off the volume":
            assert want[:, :, :ww // 4].sum() == 0 and want.any()
        elif wh * ww >= 9:
            assert want.any(), name


def test_batches(scan, dev):
    st, origin, voxel = S.big_wavy()
    vol = volume_of(dev, st, origin, voxel)
    poses, rows, wh, ww = S.batch_case()
    want = S.raycast(st, origin, voxel, poses, rows, wh, ww)
    got = cast(scan, vol, poses, rows, wh, ww)
    same(got, want, "B = 7")
    assert not want[4].any() and not want[5].any() and all(want[b].any() for b in (0, 1, 2, 3, 6))
    gd = S.ray_setup(origin, voxel, (13, 9, 7), poses[6], rows[6], wh, ww)[1]
    assert np.array_equal(gd[:, 16, 33], [0.0, 0.0, 1.0 / voxel])                       # the ray along the axis exactly
    assert got.tobytes() == cast(scan, vol, poses, rows, wh, ww).tobytes()              # two runs
    for b in range(7):                                                                  # a sample alone, bit for bit
        assert cast(scan, vol, poses[b:b + 1], rows[b:b + 1], wh, ww).tobytes() == got[b:b + 1].tobytes(), b
    two = FR.wavy_state((13, 9, 7), 6, zeros=10, unknown=10)
    two[..., 2], two[..., 3] = -two[..., 0], 1                                          # min_count 2 with single votes: the deep band
    vol2 = volume_of(dev, two, origin, voxel)
    for mc in (1, 2):
        for step_voxels in (0.25, 0.5, 1.0):
            w = S.raycast(two, origin, voxel, poses[:4], rows[:4], wh, ww, step_voxels * voxel, mc)
            same(cast(scan, vol2, poses[:4], rows[:4], wh, ww, step=step_voxels * voxel, min_count=mc), w, (mc, step_voxels))
            assert w.any()


@pytest.mark.parametrize("rows,reload", [(0, 1), (1, 0), (1, 1)])
def test_the_kernel_forms_kept_for_measuring(scan, dev, knobs, rows, reload):
    """A wave as 64 pixels of a row, and the cell reloaded at every sample: the same pixels as the product's form."""
    knobs("CLOUDAAE_RAYCAST_ROWS", rows)
    knobs("CLOUDAAE_RAYCAST_RELOAD", reload)
    st, origin, voxel = S.big_wavy()
    vol = volume_of(dev, st, origin, voxel)
    for name, wh, ww, pose, row in S.window_cases():
        same(cast(scan, vol, pose[None], row[None], wh, ww), S.raycast(st, origin, voxel, pose[None], row[None], wh, ww), name)
    poses, rws, wh, ww = S.batch_case()
    same(cast(scan, vol, poses, rws, wh, ww), S.raycast(st, origin, voxel, poses, rws, wh, ww), "B = 7")
    for name, c in S.hand_cases():
        got = cast(scan, volume_of(dev, c['state'], c['origin'], c['voxel']), c['poses'], c['intr_win'], c['wh'], c['ww'], step=c['step'],
                   min_count=c['min_count'], z_near=c['z_near'])
        same(got, S.run_case(c), name)


def test_fused_cube_and_sphere_from_the_14_views(scan, dev):
    from cloudaae_amd.utils import fuse
    s = FR.scene('cube', 0.004)
    vol = fuse.Volume(s['origin'], s['voxel'], s['dims'], dev)
    fuse.integrate(vol, s['depth'], s['intr'], s['poses'])
    torch.cuda.synchronize()
    assert np.array_equal(vol.state.cpu().numpy(), s['state'])
    want = S.raycast(s['state'], s['origin'], 0.004, s['poses'], s['intr'], FR.SCENE_H, FR.SCENE_W)
    same(cast(scan, vol, s['poses'], s['intr'], FR.SCENE_H, FR.SCENE_W), want, "cube")
    assert all(w.any() for w in want)
    st = FR.sphere_state()
    poses = np.stack([FR.look_at(d, np.full(3, 12 * 0.004)) for d in FR.view_directions()])
    rows = np.tile(np.array([600.0, 600.0, 49.5, 49.5, 10000.0], np.float32), (14, 1))
    want = S.raycast(st, [0.0, 0.0, 0.0], 0.004, poses, rows, 100, 100)
    same(cast(scan, volume_of(dev, st, [0.0, 0.0, 0.0], 0.004), poses, rows, 100, 100), want, "sphere")
    assert all(int((w != 0).sum()) > 3000 for w in want)


def test_errors_launch_nothing(hip, dev):
    L = hip.lib()
    d = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    image = torch.full((64,), 0x5555, dtype=torch.int16, device=dev)
    inf, nan = float('inf'), float('nan')

    def ray(nx=2, ny=2, nz=2, o=0.0, voxel=1.0, state=p, min_count=1, B=1, wh=4, ww=4, intr=p, poses=p, step=0.5, z_near=0.05,
            out=image.data_ptr()):
        return L.cloudaae_tsdf_raycast(nx, ny, nz, o, o, o, voxel, state, min_count, B, wh, ww, intr, poses, step, z_near, out,
                                       hip.stream())
    for kw in (dict(nx=1), dict(ny=513), dict(nx=512, ny=512, nz=513), dict(o=nan), dict(o=inf), dict(voxel=0.0), dict(voxel=-1.0),
               dict(voxel=inf), dict(voxel=nan), dict(state=None), dict(state=p + 4), dict(state=p + 8), dict(min_count=0),
               dict(min_count=-1), dict(B=0), dict(wh=0), dict(ww=0), dict(wh=1 << 13, ww=(1 << 11) + 1),
               dict(B=17, wh=1 << 12, ww=1 << 12), dict(intr=None), dict(poses=None), dict(out=None), dict(step=0.0),
               dict(step=-0.5), dict(step=nan), dict(step=inf), dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=nan), dict(z_near=inf)):
        assert ray(**kw) != 0, kw
        assert b"cloudaae_tsdf_raycast" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0 and bool((image == 0x5555).all())                    # nothing read into, the output untouched
    assert ray() == 0                                                                   # the defaults are a valid call:
    torch.cuda.synchronize()                                                            # every pixel is written, nothing else
    assert bool((image[:16] == 0).all()) and bool((image[16:] == 0x5555).all())


def test_python_refuses_what_the_entry_refuses(scan, dev, hip):
    st, origin, voxel = S.big_wavy()
    vol = volume_of(dev, st, origin, voxel)
    poses, rows, wh, ww = S.batch_case()
    with pytest.raises(ValueError):
        scan.raycast(vol, poses, rows[:3], wh, ww)
    with pytest.raises(ValueError):
        scan.raycast(vol, poses, rows, 0, ww)
    with pytest.raises(ValueError):
        scan.raycast(None, poses, rows, wh, ww)
    for kw in (dict(step=0.0), dict(step=float('nan')), dict(min_count=0), dict(z_near=0.0)):
        with pytest.raises(hip.HipLibraryError):
            scan.raycast(vol, poses, rows, wh, ww, **kw)


# ---- the loop --------------------------------------------------------------------------------------------------------------
def run_scan(scan, depth, truth, **kw):
    return scan.scan_object(depth, FR.SCENE_INTR, S.ORBIT_VOXEL, first_pose=truth[0], aabb=S.cube_aabb(), **dict(S.ORBIT_SETTINGS, **kw))


@pytest.fixture(scope="module")
def orbit_gpu(scan, dev):
    """The orbit scanned on the GPU, with what every step and every frame saw."""
    o = S.orbit()
    steps, states = [], []
    s = run_scan(scan, o['depth'], o['truth'], on_step=lambda f, info: steps.append((f, {
        k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()})),
        on_frame=lambda f, pose, volume: states.append(volume.state.cpu().numpy()))
    return dict(ref=o, scan=s, steps=steps, states=states)


def test_orbit_step_by_step(orbit_gpu):
    """From the GPU's own pose and state before a step: the restatement's raycast equals the GPU's image, its single
    align_step gives the GPU's next pose within 1e-9; after a frame the GPU's volume equals the restatement's integration
    at the GPU's pose, bit for bit.  (An independent CPU loop may differ by a depth quantum once poses differ in the last bits.)"""
    o, s = orbit_gpu['ref'], orbit_gpu['scan']
    r = o['result']
    origin3, voxel, depth = r['origin'], S.ORBIT_VOXEL, o['depth']
    assert s.volume.dims == r['dims'] and np.array_equal(np.array(s.volume.origin), origin3)
    assert np.array_equal(orbit_gpu['states'][0], r['states'][0])
    assert len(orbit_gpu['steps']) == 4 * (len(depth) - 1)
    factor = np.float64(FR.SCENE_INTR[4])
    gu, ju = (V.tau_units(np.array([S.ORBIT_SETTINGS[k]], np.float64), factor) for k in ('gate', 'jump'))
    worst = 0.0
    for f, info in orbit_gpu['steps']:
        state = orbit_gpu['states'][f - 1]
        hyp = info['depth_hyp'].view(np.uint16)
        want = S.raycast(state, origin3, voxel, info['pose_in'], info['rows'], info['wh'], info['ww'])
        same(hyp, want, "frame %d" % f)
        st = TR.step(depth, np.array([info['frame_of']], np.int32), info['origin'], hyp, info['rows'], gu, ju, S.ORBIT_SETTINGS['cos_min'],
                     info['pose_in'])
        assert int(info['status'][0]) == int(st['status'][0]) == 0 and int(info['n_pairs'][0]) == int(st['n_pairs'][0])
        worst = max(worst, float(np.abs(info['pose_out'][0] - st['pose_out'][0]).max()))
    print("largest difference of a step's pose from the restatement's step: %.3g" % worst)
    assert worst <= 1e-9
    for f in range(1, len(depth)):
        assert not s.lost[f]
        want = FR.integrate(orbit_gpu['states'][f - 1].copy(), origin3, voxel, depth[f:f + 1], FR.SCENE_INTR[None], s.poses[f][None],
                            FR.FRONT_VOXELS * voxel, FR.BEHIND_VOXELS * voxel)
        assert np.array_equal(orbit_gpu['states'][f], want), f


def test_orbit_end_to_end(scan, orbit_gpu):
    o, s = orbit_gpu['ref'], orbit_gpu['scan']
    ref_err = S.pose_errors(o['result']['poses'], o['truth'])
    err = S.pose_errors(s.poses, o['truth'])
    print("pose error per frame, the restatement: %s" % np.array2string(ref_err[1:], precision=6))
    print("pose error per frame, the GPU:         %s" % np.array2string(err[1:], precision=6))
    assert not s.lost.any() and np.all(s.status == 0)
    assert np.all(err <= ref_err + 1e-5)
    assert np.all(2 * s.num[1:] >= s.den[1:])
    # the frames from the GPU renderer
    depth = S.orbit_depth(o['truth'], renderer=gpu_renderer)
    g = run_scan(scan, depth, o['truth'])
    err = S.pose_errors(g.poses, o['truth'])
    print("pose error per frame, GPU frames:      %s" % np.array2string(err[1:], precision=6))
    assert not g.lost.any() and np.all(err <= ref_err + 1e-5)


def test_scan_is_the_frame_attempt_replayed_by_hand(scan, dev):
    """Three frames of the orbit, then the same frames by hand from the recorded start poses with the bindings alone --
    track.pose_windows, scan.raycast, track.align_step, detect.fit_counts_window, fuse.integrate: every step's image and pose,
    every frame's volume and every column of the Scan are equal bit for bit."""
    from cloudaae_amd.utils import detect, fuse, track
    o = S.orbit()
    depth, truth, aabb = o['depth'][:3], o['truth'], S.cube_aabb()
    steps, states = [], []
    s = run_scan(scan, depth, truth, on_step=lambda f, info: steps.append((f, {
        k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()})),
        on_frame=lambda f, pose, volume: states.append(volume.state.cpu().numpy()))
    assert len(steps) == 8 and len(states) == 3

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)
    dt = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(dev)
    intr = up(np.tile(FR.SCENE_INTR, (3, 1)), np.float32)
    vol = fuse.volume_for(aabb, S.ORBIT_VOXEL, device=dev)
    fuse.integrate(vol, dt[:1], intr[:1], up(truth[:1], np.float64))
    assert states[0].tobytes() == vol.state.cpu().numpy().tobytes()
    assert s.poses[0].tobytes() == truth[0].tobytes() and (s.num[0], s.den[0], s.lost[0]) == (0, 1, False)
    factor = np.float64(FR.SCENE_INTR[4])
    gate, jump, tau = (up(V.tau_units(np.array([q], np.float64), factor), np.int32)
                       for q in (S.ORBIT_SETTINGS['gate'], S.ORBIT_SETTINGS['jump'], 0.01))
    last = truth[0]
    for f in (1, 2):
        mine = [info for g, info in steps if g == f]
        start = mine[0]['pose_in']
        assert start.tobytes() == last[None].tobytes()                                  # at rest: the frame starts from the last pose
        origin, wh, ww, ok = track.pose_windows(start, aabb[None], FR.SCENE_INTR[None], FR.SCENE_H, FR.SCENE_W, S.ORBIT_SETTINGS['margin'])
        assert ok[0]
        rows_host = np.asarray(FR.SCENE_INTR, np.float32)[None].copy()
        rows_host[:, 2] = FR.SCENE_INTR[2] - origin[:, 0].astype(np.float32)
        rows_host[:, 3] = FR.SCENE_INTR[3] - origin[:, 1].astype(np.float32)
        rows, org, frame = up(rows_host, np.float32), up(origin, np.int32), up([f], np.int32)
        pose = up(start, np.float64)
        for i in range(4):
            d = scan.raycast(vol, pose, rows, wh, ww)
            r = track.align_step(dt, frame, org, d, rows, gate, jump, S.ORBIT_SETTINGS['cos_min'], pose)
            assert mine[i]['pose_in'].tobytes() == pose.cpu().numpy().tobytes(), (f, i)
            assert mine[i]['depth_hyp'].tobytes() == d.cpu().numpy().tobytes(), (f, i)
            assert mine[i]['pose_out'].tobytes() == r['pose_out'].cpu().numpy().tobytes(), (f, i)
            assert (mine[i]['wh'], mine[i]['ww'], mine[i]['frame_of']) == (wh, ww, f) and np.array_equal(mine[i]['origin'], origin)
            assert mine[i]['rows'].tobytes() == rows_host.tobytes()
            pose = r['pose_out']
        d = scan.raycast(vol, pose, rows, wh, ww)
        c = detect.fit_counts_window(dt, None, frame, None, org, d.view(1, 1, wh, ww), tau)['counts'].cpu().numpy().reshape(6).astype(np.int64)
        num, den = int(c[1]), int(c[1] + c[2] + c[3])
        num, den = (num, den) if den > 0 else (0, 1)
        lost = num * 2 < 1 * den
        if not lost:
            fuse.integrate(vol, dt[f:f + 1], intr[f:f + 1], pose)
            last = pose.cpu().numpy()[0]
        print("frame %d: score %d / %d, pairs %d" % (f, num, den, int(r['n_pairs'][0])))
        assert states[f].tobytes() == vol.state.cpu().numpy().tobytes(), f
        assert s.poses[f].tobytes() == last.tobytes(), f
        assert (int(s.num[f]), int(s.den[f]), bool(s.lost[f])) == (num, den, lost), f
        assert (int(s.n_pairs[f]), int(s.status[f])) == (int(r['n_pairs'][0]), int(r['status'][0])), f
    assert s.poses.dtype == np.float64 and s.n_pairs.dtype == np.int32 and s.status.dtype == np.int32 and s.lost.dtype == bool


def test_lost_and_resumed(scan, dev):
    from cloudaae_amd.utils import mesh_models
    o = S.orbit(8, S.ORBIT_VOXEL, S.STEP_VOXELS, (5,))
    r = o['result']
    states = []
    s = run_scan(scan, o['depth'], o['truth'], on_frame=lambda f, pose, volume: states.append(volume.state.cpu().numpy()))
    assert s.lost.tolist() == r['lost'].tolist() == [False] * 5 + [True, False, False]
    assert np.array_equal(states[5], states[4]) and np.array_equal(s.poses[5], s.poses[4])
    assert (s.num[5], s.den[5]) == (0, 1)
    err, ref_err = S.pose_errors(s.poses, o['truth']), S.pose_errors(r['poses'], o['truth'])
    print("removed in frame 5: pose error per frame %s" % np.array2string(err, precision=5))
    assert np.all(err <= ref_err + 1e-5)
    v, t = s.mesh()
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and int(t.shape[0]) > 1000
    p = mesh_models.pack_meshes([(v, t)], device=dev)
    assert int(p.num_triangles[0]) == int(t.shape[0])


def test_default_first_pose_and_box(scan, dev):
    """Without first_pose and aabb: no rotation, the centre of the used pixels' box, the box grown by half its largest side."""
    o = S.orbit()
    depth = o['depth'][:3]
    s = scan.scan_object(depth, FR.SCENE_INTR, S.ORBIT_VOXEL)
    first = S.default_first_pose(depth[0], None, FR.SCENE_INTR, 0)
    assert np.allclose(s.poses[0], first, atol=1e-12) and np.array_equal(s.poses[0][:3, :3], np.eye(3))
    box = S.grown(S.used_points_aabb(depth[0], None, FR.SCENE_INTR, first, 0), 0.5)
    assert np.allclose(s.aabb, box, atol=1e-12) and s.volume.dims == FR.volume_for(box, S.ORBIT_VOXEL)[1]
    assert not s.lost.any()
    # the camera's motion against the truth's, since the object's frame is another one
    rel, rel_true = s.poses[2] @ np.linalg.inv(s.poses[0]), o['truth'][2] @ np.linalg.inv(o['truth'][0])
    print("default first pose and box: %s voxels, relative motion off by %.3g" % (s.volume.dims, np.abs(rel - rel_true).max()))
    assert np.abs(rel - rel_true).max() < 4e-3


def test_command_line_scans_a_record_file(scan, tmp_path, capsys):
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import mesh_models, render
    o = S.orbit()
    n = 4
    depth, truth = o['depth'][:n], o['truth'][:n]
    label = (depth != 0).astype(np.uint8) * 4                                           # class 3
    intr = np.tile(FR.SCENE_INTR, (n, 1))
    payloads = render.frame_records(depth, label, intr, [[T] for T in truth], [[3]] * n, 7, list(range(n)))
    path, out = str(tmp_path / "0007_pcnn.tfrecord"), str(tmp_path / "model.ply")
    tfrecord_io.write_records(path, payloads)
    assert scan.main(["--files", path, "--target_cls", "3", "--voxel", "0.004", "--out", out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    assert len(lines) == n + 2 and all(" lost 0 " in l for l in lines[:n])
    assert all(float(l.split()[-1]) < 4e-3 for l in lines[:n])                          # trans_err_m, for reporting: within a voxel
    rv, rt, _ = mesh_models.read_ply(out)
    w = lines[-1].split()
    assert (int(w[0]), int(w[2])) == (len(rv), len(rt)) and len(rt) > 1000
