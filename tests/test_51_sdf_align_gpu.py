"""GPU: cloudaae_tsdf_align_step against the NumPy restatement of DESIGN.md "Scanning on the field"
(tests/sdf_align_reference.py) from identical inputs -- the rows and the status equal, the solution and the pose within 1e-9,
the bound tests/test_42 and tests/test_45 use for the same solve (tests/test_sdf_align_host.py shows that the cases' solutions
move by less than 1e-10 between the kernel's order of the sums and the restatement's); then scan_object(align='sdf'): step by
step against the restatement from the GPU's own poses and states, end to end on the 30 degree orbit, and the command line."""
import numpy as np
import pytest
import torch

import fuse_reference as FR
import scan_reference as S
import sdf_align_reference as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scan(hip):
    from cloudaae_amd.utils import scan
    return scan


def volume_of(dev, state, origin, voxel):
    from cloudaae_amd.utils import fuse
    nz, ny, nx, _ = state.shape
    vol = fuse.Volume(origin, voxel, (nx, ny, nz), dev)
    vol.state.copy_(torch.from_numpy(np.ascontiguousarray(state)))
    return vol


def up(dev, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def gpu_step(scan, dev, c, vol=None):
    """A case of the restatement through scan.align_volume_step -> dict of numpy arrays."""
    vol = volume_of(dev, c['state'], c['vol_origin'], c['voxel']) if vol is None else vol
    depth = torch.from_numpy(c['depth'].view(np.int16)).to(dev)
    label = None if c['label'] is None else up(dev, c['label'], np.uint8)
    want = None if c['want'] is None else up(dev, c['want'], np.int32)
    pose, x, n, st = scan.align_volume_step(vol, depth, up(dev, c['intr_win'], np.float32), up(dev, c['pose_in'], np.float64),
                                            up(dev, c['frame_of'], np.int32), up(dev, c['origin'], np.int32), c['wh'], c['ww'], label, want,
                                            c['front'], c['min_count'])
    torch.cuda.synchronize()
    b = len(c['frame_of'])
    assert pose.dtype == torch.float64 and tuple(pose.shape) == (b, 4, 4) and x.dtype == torch.float64 and tuple(x.shape) == (b, 6)
    assert n.dtype == torch.int32 and tuple(n.shape) == (b,) and st.dtype == torch.int32 and tuple(st.shape) == (b,)
    return dict(pose_out=pose.cpu().numpy(), x=x.cpu().numpy(), n_pairs=n.cpu().numpy(), status=st.cpu().numpy())


def held(got, want, pose_in, name):
    """The rows and the status equal; on status 0 the solution and the pose within 1e-9; else zeros and pose_in's bits."""
    assert got['n_pairs'].tolist() == want['n_pairs'].tolist(), name
    assert got['status'].tolist() == want['status'].tolist(), name
    worst = 0.0
    for i, st in enumerate(want['status']):
        if st == 0:
            worst = max(worst, float(np.abs(got['x'][i] - want['x'][i]).max()), float(np.abs(got['pose_out'][i] - want['pose_out'][i]).max()))
        else:
            assert not got['x'][i].any() and got['pose_out'][i].tobytes() == np.asarray(pose_in[i], np.float64).tobytes(), (name, i)
    print("%s: rows %s, status %s, largest difference %.3g" % (name, want['n_pairs'].tolist(), want['status'].tolist(), worst))
    assert worst <= 1e-9, name


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ('pose_out', 'x', 'n_pairs', 'status'))


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["volumes", "windows", "filters", "min_count", "sphere"])
def test_cases_equal_the_restatement(scan, dev, group):
    cases = dict(volumes=A.volume_cases, windows=A.window_cases, filters=A.filter_cases, min_count=A.min_count_cases,
                 sphere=lambda: [A.sphere_case()])[group]()
    for name, c in cases:
        held(gpu_step(scan, dev, c), A.run_case(c), c['pose_in'], name)


def test_batch_alone_and_twice(scan, dev):
    name, c = A.batch_case()
    vol = volume_of(dev, c['state'], c['vol_origin'], c['voxel'])
    got = gpu_step(scan, dev, c, vol)
    want = A.run_case(c)
    held(got, want, c['pose_in'], name)
    assert want['status'].tolist() == [0, 0, 1, 1, 4, 4, 0]
    assert same_bits(got, gpu_step(scan, dev, c, vol))                                   # two runs
    for i in range(7):                                                                  # a sample alone, bit for bit
        one = gpu_step(scan, dev, A.alone(c, i), vol)
        assert same_bits(one, {k: v[i:i + 1] for k, v in got.items()}), i


def test_volume_fused_on_the_gpu_from_the_14_cube_views(scan, dev):
    from cloudaae_amd.utils import fuse
    s = FR.scene('cube', 0.004)
    vol = fuse.Volume(s['origin'], s['voxel'], s['dims'], dev)
    fuse.integrate(vol, s['depth'], s['intr'], s['poses'])
    torch.cuda.synchronize()
    assert np.array_equal(vol.state.cpu().numpy(), s['state'])
    centre = s['aabb'].mean(axis=0)
    poses = np.array([A.off_pose(T, 0.5, 0.002, centre) for T in s['poses']])
    name, c = A.case("fused cube, 14 views", s['state'], s['origin'], 0.004, s['depth'], np.arange(14), np.zeros((14, 2)), FR.SCENE_H,
                     FR.SCENE_W, s['intr'], poses)
    want = A.run_case(c)
    held(gpu_step(scan, dev, c, vol), want, poses, name)
    assert np.all(want['status'] == 0) and np.all(want['n_pairs'] > 3000)


def test_errors_launch_nothing_and_outputs_beyond_b_stay(hip, dev):
    L = hip.lib()
    d = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    nbytes = int(L.cloudaae_tsdf_align_step_workspace(1, 4, 4))
    assert nbytes == 28 * 8 + 8
    for b, wh, ww in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1 << 13, (1 << 11) + 1), (17, 1 << 12, 1 << 12)):
        assert int(L.cloudaae_tsdf_align_step_workspace(b, wh, ww)) == 0
    assert int(L.cloudaae_tsdf_align_step_workspace(3, 23, 89)) == 3 * (28 * 8 + 4) + 4      # 2047 pixels: one run; padded to 8
    assert int(L.cloudaae_tsdf_align_step_workspace(1, 3, 683)) == 2 * (28 * 8 + 4)          # 2049: two runs
    pose_out = torch.full((32,), 7.5, dtype=torch.float64, device=dev)
    x = torch.full((12,), 7.5, dtype=torch.float64, device=dev)
    n_pairs = torch.full((2,), 0x5555, dtype=torch.int32, device=dev)
    status = torch.full((2,), 0x5555, dtype=torch.int32, device=dev)
    ws = torch.full((nbytes + 8,), 0x55, dtype=torch.uint8, device=dev)
    inf, nan = float('inf'), float('nan')

    def step(nx=2, ny=2, nz=2, o=0.0, voxel=1.0, state=p, min_count=1, front=4.0, f=1, h=4, w=4, depth=p, label=None, want=None, b=1,
             frame_of=p, origin=p, wh=4, ww=4, intr=p, pose_in=p, n=n_pairs.data_ptr(), xs=x.data_ptr(), st=status.data_ptr(),
             out=pose_out.data_ptr(), work=ws.data_ptr(), work_bytes=nbytes):
        return L.cloudaae_tsdf_align_step(nx, ny, nz, o, o, o, voxel, state, min_count, front, f, h, w, depth, label, want, b, frame_of,
                                          origin, wh, ww, intr, pose_in, n, xs, st, out, work, work_bytes, hip.stream())
    for kw in (dict(nx=1), dict(ny=513), dict(nx=512, ny=512, nz=513), dict(o=nan), dict(o=inf), dict(voxel=0.0), dict(voxel=-1.0),
               dict(voxel=inf), dict(voxel=nan), dict(state=None), dict(state=p + 4), dict(state=p + 8), dict(min_count=0),
               dict(min_count=-1), dict(front=0.0), dict(front=-1.0), dict(front=nan), dict(front=inf), dict(f=0), dict(h=0), dict(w=0),
               dict(b=0), dict(wh=0), dict(ww=0), dict(h=1 << 13, w=(1 << 11) + 1), dict(wh=1 << 13, ww=(1 << 11) + 1),
               dict(b=17, wh=1 << 12, ww=1 << 12), dict(depth=None), dict(frame_of=None), dict(origin=None), dict(intr=None),
               dict(pose_in=None), dict(n=None), dict(xs=None), dict(st=None), dict(out=None), dict(work=None),
               dict(work=ws.data_ptr() + 4), dict(work_bytes=nbytes - 1), dict(work_bytes=0)):
        assert step(**kw) != 0, kw
        assert b"cloudaae_tsdf_align_step" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0                                                      # nothing read into
    assert bool((pose_out == 7.5).all()) and bool((x == 7.5).all()) and bool((n_pairs == 0x5555).all())
    assert bool((status == 0x5555).all()) and bool((ws == 0x55).all())                  # the outputs untouched
    # the defaults are a valid call (a label without want, and want without a label, are no filter): an empty frame gives no
    # row, status 1, x zeros and pose_in; what lies beyond b = 1 and beyond the workspace's bytes stays
    lab = torch.full((16,), 9, dtype=torch.uint8, device=dev)
    assert step() == 0 and step(label=lab.data_ptr()) == 0 and step(want=p) == 0
    torch.cuda.synchronize()
    assert n_pairs.tolist() == [0, 0x5555] and status.tolist() == [1, 0x5555]
    assert bool((x[:6] == 0).all()) and bool((x[6:] == 7.5).all())
    assert bool((pose_out[:16] == 0).all()) and bool((pose_out[16:] == 7.5).all())
    assert bool((ws[nbytes:] == 0x55).all()) and int(d.abs().sum()) == 0


def test_python_refuses_what_the_entry_refuses(scan, dev, hip):
    name, c = A.window_cases()[2]
    vol = volume_of(dev, c['state'], c['vol_origin'], c['voxel'])
    depth = torch.from_numpy(c['depth'].view(np.int16)).to(dev)
    rows, pose = up(dev, c['intr_win'], np.float32), up(dev, c['pose_in'], np.float64)
    fo, org = up(dev, c['frame_of'], np.int32), up(dev, c['origin'], np.int32)
    ok = dict(volume=vol, depth=depth, intr_win=rows, poses=pose, frame_of=fo, origin=org, wh=c['wh'], ww=c['ww'])
    lab = torch.zeros(depth.shape, dtype=torch.uint8, device=dev)
    for kw in (dict(volume=None), dict(intr_win=rows.repeat(2, 1)), dict(frame_of=fo.to(torch.int64)), dict(origin=org.reshape(2)),
               dict(wh=0), dict(depth=depth.to(torch.float32)), dict(label=lab), dict(label=lab[:, :1], want=torch.zeros(2, dtype=torch.int32, device=dev)),
               dict(poses=pose.reshape(16))):
        with pytest.raises(ValueError):
            scan.align_volume_step(**dict(ok, **kw))
    for kw in (dict(front=0.0), dict(front=float('nan')), dict(min_count=0)):
        with pytest.raises(hip.HipLibraryError):
            scan.align_volume_step(**dict(ok, **kw))
    with pytest.raises(ValueError):
        scan.scan_object(c['depth'], FR.SCENE_INTR, 0.004, align="icp")


# ---- the loop --------------------------------------------------------------------------------------------------------------
def run_scan(scan, depth, truth, **kw):
    return scan.scan_object(depth, FR.SCENE_INTR, S.ORBIT_VOXEL, first_pose=truth[0], aabb=S.cube_aabb(), align="sdf",
                            **dict(S.ORBIT_SETTINGS, **kw))


@pytest.fixture(scope="module")
def orbit_gpu(scan, dev):
    """The 30 degree orbit scanned on the field on the GPU, with what every step and every frame saw."""
    o = A.orbit()
    steps, states = [], []
    s = run_scan(scan, o['depth'], o['truth'], on_step=lambda f, info: steps.append((f, {
        k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()})),
        on_frame=lambda f, pose, volume: states.append(volume.state.cpu().numpy()))
    return dict(ref=o, scan=s, steps=steps, states=states)


def test_orbit_step_by_step(orbit_gpu):
    """From the GPU's own pose and state before a step, the restatement's single step gives the GPU's next pose within 1e-9;
    a frame's steps chain; after a frame the GPU's volume equals the restatement's integration at the GPU's pose, bit for bit."""
    o, s = orbit_gpu['ref'], orbit_gpu['scan']
    r = o['result']
    origin3, voxel, depth = r['origin'], S.ORBIT_VOXEL, o['depth']
    front = FR.FRONT_VOXELS * voxel
    assert s.volume.dims == r['dims'] and np.array_equal(np.array(s.volume.origin), origin3)
    assert np.array_equal(orbit_gpu['states'][0], r['states'][0])
    assert len(orbit_gpu['steps']) == 4 * (len(depth) - 1)
    worst, before = 0.0, None
    for k, (f, info) in enumerate(orbit_gpu['steps']):
        assert 'depth_hyp' not in info
        if k % 4:
            assert info['pose_in'].tobytes() == before.tobytes(), (f, k)
        st = A.step(orbit_gpu['states'][f - 1], origin3, voxel, 1, front, depth, None, None, np.array([info['frame_of']], np.int32),
                    info['origin'], info['wh'], info['ww'], info['rows'], info['pose_in'])
        assert int(info['status'][0]) == int(st['status'][0]) == 0 and int(info['n_pairs'][0]) == int(st['n_pairs'][0])
        worst = max(worst, float(np.abs(info['pose_out'][0] - st['pose_out'][0]).max()))
        before = info['pose_out']
    print("largest difference of a step's pose from the restatement's step: %.3g" % worst)
    assert worst <= 1e-9
    for f in range(1, len(depth)):
        assert not s.lost[f]
        assert s.poses[f].tobytes() == orbit_gpu['steps'][4 * f - 1][1]['pose_out'][0].tobytes()
        want = FR.integrate(orbit_gpu['states'][f - 1].copy(), origin3, voxel, depth[f:f + 1], FR.SCENE_INTR[None], s.poses[f][None],
                            front, FR.BEHIND_VOXELS * voxel)
        assert np.array_equal(orbit_gpu['states'][f], want), f


def test_orbit_end_to_end_and_the_tracking_condition(orbit_gpu):
    """Per frame the GPU's error is at most the restatement's + 1e-5; nothing is lost; and the tracking condition: every frame's
    error is below a quarter of what holding the previous frame's true pose gives (computed from the scene's true poses)."""
    o, s = orbit_gpu['ref'], orbit_gpu['scan']
    ref_err, err = S.pose_errors(o['result']['poses'], o['truth']), S.pose_errors(s.poses, o['truth'])
    hold = A.hold_errors(o['truth'])
    print("pose error per frame, the restatement: %s" % np.array2string(ref_err[1:], precision=6))
    print("pose error per frame, the GPU:         %s" % np.array2string(err[1:], precision=6))
    print("holding the previous true pose:        %s" % np.array2string(hold, precision=6))
    assert not s.lost.any() and np.all(s.status == 0)
    assert np.all(err <= ref_err + 1e-5)
    assert np.all(err[1:] < hold / 4.0)
    assert np.all(2 * s.num[1:] >= s.den[1:])


def test_raycast_stays_the_default(scan, dev):
    """Three frames without align= and with align='raycast': the same bits, and other ones than align='sdf' gives."""
    o = S.orbit()
    kw = dict(first_pose=o['truth'][0], aabb=S.cube_aabb(), **S.ORBIT_SETTINGS)
    a = scan.scan_object(o['depth'][:3], FR.SCENE_INTR, S.ORBIT_VOXEL, **kw)
    b = scan.scan_object(o['depth'][:3], FR.SCENE_INTR, S.ORBIT_VOXEL, align="raycast", **kw)
    c = scan.scan_object(o['depth'][:3], FR.SCENE_INTR, S.ORBIT_VOXEL, align="sdf", **kw)
    assert a.poses.tobytes() == b.poses.tobytes() and a.volume.state.cpu().numpy().tobytes() == b.volume.state.cpu().numpy().tobytes()
    assert a.poses[1:].tobytes() != c.poses[1:].tobytes() and not c.lost.any()


def test_command_line_scans_a_record_file_on_the_field(scan, tmp_path, capsys):
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import mesh_models, render
    o = A.orbit()
    n = 4
    depth, truth = o['depth'][:n], o['truth'][:n]
    label = (depth != 0).astype(np.uint8) * 4                                           # class 3
    intr = np.tile(FR.SCENE_INTR, (n, 1))
    payloads = render.frame_records(depth, label, intr, [[T] for T in truth], [[3]] * n, 7, list(range(n)))
    path, out = str(tmp_path / "0007_pcnn.tfrecord"), str(tmp_path / "model.ply")
    tfrecord_io.write_records(path, payloads)
    assert scan.main(["--files", path, "--target_cls", "3", "--voxel", "0.004", "--out", out, "--align", "sdf"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    assert len(lines) == n + 2 and all(" lost 0 " in l for l in lines[:n])
    # the restatement of what the command runs: the label's filter, the true first pose, the default box
    ref = A.scan(depth, FR.SCENE_INTR, 0.004, label=label, want=4, first_pose=truth[0])['poses']
    for f, l in enumerate(lines[:n]):
        want = float(np.sqrt(((ref[f][:3, 3] - truth[f][:3, 3]) ** 2).sum()))
        assert float(l.split()[-1]) <= want + 1e-5 + 1e-6, l                            # trans_err_m, printed with 6 decimals
    rv, rt, _ = mesh_models.read_ply(out)
    w = lines[-1].split()
    assert (int(w[0]), int(w[2])) == (len(rv), len(rt)) and len(rt) > 1000
