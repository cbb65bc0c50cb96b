"""GPU: cloudaae_tsdf_integrate, cloudaae_tsdf_count and cloudaae_tsdf_emit against the NumPy restatement of DESIGN.md "Fused
models" (tests/fuse_reference.py) from identical inputs, then utils/fuse.py end to end on the scenes whose conditions
tests/test_fuse_host.py asserts for the restatement alone.

Everything the kernels write is an integer or a float64 formed in a fixed order from exactly widened values, so every
comparison is for equality: the four sums per voxel, tri_count, tri_key, and tri_pos as bits."""
import numpy as np
import pytest
import torch

import detect_reference as DR
import fuse_reference as FR
import track_reference as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fuse(hip):
    from cloudaae_amd.utils import fuse
    return fuse


def gpu_renderer(meshes, frames, intr, H, W):
    from cloudaae_amd.utils import render
    return render.render_frames(meshes, frames, intr, H, W)['depth'].cpu().numpy().view(np.uint16)


def integrate(fuse, dev, origin, voxel, dims, depth, intr, poses, label=None, want=None, volume=None, **kw):
    """fuse.integrate on numpy inputs -> (state as numpy, the Volume)."""
    vol = fuse.Volume(origin, voxel, dims, dev) if volume is None else volume
    fuse.integrate(vol, depth, intr, poses, label=label, want=want, **kw)
    torch.cuda.synchronize()
    return vol.state.cpu().numpy(), vol


def extract(fuse, dev, state, origin, voxel, min_count=1):
    """fuse.extract_triangles on a state written by hand -> (tri_count, tri_pos, tri_key) as numpy."""
    nz, ny, nx, _ = state.shape
    vol = fuse.Volume(origin, voxel, (nx, ny, nz), dev)
    vol.state.copy_(torch.from_numpy(state))
    pos, key, count = fuse.extract_triangles(vol, min_count)
    torch.cuda.synchronize()
    return count.cpu().numpy(), pos.cpu().numpy(), key.cpu().numpy()


def same_triangles(got, want, what):
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want[0]), what
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2]), what
    assert got[1].shape == want[1].shape and got[1].tobytes() == np.ascontiguousarray(want[1]).tobytes(), what


# ---- integrate -------------------------------------------------------------------------------------------------------------
def test_hand_cases_equal_the_restatement(fuse, dev):
    for name, c in FR.hand_cases():
        a = dict(c)
        got, _ = integrate(fuse, dev, a.pop('origin'), a.pop('voxel'), a.pop('dims'), a.pop('depth'), a.pop('intr'), a.pop('poses'), **a)
        want = FR.run_case(c)
        print("%s: %d votes" % (name, int(want[..., 1].sum() + want[..., 3].sum())))
        assert got.dtype == np.int32 and np.array_equal(got, want), name


def test_small_volumes_frames_labels_splits_and_orders(fuse, dev):
    fr = FR.small_frames()
    for name, origin, voxel, dims in FR.small_volumes():
        for labelled in (False, True):
            lab = dict(label=fr['label'], want=fr['want']) if labelled else {}
            want = FR.integrate(FR.new_state(dims), origin, voxel, fr['depth'], fr['intr'], fr['poses'], 4 * voxel, 1.5 * voxel, **lab)
            got, _ = integrate(fuse, dev, origin, voxel, dims, fr['depth'], fr['intr'], fr['poses'], **lab)
            again, _ = integrate(fuse, dev, origin, voxel, dims, fr['depth'], fr['intr'], fr['poses'], **lab)
            assert np.array_equal(got, want), (name, labelled)
            assert got.tobytes() == again.tobytes(), (name, labelled)                  # two runs, bit for bit

            def part(sel, volume=None, flip=False):
                o = slice(None, None, -1) if flip else slice(None)
                sub = {k: v[sel][o] for k, v in lab.items()}
                return integrate(fuse, dev, origin, voxel, dims, fr['depth'][sel][o], fr['intr'][sel][o], fr['poses'][sel][o],
                                 volume=volume, **sub)
            _, vol = part(slice(0, 8))
            split, _ = part(slice(8, 17), vol)
            assert split.tobytes() == got.tobytes(), (name, labelled)                  # frames [0, 8) then [8, 17)
            _, vol = part(slice(8, 17), flip=True)
            rev, _ = part(slice(0, 8), vol, flip=True)
            assert rev.tobytes() == got.tobytes(), (name, labelled)                    # the reversed order
            one, _ = part(slice(5, 6))                                                  # F = 1
            assert np.array_equal(one, FR.integrate(FR.new_state(dims), origin, voxel, fr['depth'][5:6], fr['intr'][5:6], fr['poses'][5:6],
                                                    4 * voxel, 1.5 * voxel, **{k: v[5:6] for k, v in lab.items()})), (name, labelled)
    half = FR.integrate(FR.new_state((20, 4, 4)), [0.0, 0.0, 0.0], 0.03, fr['depth'], fr['intr'], fr['poses'], 0.12, 0.045)
    votes = half[..., 1] + half[..., 3]
    assert (votes == 0).any() and (votes > 0).any()                                     # the volume does straddle the frustum


@pytest.fixture(scope="module")
def cube(fuse, dev):
    """The cube scene with its depth from the GPU renderer, fused on the GPU."""
    s = FR.scene('cube', 0.004)
    depth = FR.scene_inputs('cube', 0.004, gpu_renderer)['depth']
    state, vol = integrate(fuse, dev, s['origin'], s['voxel'], s['dims'], depth, s['intr'], s['poses'])
    return dict(ref=s, depth=depth, state=state, volume=vol)


def test_cube_scene_state(cube):
    assert np.array_equal(cube['depth'], cube['ref']['depth'])                          # the two renderers agree first
    assert np.array_equal(cube['state'], cube['ref']['state'])


# ---- count and emit --------------------------------------------------------------------------------------------------------
def test_all_256_patterns(fuse, dev):
    rng = np.random.default_rng(11)
    for mask in range(256):
        st = FR.pattern_state(mask, rng.uniform(0.1, 0.9, 8))
        same_triangles(extract(fuse, dev, st, [0.25, -0.5, 1.0], 0.125), FR.extract_triangles(st, [0.25, -0.5, 1.0], 0.125), mask)


def test_fields_written_into_the_state(fuse, dev):
    cases = [("sphere", FR.sphere_state(), 1), ("random field", FR.random_field_state(), 1),
             ("unknown corners and zeros", FR.wavy_state((13, 9, 7), 4, zeros=40, unknown=40), 1),
             ("min_count 2", FR.wavy_state((13, 9, 7), 5, zeros=10, unknown=10, count=2), 2),
             ("nx - 1 = 1", FR.wavy_state((2, 6, 6), 0, zeros=2, unknown=1), 1)]
    cases += [("nx - 1 = %d" % (nx - 1), FR.wavy_state((nx, 3, 3), 1, zeros=5, unknown=3), 1) for nx in (64, 65, 66)]
    mixed = FR.wavy_state((13, 9, 7), 6)
    mixed[..., 2], mixed[..., 3] = -mixed[..., 0], 1                                   # min_count 2 with single votes: the deep band
    cases.append(("deep band", mixed, 2))
    for name, st, min_count in cases:
        origin, voxel = [0.1, -0.2, 0.3], 0.003
        want = FR.extract_triangles(st, origin, voxel, min_count)
        got = extract(fuse, dev, st, origin, voxel, min_count)
        print("%s: %d triangles in %d cells" % (name, len(want[1]), len(want[0])))
        assert len(want[1]) > 0, name
        same_triangles(got, want, name)
        # every occurrence of a key carries identical position bits
        keys, first, inverse = np.unique(got[2].reshape(-1), return_index=True, return_inverse=True)
        flat = got[1].reshape(-1, 3)
        assert flat[first][inverse.reshape(-1)].tobytes() == flat.tobytes(), name


def test_empty_surfaces(fuse, dev):
    for field in (0.5, 0.0):                                                            # all outside; v == 0 is outside too
        st = FR.state_from_field(np.full((5, 4, 3), field))
        count, pos, key = extract(fuse, dev, st, [0.0, 0.0, 0.0], 1.0)
        assert count.shape == (24,) and count.sum() == 0 and pos.shape == (0, 3, 3) and key.shape == (0, 3)
    vol = fuse.Volume([0.0, 0.0, 0.0], 1.0, (3, 4, 5), dev)                             # nothing integrated: all unknown
    v, t = fuse.extract_mesh(vol)
    assert v.shape == (0, 3) and v.dtype == torch.float32 and t.shape == (0, 3) and t.dtype == torch.int32


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_fused_cube_and_prism_meshes(fuse, dev, cube):
    v, t = fuse.extract_mesh(cube['volume'])
    assert v.dtype == torch.float32 and t.dtype == torch.int32
    assert v.cpu().numpy().tobytes() == cube['ref']['vertices'].tobytes() and np.array_equal(t.cpu().numpy(), cube['ref']['triangles'])
    s = FR.scene('prism', 0.0025)
    depth = FR.scene_inputs('prism', 0.0025, gpu_renderer)['depth']
    assert np.array_equal(depth, s['depth'])
    # fuse_frames with the box given: the same volume as the restatement's
    v, t, vol = fuse.fuse_frames(depth, None, s['intr'], s['poses'], None, 0.0025, aabb=s['aabb'])
    assert vol.dims == s['dims'] and np.array_equal(vol.state.cpu().numpy(), s['state'])
    assert v.cpu().numpy().tobytes() == s['vertices'].tobytes() and np.array_equal(t.cpu().numpy(), s['triangles'])
    # without a box it comes from the back-projected pixels: it holds the object, and the mesh is closed again
    v, t, vol = fuse.fuse_frames(depth, None, s['intr'], s['poses'], None, 0.0025)
    lo = np.array(vol.origin) + 4 * vol.voxel
    hi = lo + (np.array(vol.dims) - 8) * vol.voxel
    assert np.all(lo <= s['aabb'][0] + 0.002) and np.all(hi >= s['aabb'][1] - 0.002) and np.all(hi - lo <= s['aabb'][1] - s['aabb'][0] + 0.01)
    m = FR.mesh_stats(v.cpu().numpy(), t.cpu().numpy())
    assert m['boundary'] == 0 and m['components'] == 1 and m['euler'] == 2 and m['volume'] > 0
    assert fuse.mesh_counts(v, t) == (m['V'], m['T'], 0, 1)
    # the mesh is one pack_meshes takes
    from cloudaae_amd.utils import mesh_models
    p = mesh_models.pack_meshes([(v, t)], device=dev)
    assert int(p.num_triangles[0]) == m['T']


def test_ply_round_trip(fuse, cube, tmp_path):
    from cloudaae_amd.utils import mesh_models
    v, t = fuse.extract_mesh(cube['volume'])
    path = str(tmp_path / "cube.ply")
    mesh_models.write_ply(path, v, t)
    rv, rt, rc = mesh_models.read_ply(path)
    assert rc is None and rv.dtype == np.float32 and rt.dtype == np.int32
    assert rv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(rt, t.cpu().numpy())
    mesh_models.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    rv, rt, _ = mesh_models.read_ply(path)
    assert rv.shape == (0, 3) and rt.shape == (0, 3)


def test_fused_cube_tracks_like_the_restatement(fuse, dev, cube):
    """The fused cube in the CAD cube's place, one frame of the slow sequence, from the off pose of tests/test_42_track_gpu.py.
    The scene's cube spans [0, 7 cm]^3 and the sequence's is centred, hence the shift."""
    from cloudaae_amd.utils import mesh_models, track
    v, t = fuse.extract_mesh(cube['volume'])
    fused = ((v.cpu().numpy() - np.float32(0.035)).astype(np.float32), t.cpu().numpy())
    meshes = list(DR.scene_meshes())
    meshes[TR.CUBE] = fused
    depth, truth = TR.frames(TR.SLOW)
    start = TR.off_pose(truth[0])
    want = TR.align(depth[:1], TR.SCENE_INTR, meshes, [TR.CUBE], [0], start[None])
    ref_err = TR.pose_error(want['poses'][-1, 0], truth[0])
    a = track.align_poses(depth[:1], TR.SCENE_INTR, mesh_models.pack_meshes(meshes, device=dev), [TR.CUBE], [0], start[None])
    got_err = TR.pose_error(a['poses'].cpu().numpy()[0], truth[0])
    print("fused cube, frame 0: the restatement's loop ends %.3g from the truth, the GPU's %.3g" % (ref_err, got_err))
    assert np.all(want['status'] == 0) and int(a['status'][0]) == 0
    # The restatement's loop does not stay within 2e-3 with this mesh: it ends 6.5e-3 from the truth (largest difference of
    # a pose entry; 3.2e-3 after the first step, then 7.2e-3, 6.4e-3, 6.5e-3) where the CAD cube ends at 4.6e-5.  One voxel is
    # 4 mm and the fused surface lies up to 0.76 voxel off the cube's, mostly outside it.  So only what was found is
    # asserted: that figure rounded up, and the GPU loop within 1e-3 of it.
    assert ref_err <= 7e-3
    assert abs(got_err - ref_err) <= 1e-3


def test_command_line_fuses_a_record_file(fuse, cube, tmp_path, capsys):
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import mesh_models, render
    s = cube['ref']
    n = len(s['poses'])
    label = (s['depth'] != 0).astype(np.uint8) * 4                                      # class 3
    payloads = render.frame_records(s['depth'], label, s['intr'], [[T] for T in s['poses']], [[3]] * n, 7, list(range(n)))
    path, out = str(tmp_path / "0007_pcnn.tfrecord"), str(tmp_path / "model.ply")
    tfrecord_io.write_records(path, payloads)
    assert fuse.main(["--files", path, "--target_cls", "3", "--voxel", "0.004", "--out", out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    w = lines[-1].split()
    rv, rt, _ = mesh_models.read_ply(out)
    assert (int(w[0]), int(w[2])) == (len(rv), len(rt)) and w[4:6] == ["0", "boundary"] and w[7:9] == ["1", "components"]
    side = rv.max(axis=0) - rv.min(axis=0)
    assert np.all(np.abs(side - 0.07) < 0.004)                                          # (the record's poses are float32)


# ---- error returns ---------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(hip, dev):
    L = hip.lib()
    d = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    inf, nan = float('inf'), float('nan')

    def integ(nx=2, ny=2, nz=2, o=0.0, voxel=1.0, state=p, f=1, h=4, w=4, depth=p, intr=p, poses=p, front=4.0, behind=1.5, z_near=0.05):
        return L.cloudaae_tsdf_integrate(nx, ny, nz, o, o, o, voxel, state, f, h, w, depth, None, None, intr, poses, front, behind,
                                         z_near, hip.stream())
    for kw in (dict(nx=1), dict(ny=513), dict(nx=512, ny=512, nz=513), dict(nx=512, ny=512, nz=512 + 1), dict(o=nan), dict(voxel=0.0),
               dict(voxel=-1.0), dict(voxel=inf), dict(voxel=nan), dict(state=None), dict(state=p + 4), dict(f=0), dict(f=(1 << 19) + 1),
               dict(h=0), dict(h=1 << 13, w=(1 << 11) + 1), dict(depth=None), dict(intr=None), dict(poses=None), dict(front=nan),
               dict(front=inf), dict(front=1.5), dict(front=1.0), dict(behind=0.0), dict(behind=-1.0), dict(behind=nan),
               dict(z_near=0.0), dict(z_near=nan), dict(z_near=inf)):
        assert integ(**kw) != 0, kw
        assert b"cloudaae_tsdf_integrate" in L.cloudaae_last_error(), kw

    def count(nx=2, ny=2, nz=2, state=p, min_count=1, out=p):
        return L.cloudaae_tsdf_count(nx, ny, nz, state, min_count, out, hip.stream())
    for kw in (dict(nz=1), dict(nx=513), dict(state=None), dict(out=None), dict(min_count=0), dict(state=p + 8)):
        assert count(**kw) != 0, kw
        assert b"cloudaae_tsdf_count" in L.cloudaae_last_error(), kw

    def emit(nx=2, ny=2, nz=2, voxel=1.0, state=p, min_count=1, offset=p, total=1, pos=p, key=p):
        return L.cloudaae_tsdf_emit(nx, ny, nz, 0.0, 0.0, 0.0, voxel, state, min_count, offset, total, pos, key, hip.stream())
    for kw in (dict(ny=1), dict(voxel=0.0), dict(voxel=nan), dict(state=None), dict(offset=None), dict(pos=None), dict(key=None),
               dict(min_count=0), dict(total=-1), dict(total=13)):
        assert emit(**kw) != 0, kw
        assert b"cloudaae_tsdf_emit" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0


def test_python_refuses_what_the_entry_points_refuse(fuse, dev, hip):
    fr = FR.small_frames()
    with pytest.raises(ValueError):
        fuse.Volume([0.0, 0.0, 0.0], 0.01, (1, 4, 4), dev)
    with pytest.raises(ValueError):
        fuse.Volume([0.0, 0.0, 0.0], 0.0, (4, 4, 4), dev)
    vol = fuse.Volume([0.0, 0.0, 0.0], 0.01, (4, 4, 4), dev)
    for kw in (dict(front=0.01, behind=0.01), dict(front=float('nan')), dict(behind=0.0), dict(z_near=0.0)):
        with pytest.raises(hip.HipLibraryError):
            fuse.integrate(vol, fr['depth'], fr['intr'], fr['poses'], **kw)
    with pytest.raises(ValueError):
        fuse.integrate(vol, fr['depth'], fr['intr'], fr['poses'], label=fr['label'])          # a label without want
    with pytest.raises(ValueError):
        fuse.integrate(vol, fr['depth'], fr['intr'][:3], fr['poses'])
    with pytest.raises(ValueError):
        fuse.extract_mesh(vol, min_count=0)
    torch.cuda.synchronize()
    assert int(vol.state.abs().sum()) == 0
