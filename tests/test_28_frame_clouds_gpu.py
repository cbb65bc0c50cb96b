"""GPU: cloudaae_frame_clouds (csrc/frame_clouds.hip), cloudaae_rendered_scene (csrc/pose_sample.hip) and
utils/rendered_data.rendered_element against the NumPy restatement of DESIGN.md "Rendered training clouds"
(tests/frame_clouds_reference.py).  Clouds, counts and sources are compared for equality, every byte of them; the outputs
of the raw calls sit between guard bytes that must survive.  Two floating comparisons are not bitwise, for a stated
reason: the occluder's centre against the NumPy restatement goes through logf / cosf / sinf of the device, which NumPy's
differ from in the last place (the tolerance is pose_sampling_reference.float_tolerances', as in test_21); against the
device's own cloudaae_random_object_occluder the centre IS compared for equality.

Shapes: frames of 37 x 53 = 1961 pixels (no multiple of 64, 256 or the 1024-pixel tile: two tiles, the second partial),
F = 3, rows in {1, 5, 64, 300}; 48 x 64 frames for the rendered chain."""

import numpy as np
import pytest
import torch

import frame_clouds_reference as R
import mesh_models_reference as M
import pose_sampling_reference as P

pytestmark = pytest.mark.gpu

H, W, F = 37, 53, 3
HW = H * W
SEED = 20240607
ROWS = (1, 5, 64, 300)
# frame 1: label value -> number of masked pixels, scattered over the whole frame by a seeded shuffle (every label also
# owns three pixels without depth, which are not in its mask)
PALETTE = {10: 1, 11: 2, 12: 4, 13: 5, 14: 6, 15: 63, 16: 64, 17: 65, 18: 299, 19: 300, 20: 301}
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _frames():
    rng = np.random.default_rng(11)
    depth = rng.integers(1, 65536, (F, HW)).astype(np.uint16)
    label = np.zeros((F, HW), np.uint8)
    # frame 0: two labels in overlapping boxes with holes inside them, a mask wholly inside the last partial pass of the
    # last tile (pixels 1800 ..), one across the tile edge at 1024 and one across a wave and a pass edge (250 .. 262)
    lab0 = label[0].reshape(H, W)
    lab0[5:31, 4:41] = 1
    lab0[0:21, 30:53] = 2
    depth[0][rng.random(HW) < 0.1] = 0
    label[0][1800:1961] = 7
    label[0][1000:1051] = 8
    label[0][250:263] = 9
    # frame 1: the palette
    assign = np.concatenate([np.full(n + 3, lab, np.uint8) for lab, n in PALETTE.items()])
    assign = np.concatenate([assign, np.zeros(HW - len(assign), np.uint8)])
    holes = np.concatenate([np.r_[np.zeros(n, bool), np.ones(3, bool)] for n in PALETTE.values()])
    holes = np.concatenate([holes, np.zeros(HW - len(holes), bool)])
    perm = rng.permutation(HW)
    label[1][perm] = assign
    depth[1][perm[holes]] = 0
    # frame 2: one label everywhere, depth everywhere: n = H W
    label[2][:] = 1
    intr = np.array([[60.0, 61.5, 25.75, 18.25, 10000.0], [55.5, 54.0, 27.0, 17.5, 5000.0], [70.0, 70.0, 26.5, 18.5, 1000.0]],
                    np.float32)
    return depth.reshape(F, H, W), label.reshape(F, H, W), intr


def _clouds():
    """(frame_of, want, index): every n case for every rows of ROWS, different labels of one frame, frames out of range."""
    rows = [(0, 1, 3), (0, 2, (1 << 39) - 1), (0, 7, 1 << 33), (0, 8, 0), (0, 9, 12), (0, 99, 4)]
    rows += [(1, lab, 100 + lab) for lab in PALETTE]
    rows += [(2, 1, 77), (2, 2, 78), (-1, 1, 5), (F, 1, 6), (1, 18, 1 << 39), (1, 18, -1)]
    a = np.array(rows, np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].copy()


@pytest.fixture(scope="module")
def frames(dev):
    depth, label, intr = _frames()
    assert (label[1] == 18).sum() == 302 and ((label[1] == 18) & (depth[1] != 0)).sum() == 299
    return dict(depth=depth, label=label, intr=intr, d=torch.from_numpy(depth.view(np.int16)).to(dev),
                l=torch.from_numpy(label).to(dev), k=torch.from_numpy(intr).to(dev))


@pytest.fixture(scope="module")
def reference(frames):
    """rows -> the restatement of the whole cloud list, computed once and left unchanged."""
    fo, want, index = _clouds()
    fb = np.arange(3 * len(fo), dtype=np.float32).reshape(-1, 3) + np.float32(0.5)
    out = {r: R.frame_clouds(frames['depth'], frames['label'], frames['intr'], fo, want, index, r, SEED, fb) for r in ROWS}
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out, fb


class Guarded(object):
    """A device buffer of `nbytes` between two guard zones, everything filled with FILL."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)

    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def body(self, dtype, shape):
        return self.raw[GUARD:GUARD + self.n].cpu().numpy().view(dtype).reshape(shape)

    def guards_intact(self):
        g = self.raw.cpu().numpy()
        return bool((g[:GUARD] == FILL).all() and (g[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.raw.cpu().numpy() == FILL).all())


def _raw(hip, dev, fr, fo, want, index, rows, seed, fallback, f=F, h=H, w=W, c=None, null_output=False):
    """The C entry point on guarded outputs.  -> (rc, dict of numpy outputs, the Guarded buffers)."""
    L = hip.lib()
    C = len(fo) if c is None else c
    n = max(len(fo), 1)
    t_fo = torch.from_numpy(np.asarray(fo, np.int32)).to(dev)
    t_want = torch.from_numpy(np.asarray(want, np.int32)).to(dev)
    t_index = torch.from_numpy(np.asarray(index, np.int64)).to(dev)
    t_fb = torch.from_numpy(np.asarray(fallback, np.float32)).to(dev) if fallback is not None else None
    r = max(min(int(rows), 1 << 12), 1)              # (buffers of a refused call need not fit its rows)
    bufs = dict(cloud=Guarded(n * r * 12, dev), num_pixels=Guarded(n * 4, dev), num_distinct=Guarded(n * 8, dev),
                row_src=Guarded(n * r * 4, dev))
    nbytes = int(L.cloudaae_frame_clouds_workspace_bytes(f, h, w, C, rows))
    ws = Guarded(max(nbytes, 256), dev)
    rc = L.cloudaae_frame_clouds(f, h, w, fr['d'].data_ptr(), fr['l'].data_ptr(), fr['k'].data_ptr(), C, t_fo.data_ptr(),
                                 t_want.data_ptr(), t_index.data_ptr(), t_fb.data_ptr() if t_fb is not None else None,
                                 rows, seed, bufs['cloud'].ptr(), bufs['num_pixels'].ptr(),
                                 None if null_output else bufs['num_distinct'].ptr(), bufs['row_src'].ptr(), ws.ptr(),
                                 max(nbytes, 256), hip.stream())
    torch.cuda.synchronize()
    bufs['workspace'] = ws
    if rc != 0:
        return rc, None, bufs
    out = dict(cloud=bufs['cloud'].body(np.float32, (n, r, 3)), num_pixels=bufs['num_pixels'].body(np.int32, (n,)),
               num_distinct=bufs['num_distinct'].body(np.int64, (n,)), row_src=bufs['row_src'].body(np.int32, (n, r)))
    return rc, out, bufs


def _same(got, want, where=""):
    for k in ("num_pixels", "num_distinct", "row_src"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert got['cloud'].tobytes() == want['cloud'].tobytes(), (where, "cloud")


@pytest.mark.parametrize("rows", ROWS)
def test_clouds_equal_the_restatement(hip, dev, frames, reference, rows):
    ref, fb = reference
    fo, want, index = _clouds()
    rc, got, bufs = _raw(hip, dev, frames, fo, want, index, rows, SEED, fb)
    assert rc == 0
    n = ref[rows]['num_pixels']
    print("rows %d: n = %s" % (rows, n.tolist()))
    # the cases are all there: n = 0, 1, < rows, = rows, rows + 1, >> rows, H W; the last partial pass; the tile edge
    assert {0, 1, HW, rows - 1, rows, rows + 1} <= set(n.tolist())
    assert np.isfinite(got['cloud']).all()
    _same(got, ref[rows], "rows %d" % rows)
    assert all(b.guards_intact() for b in bufs.values())
    # clouds out of range: the fallback and nothing else
    for c in np.flatnonzero((fo < 0) | (fo >= F) | (index < 0) | (index >= (1 << 39))):
        assert got['num_pixels'][c] == 0 and got['num_distinct'][c] == 1 and not got['row_src'][c].any()
        assert np.array_equal(got['cloud'][c], np.tile(fb[c], (rows, 1)))


def test_without_a_fallback_empty_clouds_are_zeros(hip, dev, frames):
    rc, got, bufs = _raw(hip, dev, frames, [0, 5, 1], [99, 1, 10], [1, 2, 3], 5, SEED, None)
    assert rc == 0 and got['num_pixels'].tolist() == [0, 0, 1]
    assert not got['cloud'][:2].any() and got['cloud'][2].any()
    assert np.array_equal(got['cloud'][2], np.tile(got['cloud'][2, 0], (5, 1))) and not got['row_src'][2].any()
    assert all(b.guards_intact() for b in bufs.values())


def test_a_cloud_does_not_depend_on_the_batch_or_the_run(hip, dev, frames, reference):
    from cloudaae_amd.utils import rendered_data
    ref, fb = reference
    fo, want, index = _clouds()
    rows = 64
    for c in (1, 8, 11, 17):                        # n >> rows, n = 4 and n = 63 < rows, n = H W
        alone = rendered_data.frame_clouds(frames['d'], frames['l'], frames['k'], fo[c:c + 1], want[c:c + 1], index[c:c + 1],
                                           rows, SEED, fallback=fb[c:c + 1])
        # the same cloud at position 4 of six, reading a frame that sits elsewhere in a longer batch
        d2 = torch.cat([frames['d'][2:3], frames['d']], dim=0)
        l2 = torch.cat([frames['l'][2:3], frames['l']], dim=0)
        k2 = torch.cat([frames['k'][2:3], frames['k']], dim=0)
        fo6 = np.array([1, 0, 3, 2, fo[c] + 1, 9], np.int32)
        want6 = np.array([1, 2, 1, 11, want[c], 1], np.int32)
        index6 = np.array([9, 8, 7, 6, index[c], 5], np.int64)
        fb6 = np.concatenate([fb[:4], fb[c:c + 1], fb[:1]])
        six = rendered_data.frame_clouds(d2, l2, k2, fo6, want6, index6, rows, SEED, fallback=fb6)
        again = rendered_data.frame_clouds(d2, l2, k2, fo6, want6, index6, rows, SEED, fallback=fb6)
        for k in ("cloud", "num_pixels", "num_distinct", "row_src"):
            assert torch.equal(alone[k][0], six[k][4]), (c, k)
            assert six[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (c, k)
            assert np.array_equal(alone[k][0].cpu().numpy(), ref[rows][k][c]), (c, k)


def test_limits_are_refused_and_nothing_is_written(hip, dev, frames):
    L = hip.lib()
    fo, want, index = [0, 1], [1, 10], [1, 2]
    cases = [dict(rows=0), dict(rows=(1 << 20) + 1), dict(h=1 << 13, w=(1 << 11) + 1), dict(f=(1 << 28) // HW + 1), dict(c=0),
             dict(f=0), dict(null_output=True)]
    for kw in cases:
        q = dict(f=F, h=H, w=W, c=2, rows=5)
        q.update({k: v for k, v in kw.items() if k != 'null_output'})
        if 'null_output' not in kw:
            assert int(L.cloudaae_frame_clouds_workspace_bytes(q['f'], q['h'], q['w'], q['c'], q['rows'])) == 0, kw
        args = dict(rows=5)
        args.update(kw)
        rows = args.pop('rows')
        rc, got, bufs = _raw(hip, dev, frames, fo, want, index, rows, SEED, None, **args)
        assert rc != 0 and got is None, kw
        msg = L.cloudaae_last_error().decode()
        assert msg.startswith("cloudaae_frame_clouds:"), (kw, msg)
        assert all(b.untouched() for b in bufs.values()), kw
    assert int(L.cloudaae_frame_clouds_workspace_bytes(F, H, W, 2, 5)) >= 2 * 2 * 4
    from cloudaae_amd.utils import rendered_data
    with pytest.raises(ValueError):
        rendered_data.frame_clouds(frames['d'], frames['l'], frames['k'], fo, want, index, 0, SEED)


# ---- scene assembly --------------------------------------------------------------------------------------------------------
def _meshes():
    """Three small meshes of different sizes, in metres: a tetrahedron (4 vertices, 4 triangles), a box (8, 12) and an
    icosphere (42, 80)."""
    tv = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * np.float32(0.04)
    tt = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    cv, ct, _ = M.cube()
    bv = (cv - np.float32(0.5)) * np.array([0.10, 0.14, 0.08], np.float32)
    iv, it = M.icosphere(1)
    return [(tv, tt), (bv.astype(np.float32), ct), ((np.asarray(iv) * 0.05).astype(np.float32), np.asarray(it, np.int32))]


CAMERA = dict(fx=106.6778, fy=106.7487, cx=31.29869, cy=24.13109, width=64., height=48.)      # the ycbv view at 48 x 64


@pytest.fixture(scope="module")
def packed(dev):
    from cloudaae_amd.utils import mesh_models
    return mesh_models.pack_meshes(_meshes(), device=dev)


def _np(t):
    return t.detach().cpu().numpy()


def test_scene_equals_the_occluder_entry_and_the_restatement(hip, dev, packed):
    from cloudaae_amd.utils import generate_occluder, rendered_data, sample_pose_in_frustum as spf
    B, seed, first = 3, 99, 1000
    rec = spf.sample_poses(B, seed, first, num_models=3, device=dev)
    mesh_index = [2, 0, 1]
    scene = rendered_data.rendered_scene(rec, packed, mesh_index, seed, first, return_centre=True)
    # the class and the centre of the existing entry: a model of zeros makes its points the centre itself
    x = dict(obj_model=torch.zeros((3, 4, 6), device=dev), translation=rec['translation'], rot_mat64=rec['rot_mat64'])
    x = generate_occluder.get_random_object_occluder(x, 3, seed=seed, first_index=first, per=1)
    assert torch.equal(scene['occluder_class'], x['occluder_class'])
    assert torch.equal(scene['occluder_centre'], x['occluder'][:, 0, :])
    want = R.rendered_scene(_np(rec['class_id']), mesh_index, _np(rec['rot_mat64']), _np(rec['translation']), seed, first,
                            42, 80, [0, 1, 2])
    for k in ("inst_offsets", "inst_mesh", "inst_label", "vert_base", "tri_base", "occluder_class"):
        assert np.array_equal(_np(scene[k]), want[k]), k
    tol = P.float_tolerances(seed, 4096, 'ycbv', np.zeros((3, 512, 6), np.float32), [0, 1, 2])['occluder']
    err = np.abs(_np(scene['occluder_centre']).astype(np.float64) - want['occluder_centre']).max()
    print("centre against the NumPy restatement: off by %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol
    pose, wpose = _np(scene['inst_pose']).reshape(-1, 4, 4), want['inst_pose'].reshape(-1, 4, 4)
    own = wpose.copy()
    own[2::3, :3, 3] = _np(scene['occluder_centre']).astype(np.float64)
    assert np.array_equal(pose, own)               # everything but the centre's last place is exact


def test_strided_render_equals_the_restatement(hip, dev, packed):
    from cloudaae_amd.utils import render, rendered_data, sample_pose_in_frustum as spf
    B, seed, first = 3, 5, 40
    rec = spf.sample_poses(B, seed, first, num_models=3, camera=CAMERA, device=dev)
    rec['class_id'] = torch.tensor([2, 0, 1], device=dev)
    scene = rendered_data.rendered_scene(rec, packed, None, seed, first, camera=CAMERA)
    intr = rendered_data.frame_intrinsics(2 * B, 48, 64, device=dev)
    depth, label, tri, counts = render.render_instances_strided(packed, intr, scene['inst_offsets'], scene['inst_mesh'],
                                                                scene['inst_label'], scene['inst_pose'], scene['vert_base'],
                                                                scene['tri_base'], 48, 64, return_tri=True)
    host = {k: _np(v) for k, v in scene.items()}
    want = R.render_strided(_meshes(), host, _np(intr), 48, 64)
    got_d = _np(depth).view(np.uint16)
    print("pixels drawn per frame:", (got_d != 0).reshape(2 * B, -1).sum(1).tolist())
    assert (got_d != 0).any()
    assert np.array_equal(got_d, want['depth']) and np.array_equal(_np(label), want['label'])
    assert np.array_equal(_np(tri), want['tri'])


# ---- the chain -------------------------------------------------------------------------------------------------------------
def _expected_element(el, B, N, seed, g0, min_visible):
    fr = el['frames']
    i = np.arange(B)
    t = _np(el['translation'])
    seen = R.frame_clouds(_np(fr['depth']), _np(fr['label']), _np(fr['intrinsics']), np.r_[2 * i + 1, 2 * i], np.ones(2 * B),
                          np.r_[4 * (g0 + i) + 1, 4 * (g0 + i)], N, seed, np.r_[t, t])
    org = R.frame_clouds(_np(fr['clean_depth']), _np(fr['clean_label']), _np(fr['intrinsics']), 2 * i, np.ones(B),
                         4 * (g0 + i) + 2, 4 * N, seed, t)
    n_occ, n_alone = seen['num_pixels'][:B], seen['num_pixels'][B:]
    out = n_occ < min_visible
    return dict(visiblePoints=np.where(out[:, None, None], seen['cloud'][B:], seen['cloud'][:B]),
                visiblePoints_org=org['cloud'], num_vis_point_org=org['num_distinct'], visiblePoints_org_src=org['row_src'],
                num_vis_point=np.where(out, n_alone, n_occ), occluded_out=out)


def _check_element(el, B, N, seed, g0, min_visible):
    want = _expected_element(el, B, N, seed, g0, min_visible)
    for k, w in want.items():
        assert _np(el[k]).tobytes() == w.astype(_np(el[k]).dtype).tobytes(), k
    assert tuple(el['visiblePoints'].shape) == (B, N, 3) and tuple(el['visiblePoints_org'].shape) == (B, 4 * N, 3)
    assert torch.isfinite(el['visiblePoints']).all() and torch.isfinite(el['visiblePoints_org']).all()
    return want


@pytest.mark.parametrize("sensor", [None, 'kinect1'])
def test_rendered_element_equals_the_restatement_on_its_own_frames(hip, dev, packed, sensor):
    from cloudaae_amd.utils import rendered_data, sample_pose_in_frustum as spf
    B, N, seed, g0 = 4, 32, 31, 200
    kw = dict(camera=CAMERA, height=48, width=64, sensor=sensor, sensor_seed=8, min_visible=16)
    rec = spf.sample_poses(B, seed, g0, num_models=3, camera=CAMERA, device=dev)
    el = rendered_data.rendered_element(rec, packed, None, N, seed, g0, return_frames=True, **kw)
    want = _check_element(el, B, N, seed, g0, 16)
    fr = el['frames']
    print("sensor %s: target pixels occluded %s, alone %s; clean alone %s" %
          (sensor, _np(el['num_pixels_occluded']).tolist(), _np(el['num_pixels_alone']).tolist(),
           _np(el['num_pixels_org']).tolist()))
    assert _np(el['num_pixels_org']).max() > 0, "nothing was rendered"
    if sensor is None:
        assert fr['depth'] is fr['clean_depth']
    else:
        assert not torch.equal(fr['depth'], fr['clean_depth'])
    # the keys describe the target: rows below the count distinct, the others copies of their source
    org, src, cnt = want['visiblePoints_org'], want['visiblePoints_org_src'], want['num_vis_point_org']
    for b in range(B):
        assert np.array_equal(org[b], org[b][src[b]]) and src[b].max() < cnt[b]
    # the same samples as 2 + 2: identical clouds
    for lo in (0, 2):
        part = rendered_data.rendered_element(spf.sample_poses(2, seed, g0 + lo, num_models=3, camera=CAMERA, device=dev),
                                              packed, None, N, seed, g0 + lo, **kw)
        for k in ("visiblePoints", "visiblePoints_org", "num_vis_point_org", "visiblePoints_org_src", "num_vis_point",
                  "occluded_out", "occluder_class", "class_id"):
            assert torch.equal(part[k], el[k][lo:lo + 2]), (lo, k)


def test_an_occluder_in_front_switches_to_the_alone_view(hip, dev, packed):
    from cloudaae_amd.utils import rendered_data, sample_pose_in_frustum as spf
    B, N, seed, g0 = 2, 32, 31, 500
    rec = spf.sample_poses(B, seed, g0, num_models=3, camera=CAMERA, device=dev)
    # both targets in the middle of the view at 0.6 m; sample 1 is the ball
    rec['translation'] = torch.tensor([[0.0, 0.0, 0.6], [0.0, 0.0, 0.6]], device=dev)
    rec['class_id'] = torch.tensor([1, 2], device=dev)
    scene = rendered_data.rendered_scene(rec, packed, None, seed, g0, camera=CAMERA)
    pose = scene['inst_pose'].view(-1, 4, 4)
    pose[2, :3, 3] = torch.tensor([10.0, 0.0, 0.6], dtype=torch.float64, device=dev)      # sample 0: out of the view
    pose[5, :3, 3] = torch.tensor([0.0, 0.0, 0.3], dtype=torch.float64, device=dev)       # sample 1: right in front
    scene['inst_mesh'][5] = 1                                                            # ... and it is the box
    el = rendered_data.rendered_element(rec, packed, None, N, seed, g0, camera=CAMERA, height=48, width=64,
                                        sensor='kinect1', min_visible=16, scene=scene, return_frames=True)
    _check_element(el, B, N, seed, g0, 16)
    n_occ, n_alone = _np(el['num_pixels_occluded']), _np(el['num_pixels_alone'])
    print("occluded %s alone %s" % (n_occ.tolist(), n_alone.tolist()))
    assert _np(el['occluded_out']).tolist() == [False, True]
    assert n_occ[1] < 16 <= n_alone[1] and n_occ[0] >= 16
    assert torch.equal(el['visiblePoints'][1], el['input_clouds']['cloud'][B + 1])
    assert torch.equal(el['visiblePoints'][0], el['input_clouds']['cloud'][0])
    assert _np(el['num_vis_point']).tolist() == [int(n_occ[0]), int(n_alone[1])]
