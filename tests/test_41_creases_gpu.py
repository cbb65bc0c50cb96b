"""GPU: cloudaae_depth_creases through the C ABI against the NumPy restatement of DESIGN.md "Creases"
(tests/creases_reference.py), then utils/depth_components.py (find_creases, segment_depth(creases=...)) and a detection
across two touching objects through utils/detect.py.

Every output is an integer and is compared for equality, no entry left out: smooth_map, crease, tested, fg_cut and
n_crease.  tests/test_creases_host.py anchors the restatement and states the coverage of the random cases.  Outputs sit
between guard rows filled with a byte pattern (as in tests/test_37_depth_components_gpu.py), so every call starts on
garbage and a write past an image shows."""
import numpy as np
import pytest
import torch

import creases_reference as C
import depth_components_reference as D
import detect_reference as DR

pytestmark = pytest.mark.gpu

GUARD = 4
FILL = 0xA5
IMAGES = ("smooth_map", "crease", "tested", "fg_cut")
ASSIGN_INT = ("pair_hyp", "pair_num", "pair_den", "det_class", "det_hyp", "det_num", "det_den", "det_rank", "alt_class",
              "alt_num", "alt_den", "n_det")                   # what cloudaae_detect_assign writes
ASSIGN_F64 = ("pair_score", "det_score", "det_pose")


class Guarded(object):
    def __init__(self, rows, cols, dtype, dev):
        item = torch.empty((), dtype=dtype).element_size()
        self.rb = cols * item
        self.full = torch.full(((rows + 2 * GUARD) * self.rb,), FILL, dtype=torch.uint8, device=dev)
        self.view = self.full[GUARD * self.rb:(GUARD + rows) * self.rb].view(dtype).view(rows, cols)
        self.rows = rows

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        full = self.full.cpu().numpy()
        edge = GUARD * self.rb
        assert np.all(full[:edge] == FILL) and np.all(full[edge + self.rows * self.rb:] == FILL), "guard rows were written"
        return self.view.cpu().numpy()

    def untouched(self):
        return bool((self.full == FILL).all())


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _d(a, ty, dev):
    return torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)


def _depth(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(dev)


def run_creases(hip, dev, depth, fg, intr, jump_units, step, smooth, cos2):
    """The call on guarded outputs and a guarded workspace -> the restatement's dict."""
    F, H, W = depth.shape
    L = hip.lib()
    g = [_depth(depth, dev), _d(fg, np.uint8, dev), _d(intr, np.float32, dev), _d(jump_units, np.int32, dev)]
    out = {k: Guarded(F * H, W, torch.uint8, dev) for k in IMAGES[1:]}
    n_crease = Guarded(F, 1, torch.int32, dev)
    nbytes = int(L.cloudaae_depth_creases_workspace_bytes(F, H, W))
    assert nbytes >= 4 * F * H * W and nbytes % 4 == 0
    ws = Guarded(1, nbytes // 4, torch.int32, dev)
    hip.check(L.cloudaae_depth_creases(F, H, W, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), step, smooth,
                                       float(cos2), out["crease"].ptr(), out["tested"].ptr(), out["fg_cut"].ptr(), n_crease.ptr(),
                                       ws.ptr(), nbytes, hip.stream()), "cloudaae_depth_creases")
    torch.cuda.synchronize()
    r = {k: v.numpy().reshape(F, H, W).copy() for k, v in out.items()}
    r["smooth_map"] = ws.numpy().ravel()[:F * H * W].view(np.uint32).reshape(F, H, W).copy()     # the documented first words
    r["n_crease"] = n_crease.numpy().ravel().copy()
    return r


def assert_equal(got, want, what):
    for k in IMAGES + ("n_crease",):
        print("%s: %s differs in %d of %d entries" % (what, k, int((got[k] != want[k]).sum()), want[k].size))
    for k in IMAGES + ("n_crease",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


# ---- the call against the restatement: shapes, parameters at their ends, cos2 at its ends, the packing's bound ---------------
@pytest.mark.parametrize("name", [c[0] for c in C.CASES])
def test_creases_equal_the_restatement(hip, dev, name):
    c, want = C.case_inputs(name), C.case_result(name)
    got = run_creases(hip, dev, c['depth'], c['fg'], c['intr'], c['jump_units'], c['step'], c['smooth'], c['cos2'])
    print("%s: step %d smooth %d cos2 %r: tested pixels %d, crease pixels %s" % (
        name, c['step'], c['smooth'], c['cos2'], int((want['tested'] != 0).sum()), want['n_crease'].tolist()))
    assert_equal(got, want, name)
    again = run_creases(hip, dev, c['depth'], c['fg'], c['intr'], c['jump_units'], c['step'], c['smooth'], c['cos2'])
    for k in IMAGES + ("n_crease",):
        assert np.array_equal(again[k], got[k]), k                  # n_crease is zeroed by the call, not added to


def test_a_frame_does_not_depend_on_its_batch(hip, dev):
    name = "40x72x3"
    c, want = C.case_inputs(name), C.case_result(name)
    for f in (2, 0):
        alone = run_creases(hip, dev, c['depth'][f:f + 1], c['fg'][f:f + 1], c['intr'][f:f + 1], c['jump_units'][f:f + 1], c['step'],
                            c['smooth'], c['cos2'])
        for k in IMAGES + ("n_crease",):
            assert np.array_equal(alone[k][0], want[k][f]), (f, k)
    assert want['n_crease'][2] > 0 and want['n_crease'][0] == 0


def test_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    F, H, W = 1, 33, 40
    c = C.case_inputs("65535")
    g = [_depth(c['depth'], dev), _d(c['fg'], np.uint8, dev), _d(c['intr'], np.float32, dev), _d(c['jump_units'], np.int32, dev)]
    out = [Guarded(F * H, W, torch.uint8, dev) for _ in range(3)]
    n_crease = Guarded(F, 1, torch.int32, dev)
    nbytes = int(L.cloudaae_depth_creases_workspace_bytes(F, H, W))
    ws = Guarded(1, nbytes // 4, torch.int32, dev)

    def call(f=F, h=H, w=W, step=3, smooth=1, cos2=0.75, first=g[0].data_ptr(), fg=g[1].data_ptr(), k=g[2].data_ptr(),
             ju=g[3].data_ptr(), crease=out[0].ptr(), tested=out[1].ptr(), cut=out[2].ptr(), n=n_crease.ptr(), space=ws.ptr(),
             size=nbytes):
        return L.cloudaae_depth_creases(f, h, w, first, fg, k, ju, step, smooth, cos2, crease, tested, cut, n, space, size,
                                        hip.stream())
    assert call(step=0) != 0
    assert b"cloudaae_depth_creases" in L.cloudaae_last_error()
    assert call(step=9) != 0 and call(smooth=-1) != 0 and call(smooth=8) != 0
    assert call(cos2=-1e-9) != 0 and call(cos2=1.0 + 1e-9) != 0 and call(cos2=float("nan")) != 0 and call(cos2=float("inf")) != 0
    assert call(first=None) != 0 and call(fg=None) != 0 and call(k=None) != 0 and call(ju=None) != 0 and call(crease=None) != 0
    assert call(tested=None) != 0 and call(cut=None) != 0 and call(n=None) != 0 and call(space=None) != 0
    assert call(size=nbytes - 1) != 0 and call(size=0) != 0
    assert call(h=0) != 0 and call(w=0) != 0 and call(f=-1) != 0 and call(h=4097, w=4096) != 0 and call(f=1 << 16, h=4096, w=4096) != 0
    assert L.cloudaae_depth_creases_workspace_bytes(1, 4097, 4096) == 0 and L.cloudaae_depth_creases_workspace_bytes(-1, 4, 4) == 0
    assert call(f=0) == 0                                            # no frame: a defined no-op
    assert call(f=0, first=None, space=None, size=0) == 0
    torch.cuda.synchronize()
    for buf in out + [n_crease, ws]:
        assert buf.untouched()
    assert call(step=8, smooth=7, cos2=0.0) == 0 and call(cos2=1.0) == 0
    torch.cuda.synchronize()
    assert not any(buf.untouched() for buf in out + [n_crease, ws])
    for buf in out + [n_crease, ws]:
        buf.numpy()                                                  # the guards


# ---- find_creases and segment_depth(creases=...) ----------------------------------------------------------------------------------
def test_find_creases_returns_the_five_tensors(hip, dev):
    from cloudaae_amd.utils import depth_components as dc
    name = "40x72x3"
    c = C.case_inputs(name)
    want = C.creases_batch(c['depth'], c['fg'], c['intr'], c['jump_units'], dc.STEP, dc.SMOOTH, C.cos2_of(dc.ANGLE))
    assert (dc.STEP, dc.SMOOTH, dc.ANGLE) == (C.DEFAULTS['step'], C.DEFAULTS['smooth'], C.DEFAULTS['angle'])
    r = dc.find_creases(c['depth'], _d(c['fg'], np.uint8, dev), c['intr'], c['jump_units'])
    got = {k: r[k].cpu().numpy() for k in IMAGES + ("n_crease",)}
    got['smooth_map'] = got['smooth_map'].view(np.uint32)
    assert_equal(got, want, "find_creases")
    other = dc.find_creases(_depth(c['depth'], dev), _d(c['fg'], np.uint8, dev), _d(c['intr'], np.float32, dev),
                            _d(c['jump_units'], np.int32, dev), step=2, smooth=0, angle=45.0)
    want = C.creases_batch(c['depth'], c['fg'], c['intr'], c['jump_units'], 2, 0, C.cos2_of(45.0))
    assert np.array_equal(other['crease'].cpu().numpy(), want['crease']) and other['n_crease'].tolist() == want['n_crease'].tolist()
    for bad in (dict(step=0), dict(step=9), dict(smooth=8), dict(smooth=-1)):
        with pytest.raises(ValueError):
            dc.find_creases(c['depth'], _d(c['fg'], np.uint8, dev), c['intr'], c['jump_units'], **bad)


def _assert_segments(seg, ref, f=0):
    for k in ("label", "root", "fg"):
        assert np.array_equal(getattr(seg, k)[f].cpu().numpy(), ref[k]), k
    assert seg.n_components[f] == ref['n_components'] and seg.n_candidates[f] == ref['n_candidates']
    for k in ("comp_root", "comp_size", "comp_box"):
        assert np.array_equal(getattr(seg, k)[f], ref[k]), k


@pytest.mark.parametrize("scene", ["clean", "noisy"])
def test_segment_depth_cuts_the_touching_spheres_apart(hip, dev, scene):
    from cloudaae_amd.utils import depth_components as dc
    if scene == "clean":
        (depth, label), intr, cut, min_pixels = C.sphere_scene(C.TOUCHING_SPHERES, D.SCENE_INTR, D.SCENE_H, D.SCENE_W), D.SCENE_INTR, \
            C.CLEAN_CUT, 16
        key = 'touch'
    else:
        (depth, _), (_, label), intr, cut, min_pixels = C.big_scene(noise=True), C.big_scene(noise=False), C.BIG_INTR, C.NOISY_CUT, \
            C.BIG_MIN_PIXELS
        key = 'bignoisy'
    kw = dict(jump=D.SCENE_JUMP_UNITS / float(intr[0, 4]), min_pixels=min_pixels, max_components=32, device=dev, **D.SCENE_PARAMS)
    plain_ref, cut_ref = C.scene_segments(depth, intr, None, min_pixels, key), C.scene_segments(depth, intr, cut, min_pixels, key)
    plain = dc.segment_depth(depth, intr, **kw)
    assert plain.jump_units.tolist() == [D.SCENE_JUMP_UNITS]
    _assert_segments(plain, plain_ref)
    assert plain.n_components.tolist() == [2] and not hasattr(plain, "crease") and not hasattr(plain, "n_crease")
    got = dc.segment_depth(depth, intr, creases=cut, **kw)
    _assert_segments(got, cut_ref)
    for k in ("crease", "fg_cut"):
        assert np.array_equal(getattr(got, k)[0].cpu().numpy(), cut_ref[k]), k
    assert got.n_crease.dtype == np.int32 and got.n_crease.tolist() == [cut_ref['n_crease']]
    sh = C.shares(dict(label=got.label[0].cpu().numpy(), n_components=got.n_components[0]), label[0])
    print("%s: crease pixels %d, components %s, pixels on (table, sphere 1, 2, 3) %s" % (scene, got.n_crease[0],
                                                                                       got.comp_size[0, :4].tolist(), sh.tolist()))
    assert got.n_components.tolist() == [3] and [int(np.argmax(row[1:])) for row in sh] == [0, 1, 2]
    assert torch.equal(got.fg, plain.fg) and torch.equal(got.plane, plain.plane)
    # creases=True is the defaults; what is given is kept beside them
    if cut == C.NOISY_CUT:
        same = dc.segment_depth(depth, intr, creases=True, **kw)
        assert torch.equal(same.label, got.label) and torch.equal(same.crease, got.crease)
        part = dc.segment_depth(depth, intr, creases=dict(angle=30.0), **kw)
        assert torch.equal(part.label, got.label)


# ---- a detection across a touch ---------------------------------------------------------------------------------------------------
def test_touching_spheres_are_detected_one_by_one(hip, dev):
    from cloudaae_amd.utils import depth_components as dc
    from cloudaae_amd.utils import detect
    from cloudaae_amd.utils import mesh_models as mm
    packed = mm.pack_meshes([m[:2] for m in C.detect_meshes()], device=dev)
    for cut, n_det in ((None, 2), (C.CLEAN_CUT, 3)):
        s, cpu = C.detect_scene(cut), C.detect_score(cut)
        seg = dc.segment_depth(s['depth'], s['intr'], device=dev, creases=cut, **C.DETECT_SEGMENT)
        assert np.array_equal(seg.label[0].cpu().numpy(), s['seg']['label']) and seg.n_components.tolist() == [n_det]
        poses = s['poses']
        F, K, Cn, P = poses.shape[:4]
        got = detect.score_candidates(seg, _d(poses, np.float64, dev), None, packed, [0, 1, 2], s['intr'], _depth(s['depth'], dev),
                                      keep_depth=True)
        dh = got['depth_hyp'].cpu().numpy().view(np.uint16)
        print("creases %s: rendered windows differ from the NumPy renderer's in %d pixels" % (cut, int((dh != cpu['depth_hyp']).sum())))
        ref = DR.score(s['seg']['label'][None], s['seg']['comp_box'][None], np.array([n_det], np.int32), poses, None, None, None,
                       s['intr'], s['depth'], depth_hyp=dh)
        for k in ('counts', 'seg_total', 'abs_sum'):
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
        for k in ASSIGN_INT:
            assert np.array_equal(got[k].cpu().numpy().reshape(ref[k].shape), ref[k]), k
        for k in ASSIGN_F64:
            assert np.array_equal(got[k].cpu().numpy().reshape(ref[k].shape).view(np.uint64), ref[k].view(np.uint64)), k
        t = got['table']
        print("creases %s: det_class %s score %s" % (cut, t['det_class'].tolist(), t['det_score'].tolist()))
        assert np.array_equal(t['det_class'], cpu['det_class']) and np.array_equal(t['det_hyp'], cpu['det_hyp'])
        assert t['n_det'].tolist() == cpu['n_det'].tolist() and t['n_det'][0] <= n_det
        if cut is not None:
            assert t['n_det'].tolist() == [3] and t['det_class'][0].tolist() == s['object_of'] == [0, 1, 2]


def test_detect_objects_forwards_the_cut_to_the_segmentation(hip, dev, monkeypatch):
    from cloudaae_amd.utils import depth_components as dc
    from cloudaae_amd.utils import detect
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import ppf
    meshes = [m[:2] for m in C.detect_meshes()]
    packed = mm.pack_meshes(meshes, device=dev)
    models = ppf.PPFModels.from_meshes(meshes, num_point=96, device=dev)
    seen = []
    real = dc.segment_depth

    def spy(*args, **kw):
        seen.append(kw.get("creases"))
        return real(*args, **kw)
    monkeypatch.setattr(dc, "segment_depth", spy)
    params = {k: v for k, v in C.DETECT_SEGMENT.items() if k != 'seed'}
    for cut, n in ((None, 2), (C.CLEAN_CUT, 3)):
        s = C.detect_scene(cut)
        d = detect.detect_objects(s['depth'], s['intr'], packed, models, num_point=48, top=2, seed=C.DETECT_SEGMENT['seed'],
                                  components=dict(params, creases=cut) if cut else params)
        assert seen[-1] == cut and d.segments.n_components.tolist() == [n]
        assert np.array_equal(d.segments.label[0].cpu().numpy(), s['seg']['label'])
        assert hasattr(d.segments, "fg_cut") == (cut is not None)
        print("creases %s: det_class %s score %s of components that show %s" % (cut, d.table['det_class'].tolist(),
                                                                               d.table['det_score'].tolist(), s['object_of']))
