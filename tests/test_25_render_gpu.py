"""GPU: cloudaae_render_frames through the C ABI against the NumPy restatement of DESIGN.md "Rendered frames"
(tests/render_reference.py), then utils/render.py: a rendered sphere through the existing back-projection, and the
command line's frame records through element_from_frames, evaluate_batch and evaluate_cloudAAE_ycbv.main(--files).

Every output of the kernel is an integer (fixed-point screen coordinates, int64 edge values, a quantised depth taken
from one un-fused fp64 expression, an integer minimum), so depth, label, tri, dropped and degenerate are compared for
equality, with no tolerance and no pixel left out.  Outputs and the workspace sit between guard rows.  Poses carry a
scale (the top three rows of the 4x4 are read as they are), which is how one mesh is made to cover few or many pixels."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_models_reference as MR
import render_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "cloudaae_amd", "csrc", "render.hip")).read()
RN_SMALL = int(re.search(r"#define CLOUDAAE_RN_SMALL (\d+)", SRC).group(1))
EMPTY_MESH = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
GUARD = 4                  # rows kept before and after every output
FILL = 0xA5


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_23_mesh_models_gpu.py)."""

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


def _write_ply(path, v, t, c):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", "element face %d" % len(t),
            "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r %d %d %d" % (tuple(float(x) for x in p) + tuple(int(x) for x in q)) for p, q in zip(v, c)]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def place(scale, rotvec, trans, centre=(0.0, 0.0, 0.0)):
    """A pose that scales the mesh about `centre`, rotates it and moves it to `trans`."""
    T = R.pose_matrix(rotvec, trans)
    T[:3, :3] *= float(scale)
    T[:3, 3] -= T[:3, :3] @ np.asarray(centre, np.float64)
    return T


def launch(hip, dev, meshes, frames, intr, H, W, z_near=0.05, with_tri=True):
    """cloudaae_render_frames on guarded buffers -> dict like render_reference.render's (without box)."""
    L = hip.lib()
    vo, to, v, t, _ = MR.pack([m[:2] for m in meshes])
    offs, mesh, lab, poses, vb, tb = R.instance_bases(meshes, frames)
    F, J = len(frames), len(mesh)
    d = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)
    g = dict(vo=d(vo, np.int32), to=d(to, np.int32), v=d(v, np.float32), t=d(t, np.int32), intr=d(intr, np.float32),
             offs=d(offs, np.int32), mesh=d(mesh, np.int32), lab=d(lab, np.int32), poses=d(poses, np.float64),
             vb=d(vb, np.int32), tb=d(tb, np.int32))
    depth, label = Guarded(F * H, W, torch.int16, dev), Guarded(F * H, W, torch.uint8, dev)
    tri = Guarded(F * H, W, torch.int32, dev) if with_tri else None
    dropped, degenerate = Guarded(J, 1, torch.int32, dev), Guarded(J, 1, torch.int32, dev)
    nbytes = int(L.cloudaae_render_workspace_bytes(F, H, W, J, int(vb[-1]), int(tb[-1])))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = Guarded(nbytes // 8, 1, torch.int64, dev)
    hip.check(L.cloudaae_render_frames(len(meshes), g['vo'].data_ptr(), g['to'].data_ptr(), len(v), len(t), g['v'].data_ptr(),
                                       g['t'].data_ptr(), F, H, W, g['intr'].data_ptr(), g['offs'].data_ptr(), J,
                                       g['mesh'].data_ptr(), g['lab'].data_ptr(), g['poses'].data_ptr(), g['vb'].data_ptr(),
                                       g['tb'].data_ptr(), int(vb[-1]), int(tb[-1]), float(z_near), depth.ptr(), label.ptr(),
                                       tri.ptr() if with_tri else None, dropped.ptr(), degenerate.ptr(), ws.ptr(), nbytes,
                                       hip.stream()), "cloudaae_render_frames")
    torch.cuda.synchronize()
    ws.numpy()                                            # (the guard rows of the workspace)
    out = dict(depth=depth.numpy().view(np.uint16).reshape(F, H, W), label=label.numpy().reshape(F, H, W),
               dropped=dropped.numpy().ravel(), degenerate=degenerate.numpy().ravel(), tri_base=tb)
    if with_tri:
        out['tri'] = tri.numpy().reshape(F, H, W)
    return out


def assert_equal(got, want, what):
    for k in ('depth', 'label', 'tri', 'dropped', 'degenerate'):
        differ = int((got[k] != want[k]).sum())
        print("%s: %s differs in %d of %d entries" % (what, k, differ, want[k].size))
    for k in ('depth', 'label', 'tri', 'dropped', 'degenerate'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


# ---- (a) ragged shapes ---------------------------------------------------------------------------------------------------
def test_ragged_frames_equal_the_restatement(hip, dev):
    """70 x 45 (no multiple of 8 or 64), three frames with their own cameras, the middle one without an instance; an
    instance of an empty mesh; the soup with its zero-area, repeated-vertex and out-of-range triangles."""
    ico = MR.icosphere(2)
    meshes = [MR.cube(), ico, EMPTY_MESH, MR.soup(200, seed=1, degenerate=True)]
    intr = np.array([[60, 61, 34.6, 22.3, 10000], [50, 50, 35, 22, 1000], [75.5, 70.25, 30.1, 25.7, 5000]], np.float32)
    frames = [[(0, 1, place(0.2, [0.3, 0.5, -0.2], [-0.15, 0.02, 0.8], (0.5, 0.5, 0.5))),
               (1, 2, place(0.12, [0.1, 0.2, 0.3], [0.1, -0.03, 0.7]))],
              [],
              [(2, 9, place(1.0, [0, 0, 0], [0, 0, 1])), (3, 255, place(0.15, [1.0, -0.4, 0.2], [0.02, 0.0, 0.9])),
               (0, 4, place(0.1, [-0.7, 0.1, 0.9], [0.12, 0.1, 0.6], (0.5, 0.5, 0.5)))]]
    got = launch(hip, dev, meshes, frames, intr, 45, 70)
    want = R.render(meshes, frames, intr, 45, 70)
    assert_equal(got, want, "ragged")
    assert not got['depth'][1].any() and np.all(got['tri'][1] == -1)
    assert set(np.unique(got['label'][0])) == {0, 1, 2} and {255, 4} <= set(np.unique(got['label'][2]))
    assert want['dropped'][3] >= 1 and want['degenerate'][3] >= 2 and want['dropped'][2] == 0
    # without the optional output: the same depth and label
    bare = launch(hip, dev, meshes, frames, intr, 45, 70, with_tri=False)
    assert np.array_equal(bare['depth'], got['depth']) and np.array_equal(bare['label'], got['label'])


# ---- (b) both raster paths -------------------------------------------------------------------------------------------------
def test_lane_path_and_wave_path(hip, dev):
    """A cube close to the camera (every box above RN_SMALL samples: the queue and one wave per triangle), an
    icosphere(3) far away (every box at most RN_SMALL: the setup lane) and an icosphere(2) sized so that its boxes land
    on both sides."""
    meshes = [MR.cube(), MR.icosphere(3), MR.icosphere(2)]
    H, W = 100, 150
    intr = np.array([[120, 120, 74.5, 49.5, 10000]] * 3, np.float32)
    frames = [[(0, 1, place(0.3, [0.4, 0.6, 0.1], [0.0, 0.0, 0.6], (0.5, 0.5, 0.5)))],
              [(1, 2, place(0.12, [0.2, 0.1, 0.0], [0.1, 0.05, 1.0]))],
              [(2, 3, place(0.1, [0.5, -0.3, 0.2], [-0.05, 0.0, 0.7]))]]
    want = R.render(meshes, frames, intr, H, W)
    tb = R.instance_bases(meshes, frames)[5]
    box = [want['box'][tb[j]:tb[j + 1]] for j in range(3)]
    print("RN_SMALL = %d; boxes: cube %d .. %d, far sphere %d .. %d, middle sphere %d .. %d (%d small, %d large)"
          % (RN_SMALL, box[0].min(), box[0].max(), box[1].min(), box[1].max(), box[2].min(), box[2].max(),
             ((box[2] <= RN_SMALL) & (box[2] > 0)).sum(), (box[2] > RN_SMALL).sum()))
    assert box[0].min() > RN_SMALL                                   # the wave path alone
    assert 0 < box[1].max() <= RN_SMALL                              # the lane path alone
    assert ((box[2] > 0) & (box[2] <= RN_SMALL)).sum() >= 20 and (box[2] > RN_SMALL).sum() >= 20
    got = launch(hip, dev, meshes, frames, intr, H, W)
    assert_equal(got, want, "paths")
    for f in range(3):
        assert (got['label'][f] == f + 1).sum() > 50


# ---- (c), (d), (e): occlusion, ties, borders ------------------------------------------------------------------------------------
def _scenes():
    meshes = [MR.icosphere(2), MR.cube(), MR.soup(64, seed=6)]
    intr = np.array([[60, 61, 34.6, 22.3, 10000], [64, 64, 35, 22, 1000], [40, 40, 35.5, 22.5, 10000]], np.float32)
    c = (0.5, 0.5, 0.5)
    frames = [
        # (c) two interpenetrating spheres: the same mesh placed twice
        [(0, 1, place(0.15, [0.1, 0.2, 0.3], [-0.05, 0.0, 0.7])), (0, 2, place(0.15, [0.3, 0.0, -0.1], [0.06, 0.02, 0.74]))],
        # (d) two coincident instances: every pixel is a tie in depth, the lower rank wins
        [(1, 3, place(0.25, [0.4, 0.6, 0.1], [0.0, 0.0, 0.8], c)), (1, 7, place(0.25, [0.4, 0.6, 0.1], [0.0, 0.0, 0.8], c))],
        # (e) a cube through the near plane, a soup across all four borders, a cube wholly outside the guard band
        [(1, 4, place(0.5, [0.2, 0.3, 0.1], [0.05, 0.0, 0.25], c)), (2, 5, place(1.5, [0.5, 0.1, -0.4], [0.0, 0.0, 1.6])),
         (1, 6, place(0.2, [0, 0, 0], [5000.0, 0.0, 1.0], c))]]
    return meshes, frames, intr, 45, 70


@pytest.fixture(scope="module")
def scenes():
    return _scenes()


@pytest.fixture(scope="module")
def scenes_ref(scenes):
    meshes, frames, intr, H, W = scenes
    return R.render(meshes, frames, intr, H, W)


@pytest.fixture(scope="module")
def scenes_got(hip, dev, scenes):
    return launch(hip, dev, *scenes)


def test_occlusion_ties_and_borders(scenes_got, scenes_ref):
    got, want = scenes_got, scenes_ref
    assert_equal(got, want, "scenes")
    assert (got['label'][0] == 1).sum() > 100 and (got['label'][0] == 2).sum() > 100       # both spheres show
    hit = got['depth'][1] != 0
    tb, ranks = got['tri_base'], got['tri'][1][hit]
    assert hit.sum() > 200 and np.all(got['label'][1][hit] == 3) and ranks.min() >= tb[2] and ranks.max() < tb[3]
    d = got['depth'][2]
    assert d[0].any() and d[-1].any() and d[:, 0].any() and d[:, -1].any()                # every border is crossed
    assert 0 < got['dropped'][4] < 12 and got['dropped'][6] == 12 and not (got['label'][2] == 6).any()
    assert (got['label'][2] == 4).any() and (got['label'][2] == 5).any()


def test_coincident_instances_reversed(hip, dev, scenes):
    meshes, frames, intr, H, W = scenes
    rev = [[frames[1][1], frames[1][0]]]
    got = launch(hip, dev, meshes, rev, intr[1:2], H, W)
    hit = got['depth'][0] != 0
    assert hit.sum() > 200 and np.all(got['label'][0][hit] == 7) and got['tri'][0][hit].max() < 12


# ---- (f), (g): independence of the batch and of the run ---------------------------------------------------------------------
def test_frames_do_not_depend_on_the_batch(hip, dev, scenes, scenes_got):
    meshes, frames, intr, H, W = scenes
    tb = scenes_got['tri_base']
    first = np.cumsum([0] + [len(f) for f in frames])
    for k in range(len(frames)):
        alone = launch(hip, dev, meshes, [frames[k]], intr[k:k + 1], H, W)
        assert np.array_equal(alone['depth'][0], scenes_got['depth'][k]), k
        assert np.array_equal(alone['label'][0], scenes_got['label'][k]), k
        rebased = np.where(alone['tri'][0] >= 0, alone['tri'][0] + int(tb[first[k]]), -1)
        assert np.array_equal(rebased, scenes_got['tri'][k]), k
        assert np.array_equal(alone['dropped'], scenes_got['dropped'][first[k]:first[k + 1]]), k
        assert np.array_equal(alone['degenerate'], scenes_got['degenerate'][first[k]:first[k + 1]]), k


def test_same_call_twice_gives_identical_bytes(hip, dev, scenes, scenes_got):
    again = launch(hip, dev, *scenes)
    for k in ('depth', 'label', 'tri', 'dropped', 'degenerate'):
        assert np.array_equal(again[k].view(np.uint8), scenes_got[k].view(np.uint8)), k


# ---- (h) the limits ------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_without_a_write(hip, dev):
    L = hip.lib()
    q = L.cloudaae_render_workspace_bytes
    assert q(1, 45, 70, 2, 16, 24) > 0
    assert q(1, 4096, 4096, 1, 8, 12) > 0 and q(1, 4097, 4096, 1, 8, 12) == 0          # H W above 2^24
    assert q(17, 4096, 4096, 1, 8, 12) == 0                                             # F H W above 2^28
    assert q(1, 45, 70, 1000, 16, (1 << 31) - 1) > 0 and q(1, 45, 70, 1000, 16, 1 << 31) == 0      # the rank total
    assert q(1, 45, 70, 1, 8, 1 << 24) > 0 and q(1, 45, 70, 1, 8, (1 << 24) + 1) == 0   # 2^24 triangles per mesh
    assert q(0, 45, 70, 1, 8, 12) == 0 and q(1, 45, 70, 0, 0, 0) == 0 and q(1, 0, 70, 1, 8, 12) == 0
    cv, ct, _ = MR.cube()
    d = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)
    vo, to, v, t = d([0, 8], np.int32), d([0, 12], np.int32), d(cv, np.float32), d(ct, np.int32)
    intr, offs = d([[60, 60, 35, 22, 1000]], np.float32), d([0, 1], np.int32)
    mesh, lab, pose = d([0], np.int32), d([1], np.int32), d(place(0.2, [0, 0, 0], [0, 0, 1]).reshape(1, 16), np.float64)
    vb, tb = d([0, 8], np.int32), d([0, 12], np.int32)
    H, W = 45, 70
    depth, label, tri = Guarded(H, W, torch.int16, dev), Guarded(H, W, torch.uint8, dev), Guarded(H, W, torch.int32, dev)
    dropped, degenerate = Guarded(1, 1, torch.int32, dev), Guarded(1, 1, torch.int32, dev)
    nbytes = int(q(1, H, W, 1, 8, 12))
    ws = Guarded(nbytes // 8, 1, torch.int64, dev)

    def call(h=H, w=W, j=1, sv=8, st=12, z_near=0.05, ws_bytes=nbytes, dep=depth.ptr()):
        return L.cloudaae_render_frames(1, vo.data_ptr(), to.data_ptr(), 8, 12, v.data_ptr(), t.data_ptr(), 1, h, w,
                                        intr.data_ptr(), offs.data_ptr(), j, mesh.data_ptr(), lab.data_ptr(), pose.data_ptr(),
                                        vb.data_ptr(), tb.data_ptr(), sv, st, z_near, dep, label.ptr(), tri.ptr(),
                                        dropped.ptr(), degenerate.ptr(), ws.ptr(), ws_bytes, hip.stream())
    assert call(h=4097, w=4096) != 0
    assert b"cloudaae_render_frames" in L.cloudaae_last_error()
    assert call(st=1 << 31) != 0 and call(st=(1 << 24) + 1) != 0 and call(sv=1 << 31) != 0 and call(j=0) != 0
    assert call(z_near=0.0) != 0 and call(ws_bytes=nbytes - 1) != 0 and call(dep=None) != 0
    torch.cuda.synchronize()
    for buf in (depth, label, tri, dropped, degenerate, ws):
        assert np.all(buf.numpy().view(np.uint8) == FILL)              # nothing was written, guards included
    assert call() == 0
    torch.cuda.synchronize()
    assert (label.numpy() == 1).sum() > 50 and dropped.numpy()[0, 0] == 0


# ---- through Python ------------------------------------------------------------------------------------------------------------
def test_rendered_sphere_back_projects_onto_the_sphere(hip, dev):
    """render_frames -> extract_segments on the returned tensors: every back-projected point, taken into the model frame
    by the inverse pose, lies between the mesh's inscribed sphere and its circumscribed one, to e = 1 / factor_depth:
    half a depth unit along a ray of obliquity < 1.1 (the camera's corner: sqrt(1 + 0.30^2 + 0.225^2) = 1.07), plus the
    vertices' snap to 1/256 pixel (1.4e-6 m at this depth) and the fp32 rounding of the back-projection (1e-7 m)."""
    from cloudaae_amd.utils import pose_score, render, segment
    from cloudaae_amd.utils import sample_pose_in_frustum as spf
    r, factor = 0.08, 10000.0
    v, t = MR.icosphere(3)
    cam = spf.camera_parameters('ycbv')
    intr = np.array([[cam['fx'], cam['fy'], cam['cx'], cam['cy'], factor]], np.float32)
    p = spf.sample_poses(1, 2025, 3, device=dev)
    out = render.render_frames([(v, t)], [[(0, 6, (p['axisangle'][0], p['translation'][0]))]], intr, 480, 640, scale=r,
                               return_tri=True, device=dev)
    assert out['depth'].dtype == torch.int16 and out['label'].dtype == torch.uint8 and out['depth'].is_cuda
    assert out['dropped'].sum() == 0 and out['degenerate'].sum() == 0
    seg = segment.extract_segments(out['depth'], out['label'], intr, classes=[[5]], device=dev)
    n = int(seg.offsets[1])
    pts = seg.xyz[:n].cpu().numpy().astype(np.float64)
    T = pose_score.pose_matrix(p['axisangle'], p['translation'])[0].cpu().numpy()
    model = (pts - T[:3, 3]) @ T[:3, :3]                                  # R^T (p - t)
    v32 = (v.astype(np.float64) * r).astype(np.float32).astype(np.float64)
    a, b, c = v32[t[:, 0]], v32[t[:, 1]], v32[t[:, 2]]
    nrm = np.cross(b - a, c - a)
    r_in = float(np.min(np.abs((nrm * a).sum(1)) / np.linalg.norm(nrm, axis=1)))
    r_out = float(np.linalg.norm(v32, axis=1).max())
    dist = np.linalg.norm(model, axis=1)
    e = 1.0 / factor
    print("sphere of %g m at %s: %d points, |p| in [%.7f, %.7f], mesh in [%.7f, %.7f], e = %g"
          % (r, T[:3, 3], n, dist.min(), dist.max(), r_in, r_out, e))
    assert n == int((out['label'] == 6).sum()) and n > 2000
    assert dist.min() >= r_in - e and dist.max() <= r_out + e


def _ply_meshes(directory):
    """Two made-up meshes in millimetres: a ball of 6 cm radius and a plate of 24 x 24 x 3 cm."""
    os.makedirs(directory)
    iv, it = MR.icosphere(3)
    cv, ct, _ = MR.cube()
    plate = (cv - np.float32(0.5)) * np.array([240.0, 240.0, 30.0], np.float32)
    _write_ply(os.path.join(directory, "obj_000001.ply"), iv * np.float32(60.0), it, np.full((len(iv), 3), 50))
    _write_ply(os.path.join(directory, "obj_000002.ply"), plate, ct, np.full((len(cv), 3), 200))


@pytest.fixture(scope="module")
def rendered_records(hip, dev, tmp_path_factory):
    from cloudaae_amd.utils import render
    tmp = tmp_path_factory.mktemp("render")
    _ply_meshes(str(tmp / "meshes"))
    render.main(["--meshes", str(tmp / "meshes"), "--out", str(tmp / "data"), "--frames", "4", "--objects", "2", "--seq", "48",
                 "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    return tmp, str(tmp / "data" / "0048_pcnn.tfrecord")


def test_rendered_records_evaluate_end_to_end(hip, dev, rendered_records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import render
    tmp, path = rendered_records
    files = mm.mesh_files(str(tmp / "meshes"))
    models = mm.models_from_meshes(files, scale=0.001, oversample=2, device=dev)
    frames = tfrecord_io.read_frames(path, verify=True)
    assert len(frames) == 4 and frames[0]['depth'].shape == (120, 160) and int(frames[3]['frame_id']) == 3
    classes, poses = render.sample_scenes(4, 2, 2, seed=11, device=dev)
    assert all(list(fr['class_one_hot'][:2]) == [1, 1] and fr['class_one_hot'].sum() == 2 for fr in frames)
    N = 128
    el = E.element_from_frames(frames, 0, N, models, seed=4, device=dev)
    assert el is not None and len(el['class_id']) >= 1
    for b, f in enumerate(el['frame_id']):
        k = list(classes[f]).index(0)
        assert np.array_equal(el['translation'][b].cpu().numpy(), poses[f, k, :3, 3].astype(np.float32))
        got = R.pose_matrix(el['axisangle'][b].cpu().numpy(), [0, 0, 0])[:3, :3]
        assert np.abs(got - poses[f, k, :3, :3]).max() <= 1e-6              # float32 quaternion and axis-angle on the way
    print("frames kept for class 0: %s of 4; points in segment: %s" % (list(el['frame_id']), list(el['num_valid_points_in_segment'])))
    B = len(el['class_id'])
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    out = E.evaluate_batch(graph, {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}, score=True)
    for k in ("trans_loss", "axag_loss", "xyz_loss", "add_pred", "adds_pred"):
        assert torch.isfinite(out[k]).all(), k


def test_evaluate_reads_the_files_it_is_given(hip, dev, rendered_records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    tmp, path = rendered_records
    obj = str(tmp / "obj_models.tfrecords")
    mm.main(["--meshes", str(tmp / "meshes"), "--out", obj, "--scale", "0.001", "--oversample", "2"])
    graph = T.TrainGraph({"num_point": 128, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    capsys.readouterr()
    assert E.main(["--files", path + "," + path, "--object_model", obj, "--trained_model", ckpt[:-len(".npz")],
                   "--target_cls", "0", "--num_point", "128", "--batch_size", "1", "--score"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    size = [ln for ln in lines if ln.startswith("batch size ")]
    assert len(size) == 1 and int(size[0].split()[-1]) >= 2 and int(size[0].split()[-1]) % 2 == 0, lines[-10:]
