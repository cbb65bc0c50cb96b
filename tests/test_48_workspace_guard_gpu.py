"""GPU: every entry point whose workspace holds more than one region stays inside the bytes its query asks for.

Each Python wrapper runs twice on the same input: once as it is, once with the library's entry point replaced by a shim
that swaps the wrapper's workspace for the interior of a block of query + 512 bytes filled with 0xA5 -- the pointer 256
bytes in, exactly `query` bytes as the size.  Both 256-byte guard bands must come back untouched and every output must
equal the plain run's bit for bit.  The shapes are the smallest at which each region ends inside its 256-byte pad and
more than one workgroup writes."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


class Guarded(object):
    """Stands in for entry point `fn` of the loaded library: the call goes through with the workspace argument (at
    ws_index; its size follows it, or comes from size_of(args) for an entry that takes none) replaced by the guarded one."""

    def __init__(self, hip, monkeypatch, dev, fn, ws_index, size_of=None):
        self.inner = getattr(hip.lib(), fn)
        self.dev, self.ws_index, self.size_of = dev, ws_index, size_of
        self.calls = []                                # (bytes asked for, the block)
        monkeypatch.setattr(hip.lib(), fn, self)

    def __call__(self, *args):
        args = list(args)
        need = int(args[self.ws_index + 1]) if self.size_of is None else int(self.size_of(args))
        block = torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        assert block.data_ptr() % 256 == 0
        args[self.ws_index] = block.data_ptr() + GUARD
        self.calls.append((need, block))
        return self.inner(*args)

    def check(self, want_bytes):
        """one call, with exactly the query's bytes, and both guard bands as they were filled"""
        torch.cuda.synchronize()
        assert len(self.calls) == 1
        need, block = self.calls[0]
        assert need == want_bytes
        host = block.cpu().numpy()
        assert (host[:GUARD] == FILL).all(), "bytes in front of the workspace were written"
        assert (host[GUARD + need:] == FILL).all(), "bytes behind the workspace were written"
        assert (host[GUARD:GUARD + need] != FILL).any()      # (the workspace itself was used)


def same(a, b, what):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def test_render_frames(hip, dev, monkeypatch):
    from cloudaae_amd.utils import render
    F, H, W = 2, 9, 11
    verts = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.05], [0.0, 0.2, 0.05], [0.1, 0.1, 0.25]], np.float32)
    tris = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], np.int32)

    def pose(x, y, z):
        m = np.eye(4)
        m[:3, 3] = (x, y, z)
        return m
    instances = [[(0, 1, pose(-0.1, -0.1, 0.5)), (0, 2, pose(-0.05, -0.12, 0.45))], [(0, 7, pose(-0.12, -0.06, 0.6))]]
    intr = np.array([[14.0, 15.0, 5.25, 4.5, 10000.0], [13.0, 13.5, 5.0, 4.0, 10000.0]], np.float32)

    def run():
        return render.render_frames([(verts, tris)], instances, intr, H, W, return_tri=True, device=dev)
    plain = run()
    shim = Guarded(hip, monkeypatch, dev, "cloudaae_render_frames", 26)
    guarded = run()
    shim.check(int(hip.lib().cloudaae_render_workspace_bytes(F, H, W, 3, 12, 12)))
    assert (plain["depth"] != 0).any() and len(torch.unique(plain["label"])) == 4
    for k in ("depth", "label", "tri", "dropped", "degenerate"):
        same(guarded[k], plain[k], k)


def test_mesh_weights(hip, dev, monkeypatch):
    from cloudaae_amd.utils import mesh_models
    rng = np.random.default_rng(48)
    meshes = []
    for nv, nt in ((60, 200), (31, 57)):               # 257 triangles: two scan blocks
        meshes.append((rng.standard_normal((nv, 3)).astype(np.float32), rng.integers(0, nv, (nt, 3)).astype(np.int32)))
    packed = mesh_models.pack_meshes(meshes, device=dev)
    plain = mesh_models.mesh_weights(packed)
    shim = Guarded(hip, monkeypatch, dev, "cloudaae_mesh_weights", 11)
    guarded = mesh_models.mesh_weights(packed)
    shim.check(int(hip.lib().cloudaae_mesh_weights_workspace_bytes(257)))
    assert int(plain["cum"][-1]) > 0
    for k in ("weights", "cum", "a2max", "invalid"):
        same(guarded[k], plain[k], k)


def test_component_labels(hip, dev, monkeypatch):
    from cloudaae_amd.utils import depth_components as DC
    F, H, W = 3, 33, 35                                # crosses a 32 x 32 tile in both directions
    rng = np.random.default_rng(49)
    v, u = np.mgrid[0:H, 0:W]
    depth = np.empty((F, H, W), np.uint16)
    for f in range(F):
        d = 10000 + 3 * u + 2 * v + rng.integers(-1, 2, (H, W))       # a table, a little tilted
        d[4:12, 3 + f:14 + f] -= 600                                    # objects on it: one across the tile seam
        d[20:33, 25:35] -= 900
        d[15:19, 8:12] -= 400
        depth[f] = d
    intr = np.tile(np.array([40.0, 40.0, 17.0, 16.0, 10000.0], np.float32), (F, 1))

    def run():
        return DC.segment_depth(depth, intr, seed=5, n_hyp=64, stride=1, min_pixels=4, device=dev)
    plain = run()
    shim = Guarded(hip, monkeypatch, dev, "cloudaae_component_labels", 12)
    guarded = run()
    shim.check(int(hip.lib().cloudaae_component_labels_workspace_bytes(F, H, W)))
    assert list(plain.n_components) == [3, 3, 3]      # (tests/depth_components_reference.py on this scene)
    for k in ("label", "root", "fg", "n_components", "n_candidates", "comp_root", "comp_size", "comp_box"):
        same(getattr(guarded, k), getattr(plain, k), k)


def test_frame_segments_and_radius_outlier(hip, dev, monkeypatch):
    """s = 3 segments of 130, 1 and 171 points, in two frames of 17 x 19 pixels (two 256-pixel blocks each)"""
    from cloudaae_amd.utils import segment as S
    F, H, W = 2, 17, 19
    rng = np.random.default_rng(50)
    depth = rng.integers(7000, 7400, (F, H * W)).astype(np.uint16)
    label = np.zeros((F, H * W), np.uint8)
    label[0, 30:160] = 1                               # class 0: 130 pixels
    label[0, 300] = 2                                  # class 1: one pixel, in the second block
    label[1, 120:291] = 3                              # class 2: 171 pixels across the block boundary
    depth[1, 130] = 0                                  # (no depth: not a point) ...
    label[1, 291] = 3                                  # ... so one more pixel makes the 171
    depth, label = depth.reshape(F, H, W), label.reshape(F, H, W)
    intr = np.array([[60.0, 61.0, 9.5, 8.0, 10000.0], [58.0, 59.0, 9.0, 8.5, 10000.0]], np.float32)

    def run():
        return S.extract_segments(depth, label, intr, classes=[[0, 1], [2]], threshold=np.float32(10.0), nb_points=10,
                                  radius=np.float32(0.03), min_keep=3, device=dev)
    plain = run()
    fs = Guarded(hip, monkeypatch, dev, "cloudaae_frame_segments", 13)
    ro = Guarded(hip, monkeypatch, dev, "cloudaae_radius_outlier", 11)
    guarded = run()
    fs.check(int(hip.lib().cloudaae_frame_segments_workspace_bytes(F, H, W, 3)))
    ro.check(int(hip.lib().cloudaae_radius_outlier_workspace_bytes(3, F * H * W)))
    assert list(plain.num_point_after_filter) == [130, 1, 171]
    n_in = np.diff(plain.inlier_offsets)
    assert list(n_in) == [92, 1, 107]                  # (tests/segment_reference.py on this scene: the radius filter decides)
    for k in ("offsets", "inlier_offsets", "num_valid_points_in_segment"):
        same(getattr(guarded, k), getattr(plain, k), k)
    m, m_in = int(plain.offsets[-1]), int(plain.inlier_offsets[-1])
    same(guarded.mean, plain.mean, "mean")
    same(guarded.xyz[:m], plain.xyz[:m], "xyz")
    same(guarded.xyz_inlier_full[:m_in], plain.xyz_inlier_full[:m_in], "xyz_inlier_full")
    same(guarded.inlier_index[:m_in], plain.inlier_index[:m_in], "inlier_index")


def test_estimate_normals(hip, dev, monkeypatch):
    from cloudaae_amd.utils import normals as N
    rng = np.random.default_rng(51)
    sizes = (1, 130, 171)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    xyz = torch.from_numpy((rng.standard_normal((sum(sizes), 3)) * 0.03).astype(np.float32)).to(dev)
    queries = torch.from_numpy((rng.standard_normal((3, 9, 3)) * 0.02).astype(np.float32)).to(dev)

    def run():
        return N.estimate_normals(xyz, 0.03, queries=queries, offsets=offsets, viewpoint=(0.0, 0.0, -1.0))
    plain = run()
    shim = Guarded(hip, monkeypatch, dev, "cloudaae_estimate_normals", 15)
    guarded = run()
    shim.check(int(hip.lib().cloudaae_estimate_normals_workspace_bytes(3, sum(sizes))))
    assert int((plain[2] >= 3).sum()) >= 9
    for a, b, k in zip(guarded, plain, ("normals", "eigenvalues", "count")):
        same(a, b, k)


def test_hidden_point_removal(hip, dev, monkeypatch):
    """the entry takes no workspace size: the shim asks the query, as the wrapper does"""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    B, n = 3, 130
    rng = np.random.default_rng(52)
    pts = rng.standard_normal((B, n, 3))
    pts = 0.05 * pts / np.linalg.norm(pts, axis=2, keepdims=True) * rng.uniform(0.6, 1.0, (B, n, 1)) + [0.0, 0.0, 0.6]
    x = {"model_xyz_rot_trans": torch.from_numpy(pts.astype(np.float32)).to(dev)}
    x = hpr.sphericalFlip_org(x, None, 0.8 * math.pi)
    flipped, org = x["flippedPoints_org"], x["orgPoints_org"]
    assert tuple(flipped.shape) == (B, n + 1, 3)

    def run():
        return hpr.convexHull(flipped, org, seed=3, return_ids=True, return_src=True)
    plain = run()
    query = hip.lib().cloudaae_hpr_workspace_bytes
    shim = Guarded(hip, monkeypatch, dev, "cloudaae_hidden_point_removal_rows", 10, size_of=lambda a: query(a[0], a[1]))
    guarded = run()
    shim.check(int(query(B, n + 1)))
    num = plain[1].cpu().numpy()
    assert ((num >= 4) & (num < n + 1)).all()          # some points are hidden, some are not
    for a, b, k in zip(guarded, plain, ("visible", "num_vis", "visible_id", "row_src")):
        same(a, b, k)
