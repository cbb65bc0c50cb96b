"""GPU: cloudaae_depth_plane, cloudaae_depth_foreground, cloudaae_depth_components and cloudaae_component_labels through
the C ABI against the NumPy restatement of DESIGN.md "Depth components" (tests/depth_components_reference.py), then
utils/depth_components.py, element_from_frames(labels="components") and the evaluation's command line.

Every output is an integer, or a double copied from one hypothesis: everything is compared for equality, `plane` bit for
bit, no entry left out.  Outputs sit between guard rows that are filled with a byte pattern (as in
tests/test_33_ppf_gpu.py), so every call starts on garbage."""
import os

import numpy as np
import pytest
import torch

import depth_components_reference as D
import depth_noise_reference as DN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
FILL = 0xA5


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


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the four calls -----------------------------------------------------------------------------------------------------------
def run_plane(hip, dev, depth, intr, seed, first_frame, n_hyp, stride, tol, percent):
    F, H, W = depth.shape
    d, k = _depth(depth, dev), _d(intr, np.float32, dev)
    count, tested = Guarded(F, n_hyp, torch.int32, dev), Guarded(F, 1, torch.int32, dev)
    plane, hyp = Guarded(F, 4, torch.float64, dev), Guarded(F, 1, torch.int32, dev)
    hip.check(hip.lib().cloudaae_depth_plane(F, H, W, d.data_ptr(), k.data_ptr(), seed, first_frame, n_hyp, stride, tol, percent,
                                             count.ptr(), tested.ptr(), plane.ptr(), hyp.ptr(), hip.stream()), "cloudaae_depth_plane")
    torch.cuda.synchronize()
    return dict(count=count.numpy(), tested=tested.numpy().ravel(), plane=plane.numpy(), plane_hyp=hyp.numpy().ravel())


def run_foreground(hip, dev, depth, intr, plane, plane_hyp, tol, max_height):
    F, H, W = depth.shape
    d, k = _depth(depth, dev), _d(intr, np.float32, dev)
    pl, ph = _d(plane, np.float64, dev), _d(plane_hyp, np.int32, dev)
    fg = Guarded(F * H, W, torch.uint8, dev)
    hip.check(hip.lib().cloudaae_depth_foreground(F, H, W, d.data_ptr(), k.data_ptr(), pl.data_ptr(), ph.data_ptr(), tol, max_height,
                                                  fg.ptr(), hip.stream()), "cloudaae_depth_foreground")
    torch.cuda.synchronize()
    return fg.numpy().reshape(F, H, W)


def run_components(hip, dev, depth, fg, jump_units):
    F, H, W = depth.shape
    d, g, j = _depth(depth, dev), _d(fg, np.uint8, dev), _d(jump_units, np.int32, dev)
    root, status = Guarded(F * H, W, torch.int32, dev), Guarded(F, 1, torch.int32, dev)
    L = hip.lib()
    nbytes = int(L.cloudaae_depth_components_workspace_bytes(F, H, W))
    assert nbytes >= 4 * F * H * W
    ws = Guarded(1, nbytes, torch.uint8, dev)
    hip.check(L.cloudaae_depth_components(F, H, W, d.data_ptr(), g.data_ptr(), j.data_ptr(), root.ptr(), status.ptr(), ws.ptr(), nbytes,
                                          hip.stream()), "cloudaae_depth_components")
    torch.cuda.synchronize()
    ws.numpy()                                              # the workspace's guards
    return root.numpy().reshape(F, H, W), status.numpy().ravel()


def run_labels(hip, dev, root, min_pixels, max_components):
    F, H, W = root.shape
    r = _d(root, np.int32, dev)
    K = max_components
    label = Guarded(F * H, W, torch.uint8, dev)
    n_comp, n_cand = Guarded(F, 1, torch.int32, dev), Guarded(F, 1, torch.int32, dev)
    c_root, c_size, c_box = Guarded(F, K, torch.int32, dev), Guarded(F, K, torch.int32, dev), Guarded(F, 4 * K, torch.int32, dev)
    L = hip.lib()
    nbytes = int(L.cloudaae_component_labels_workspace_bytes(F, H, W))
    assert nbytes > 0
    ws = Guarded(1, nbytes, torch.uint8, dev)
    hip.check(L.cloudaae_component_labels(F, H, W, r.data_ptr(), min_pixels, K, label.ptr(), n_comp.ptr(), n_cand.ptr(), c_root.ptr(),
                                          c_size.ptr(), c_box.ptr(), ws.ptr(), nbytes, hip.stream()), "cloudaae_component_labels")
    torch.cuda.synchronize()
    ws.numpy()
    return dict(label=label.numpy().reshape(F, H, W), n_components=n_comp.numpy().ravel(), n_candidates=n_cand.numpy().ravel(),
                comp_root=c_root.numpy(), comp_size=c_size.numpy(), comp_box=c_box.numpy().reshape(F, K, 4))


def check_plane(hip, dev, depth, intr, seed, first_frame, n_hyp, stride, tol=0.01, percent=10, max_height=0.5):
    """The plane and the foreground of a batch against the restatement, frame by frame.  -> (got, the frames' references)."""
    got = run_plane(hip, dev, depth, intr, seed, first_frame, n_hyp, stride, tol, percent)
    fg = run_foreground(hip, dev, depth, intr, got['plane'], got['plane_hyp'], tol, max_height)
    refs = []
    for f in range(len(depth)):
        ref = D.plane(depth[f], intr[f], seed, first_frame + f, n_hyp, stride, tol, percent)
        ref['fg'] = D.foreground(depth[f], intr[f], ref['plane'], ref['plane_hyp'], tol, max_height)
        print("frame %d: plane_hyp %d / %d, count %d / %d of tested %d / %d, counts differ in %d, fg differs in %d" % (
            f, got['plane_hyp'][f], ref['plane_hyp'], got['count'][f].max(), ref['count'].max(), got['tested'][f], ref['tested'],
            (got['count'][f] != ref['count']).sum(), (fg[f] != ref['fg']).sum()))
        assert np.array_equal(got['count'][f], ref['count']) and got['tested'][f] == ref['tested']
        assert got['plane_hyp'][f] == ref['plane_hyp']
        assert np.array_equal(_bits(got['plane'][f]), _bits(ref['plane']))
        assert np.array_equal(fg[f], ref['fg'])
        refs.append(ref)
    return got, refs


# ---- cloudaae_depth_plane, cloudaae_depth_foreground ------------------------------------------------------------------------------
def test_plane_and_foreground_of_the_table_scene(hip, dev):
    depth, label, intr = D.scene()
    got, refs = check_plane(hip, dev, depth, intr, stride=D.SCENE_PARAMS['stride'], n_hyp=D.SCENE_PARAMS['n_hyp'],
                            seed=D.SCENE_PARAMS['seed'], first_frame=0)
    # the rendered table is an exact plane: many hypotheses tie at the largest count, and the lowest wins
    assert got['plane_hyp'][0] == 0 and got['count'][0, 0] == 954 and got['tested'][0] == 1040
    assert (got['count'][0] == 954).sum() > 10
    assert int(refs[0]['fg'].sum()) == 337


@pytest.mark.parametrize("first_frame", [0, 1 << 20])
@pytest.mark.parametrize("n_hyp,stride", [(50, 2), (64, 3)])
def test_plane_of_three_cameras(hip, dev, first_frame, n_hyp, stride):
    depth, _, intr = DN.rendered('planes_48x64')
    assert depth.shape == (3, 48, 64) and len(set(intr[:, 4].tolist())) == 2
    got, _ = check_plane(hip, dev, depth, intr, seed=5, first_frame=first_frame, n_hyp=n_hyp, stride=stride)
    assert np.all(got['plane_hyp'] >= 0)
    # a frame's result depends on its global index alone: frame 1 of this batch as frame 0 of a batch that starts there
    one = run_plane(hip, dev, depth[1:2], intr[1:2], 5, first_frame + 1, n_hyp, stride, 0.01, 10)
    assert np.array_equal(one['count'][0], got['count'][1]) and np.array_equal(_bits(one['plane'][0]), _bits(got['plane'][1]))


def edge_frames():
    """48 x 64: no depth at all; one image row at one depth (valid pixels, but a hypothesis that draws three of them is
    rare: the collinear triples have a test of their own below); noise (no plane above 50 %); a rendered plane."""
    rng = np.random.default_rng(3)
    depth, _, intr = DN.rendered('planes_48x64')
    frames = np.zeros((4, 48, 64), np.uint16)
    frames[1, 20, :] = 900
    frames[2] = rng.integers(400, 4000, (48, 64))
    frames[3] = depth[0]
    return frames, np.stack([intr[0]] * 4)


@pytest.mark.parametrize("stride", [1, 2, 50])
def test_plane_edge_frames(hip, dev, stride):
    frames, intr = edge_frames()
    got, refs = check_plane(hip, dev, frames, intr, seed=9, first_frame=0, n_hyp=40, stride=stride, percent=50)
    assert got['tested'][0] == 0 and not got['count'][0].any() and got['plane_hyp'][0] == -1
    assert not got['count'][1].any() and got['plane_hyp'][1] == -1          # valid pixels, but every hypothesis is void
    assert got['plane_hyp'][2] == -1                                        # below min_plane_percent
    if stride == 50:                                                        # larger than H: pixels (0, 0) and (50, 0) alone
        assert got['tested'].tolist() == [int(f[0, 0] != 0) + int(f[0, 50] != 0) for f in frames]
        assert got['tested'][2] == 2 and np.all(got['plane_hyp'] == -1)     # fewer than three inliers are no plane
    else:
        assert got['plane_hyp'][3] >= 0
        assert got['tested'][1] == (64 if stride == 1 else 32)
    for f in (0, 1, 2):                                                     # without a plane the foreground is the valid pixels
        assert np.array_equal(refs[f]['fg'] != 0, frames[f] != 0)


@pytest.mark.parametrize("shape", [(1, 64), (37, 1)])
@pytest.mark.parametrize("tol", [0.01, 0.0])
def test_collinear_triples_are_void(hip, dev, shape, tol):
    """Every pixel valid and at one depth in a single row or column: the points lie on one line, so every hypothesis has
    three valid pixels and q = 0 exactly.  None may count an inlier, with tol = 0 (where 0 <= tol^2 q would hold) either."""
    H, W = shape
    depth = np.full((2, H, W), 900, np.uint16)
    depth[1] = 1500
    intr = np.array([[58.88, 59.1, 31.5, 23.7, 1000.0], [70.4, 66.25, 30.1, 25.7, 2000.0]], np.float32)
    for f in range(2):
        n, d, q, void, pix = D.hypotheses(depth[f], D.backproject(depth[f], intr[f]), 13, f, 24)
        assert void.all() and np.all(depth[f].reshape(-1)[pix] != 0) and len(np.unique(pix)) > 3      # void by q = 0 alone
    got, refs = check_plane(hip, dev, depth, intr, seed=13, first_frame=0, n_hyp=24, stride=1, tol=tol)
    assert not got['count'].any() and got['tested'].tolist() == [H * W] * 2 and got['plane_hyp'].tolist() == [-1, -1]
    assert all(r['fg'].all() for r in refs)


def test_zero_tolerance_counts_nothing_for_void_hypotheses(hip, dev):
    """tol = 0 is a valid input: an inlier then lies on the plane exactly.  Frames with pixels without depth have void
    hypotheses, and those count 0 as with any other tol."""
    depth, _, intr = D.scene()
    pts = D.backproject(depth[0], intr[0])
    void = D.hypotheses(depth[0], pts, 1, 0, 64)[3]
    assert void.any() and not void.all()
    got, refs = check_plane(hip, dev, depth, intr, seed=1, first_frame=0, n_hyp=64, stride=2, tol=0.0, percent=0)
    assert not got['count'][0][void].any() and got['count'][0].max() < got['tested'][0]
    frames, intr4 = edge_frames()
    got, _ = check_plane(hip, dev, frames, intr4, seed=9, first_frame=0, n_hyp=40, stride=1, tol=0.0, percent=0)
    assert not got['count'][:2].any() and got['plane_hyp'][:2].tolist() == [-1, -1]


# ---- cloudaae_depth_components ------------------------------------------------------------------------------------------------------
SHAPES = [(37, 70), (48, 64), (1, 1), (1, 70), (37, 1)]


def check_components(hip, dev, depth, fg, jump):
    root, status = run_components(hip, dev, depth, fg, jump)
    assert not status.any(), status
    for f in range(len(depth)):
        want = D.components(depth[f], fg[f], int(jump[f]))
        print("frame %d: %d components, root differs in %d pixels" % (f, len(np.unique(want[want >= 0])), (root[f] != want).sum()))
        assert np.array_equal(root[f], want), f
    return root


@pytest.mark.parametrize("shape", SHAPES)
def test_component_patterns(hip, dev, shape):
    H, W = shape
    masks = [np.zeros((H, W), bool), np.ones((H, W), bool), D.checkerboard(H, W), D.serpentine(H, W)[0], D.u_shape(H, W),
             D.combs(H, W)[0]]
    fg = np.stack(masks).astype(np.uint8)
    depth = np.full(fg.shape, 1000, np.uint16)
    root = check_components(hip, dev, depth, fg, np.zeros(len(masks), np.int32))
    assert np.all(root[0] == -1) and np.all(root[1] == 0)
    assert np.array_equal(root[2][masks[2]], np.flatnonzero(masks[2]))      # every pixel its own component
    assert np.all(root[3][masks[3]] == 0) and np.all(root[4][masks[4]] == 0)
    assert len(np.unique(root[5][masks[5]])) == (2 if H >= 5 and W >= 3 else 1)
    # depth 0 is not background by itself: the foreground mask decides (the caller's fg already holds validity)
    again = check_components(hip, dev, np.zeros_like(depth), fg, np.zeros(len(masks), np.int32))
    assert np.array_equal(again, root)


def step_frame(H, W, pos, jump, vertical):
    """Two foreground strips two pixels apart, each cut at `pos` | `pos + 1` by a depth step: `jump` in the first (joined),
    `jump` + 1 in the second (not joined): three components."""
    depth = np.zeros((H, W), np.uint16)
    fg = np.zeros((H, W), np.uint8)
    d, g = (depth.T, fg.T) if vertical else (depth, fg)
    g[0, :] = g[2, :] = 1
    d[0, :pos + 1], d[0, pos + 1:] = 1000, 1000 + jump
    d[2, :pos + 1], d[2, pos + 1:] = 1000 + jump + 1, 1000
    return depth, fg


@pytest.mark.parametrize("shape", [(37, 70), (48, 64)])
def test_depth_steps_inside_tiles_and_on_seams(hip, dev, shape):
    H, W = shape
    cases = [step_frame(H, W, pos, 7, vertical) for vertical in (False, True) for pos in (10, 31)]
    depth, fg = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    root = check_components(hip, dev, depth, fg, np.full(len(cases), 7, np.int32))
    for f in range(len(cases)):
        assert len(np.unique(root[f][fg[f] != 0])) == 3, f


def test_frames_with_their_own_jump_units(hip, dev):
    rng = np.random.default_rng(11)
    H, W = 37, 70
    depth = np.stack([rng.integers(1000, 1012, (H, W)).astype(np.uint16)] * 4)
    fg = np.stack([(rng.random((H, W)) < 0.85).astype(np.uint8)] * 4)
    jump = np.array([0, 5, 65535, -1], np.int32)
    root = check_components(hip, dev, depth, fg, jump)
    sizes = [len(np.unique(root[f][fg[f] != 0])) for f in range(4)]
    assert sizes[3] == int(fg[3].sum()) and sizes[0] > sizes[1] > sizes[2]   # a negative entry joins nothing
    for f in range(4):                                                      # each frame equals its result alone
        alone, status = run_components(hip, dev, depth[f:f + 1], fg[f:f + 1], jump[f:f + 1])
        assert np.array_equal(alone[0], root[f]) and not status.any()


def test_a_serpentine_through_every_tile_of_a_camera_frame(hip, dev):
    """480 x 640: the answer is known by construction -- one component, its root the first pixel, its size its length."""
    H, W = 480, 640
    mask, length = D.serpentine(H, W)
    fg = mask.astype(np.uint8)[None]
    depth = np.full((1, H, W), 800, np.uint16)
    root, status = run_components(hip, dev, depth, fg, np.zeros(1, np.int32))
    assert not status.any()
    assert np.all(root[0][mask] == 0) and np.all(root[0][~mask] == -1)
    t = run_labels(hip, dev, root, 1, 4)
    assert t['n_components'].tolist() == [1] and t['n_candidates'].tolist() == [1]
    assert t['comp_root'][0].tolist() == [0, -1, -1, -1] and t['comp_size'][0].tolist() == [length, -1, -1, -1]
    assert t['comp_box'][0, 0].tolist() == [0, 0, W - 1, H - 2] and np.array_equal(t['label'][0] == 1, mask)


# ---- cloudaae_component_labels ----------------------------------------------------------------------------------------------------------
def check_labels(hip, dev, root, min_pixels, max_components):
    got = run_labels(hip, dev, root, min_pixels, max_components)
    for f in range(len(root)):
        want = D.table(root[f], min_pixels, max_components)
        for k in ('n_components', 'n_candidates', 'comp_root', 'comp_size', 'comp_box', 'label'):
            assert np.array_equal(got[k][f], want[k]), (f, k, got[k][f], want[k])
    return got


def blob_roots(H, W, boxes):
    """root [H,W] of separate rectangles (u0, v0, u1, v1), inclusive; a box may list pixels to leave out after it."""
    root = np.full((H, W), -1, np.int32)
    for u0, v0, u1, v1, *cut in boxes:
        root[v0:v1 + 1, u0:u1 + 1] = v0 * W + u0
        for (u, v) in cut:
            root[v, u] = -1
    return root


def test_table_order_ties_boundary_and_cap(hip, dev):
    H, W = 37, 70
    # sizes 8, 7, 6, 6 (a tie: the lower root first), 5 (one below min_pixels); each border of the frame is touched
    a = blob_roots(H, W, [(0, 0, 2, 1), (67, 10, 69, 11), (30, 35, 33, 36), (0, 20, 6, 20), (40, 5, 42, 6, (42, 6))])
    # the same with min_pixels at the smallest kept size, and a frame without any component
    b = blob_roots(H, W, [(5, 5, 9, 5), (20, 5, 25, 5)])
    root = np.stack([a, b, np.full((H, W), -1, np.int32)])
    got = check_labels(hip, dev, root, 6, 3)
    assert got['n_candidates'].tolist() == [4, 1, 0] and got['n_components'].tolist() == [3, 1, 0]
    assert got['comp_size'][0].tolist() == [8, 7, 6] and got['comp_root'][0].tolist() == [35 * W + 30, 20 * W, 0]
    assert got['comp_box'][0].tolist() == [[30, 35, 33, 36], [0, 20, 6, 20], [0, 0, 2, 1]]
    assert got['comp_size'][1].tolist() == [6, -1, -1]                      # size = min_pixels kept, one less dropped
    got = check_labels(hip, dev, root, 6, 254)
    assert got['n_components'].tolist() == [4, 1, 0] and got['comp_root'][0, 3] == 10 * W + 67
    assert got['comp_box'][0, 3].tolist() == [67, 10, 69, 11]               # the right border
    # entries that are no pixel of the frame count as background
    wild = a.copy()
    wild[36, 69], wild[36, 68] = H * W, -7
    assert np.array_equal(run_labels(hip, dev, wild[None], 6, 3)['label'][0], got['label'][0] * (got['label'][0] <= 3))


def test_three_hundred_single_pixels_and_the_largest_cap(hip, dev):
    H, W = 24, 25
    mask = D.checkerboard(H, W)
    assert int(mask.sum()) == 300
    root = np.where(mask, np.arange(H * W).reshape(H, W), -1).astype(np.int32)[None]
    got = check_labels(hip, dev, root, 1, 254)
    assert got['n_candidates'].tolist() == [300] and got['n_components'].tolist() == [254]
    assert got['comp_root'][0].tolist() == np.flatnonzero(mask)[:254].tolist() and got['label'].max() == 254
    got = check_labels(hip, dev, root, 2, 254)
    assert got['n_candidates'].tolist() == [0] and not got['label'].any()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_without_a_launch(hip, dev):
    L = hip.lib()
    H, W = 8, 16
    d, k = _depth(np.full((1, H, W), 500), dev), _d([[50, 50, 8, 4, 1000]], np.float32, dev)
    out = [Guarded(1, 64, torch.int32, dev) for _ in range(8)]
    st = hip.stream()

    def plane(f=1, h=H, w=W, n_hyp=16, stride=1, first=0, percent=10, tol=0.01, depth=d.data_ptr()):
        return L.cloudaae_depth_plane(f, h, w, depth, k.data_ptr(), 0, first, n_hyp, stride, tol, percent, out[0].ptr(), out[1].ptr(),
                                      out[2].ptr(), out[3].ptr(), st)
    for bad in (dict(n_hyp=0), dict(n_hyp=4097), dict(stride=0), dict(h=0), dict(h=1 << 13, w=1 << 12), dict(f=-1),
                dict(f=1 << 20, h=1 << 5, w=1 << 4), dict(first=-1), dict(first=(1 << 40) + 1), dict(percent=101), dict(tol=-1.0),
                dict(tol=float('nan')), dict(depth=None)):
        assert plane(**bad) != 0, bad
    fgp = out[4].ptr()
    assert L.cloudaae_depth_foreground(1, H, W, d.data_ptr(), k.data_ptr(), out[2].ptr(), out[3].ptr(), 0.01, -1.0, fgp, st) != 0
    assert L.cloudaae_depth_foreground(1, H, W, d.data_ptr(), k.data_ptr(), None, out[3].ptr(), 0.01, 0.5, fgp, st) != 0
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device=dev)
    assert L.cloudaae_depth_components_workspace_bytes(1, 1 << 13, 1 << 12) == 0
    assert L.cloudaae_component_labels_workspace_bytes(-1, H, W) == 0
    need = int(L.cloudaae_depth_components_workspace_bytes(1, H, W))
    assert L.cloudaae_depth_components(1, H, W, d.data_ptr(), fgp, out[3].ptr(), out[5].ptr(), out[6].ptr(), ws.data_ptr(), need - 1, st) != 0
    assert L.cloudaae_depth_components(1, H, W, d.data_ptr(), None, out[3].ptr(), out[5].ptr(), out[6].ptr(), ws.data_ptr(), need, st) != 0
    need = int(L.cloudaae_component_labels_workspace_bytes(1, H, W))

    def labels(min_pixels=1, k_max=4, nbytes=need, root=out[5].ptr()):
        return L.cloudaae_component_labels(1, H, W, root, min_pixels, k_max, fgp, out[0].ptr(), out[1].ptr(), out[2].ptr(), out[3].ptr(),
                                           out[6].ptr(), ws.data_ptr(), nbytes, st)
    for bad in (dict(min_pixels=0), dict(k_max=0), dict(k_max=255), dict(nbytes=need - 1), dict(root=None)):
        assert labels(**bad) != 0, bad
    assert "cloudaae_component_labels" in hip.lib().cloudaae_last_error().decode()
    # no frame is no error: nothing is launched, nothing written
    assert plane(f=0) == 0
    assert L.cloudaae_depth_foreground(0, H, W, d.data_ptr(), k.data_ptr(), out[2].ptr(), out[3].ptr(), 0.01, 0.5, fgp, st) == 0
    assert L.cloudaae_depth_components(0, H, W, d.data_ptr(), fgp, out[3].ptr(), out[5].ptr(), out[6].ptr(), ws.data_ptr(), 1 << 16, st) == 0
    assert L.cloudaae_component_labels(0, H, W, out[5].ptr(), 1, 4, fgp, out[0].ptr(), out[1].ptr(), out[2].ptr(), out[3].ptr(),
                                       out[6].ptr(), ws.data_ptr(), 1 << 16, st) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)


# ---- utils/depth_components.py and the evaluation -------------------------------------------------------------------------------------
def scene_segments(dev):
    from cloudaae_amd.utils import depth_components as DC
    depth, _, intr = D.scene()
    return DC.segment_depth(depth, intr, jump=0.02, min_pixels=16, device=dev, **D.SCENE_PARAMS)


def test_segment_depth_equals_the_restatement(hip, dev):
    s = scene_segments(dev)
    want = D.scene_result(min_pixels=16)
    assert s.jump_units.tolist() == [D.SCENE_JUMP_UNITS]
    for k in ('label', 'root', 'fg', 'count'):
        assert np.array_equal(getattr(s, k).cpu().numpy()[0], want[k]), k
    assert int(s.plane_hyp[0]) == want['plane_hyp'] and int(s.tested[0]) == want['tested']
    assert np.array_equal(_bits(s.plane.cpu().numpy()[0]), _bits(want['plane']))
    assert s.label.dtype == torch.uint8 and s.root.dtype == torch.int32 and s.plane.dtype == torch.float64
    for k in ('n_components', 'n_candidates', 'comp_root', 'comp_size', 'comp_box'):
        assert isinstance(getattr(s, k), np.ndarray) and np.array_equal(getattr(s, k)[0], want[k]), k
    assert list(zip(s.comp_root[0, :3].tolist(), s.comp_size[0, :3].tolist())) == [(1616, 192), (1731, 72), (2696, 56)]
    # the defaults cut the two small spheres (min_pixels 200 > 192): the table is empty, and that is not an error
    from cloudaae_amd.utils import depth_components as DC
    depth, _, intr = D.scene()
    assert DC.segment_depth(depth, intr, seed=1, device=dev).n_components.tolist() == [0]


def test_match_components_equals_the_restatement(hip, dev):
    from cloudaae_amd.utils import depth_components as DC
    depth, label, _ = D.scene()
    s = scene_segments(dev)
    want = D.scene_result(min_pixels=16)
    lab = torch.from_numpy(label).to(dev)
    for value in (2, 3, 4, 5):
        k, iou = DC.match_components(s.label, lab, depth, value)
        assert (int(k[0]), float(iou[0])) == D.match(want['label'], label[0], depth[0], value), value
    assert DC.match_components(s.label, lab, depth, 5)[0].tolist() == [0]
    two = DC.match_components(torch.cat([s.label, s.label]), torch.cat([lab, lab]), np.concatenate([depth, depth]), 3)
    assert two[0].tolist() == [2, 2] and two[1].dtype == np.float64


N_POINT = 64
TARGET = 1                      # the large sphere: label value 2


@pytest.fixture(scope="module")
def scene_records(hip, dev, tmp_path_factory):
    """The table scene as a frame record file (utils/render.py's writer) and a [21,2048,6] model table."""
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import render
    tmp = tmp_path_factory.mktemp("components")
    depth, label, intr = D.scene()
    _, frames = D.scene_frames()
    poses = []
    for _, _, T in frames[0]:
        P = np.eye(4)
        P[:3, 3] = T[:3, 3]
        poses.append(P)
    payloads = render.frame_records(depth, label, intr, [poses], [[lab - 1 for _, lab, _ in frames[0]]], 48, [0])
    path = str(tmp / "0048_pcnn.tfrecord")
    tfrecord_io.write_records(path, payloads)
    one, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    models = np.repeat(one, 21, axis=0)
    assert models.shape == (21, 2048, 6)
    return dict(tmp=tmp, path=path, frames=tfrecord_io.read_frames(path, verify=True), models=models)


def test_element_from_frames_on_found_components(hip, dev, scene_records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import segment as S
    frames, models = scene_records['frames'], scene_records['models']
    depth, label, intr = D.scene()
    params = dict(jump=0.02, min_pixels=16, **D.SCENE_PARAMS)
    counts = {}
    el = E.element_from_frames(frames, TARGET, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True,
                               labels="components", components=params, counts=counts)
    assert el is not None and counts == dict(frames=1, matched=1)
    want = D.scene_result(min_pixels=16)
    k, iou = D.match(want['label'], label[0], depth[0], TARGET + 1)
    relabelled = np.where(want['label'] == k, TARGET + 1, 0).astype(np.uint8)[None]
    assert el['segment_iou'].tolist() == [iou] and iou >= 0.9
    assert np.array_equal(el['frame_label'].cpu().numpy(), relabelled) and el['frame_want'].tolist() == [TARGET + 1]
    # extract_segments fed the relabelled image directly
    r = S.extract_segments(depth, relabelled, intr, classes=[[TARGET]], num_point=N_POINT, device=dev)
    smp = S.sample_segments(r, N_POINT, seed=4)
    assert r.kept.tolist() == [True]
    assert torch.equal(el['xyz'], smp['xyz']) and torch.equal(el['xyz_inlier'], smp['xyz_inlier'])
    assert tuple(el['xyz'].shape) == (1, N_POINT, 3)
    # labels="record" is the call without the argument
    base = E.element_from_frames(frames, TARGET, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True)
    same = E.element_from_frames(frames, TARGET, N_POINT, models, seed=4, device=dev, keep_frames=True, keep_labels=True,
                                 labels="record")
    assert set(base) == set(same) and "segment_iou" not in base
    for key, v in base.items():
        assert torch.equal(v, same[key]) if isinstance(v, torch.Tensor) else np.array_equal(v, same[key]), key
    assert np.array_equal(base['frame_label'].cpu().numpy(), label)
    # a class whose pixels no component covers: the frame is dropped and counted
    gone = [dict(f) for f in frames]
    for f in gone:
        f['label'] = np.where(f['label'] == TARGET + 1, 0, f['label']).astype(np.uint8)
    counts = {}
    assert E.element_from_frames(gone, TARGET, N_POINT, models, seed=4, device=dev, labels="components", components=params,
                                 counts=counts) is None
    assert counts == dict(frames=1, matched=0)
    with pytest.raises(ValueError):
        E.element_from_frames(frames, TARGET, N_POINT, models, labels="found")
    with pytest.raises(ValueError):
        E.element_from_frames(frames, TARGET, N_POINT, models, components=params)


def test_a_frame_keeps_its_global_index_among_frames_without_the_class(hip, dev, scene_records, monkeypatch):
    """Every frame of a call is segmented, so frame i draws its hypotheses from first_frame + i whether or not the frames
    before it hold the class (on the exact table the winner is the lowest hypothesis with three table pixels: it differs
    from index to index while the labels do not)."""
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import depth_components as DC
    frames, models = scene_records['frames'], scene_records['models']
    depth, label, intr = D.scene()
    other = dict(frames[0])
    other['class_one_hot'] = np.where(np.arange(21) == TARGET, 0, other['class_one_hot'])
    seen = []
    real = DC.segment_depth

    def spy(*args, **kw):
        r = real(*args, **kw)
        seen.append((int(r.label.shape[0]), kw.get('first_frame'), r.plane_hyp.tolist()))
        return r
    monkeypatch.setattr(DC, "segment_depth", spy)
    params = dict(jump=0.02, min_pixels=16, first_frame=5, **D.SCENE_PARAMS)
    el = E.element_from_frames([other, other, frames[0]], TARGET, N_POINT, models, seed=4, device=dev, keep_labels=True,
                               labels="components", components=params)
    want = [D.plane(depth[0], intr[0], 1, 5 + i, 64, 2)['plane_hyp'] for i in range(3)]
    assert len(set(want)) > 1 and seen == [(3, 5, want)]
    assert el is not None and len(el['class_id']) == 1
    assert np.array_equal(el['frame_label'].cpu().numpy()[0] != 0, D.scene_result(min_pixels=16)['label'] == 1)


def test_command_line_prints_the_components_line(hip, dev, scene_records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    tmp, models = scene_records['tmp'], scene_records['models']
    obj = str(tmp / "obj_models.tfrecords")
    tfrecord_io.write_records(obj, [tfrecord_io.encode_example({"label": np.array([c]), "model": models[c].reshape(-1)})
                                    for c in range(TARGET + 1)])
    graph = T.TrainGraph({"num_point": N_POINT, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    capsys.readouterr()
    assert E.main(["--files", scene_records['path'], "--object_model", obj, "--trained_model", ckpt[:-len(".npz")], "--target_cls",
                   str(TARGET), "--num_point", str(N_POINT), "--batch_size", "1", "--seed", "1", "--labels", "components",
                   "--components_n_hyp", "64", "--components_stride", "2", "--components_min_pixels", "16"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln for ln in lines if ln.startswith("batch size ")] == ["batch size 1"], lines
    depth, label, _ = D.scene()
    iou = D.match(D.scene_result(min_pixels=16)['label'], label[0], depth[0], TARGET + 1)[1]
    assert lines[-1] == "components class %d frames 1 matched 1 mean_iou %f" % (TARGET, iou), lines[-3:]
