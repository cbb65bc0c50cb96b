"""GPU: cloudaae_mesh_cluster_keys, _sums, _place and _triangles against the NumPy restatement of DESIGN.md "Simplified meshes"
(tests/simplify_reference.py) from identical inputs, then utils/simplify.py end to end, its hooks in utils/fuse.py and
utils/scan.py, the three command lines, and the simplified fused cube in the tracker.

Keys, ranks, counts and triangle keys are integers: compared for equality.  A term of a sum has the same bits on both sides
(float64 on exactly widened values, un-fused, the same order of operations); only the order of a cell's additions differs, so
a sum of n terms is held to 2 n 2^-53 times the sum of the terms' absolute values, the bound "Tracking" uses for its sums.  The
placement is compared on the GPU's own sums: `how` for equality, the position within 1e-9 of the cell side and the error
within 1e-9 of the sum of its terms' absolute values -- the tolerance the project applies to a solve on equal sums."""
import numpy as np
import pytest
import torch

import detect_reference as DR
import fuse_reference as FR
import simplify_reference as SR
import track_reference as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SOLVE_TOL = 1e-9


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def simp(hip):
    from cloudaae_amd.utils import simplify
    return simplify


@pytest.fixture(scope="module")
def fuse(hip):
    from cloudaae_amd.utils import fuse
    return fuse


def up(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype).contiguous() if dtype is not None else t.to(dev).contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def gpu_renderer(meshes, frames, intr, H, W):
    from cloudaae_amd.utils import render
    return render.render_frames(meshes, frames, intr, H, W)['depth'].cpu().numpy().view(np.uint16)


# ---- keys -------------------------------------------------------------------------------------------------------------------
def check_keys(simp, dev, v, origin, cell, dims, what):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    got = host(simp.cluster_keys(up(v, dev), origin, cell, dims))
    want = SR.cluster_keys(v, origin, cell, dims)
    assert got.dtype == np.int64 and np.array_equal(got, want), what
    return want


def test_keys_equal_the_restatement(simp, dev):
    rng = np.random.default_rng(1)
    for V in (1, 63, 64, 65, 4097):
        v = rng.uniform(-1.0, 1.0, (V, 3)).astype(np.float32)                           # negative coordinates
        k = check_keys(simp, dev, v, [-1.01, -1.02, -1.03], 0.13, (16, 16, 16), V)
        assert np.all(k >= 0)
        k = check_keys(simp, dev, v, [-0.5, -0.25, 0.0], 0.125, (8, 5, 3), V)           # most vertices outside the grid
        assert (k < 0).any() or V == 1
    # vertices exactly on cell boundaries (cell and origin powers of two), on the far planes, next to them, and non-finite
    nan, inf = np.float32('nan'), np.float32('inf')
    g = np.arange(-8, 9, dtype=np.float32) * np.float32(0.125)
    edge = np.stack(np.meshgrid(g, g[::4], g[::8], indexing='ij'), axis=-1).reshape(-1, 3)
    near = np.nextafter(edge, np.float32(-4.0)).astype(np.float32)
    odd = np.array([[nan, 0.0, 0.0], [0.0, nan, 0.0], [0.0, 0.0, nan], [inf, 0.0, 0.0], [0.0, -inf, 0.0], [0.0, 0.0, inf], [nan, nan, nan],
                    [-0.0, -0.0, -0.0], [1e38, 0.0, 0.0], [-1e38, 0.0, 0.0], [1e-45, 1e-45, 1e-45]], np.float32)
    v = np.concatenate([edge, near, odd])
    k = check_keys(simp, dev, v, [-0.5, -0.5, -0.5], 0.125, (8, 8, 8), "boundaries")
    assert (k >= 0).any() and (k < 0).any()
    check_keys(simp, dev, v, [-1.0, -1.0, -1.0], 0.25, (8, 8, 8), "boundaries, every vertex inside or on the far planes")
    # a 1 x 1 x 1 grid
    k = check_keys(simp, dev, v, [-0.25, -0.25, -0.25], 0.5, (1, 1, 1), "1 x 1 x 1")
    assert set(k.tolist()) == {-1, 0}
    # n = 2^20 reached by large coordinates and a small cell: keys up to 2^60
    n = 1 << 20
    big = rng.uniform(0.0, 4096.0, (4097, 3)).astype(np.float32)
    big[:4] = [[0.0, 0.0, 0.0], [4096.0, 1.0, 1.0], np.nextafter(np.float32(4096.0), np.float32(0.0)) * np.ones(3, np.float32), [4095.99, 0.0, 4095.99]]
    k = check_keys(simp, dev, big, [0.0, 0.0, 0.0], 2.0 ** -8, (n, n, n), "2^20 cells along every axis")
    assert k[1] == -1 and k[2] == (((n - 1) * n + (n - 1)) * n + (n - 1)) and k.max() > (1 << 59)
    check_keys(simp, dev, big, [0.0, 0.0, 0.0], 2.0 ** -8, (n, 1, 1), "2^20 x 1 x 1")
    assert simp.cluster_keys(torch.zeros((0, 3), dtype=torch.float32, device=dev), [0.0, 0.0, 0.0], 1.0, (1, 1, 1)).shape == (0,)


# ---- sums -------------------------------------------------------------------------------------------------------------------
def prepared(v, t, origin, cell, dims):
    """The restatement's keys, ranks and cells of a mesh."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    keys = SR.cluster_keys(v, origin, cell, dims)
    cell_key, rank, grid = SR.cells_of(keys, dims)
    return dict(v=v, t=t, origin=np.asarray(origin, np.float64), cell=float(cell), dims=dims, keys=keys, cell_key=cell_key, rank=rank,
                grid=grid)


def gpu_sums(simp, dev, m, orders=None):
    args = () if orders is None else tuple(up(o, dev) for o in orders)
    s, c = simp.cluster_sums(up(m['v'], dev), up(m['t'], dev), up(m['rank'], dev), up(m['grid'].reshape(-1, 3), dev), m['origin'],
                             m['cell'], *args)
    return host(s), host(c)


def check_sums(simp, dev, m, what, orders=None):
    want, wcounts, mags = SR.cluster_sums(m['v'], m['t'], m['rank'], m['grid'], m['origin'], m['cell'], magnitudes=True)
    got, counts = gpu_sums(simp, dev, m, orders)
    assert counts.dtype == np.int32 and np.array_equal(counts, wcounts), what
    n = np.concatenate([np.repeat(wcounts[:, :1], 3, axis=1), np.repeat(wcounts[:, 1:], 13, axis=1)], axis=1).astype(np.float64)
    bound = 2.0 * n * U * mags
    diff = np.abs(got - want)
    worst = float((diff / np.maximum(bound, 1e-300)).max()) if len(got) else 0.0
    print("%s: %d cells, corners per cell %d..%d, largest difference %.3g of its bound" % (what, len(got), wcounts[:, 1].min() if len(got) else 0,
                                                                                             wcounts[:, 1].max() if len(got) else 0, worst))
    assert got.shape == want.shape and np.all(diff <= bound), what
    assert np.all(got[:, 13:] == 0.0), what
    return got, counts


def entries_mesh(ks=(1, 63, 64, 65, 129, 1000), seed=2):
    """Cell i along x (side 1) holds ks[i] vertices, each the first corner of one triangle whose other corners are the single
    vertices of two further cells: cells of 1, 63, 64, 65, 129 and 1000 entries in either list, and two of one vertex and
    sum(ks) corners."""
    rng = np.random.default_rng(seed)
    v, t = [], []
    a, b = sum(ks), sum(ks) + 1
    for i, k in enumerate(ks):
        first = len(v)
        v += (rng.uniform(0.05, 0.95, (k, 3)) + [i, 0.0, 0.0]).tolist()
        t += [(first + j, a, b) for j in range(k)]
    v += [[len(ks) + 0.5, 0.25, 0.75], [len(ks) + 1.25, 0.5, 0.5]]
    return prepared(v, t, [0.0, 0.0, 0.0], 1.0, (len(ks) + 2, 1, 1))


def test_sums_of_cells_with_few_and_many_entries(simp, dev):
    m = entries_mesh()
    got, counts = check_sums(simp, dev, m, "cells by entries")
    assert counts.tolist() == [[k, k] for k in (1, 63, 64, 65, 129, 1000)] + [[1, 1322], [1, 1322]]
    again, _ = gpu_sums(simp, dev, m)
    assert again.tobytes() == got.tobytes()                                             # two runs, bit for bit


def test_sums_of_the_sphere_in_one_cell_and_in_many(simp, dev):
    v, t = SR.sphere_mesh()
    assert len(t) == 7752
    m = prepared(v, t, [-4.0, -4.0, -4.0], 32.0, (1, 1, 1))
    got, counts = check_sums(simp, dev, m, "the sphere in one cell")
    assert counts.tolist() == [[len(v), 3 * 7752]]
    for cells in (2, 3, 4):
        o, dims = SR.default_grid(v, float(cells))
        check_sums(simp, dev, prepared(v, t, o, float(cells), dims), "the sphere, cell %d" % cells)


def test_sums_without_triangles_and_with_dropped_ones(simp, dev):
    v, t = SR.random_soup(seed=3)
    o, dims = SR.default_grid(v, 0.2)
    m = prepared(v, np.zeros((0, 3), np.int32), o, 0.2, dims)                            # T = 0: the vertex sums alone
    got, counts = check_sums(simp, dev, m, "T = 0")
    assert np.all(counts[:, 1] == 0) and np.all(got[:, 3:] == 0.0) and counts[:, 0].sum() == len(v)
    bad_v = v.copy()
    bad_v[::17, 1] = np.nan
    bad_v[5::29, 0] = np.inf
    bad_t = t.copy()
    bad_t[::7, 2] = -1
    bad_t[3::11, 0] = len(v)
    bad_t[4::13, 1] = len(v) + 1000
    m = prepared(bad_v, bad_t, o, 0.2, (dims[0], dims[1], dims[2] - 1))                  # and a layer of vertices outside the grid
    assert SR.dropped(m['t'], m['rank']).sum() > 200 and (m['rank'] < 0).sum() > 30
    check_sums(simp, dev, m, "dropped triangles and unused vertices")


def test_sums_skip_foreign_and_out_of_range_entries(simp, dev):
    v, t = SR.random_soup(seed=4)
    o, dims = SR.default_grid(v, 0.25)
    m = prepared(v, t, o, 0.25, dims)
    C, V, T = len(m['grid']), len(v), len(t)
    want, wcounts = gpu_sums(simp, dev, m)
    rng = np.random.default_rng(9)

    def spoiled(rank_of_item, n_items):
        """The grouped order with three more entries per cell: one out of range on either side and an item of another cell."""
        order, start = [], [0]
        for c in range(C):
            mine = np.nonzero(rank_of_item == c)[0].tolist()
            foreign = int(rng.choice(np.nonzero(rank_of_item != c)[0]))
            mine.insert(len(mine) // 2, foreign)
            order += [-1 - c] + mine + [n_items + c]
            start.append(len(order))
        return np.array(order, np.int32), np.array(start, np.int64)
    corner_rank = np.where(SR.dropped(t, m['rank'])[:, None], -1, m['rank'][np.clip(t, 0, V - 1)]).reshape(-1)
    # more entries than V or 3 T is refused; so the lists are spoiled for half of the cells only, the others are left empty
    vo, vs = spoiled(m['rank'], V)
    co, cs = spoiled(corner_rank, 3 * T)
    keep_v, keep_c = np.searchsorted(vs, V, side='right') - 1, np.searchsorted(cs, 3 * T, side='right') - 1
    keep = int(min(keep_v, keep_c))
    assert keep >= C // 2
    vs2, cs2 = np.minimum(vs, vs[keep]), np.minimum(cs, cs[keep])
    got, counts = gpu_sums(simp, dev, m, (vo[:vs[keep]], vs2, co[:cs[keep]], cs2))
    # the cells with a list: the same counts, and sums within the bound (the additions meet in another order)
    _, _, mags = SR.cluster_sums(m['v'], m['t'], m['rank'], m['grid'], m['origin'], m['cell'], magnitudes=True)
    n = np.concatenate([np.repeat(wcounts[:, :1], 3, axis=1), np.repeat(wcounts[:, 1:], 13, axis=1)], axis=1).astype(np.float64)
    assert np.array_equal(counts[:keep], wcounts[:keep])
    assert np.all(np.abs(got[:keep] - want[:keep]) <= 2.0 * n[:keep] * U * mags[:keep])
    assert np.all(counts[keep:] == 0) and np.all(got[keep:] == 0.0)
    # starts that are no prefix sum: negative, beyond the list, descending -- cut to the list, nothing read outside it
    wild_v, wild_c = vs2.copy(), cs2.copy()
    wild_v[0], wild_c[0] = -(1 << 40), -5
    wild_v[-1], wild_c[-1] = 1 << 40, 1 << 62
    wild_v[C // 2], wild_c[C // 2] = 0, 0
    got, counts = gpu_sums(simp, dev, m, (vo[:vs[keep]], wild_v, co[:cs[keep]], wild_c))
    # (cell C / 2 now ranges over every list before its own, and finds its items among the others' foreign entries)
    assert np.all(np.isfinite(got)) and np.all(counts >= 0) and counts[C // 2 - 1].tolist() == [0, 0]
    calm = np.ones(C, bool)
    calm[[C // 2 - 1, C // 2]] = False
    assert np.array_equal(counts[calm], np.where(np.arange(C)[:, None] < keep, wcounts, 0)[calm])
    assert np.all(counts[C // 2] >= (wcounts[C // 2] if C // 2 < keep else 0))


def test_sums_do_not_depend_on_what_else_is_in_the_mesh(simp, dev):
    v, t = SR.random_soup(seed=6)
    v2, t2 = SR.random_soup(seed=7, V=300, T=700)
    v2 = (v2 + np.float32([3.0, 0.0, 0.0])).astype(np.float32)                          # disjoint: its own cells
    origin, cell, dims = [-0.6, -0.6, -0.6], 0.2, (25, 6, 6)
    alone = prepared(v, t, origin, cell, dims)
    both = prepared(np.concatenate([v, v2]), np.concatenate([t, t2 + len(v)]), origin, cell, dims)
    assert not set(alone['cell_key'].tolist()) & set(SR.cluster_keys(v2, origin, cell, dims).tolist())
    a, ac = check_sums(simp, dev, alone, "a mesh alone")
    b, bc = check_sums(simp, dev, both, "the mesh with a second one appended")
    at = np.searchsorted(both['cell_key'], alone['cell_key'])
    assert np.array_equal(both['cell_key'][at], alone['cell_key']) and len(both['cell_key']) > len(alone['cell_key'])
    assert b[at].tobytes() == a.tobytes() and np.array_equal(bc[at], ac)                # bit for bit on its own cells


# ---- placement --------------------------------------------------------------------------------------------------------------
def check_place(simp, dev, sums, counts, grid, origin, cell, what, eps=SR.EPS, max_share=0.01):
    """The GPU's placement of `sums` (numpy, as the GPU's sums kernel or a test wrote them) against the restatement's."""
    C = len(grid)
    pos, how, err = simp.cluster_place(up(sums, dev), up(counts, dev), up(np.asarray(grid, np.int32).reshape(-1, 3), dev), origin, cell, eps)
    pos, how, err = host(pos), host(how), host(err)
    wpos, whow, werr, info = SR.cluster_place(sums, counts, grid, origin, cell, eps, details=True)
    skip = SR.near_a_threshold(info, cell, eps)
    share = float(skip.mean()) if C else 0.0
    z = SR.cell_centres(grid, origin, cell)
    scale = SR.error_scale(sums, wpos - z)
    ok = ~skip
    with np.errstate(all='ignore'):
        dpos = np.abs(pos - wpos)[ok].max() / cell if ok.any() else 0.0
        derr = (np.abs(err - werr)[ok] / np.maximum(scale[ok], 1e-300)).max() if ok.any() else 0.0
    print("%s: %d cells, how %s, %.2f %% near a threshold, position off by %.3g cell, error by %.3g of its scale"
          % (what, C, np.bincount(whow, minlength=8).tolist(), 100 * share, dpos, derr))
    assert how.dtype == np.uint8 and pos.dtype == np.float64 and err.dtype == np.float64
    assert share <= max_share, what
    assert np.array_equal(how[ok], whow[ok]), what
    assert np.all(np.abs(pos - wpos)[ok] <= SOLVE_TOL * cell), what
    finite = np.isfinite(werr)                                                          # (sums of NaN or infinity: no figure to compare)
    assert np.array_equal(np.isfinite(err), finite), what
    with np.errstate(invalid='ignore'):
        assert np.all(np.abs(err - werr)[ok & finite] <= SOLVE_TOL * scale[ok & finite]), what
    return pos, how, err


def test_placement_on_the_gpus_own_sums(simp, dev):
    v, t = SR.sphere_mesh()
    cube = FR.scene('cube', 0.004)
    soup = SR.random_soup(seed=8)
    for name, (mv, mt), cell in [("sphere, cell 2", (v, t), 2.0), ("sphere, cell 3", (v, t), 3.0), ("sphere, cell 4", (v, t), 4.0),
                                 ("cube, cell 4 voxels", (cube['vertices'], cube['triangles']), 0.016),
                                 ("cube, cell 3 voxels", (cube['vertices'], cube['triangles']), 0.012),
                                 ("soup, cell 0.07", soup, 0.07), ("soup, cell 0.2", soup, 0.2), ("soup, cell 3", soup, 3.0)]:
        o, dims = SR.default_grid(mv, cell)
        m = prepared(mv, mt, o, cell, dims)
        sums, counts = gpu_sums(simp, dev, m)
        check_place(simp, dev, sums, counts, m['grid'], o, cell, name)
        check_place(simp, dev, sums, counts, m['grid'], o, cell, name + ", eps 0.05", eps=0.05)


def test_placement_of_the_hand_cases(simp, dev):
    for name, c in SR.hand_cases():
        m = prepared(c['vertices'], c['triangles'], SR.HAND_ORIGIN, SR.HAND_CELL, SR.HAND_DIMS)
        sums, counts = gpu_sums(simp, dev, m)
        pos, how, err = check_place(simp, dev, sums, counts, m['grid'], SR.HAND_ORIGIN, SR.HAND_CELL, name, max_share=1.0)
        # dyadic numbers throughout: the sums are exact in any order, and so is the closed form -- also where the apex sits
        # exactly at +c/2, which the threshold rule would otherwise leave out
        assert how.tolist() == [c['how']] and np.array_equal(pos[0], c['pos']), name
        assert (err[0] == 0.0) == (c['how'] < 4), name


def test_sums_that_give_no_quadric(simp, dev):
    grid, counts = np.zeros((5, 3), np.int32), np.full((5, 2), 2, np.int32)
    grid[:, 0] = np.arange(5)
    sums = np.zeros((5, 16))
    sums[:, :3] = [0.25, -0.5, 0.125]
    sums[1, SR.A0] = np.nan
    sums[2, [SR.A0, SR.A0 + 3, SR.A0 + 5]] = -1.0, -2.0, -3.0                           # negative definite
    sums[3, [SR.A0, SR.A0 + 1]] = np.inf, 1.0
    sums[4, [SR.A0, SR.A0 + 1, SR.A0 + 3]] = -2.0, 1.0, -2.0                            # negative definite, with a rotation
    pos, how, err = check_place(simp, dev, sums, counts, grid, [0.0, 0.0, 0.0], 1.0, "no quadric")
    assert how.tolist() == [4] * 5
    assert np.array_equal(pos, np.array([0.625, 0.25, 0.5625]) + np.stack([np.arange(5.0), np.zeros(5), np.zeros(5)], axis=1))
    p, h, e = simp.cluster_place(torch.zeros((0, 16), dtype=torch.float64, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev),
                                 torch.zeros((0, 3), dtype=torch.int32, device=dev), [0.0, 0.0, 0.0], 1.0)
    assert p.shape == (0, 3) and h.shape == (0,) and e.shape == (0,)


# ---- triangle keys ----------------------------------------------------------------------------------------------------------
def test_triangle_keys_equal_the_restatement(simp, dev):
    rng = np.random.default_rng(12)
    C = 1 << 21
    V = 2997
    rank = rng.integers(0, C, V).astype(np.int32)
    rank[::9] = -1
    rank[1::9] = C - 1
    rank[2::9] = rank[3::9][:len(rank[2::9])]                                           # equal ranks nearby
    rank[4::27] = 0
    for T in (1, 63, 64, 65, 5000):
        t = rng.integers(0, V, (T, 3)).astype(np.int32)
        near = rng.integers(0, V - 12, T)
        t[::2] = np.stack([near, near + rng.integers(0, 12, T), near + rng.integers(0, 12, T)], axis=1)[::2]   # all collapse kinds
        t[5::31, 0] = -1
        t[6::37, 1] = V
        t[7::41, 2] = np.iinfo(np.int32).min
        t[8::43, 2] = np.iinfo(np.int32).max
        for c, r in ((C, rank), (1000, rank), (C, np.minimum(rank, 40))):               # ranks >= C count as unused
            got = host(simp.cluster_triangles(up(t, dev), up(r, dev), c))
            want = SR.triangle_keys(t, r, c)
            assert got.dtype == np.int64 and np.array_equal(got, want), (T, c)
        if T == 5000:
            k = SR.triangle_keys(t, rank, C)
            assert (k < 0).sum() > 500 and (k >= 0).sum() > 500 and k.max() >= (C - 1) << 21
    assert simp.cluster_triangles(torch.zeros((0, 3), dtype=torch.int32, device=dev), up(rank, dev), C).shape == (0,)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def same_mesh(got_v, got_t, v, t, cell, what, placement='quadric'):
    """(got_v, got_t): device tensors of simplify_mesh against the restatement run on the same input."""
    wv, wt, info = SR.simplify(v, t, cell, placement=placement, return_info=True)
    gv, gt = host(got_v), host(got_t)
    assert gv.dtype == np.float32 and gt.dtype == np.int32, what
    assert gt.shape == wt.shape and np.array_equal(gt, wt), what                        # as integers
    assert gv.shape == wv.shape, what
    # the sums differ by their order of additions, so a cell near a threshold may be decided the other way: left out
    used = info['cell_to_vertex'] >= 0
    skip = SR.near_a_threshold(info['details'], cell)[used] if placement == 'quadric' else np.zeros(len(wv), bool)
    assert skip.mean() <= 0.01, what
    # float64 positions within the solve's tolerance, then each rounded once to float32
    tol = SOLVE_TOL * cell + np.spacing(np.abs(wv))
    assert np.all((np.abs(gv.astype(np.float64) - wv.astype(np.float64)) <= tol)[~skip]), what
    return wv, wt


@pytest.fixture(scope="module")
def cube(fuse, dev):
    """The cube scene with its depth from the GPU renderer, fused on the GPU."""
    s = FR.scene_inputs('cube', 0.004, gpu_renderer)
    vol = fuse.Volume(s['origin'], s['voxel'], s['dims'], dev)
    fuse.integrate(vol, s['depth'], s['intr'], s['poses'])
    v, t = fuse.extract_mesh(vol)
    return dict(inputs=s, volume=vol, v=v, t=t)


def test_simplify_mesh_equals_the_restatement(simp, fuse, dev, cube):
    sv, st = SR.sphere_mesh()
    p = FR.scene_inputs('prism', 0.0025, gpu_renderer)
    pv, pt, _ = fuse.fuse_frames(p['depth'], None, p['intr'], p['poses'], None, 0.0025, aabb=p['aabb'])
    for name, v, t, cells in [("sphere, cell 2", sv, st, (2.0, 3.0, 4.0)), ("cube at 4 mm", cube['v'], cube['t'], (0.012, 0.016)),
                              ("prism at 2.5 mm", pv, pt, (0.01,))]:
        hv, ht = (host(v), host(t)) if isinstance(v, torch.Tensor) else (v, t)
        for cell in cells:
            for placement in ('quadric', 'mean'):
                got_v, got_t = simp.simplify_mesh(v, t, cell, placement=placement)       # device tensors, or NumPy arrays
                wv, wt = same_mesh(got_v, got_t, hv, ht, cell, (name, cell, placement), placement)
                assert got_v.is_cuda and got_t.is_cuda
            m = FR.mesh_stats(host(got_v), host(got_t))
            print("%s, cell %g: %d -> %d triangles, Euler %d" % (name, cell, len(ht), m['T'], m['euler']))
            assert m['boundary'] == 0 and m['components'] == 1 and m['euler'] == 2
    # return_info: how and err per cell, the vertex of every cell, the map from input to output vertices
    v, t = cube['v'], cube['t']
    ov, ot, info = simp.simplify_mesh(v, t, 0.016, return_info=True)
    wv, wt, winfo = SR.simplify(host(v), host(t), 0.016, return_info=True)
    assert np.array_equal(host(info['how']), winfo['how']) and np.array_equal(host(info['map']), winfo['map'])
    assert np.array_equal(host(info['cell_vertex']), winfo['cell_to_vertex'])
    assert np.all(np.abs(host(info['pos']) - winfo['pos']) <= SOLVE_TOL * 0.016)
    assert info['dims'] == winfo['dims'] and np.array_equal(info['origin'], winfo['origin'])
    again = simp.simplify_mesh(v, t, 0.016)
    assert host(again[0]).tobytes() == host(ov).tobytes() and np.array_equal(host(again[1]), host(ot))   # two runs, bit for bit
    # an origin of the caller's; a mesh that collapses entirely; no finite vertex; no vertex at all
    got = simp.simplify_mesh(v, t, 0.016, origin=[-0.02, -0.03, -0.011])
    wv, wt = SR.simplify(host(v), host(t), 0.016, origin=[-0.02, -0.03, -0.011])
    assert np.array_equal(host(got[1]), wt) and np.all(np.abs(host(got[0]).astype(np.float64) - wv) <= SOLVE_TOL * 0.016 + np.spacing(np.abs(wv)))
    for vv, tt in ((v, t), (torch.full_like(v, float('nan')), t), (v[:0], t[:0]), (v[:0], t)):
        e = simp.simplify_mesh(vv, tt, 1.0, return_info=True)
        assert e[0].shape == (0, 3) and e[0].dtype == torch.float32 and e[1].shape == (0, 3) and e[1].dtype == torch.int32
        assert int((e[2]['map'] >= 0).sum()) == 0 and e[2]['map'].shape == (vv.shape[0],)
    for bad in (dict(cell=0.0), dict(cell=float('nan')), dict(cell=0.016, eps=0.0), dict(cell=0.016, placement='median'), dict(cell=1e-9)):
        with pytest.raises(ValueError):
            simp.simplify_mesh(v, t, **bad)


def test_hooks_in_fuse_and_scan(simp, fuse, dev, cube):
    from cloudaae_amd.utils import scan
    s, vol = cube['inputs'], cube['volume']
    ref = FR.scene('cube', 0.004)

    def same(a, b):
        return host(a[0]).tobytes() == host(b[0]).tobytes() and host(a[1]).tobytes() == host(b[1]).tobytes() and a[0].shape == b[0].shape
    # simplify=None: today's mesh bit for bit
    v, t = fuse.extract_mesh(vol, simplify=None)
    assert host(v).tobytes() == ref['vertices'].tobytes() and np.array_equal(host(t), ref['triangles'])
    assert same((v, t), fuse.extract_mesh(vol)) and same((v, t), fuse.extract_mesh(vol, 1, None))
    want = simp.simplify_mesh(v, t, 0.016)
    assert int(want[1].shape[0]) == 192
    assert same(fuse.extract_mesh(vol, simplify=0.016), want)
    fv, ft, fvol = fuse.fuse_frames(s['depth'], None, s['intr'], s['poses'], None, 0.004, aabb=s['aabb'], simplify=0.016)
    assert same((fv, ft), want) and np.array_equal(host(fvol.state), host(vol.state))
    fv, ft, _ = fuse.fuse_frames(s['depth'], None, s['intr'], s['poses'], None, 0.004, aabb=s['aabb'])
    assert same((fv, ft), (v, t))
    sc = scan.Scan()
    sc.volume, sc.min_count = vol, 1
    assert same(sc.mesh(), (v, t)) and same(sc.mesh(simplify=None), (v, t)) and same(sc.mesh(simplify=0.016), want)
    assert same(sc.mesh(0.012), simp.simplify_mesh(v, t, 0.012))


def test_ply_round_trip_pack_and_render(simp, dev, cube, tmp_path):
    from cloudaae_amd.utils import mesh_models, render
    v, t = simp.simplify_mesh(cube['v'], cube['t'], 0.016)
    path = str(tmp_path / "cube_simplified.ply")
    mesh_models.write_ply(path, v, t)
    rv, rt, rc = mesh_models.read_ply(path)
    assert rc is None and rv.tobytes() == host(v).tobytes() and np.array_equal(rt, host(t))
    p = mesh_models.pack_meshes([(v, t), (cube['v'], cube['t'])], device=dev)
    assert [int(n) for n in p.num_triangles] == [192, int(cube['t'].shape[0])]
    s = cube['inputs']
    frames = [[(0, 1, T)] for T in s['poses']] + [[(1, 1, T)] for T in s['poses']]
    out = render.render_frames(p, frames, np.tile(s['intr'], (2, 1)), FR.SCENE_H, FR.SCENE_W)
    d = host(out['depth']).view(np.uint16).astype(np.int64)
    assert int(out['dropped'].sum()) == 0
    small, full = d[:14], d[14:]
    both = (small != 0) & (full != 0)
    # The two silhouettes agree but for their rims.  Inside them both surfaces lie within 0.8 and 0.7 voxel of the cube's
    # faces along the normal (tests/test_fuse_host.py, tests/test_simplify_host.py), so 1.5 voxel apart; a ray of the eight
    # diagonal views meets a face at cos = 1 / sqrt(3), which stretches that to 2.6 voxels = 104 depth units (factor_depth
    # 10000, 4 mm voxels).  A ray that grazes a rounded edge is not bound by this: 1 % of the pixels are left to them.
    assert both.sum() > 0.97 * (full != 0).sum() and both.sum() > 0.97 * (small != 0).sum()
    apart = np.abs(small - full)[both]
    print("simplified against full: %d of %d pixels shared, depth difference: 99th percentile %d, largest %d units"
          % (both.sum(), (full != 0).sum(), np.percentile(apart, 99), apart.max()))
    assert np.percentile(apart, 99) <= 104


def test_command_lines(simp, fuse, cube, tmp_path, capsys):
    import scan_reference as S
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import mesh_models, render, scan
    s = cube['inputs']
    n = len(s['poses'])
    label = (s['depth'] != 0).astype(np.uint8) * 4                                      # class 3
    path = str(tmp_path / "0007_pcnn.tfrecord")
    tfrecord_io.write_records(path, render.frame_records(s['depth'], label, s['intr'], [[T] for T in s['poses']], [[3]] * n, 7, list(range(n))))
    full, small, again = (str(tmp_path / f) for f in ("full.ply", "small.ply", "again.ply"))
    assert fuse.main(["--files", path, "--target_cls", "3", "--voxel", "0.004", "--out", full]) == 0
    assert fuse.main(["--files", path, "--target_cls", "3", "--voxel", "0.004", "--out", small, "--simplify", "0.016"]) == 0
    capsys.readouterr()
    assert simp.main(["--in", full, "--out", again, "--cell", "0.016"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    fv, ft, _ = mesh_models.read_ply(full)
    sv, st, _ = mesh_models.read_ply(small)
    av, at, _ = mesh_models.read_ply(again)
    assert 100 < len(st) < len(ft) // 50
    assert av.tobytes() == sv.tobytes() and np.array_equal(at, st)                      # the hook and the tool: one mesh
    before, after = lines[-2].split(), lines[-1].split()
    assert (int(before[0]), int(before[2])) == (len(fv), len(ft)) and (int(after[0]), int(after[2])) == (len(sv), len(st))
    assert before[4:6] == ["0", "boundary"] and after[4:6] == ["0", "boundary"] and after[7:9] == ["1", "components"]
    # --scale: millimetres in, metres out
    mm = str(tmp_path / "mm.ply")
    mesh_models.write_ply(mm, (fv.astype(np.float64) * 1000.0).astype(np.float32), ft)
    assert simp.main(["--in", mm, "--out", again, "--cell", "0.016", "--scale", "0.001"]) == 0
    capsys.readouterr()
    assert len(mesh_models.read_ply(again)[1]) > 100
    # the scanner's command line on an orbit of the cube
    o = S.orbit()
    k = 4
    depth, truth = o['depth'][:k], o['truth'][:k]
    rec = str(tmp_path / "0008_pcnn.tfrecord")
    tfrecord_io.write_records(rec, render.frame_records(depth, (depth != 0).astype(np.uint8) * 4, np.tile(FR.SCENE_INTR, (k, 1)),
                                                        [[T] for T in truth], [[3]] * k, 8, list(range(k))))
    assert scan.main(["--files", rec, "--target_cls", "3", "--voxel", "0.004", "--out", full]) == 0
    assert scan.main(["--files", rec, "--target_cls", "3", "--voxel", "0.004", "--out", small, "--simplify", "0.016"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    fv, ft, _ = mesh_models.read_ply(full)
    sv, st, _ = mesh_models.read_ply(small)
    wv, wt = simp.simplify_mesh(fv, ft, 0.016)
    assert host(wv).tobytes() == sv.tobytes() and np.array_equal(host(wt), st) and 0 < len(st) < len(ft) // 20
    w = lines[-1].split()
    assert (int(w[0]), int(w[2])) == (len(sv), len(st))


# ---- in the tracker ---------------------------------------------------------------------------------------------------------
def test_simplified_fused_cube_tracks_like_the_restatement(simp, dev, cube):
    """The simplified fused cube (4 mm voxels, cells of 4 voxels, 192 triangles) in the CAD cube's place in align_poses, on the
    frame and the start tests/test_44_fuse_gpu.py uses for the unsimplified one.  Measured: the restatement's loop ends
    6.8e-3 from the truth with this mesh (6.5e-3 with the unsimplified one, 4.6e-5 with the CAD cube), and the GPU's at the
    same 6.8e-3; the figures are printed, and the GPU loop must end within 1e-3 of the restatement's, the existing test's
    margin."""
    from cloudaae_amd.utils import mesh_models, track
    v, t = simp.simplify_mesh(cube['v'], cube['t'], 0.016)
    small = ((host(v) - np.float32(0.035)).astype(np.float32), host(t))
    meshes = list(DR.scene_meshes())
    meshes[TR.CUBE] = small
    depth, truth = TR.frames(TR.SLOW)
    start = TR.off_pose(truth[0])
    want = TR.align(depth[:1], TR.SCENE_INTR, meshes, [TR.CUBE], [0], start[None])
    ref_err = TR.pose_error(want['poses'][-1, 0], truth[0])
    a = track.align_poses(depth[:1], TR.SCENE_INTR, mesh_models.pack_meshes(meshes, device=dev), [TR.CUBE], [0], start[None])
    got_err = TR.pose_error(a['poses'].cpu().numpy()[0], truth[0])
    print("simplified fused cube, frame 0: the restatement's loop ends %.3g from the truth, the GPU's %.3g" % (ref_err, got_err))
    assert np.all(want['status'] == 0) and int(a['status'][0]) == 0
    assert abs(got_err - ref_err) <= 1e-3


# ---- error returns ----------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(hip, dev):
    L = hip.lib()
    d = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    inf, nan = float('inf'), float('nan')
    too_many = ((1 << 31) - 1) // 3 + 1
    top = 1 << 20

    def keys(V=4, v=p, o=0.0, cell=1.0, nx=2, ny=2, nz=2, key=p):
        return L.cloudaae_mesh_cluster_keys(V, v, o, o, o, cell, nx, ny, nz, key, hip.stream())
    for kw in (dict(V=-1), dict(V=too_many), dict(v=None), dict(key=None), dict(o=nan), dict(o=inf), dict(cell=0.0), dict(cell=-1.0),
               dict(cell=nan), dict(cell=inf), dict(nx=0), dict(ny=0), dict(nz=-3), dict(nx=top + 1), dict(ny=top + 1), dict(nz=top + 1)):
        assert keys(**kw) != 0, kw
        assert b"cloudaae_mesh_cluster_keys" in L.cloudaae_last_error(), kw

    def sums(V=4, T=2, v=p, t=p, C=2, rank=p, grid=p, o=0.0, cell=1.0, vo=p, nvo=4, vs=p, co=p, nco=6, cs=p, out=p, counts=p):
        return L.cloudaae_mesh_cluster_sums(V, T, v, t, C, rank, grid, o, o, o, cell, vo, nvo, vs, co, nco, cs, out, counts, hip.stream())
    for kw in (dict(V=-1), dict(T=-1), dict(V=too_many), dict(T=too_many), dict(C=-1), dict(C=(1 << 21) + 1), dict(o=nan), dict(cell=0.0),
               dict(cell=nan), dict(cell=inf), dict(nvo=-1), dict(nvo=5), dict(nco=-1), dict(nco=7), dict(v=None), dict(t=None),
               dict(rank=None), dict(grid=None), dict(vo=None), dict(vs=None), dict(co=None), dict(cs=None), dict(out=None),
               dict(counts=None)):
        assert sums(**kw) != 0, kw
        assert b"cloudaae_mesh_cluster_sums" in L.cloudaae_last_error(), kw

    def place(C=2, s=p, counts=p, grid=p, o=0.0, cell=1.0, eps=1e-3, pos=p, how=p, err=p):
        return L.cloudaae_mesh_cluster_place(C, s, counts, grid, o, o, o, cell, eps, pos, how, err, hip.stream())
    for kw in (dict(C=-1), dict(C=(1 << 21) + 1), dict(o=inf), dict(cell=0.0), dict(cell=nan), dict(eps=0.0), dict(eps=-1.0), dict(eps=nan),
               dict(eps=inf), dict(s=None), dict(counts=None), dict(grid=None), dict(pos=None), dict(how=None), dict(err=None)):
        assert place(**kw) != 0, kw
        assert b"cloudaae_mesh_cluster_place" in L.cloudaae_last_error(), kw

    def tris(V=4, T=2, t=p, rank=p, C=2, key=p):
        return L.cloudaae_mesh_cluster_triangles(V, T, t, rank, C, key, hip.stream())
    for kw in (dict(V=-1), dict(T=-1), dict(V=too_many), dict(T=too_many), dict(C=-1), dict(C=(1 << 21) + 1), dict(t=None), dict(rank=None),
               dict(key=None)):
        assert tris(**kw) != 0, kw
        assert b"cloudaae_mesh_cluster_triangles" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0                                                      # the outputs untouched
    # nothing to do is no error
    assert keys(V=0, v=None, key=None) == 0 and sums(C=0, out=None, counts=None) == 0 and place(C=0, pos=None) == 0 and tris(T=0, key=None) == 0
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0
