"""NumPy restatement of DESIGN.md, "Simplified meshes": uniform vertex clustering with quadric-error placement.  Written
from the definition.  Keys, ranks, counts and triangle keys are integers and are expected to equal the kernels' exactly; the
terms of the sums are float64 on exactly widened float32 values, un-fused, in the order the definition writes them (NumPy does
not fuse a product into a sum), so a term has the kernels' bits and only the order of a cell's additions differs; the
placement is the definition's cyclic Jacobi routine, vectorised over the cells.

    o, dims = default_grid(vertices, cell)
    v, t = simplify(vertices, triangles, cell)                       # float32 [V',3], int32 [T',3]
"""
import numpy as np

MAX_DIM = 1 << 20
MAX_CELLS = 1 << 21
RANK_BITS = 21
SWEEPS = 8
EPS = 1e-3
# the layout of a cell's 16 sums: m [0:3], A (xx, xy, xz, yy, yz, zz) [3:9], b [9:12], e [12], zeros [13:16]
M0, A0, B0, E0 = 0, 3, 9, 12
A_INDEX = ((0, 1, 2), (1, 3, 4), (2, 4, 5))                      # A_INDEX[i][j]: where A_ij sits among the six


# ---- the grid ---------------------------------------------------------------------------------------------------------------
def default_grid(vertices, cell):
    """(origin [3] float64, dims (nx, ny, nz)): the finite vertices' lower corner - cell / 4 and the smallest dims that hold
    the upper corner; None when no vertex is finite."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return None
    c = float(cell)
    o = p.min(axis=0) - c / 4.0
    return o, dims_for(p.max(axis=0), o, c)


def dims_for(upper, origin, cell):
    return tuple(int(n) for n in np.floor((np.asarray(upper, np.float64) - origin) / float(cell)).astype(np.int64) + 1)


def cluster_keys(vertices, origin, cell, dims):
    """key [V] int64: (g_z n_y + g_y) n_x + g_x with g_a = floor((p_a - o_a) / c), or -1 for a vertex that is not finite or
    lies outside the grid (the comparison in float64, before any conversion)."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    o, c = np.asarray(origin, np.float64).reshape(3), float(cell)
    n = np.array([int(d) for d in dims], np.float64)
    assert c > 0 and np.isfinite(c) and np.all(n >= 1) and np.all(n <= MAX_DIM)
    with np.errstate(invalid='ignore', over='ignore'):
        g = np.floor((p - o) / c)
        ok = ((g >= 0.0) & (g < n)).all(axis=1)                                      # NaN and inf fail
    gi = np.where(ok[:, None], g, 0.0).astype(np.int64)
    key = (gi[:, 2] * int(dims[1]) + gi[:, 1]) * int(dims[0]) + gi[:, 0]
    return np.where(ok, key, -1).astype(np.int64)


def cells_of(keys, dims):
    """-> (cell_key [C] ascending, rank [V] int32 with -1 for unused, cell_grid [C,3] int32: g_x, g_y, g_z)."""
    keys = np.asarray(keys, np.int64)
    cell_key, inverse = np.unique(keys[keys >= 0], return_inverse=True)
    assert len(cell_key) <= MAX_CELLS
    rank = np.full(len(keys), -1, np.int32)
    rank[keys >= 0] = inverse.astype(np.int32)
    nx, ny = int(dims[0]), int(dims[1])
    grid = np.stack([cell_key % nx, (cell_key // nx) % ny, cell_key // (nx * ny)], axis=1).astype(np.int32)
    return cell_key, rank, grid.reshape(-1, 3)


def cell_centres(cell_grid, origin, cell):
    """z = o + (g + 0.5) c, float64 [C,3]."""
    return np.asarray(origin, np.float64).reshape(1, 3) + (np.asarray(cell_grid).astype(np.float64) + 0.5) * float(cell)


def dropped(triangles, rank):
    """[T] bool: an index outside [0, V) or a corner that is unused."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(rank)
    inside = ((t >= 0) & (t < V)).all(axis=1)
    r = np.asarray(rank, np.int64)[np.clip(t, 0, max(V - 1, 0))] if V else np.full(t.shape, -1, np.int64)
    return ~(inside & (r >= 0).all(axis=1))


# ---- the sums ---------------------------------------------------------------------------------------------------------------
def corner_terms(vertices, triangles, rank, cell_grid, origin, cell):
    """The corners (t, k) of the triangles that are not dropped -> (cell [N] rank of the corner's vertex, terms [N,10]: the six
    of n n^T, the three of n d, d d), in the order t, k."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    t = t[~dropped(t, rank)]
    r = np.asarray(rank, np.int64)
    z = cell_centres(cell_grid, origin, cell)
    cells, terms = [], []
    for k in range(3):
        c = r[t[:, k]]
        zc = z[c]
        q0, q1, q2 = p[t[:, 0]] - zc, p[t[:, 1]] - zc, p[t[:, 2]] - zc
        u, w = q1 - q0, q2 - q0
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        d = -((n[:, 0] * q0[:, 0] + n[:, 1] * q0[:, 1]) + n[:, 2] * q0[:, 2])
        cols = [n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                n[:, 0] * d, n[:, 1] * d, n[:, 2] * d, d * d]
        cells.append(c)
        terms.append(np.stack(cols, axis=1))
    if len(t) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 10))
    cells, terms = np.stack(cells, axis=1).reshape(-1), np.stack(terms, axis=1).reshape(-1, 10)
    return cells, terms


def cluster_sums(vertices, triangles, rank, cell_grid, origin, cell, magnitudes=False):
    """-> (sums [C,16] float64, counts [C,2] int32: n_v, n_c); with magnitudes also the sums of the terms' absolute values
    [C,16], which the bound of a comparison is stated in."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    r = np.asarray(rank, np.int64)
    C = len(cell_grid)
    z = cell_centres(cell_grid, origin, cell)
    used = r >= 0
    q = p[used] - z[r[used]]
    cells, terms = corner_terms(vertices, triangles, rank, cell_grid, origin, cell)
    sums, mags = np.zeros((C, 16)), np.zeros((C, 16))
    for a in range(3):
        sums[:, M0 + a] = np.bincount(r[used], weights=q[:, a], minlength=C)
        mags[:, M0 + a] = np.bincount(r[used], weights=np.abs(q[:, a]), minlength=C)
    for j in range(10):
        sums[:, A0 + j] = np.bincount(cells, weights=terms[:, j], minlength=C)
        mags[:, A0 + j] = np.bincount(cells, weights=np.abs(terms[:, j]), minlength=C)
    counts = np.stack([np.bincount(r[used], minlength=C), np.bincount(cells, minlength=C)], axis=1).astype(np.int32)
    return (sums, counts, mags) if magnitudes else (sums, counts)


# ---- the placement ----------------------------------------------------------------------------------------------------------
def jacobi(a6):
    """Cyclic Jacobi on symmetric 3 x 3 matrices a6 [C,6] (xx, xy, xz, yy, yz, zz): SWEEPS sweeps of the rotations (0,1), (0,2),
    (1,2).  A rotation of (p, q): nothing when a_pq == 0; else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| +
    sqrt(theta theta + 1)) (sign(0) = 1), c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0; for the third
    index r: (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq); for every row r of V, which starts as the identity: (v_rp, v_rq)
    = (c v_rp - s v_rq, s v_rp + c v_rq).  -> (lam [C,3]: the diagonal, V [C,3,3]: eigenvector i is V[:, :, i])."""
    a6 = np.asarray(a6, np.float64).reshape(-1, 6)
    C = len(a6)
    a = np.zeros((C, 3, 3))
    for i in range(3):
        for j in range(3):
            a[:, i, j] = a6[:, A_INDEX[i][j]]
    v = np.tile(np.eye(3), (C, 1, 1))
    with np.errstate(all='ignore'):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[:, p, q].copy()
                live = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(live, t, 0.0)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                a[:, p, p] = np.where(live, a[:, p, p] - t * apq, a[:, p, p])
                a[:, q, q] = np.where(live, a[:, q, q] + t * apq, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(live, 0.0, apq)
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, r, p] = a[:, p, r] = np.where(live, c * arp - s * arq, arp)
                a[:, r, q] = a[:, q, r] = np.where(live, s * arp + c * arq, arq)
                vp, vq = v[:, :, p].copy(), v[:, :, q].copy()
                v[:, :, p] = np.where(live[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                v[:, :, q] = np.where(live[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def quadric_error(sums, x):
    """E(x) = x^T A x + 2 b.x + e: ((A x).x + 2 (b.x)) + e, every dot product (t0 + t1) + t2."""
    s = np.asarray(sums, np.float64).reshape(-1, 16)
    A = [[s[:, A0 + A_INDEX[i][j]] for j in range(3)] for i in range(3)]
    with np.errstate(all='ignore'):
        ax = [(A[i][0] * x[:, 0] + A[i][1] * x[:, 1]) + A[i][2] * x[:, 2] for i in range(3)]
        xax = (ax[0] * x[:, 0] + ax[1] * x[:, 1]) + ax[2] * x[:, 2]
        bx = (s[:, B0] * x[:, 0] + s[:, B0 + 1] * x[:, 1]) + s[:, B0 + 2] * x[:, 2]
        return (xax + 2.0 * bx) + s[:, E0]


def error_scale(sums, x):
    """The sum of the absolute values of E(x)'s terms: what a tolerance on E is stated in."""
    s = np.abs(np.asarray(sums, np.float64).reshape(-1, 16))
    ax = np.abs(x)
    with np.errstate(all='ignore'):
        out = s[:, E0] + 2.0 * (s[:, B0:B0 + 3] * ax).sum(axis=1)
        for i in range(3):
            for j in range(3):
                out = out + s[:, A0 + A_INDEX[i][j]] * ax[:, i] * ax[:, j]
    return out


def cluster_place(sums, counts, cell_grid, origin, cell, eps=EPS, placement='quadric', details=False):
    """-> (pos [C,3] float64, how [C] uint8, err [C] float64).  how: the number of kept eigenvalues; 4: no usable quadric, the
    mean; + 4: the quadric's point left the cell (or is not finite), the mean.  placement='mean' takes the mean everywhere with
    how = 4.  details: also dict(ratio [C,3]: lam_i / lam_max, x [C,3]: the quadric's point before the cell test)."""
    s = np.asarray(sums, np.float64).reshape(-1, 16)
    n_v = np.asarray(counts).reshape(-1, 2)[:, 0].astype(np.float64)
    c = float(cell)
    z = cell_centres(cell_grid, origin, c)
    with np.errstate(all='ignore'):
        mean = s[:, M0:M0 + 3] / n_v[:, None]
        lam, v = jacobi(s[:, A0:A0 + 6])
        lmax = np.where(lam[:, 1] > lam[:, 0], lam[:, 1], lam[:, 0])
        lmax = np.where(lam[:, 2] > lmax, lam[:, 2], lmax)
        usable = np.isfinite(lam).all(axis=1) & (lmax > 0.0)
        if placement == 'mean':
            usable = np.zeros(len(s), bool)
        A = [[s[:, A0 + A_INDEX[i][j]] for j in range(3)] for i in range(3)]
        r = np.stack([-s[:, B0 + i] - ((A[i][0] * mean[:, 0] + A[i][1] * mean[:, 1]) + A[i][2] * mean[:, 2]) for i in range(3)], axis=1)
        x = mean.copy()
        how = np.zeros(len(s), np.int64)
        for i in range(3):
            keep = usable & (lam[:, i] > eps * lmax)
            coef = ((v[:, 0, i] * r[:, 0] + v[:, 1, i] * r[:, 1]) + v[:, 2, i] * r[:, 2]) / lam[:, i]
            x = np.where(keep[:, None], x + v[:, :, i] * coef[:, None], x)
            how += keep
        xq = x.copy()
        how = np.where(usable, how, 4)
        outside = usable & ~(np.abs(x) <= c / 2.0).all(axis=1)                       # a NaN is outside
        x = np.where(outside[:, None], mean, x)
        how = np.where(outside, how + 4, how)
        pos = z + x
        err = quadric_error(s, x)
        ratio = lam / lmax[:, None]
    if details:
        return pos, how.astype(np.uint8), err, dict(ratio=ratio, x=xq, mean=mean, usable=usable)
    return pos, how.astype(np.uint8), err


def near_a_threshold(info, cell, eps=EPS, rel=1e-6):
    """[C] bool: cells whose decision another rounding could turn -- an eigenvalue ratio within a factor 1 +- rel of eps, or a
    coordinate of the quadric's point within rel c of +-c / 2."""
    with np.errstate(all='ignore'):
        ratio = np.abs(info['ratio'] / eps - 1.0) <= rel
        edge = np.abs(np.abs(info['x']) - float(cell) / 2.0) <= rel * float(cell)
    return info['usable'] & (ratio.any(axis=1) | edge.any(axis=1))


# ---- the triangles ----------------------------------------------------------------------------------------------------------
def triangle_keys(triangles, rank, C):
    """tri_key [T] int64: -1 for a dropped triangle, a rank outside [0, C) or two equal ranks; else the ranks rotated so that the
    smallest comes first, packed as (r_a 2^21 + r_b) 2^21 + r_c."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    rk = np.asarray(rank, np.int64)
    V = len(rk)
    bad = dropped(t, rk)
    r = rk[np.clip(t, 0, max(V - 1, 0))] if V else np.zeros(t.shape, np.int64)
    bad |= ((r < 0) | (r >= int(C))).any(axis=1)
    bad |= (r[:, 0] == r[:, 1]) | (r[:, 1] == r[:, 2]) | (r[:, 2] == r[:, 0])
    first = np.argmin(np.where(bad[:, None], 0, r), axis=1)
    rows = np.arange(len(t))
    ra, rb, rc = r[rows, first], r[rows, (first + 1) % 3], r[rows, (first + 2) % 3]
    key = ((ra << RANK_BITS) + rb << RANK_BITS) + rc
    return np.where(bad, -1, key).astype(np.int64)


def assemble(tri_key, pos):
    """The kept triangles and the vertices they use -> (vertices [V',3] float32 in ascending cell order, triangles [T',3] int32
    in input order, cell_to_vertex [C] int64 with -1 for a cell that gives no vertex)."""
    key = np.asarray(tri_key, np.int64)
    C = len(pos)
    idx = np.nonzero(key >= 0)[0]
    _, first = np.unique(key[idx], return_index=True)                                # the first occurrence: the lowest index
    kept = np.sort(idx[first])
    k = key[kept]
    mask = (1 << RANK_BITS) - 1
    tri = np.stack([k >> (2 * RANK_BITS), (k >> RANK_BITS) & mask, k & mask], axis=1)
    used = np.unique(tri)
    cell_to_vertex = np.full(C, -1, np.int64)
    cell_to_vertex[used] = np.arange(len(used))
    vertices = np.asarray(pos, np.float64).reshape(-1, 3)[used].astype(np.float32)
    return vertices.reshape(-1, 3), cell_to_vertex[tri].astype(np.int32).reshape(-1, 3), cell_to_vertex


def simplify(vertices, triangles, cell, origin=None, eps=EPS, placement='quadric', return_info=False):
    """The whole definition.  -> (vertices float32 [V',3], triangles int32 [T',3]); with return_info also dict(how, err, map:
    input vertex -> output vertex or -1, pos, sums, counts, cell_grid, origin, dims, rank, details)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    grid = default_grid(v, cell)
    if grid is None:
        return empty + (dict(map=np.full(len(v), -1, np.int64)),) if return_info else empty
    if origin is None:
        o, dims = grid
    else:
        o = np.asarray(origin, np.float64).reshape(3)
        dims = tuple(max(n, 1) for n in dims_for(v.astype(np.float64)[np.isfinite(v).all(axis=1)].max(axis=0), o, cell))
    keys = cluster_keys(v, o, cell, dims)
    _, rank, cell_grid = cells_of(keys, dims)
    sums, counts = cluster_sums(v, t, rank, cell_grid, o, cell)
    pos, how, err, details = cluster_place(sums, counts, cell_grid, o, cell, eps, placement, details=True)
    out_v, out_t, cell_to_vertex = assemble(triangle_keys(t, rank, len(cell_grid)), pos)
    if not return_info:
        return out_v, out_t
    vmap = np.where(rank >= 0, cell_to_vertex[np.clip(rank, 0, None)] if len(cell_to_vertex) else -1, -1)
    return out_v, out_t, dict(how=how, err=err, map=vmap, pos=pos, sums=sums, counts=counts, cell_grid=cell_grid, origin=o, dims=dims,
                              rank=rank, details=details, cell_to_vertex=cell_to_vertex)


# ---- hand cases -------------------------------------------------------------------------------------------------------------
def hand_cases():
    """Cells whose vertex has a closed form, with dyadic coordinates so that the closed form is exact: cell side 1, origin 0,
    2 x 2 x 2 cells, everything in cell (0, 0, 0) whose centre is (0.5, 0.5, 0.5).  Every triangle has its three corners in
    that cell, so it adds three corners to the sums and emits nothing.  The vertex count is a power of two (unreferenced
    vertices at the centre fill it up) so that the mean is exact.  -> [(name, dict(vertices, triangles, pos [3], how))]."""
    sheet_z = [(0.25, 0.25, 0.25), (0.75, 0.25, 0.25), (0.25, 0.75, 0.25)]           # in z = 0.25, n = (0, 0, 0.25)
    sheet_x = [(0.25, 0.25, 0.5), (0.25, 0.75, 0.5), (0.25, 0.25, 0.75)]             # in x = 0.25, n = (0.125, 0, 0)
    sheet_y = [(0.5, 0.25, 0.5), (0.75, 0.25, 0.5), (0.5, 0.25, 0.75)]               # in y = 0.25, n = (0, -0.0625, 0)
    slant = [(0.5, 0.75, 0.75), (0.75, 0.75, 0.75), (0.5, 0.875, 0.625)]             # in y + z = 1.5, n = (0, 1, 1) / 32
    plus = [(0.5, 0.75, 0.25), (0.625, 0.625, 0.25), (0.5, 0.75, 0.75)]              # in x + y = 1.25, n = -(1, 1, 0) / 16
    minus = [(0.75, 0.0, 0.25), (0.875, 0.125, 0.25), (0.75, 0.0, 0.75)]             # in x - y = 0.75, n = (1, -1, 0) / 16

    def case(name, sheets, total, pos, how, extra=()):
        v = [p for s in sheets for p in s] + list(extra)
        v += [(0.5, 0.5, 0.5)] * (total - len(v))
        t = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(sheets))]
        v = np.array(v, np.float32)
        if pos is None:                                                               # the mean
            pos = v.astype(np.float64).sum(axis=0) / total
        elif any(p is None for p in pos):                                             # the mean along the free axes
            m = v.astype(np.float64).sum(axis=0) / total
            pos = [m[a] if p is None else p for a, p in enumerate(pos)]
        return name, dict(vertices=v, triangles=np.array(t, np.int32), pos=np.array(pos, np.float64), how=how)
    above = [(0.25, 0.25, 0.75), (0.75, 0.25, 0.75), (0.25, 0.75, 0.75), (0.75, 0.75, 0.75), (0.75, 0.75, 0.25)]
    return [case("a flat sheet: the mean moved onto the plane", [sheet_z], 8, (None, None, 0.25), 1, extra=above),
            case("two planes: on their line", [sheet_z, sheet_x], 8, (0.25, None, 0.25), 2),
            case("a corner with its apex inside the cell: the apex", [sheet_z, sheet_x, sheet_y], 16, (0.25, 0.25, 0.25), 3),
            case("a corner with its apex outside the cell: the mean", [sheet_z, sheet_x, slant], 16, None, 7),
            case("an apex exactly at +c/2: accepted", [sheet_z, plus, minus], 16, (1.0, 0.25, 0.25), 3)]


HAND_ORIGIN, HAND_CELL, HAND_DIMS = np.zeros(3), 1.0, (2, 2, 2)


# ---- what the host and the GPU tests share ----------------------------------------------------------------------------------
def barycentric_samples(vertices, triangles, per_side=7):
    """per_side points per side of every triangle, its border included: [T * per_side (per_side + 1) / 2, 3] float64."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    w = np.array([(i, j, per_side - 1 - i - j) for i in range(per_side) for j in range(per_side - i)], np.float64) / (per_side - 1)
    return np.einsum('sk,tkc->tsc', w, v[t]).reshape(-1, 3)


def random_soup(seed=0, V=400, T=900, spread=1.0):
    """A triangle soup with repeated, degenerate and far-apart triangles: vertices uniform in a box of side `spread`."""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-0.5, 0.5, (V, 3)) * spread).astype(np.float32)
    near = rng.integers(0, V, T)
    t = np.stack([near, (near + rng.integers(1, 12, T)) % V, (near + rng.integers(1, 12, T)) % V], axis=1).astype(np.int32)
    t[::50, 1] = t[::50, 0]                                                          # a repeated index
    return v, t


def sphere_mesh():
    """fuse_reference.sphere_state() cut into its mesh (s = 1, origin 0): 7752 triangles."""
    import fuse_reference as FR
    return FR.extract_mesh(FR.sphere_state(), [0.0, 0.0, 0.0], 1.0)
