"""Simplified meshes: uniform vertex clustering with quadric-error placement.  All vertices of a grid cell become one vertex,
placed where the summed squared distances to the planes of the cell's triangles are smallest (flat faces stay flat, edges and
corners stay sharp); triangles whose corners fall into fewer than three cells disappear.  Four kernels (csrc/mesh_cluster.hip)
with torch.unique and a stable torch.sort between them.  Takes any mesh the project handles -- fused, scanned or CAD -- and
gives what mesh_models.pack_meshes, render.render_frames, track and detect take.  The definition is in DESIGN.md ("Simplified
meshes").

    vertices, triangles = simplify_mesh(vertices, triangles, 0.008)              # float32 [V',3], int32 [T',3] on the device
    vertices, triangles = fuse.extract_mesh(volume, simplify=0.008)              # the same, inside the fusion
    vertices, triangles, info = simplify_mesh(v, t, 0.008, return_info=True)     # how, err [C]; map [V]: input -> output vertex

    python -m cloudaae_amd.utils.simplify --in a.ply --out b.ply --cell METRES [--scale S]
"""
import argparse

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

# a choice, not a measurement on data
EPS = 1e-3                # eigenvalues up to EPS times the largest do not move the vertex off the cell's mean

MAX_ITEMS = ((1 << 31) - 1) // 3
MAX_DIM = 1 << 20
MAX_CELLS = 1 << 21
RANK_BITS = 21


def _grid_args(origin, cell, dims=None):
    o = tuple(float(v) for v in np.asarray(origin, np.float64).reshape(3))
    c = float(cell)
    require(all(np.isfinite(o)) and np.isfinite(c) and c > 0.0, "the origin must be finite and the cell finite and positive")
    if dims is None:
        return o, c
    d = tuple(int(n) for n in dims)
    require(len(d) == 3 and all(1 <= n <= MAX_DIM for n in d), "dims must be (nx, ny, nz), each in [1, 2^20]")
    return o, c, d


def _mesh(vertices, triangles, device=None):
    """The mesh as contiguous device tensors: float32 [V,3], int32 [T,3]."""
    def tensor(x, dtype, name, dev):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if dev is None:
            dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        t = t.to(device=dev, dtype=dtype).contiguous()
        require(t.dim() == 2 and int(t.shape[1]) == 3, "%s must be [N, 3]" % name)
        require(int(t.shape[0]) <= MAX_ITEMS, "%s: at most 2^31 / 3 rows" % name)
        return t
    v = tensor(vertices, torch.float32, "vertices", device)
    return v, tensor(triangles, torch.int32, "triangles", v.device)


# ---- the stage bindings -----------------------------------------------------------------------------------------------------
def cluster_keys(vertices, origin, cell, dims):
    """cloudaae_mesh_cluster_keys.  vertices [V,3] float32 on the device; origin [3], cell, dims (nx, ny, nz) on the host.  ->
    key [V] int64: (g_z n_y + g_y) n_x + g_x, or -1 for a vertex that is not finite or outside the grid.  No read-back."""
    o, c, d = _grid_args(origin, cell, dims)
    V = int(vertices.shape[0])
    key = _lib.empty((V,), dtype=torch.int64, device=vertices.device)
    with torch.cuda.device(vertices.device):
        _lib.check(_lib.lib().cloudaae_mesh_cluster_keys(V, ptr(vertices), o[0], o[1], o[2], c, d[0], d[1], d[2], ptr(key), stream()),
                   "cloudaae_mesh_cluster_keys")
    return key


def grouped(rank, C):
    """Items grouped by rank, ascending index inside a group: (order [N] int32, start [C+1] int64) for cluster_sums; the items
    of rank -1 come first and belong to no group.  A stable sort; no read-back."""
    r = rank.to(torch.int64)
    ranks, order = torch.sort(r, stable=True)
    start = torch.searchsorted(ranks, torch.arange(C + 1, dtype=torch.int64, device=r.device))
    return order.to(torch.int32).contiguous(), start.contiguous()


def corner_ranks(triangles, rank):
    """[3T] int32: the rank of corner 3 t + k's vertex, -1 for every corner of a dropped triangle (an index outside [0, V) or an
    unused corner)."""
    V = int(rank.shape[0])
    idx = triangles.to(torch.int64)
    if V == 0:
        return torch.full((int(idx.numel()),), -1, dtype=torch.int32, device=triangles.device)
    inside = ((idx >= 0) & (idx < V)).all(dim=1)
    r = rank[idx.clamp(0, V - 1)]
    live = inside & (r >= 0).all(dim=1)
    return torch.where(live.unsqueeze(1), r, torch.full_like(r, -1)).reshape(-1).contiguous()


def cluster_sums(vertices, triangles, rank, cell_grid, origin, cell, vert_order=None, vert_start=None, corner_order=None,
                 corner_start=None):
    """cloudaae_mesh_cluster_sums.  rank [V] int32 (-1 unused), cell_grid [C,3] int32; the two orders with their starts
    (default: grouped() of the ranks and of corner_ranks()).  -> (sums [C,16] float64: m, A (xx, xy, xz, yy, yz, zz), b, e,
    three zeros; counts [C,2] int32: vertices, corners).  No read-back."""
    o, c = _grid_args(origin, cell)
    V, T, C = int(vertices.shape[0]), int(triangles.shape[0]), int(cell_grid.shape[0])
    dev = vertices.device
    if vert_order is None:
        vert_order, vert_start = grouped(rank, C)
    if corner_order is None:
        corner_order, corner_start = grouped(corner_ranks(triangles, rank), C)
    require(int(vert_start.numel()) == C + 1 and int(corner_start.numel()) == C + 1, "the starts must hold C + 1 entries")
    sums = _lib.empty((C, 16), dtype=torch.float64, device=dev)
    counts = _lib.empty((C, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_mesh_cluster_sums(V, T, ptr(vertices), ptr(triangles), C, ptr(rank), ptr(cell_grid), o[0], o[1],
                                                         o[2], c, ptr(vert_order), int(vert_order.numel()), ptr(vert_start),
                                                         ptr(corner_order), int(corner_order.numel()), ptr(corner_start), ptr(sums),
                                                         ptr(counts), stream()), "cloudaae_mesh_cluster_sums")
    return sums, counts


def cluster_place(sums, counts, cell_grid, origin, cell, eps=EPS):
    """cloudaae_mesh_cluster_place.  -> (pos [C,3] float64, how [C] uint8, err [C] float64).  how: the number of eigenvalues
    kept; 4: no usable quadric, the cell's mean; 5..7: the quadric's point left the cell, the mean.  No read-back."""
    o, c = _grid_args(origin, cell)
    C = int(cell_grid.shape[0])
    dev = sums.device
    pos = _lib.empty((C, 3), dtype=torch.float64, device=dev)
    how = _lib.empty((C,), dtype=torch.uint8, device=dev)
    err = _lib.empty((C,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_mesh_cluster_place(C, ptr(sums), ptr(counts), ptr(cell_grid), o[0], o[1], o[2], c, float(eps),
                                                          ptr(pos), ptr(how), ptr(err), stream()), "cloudaae_mesh_cluster_place")
    return pos, how, err


def cluster_triangles(triangles, rank, C):
    """cloudaae_mesh_cluster_triangles.  -> tri_key [T] int64: -1 (dropped, or two corners in one cell), else the three ranks,
    smallest first in the triangle's cyclic order, as (r_a 2^21 + r_b) 2^21 + r_c.  No read-back."""
    V, T = int(rank.shape[0]), int(triangles.shape[0])
    key = _lib.empty((T,), dtype=torch.int64, device=triangles.device)
    with torch.cuda.device(triangles.device):
        _lib.check(_lib.lib().cloudaae_mesh_cluster_triangles(V, T, ptr(triangles), ptr(rank), int(C), ptr(key), stream()),
                   "cloudaae_mesh_cluster_triangles")
    return key


# ---- the whole ---------------------------------------------------------------------------------------------------------------
def mesh_box(vertices):
    """The box of the finite vertices, float64 [2,3] on the host (one read-back), or None when there is none."""
    if int(vertices.shape[0]) == 0:
        return None
    p = vertices.to(torch.float64)
    finite = torch.isfinite(p).all(dim=1, keepdim=True)
    big = torch.full_like(p, float('inf'))
    box = torch.stack([torch.where(finite, p, big).amin(dim=0), torch.where(finite, p, -big).amax(dim=0)]).cpu().numpy()
    return box if np.all(np.isfinite(box)) else None


def default_grid(box, cell, origin=None):
    """(origin [3] float64, dims): the box's lower corner - cell / 4 unless given, and the smallest dims that hold its upper
    corner (at least 1)."""
    c = float(cell)
    o = box[0] - c / 4.0 if origin is None else np.asarray(origin, np.float64).reshape(3)
    dims = np.maximum(np.floor((box[1] - o) / c), 0.0) + 1.0
    require(np.all(dims <= MAX_DIM), "the mesh needs more than 2^20 cells along an axis: choose a larger cell")
    return o, tuple(int(n) for n in dims)


def _empty(dev):
    return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)


def simplify_mesh(vertices, triangles, cell, origin=None, eps=EPS, placement='quadric', return_info=False):
    """The mesh clustered on a grid of side `cell` (metres).  vertices [V,3], triangles [T,3]: device tensors or NumPy arrays.
    origin: the grid's low corner (default: the finite vertices' lower corner - cell / 4, a choice); the grid always reaches the
    upper corner.  placement 'quadric', or 'mean': every cell's vertex at the mean of its vertices (the same triangles).  ->
    (vertices [V',3] float32 in ascending cell order, triangles [T',3] int32 in input order) on the device; an input that
    collapses entirely gives two empty tensors.  With return_info a third value: dict(how [C] uint8, err [C] float64, pos
    [C,3] float64, cell_vertex [C] int64: the cell's output vertex or -1, map [V] int64: input vertex -> output vertex or -1,
    origin, dims).  Read-backs: the box of the vertices, and the sizes C, T' and V'."""
    require(placement in ('quadric', 'mean'), "placement must be 'quadric' or 'mean'")
    require(np.isfinite(float(cell)) and float(cell) > 0.0 and np.isfinite(float(eps)) and float(eps) > 0.0,
            "cell and eps must be finite and > 0")
    v, t = _mesh(vertices, triangles)
    dev = v.device
    V = int(v.shape[0])
    box = mesh_box(v)

    def result(out_v, out_t, info):
        return (out_v, out_t, info) if return_info else (out_v, out_t)
    nothing = dict(how=torch.zeros((0,), dtype=torch.uint8, device=dev), err=torch.zeros((0,), dtype=torch.float64, device=dev),
                   pos=torch.zeros((0, 3), dtype=torch.float64, device=dev), cell_vertex=torch.zeros((0,), dtype=torch.int64, device=dev),
                   map=torch.full((V,), -1, dtype=torch.int64, device=dev), origin=None, dims=None)
    if box is None:
        return result(*_empty(dev), nothing)
    o, dims = default_grid(box, cell, origin)
    key = cluster_keys(v, o, cell, dims)
    cells, inverse = torch.unique(key, sorted=True, return_inverse=True)
    unused = (cells[:1] < 0).to(torch.int64)                                          # 1 when the key -1 occurs: it sorts first
    rank = (inverse - unused).to(torch.int32).contiguous()
    C = int(cells.numel() - unused)                                                   # a size: read back
    if C == 0:
        return result(*_empty(dev), nothing)
    require(C <= MAX_CELLS, "more than 2^21 occupied cells: choose a larger cell")
    cells = cells[int(cells.numel()) - C:]
    nx, ny = dims[0], dims[1]
    cell_grid = torch.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], dim=1).to(torch.int32).contiguous()
    sums, counts = cluster_sums(v, t, rank, cell_grid, o, cell)
    if placement == 'mean':                                                           # no eigenvalue passes: x = mean, err = E(mean)
        pos, how, err = cluster_place(sums, counts, cell_grid, o, cell, float(np.finfo(np.float64).max))
        how = torch.full_like(how, 4)
    else:
        pos, how, err = cluster_place(sums, counts, cell_grid, o, cell, eps)
    tri_key = cluster_triangles(t, rank, C)

    # of the triangles with one key the lowest index stays; the kept ones stay in input order
    idx = torch.nonzero(tri_key >= 0).reshape(-1)                                     # (a size: T with a key)
    uniq, inv = torch.unique(tri_key[idx], sorted=True, return_inverse=True)
    first = torch.full((int(uniq.numel()),), int(tri_key.numel()), dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inv, idx, reduce='amin')
    k = tri_key[torch.sort(first).values]                                             # [T']
    mask = (1 << RANK_BITS) - 1
    tri = torch.stack([k >> (2 * RANK_BITS), (k >> RANK_BITS) & mask, k & mask], dim=1)
    used = torch.unique(tri, sorted=True)                                             # (a size: V')
    cell_vertex = torch.full((C,), -1, dtype=torch.int64, device=dev)
    cell_vertex[used] = torch.arange(int(used.numel()), dtype=torch.int64, device=dev)
    out_v = pos[used].to(torch.float32).reshape(-1, 3).contiguous()
    out_t = cell_vertex[tri].to(torch.int32).reshape(-1, 3).contiguous()
    info = None
    if return_info:
        vmap = torch.where(rank >= 0, cell_vertex[rank.to(torch.int64).clamp(min=0)], torch.full((V,), -1, dtype=torch.int64, device=dev))
        info = dict(how=how, err=err, pos=pos, cell_vertex=cell_vertex, map=vmap, origin=o, dims=dims)
    return result(out_v, out_t, info)


# ---- command line -----------------------------------------------------------------------------------------------------------
def main(argv=None):
    parser = argparse.ArgumentParser(description="simplify a PLY mesh by quadric vertex clustering")
    parser.add_argument("--in", dest="src", required=True, help="the PLY file to read")
    parser.add_argument("--out", required=True, help="the PLY file to write")
    parser.add_argument("--cell", type=float, required=True, help="cell side in metres (after --scale)")
    parser.add_argument("--scale", type=float, default=1.0, help="multiplies the file's coordinates (0.001 for millimetres)")
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    from . import fuse, mesh_models
    torch.cuda.set_device(args.gpu)
    v, t, _ = mesh_models.read_ply(args.src, args.scale)
    out_v, out_t = simplify_mesh(v, t, args.cell)
    mesh_models.write_ply(args.out, out_v, out_t)
    print("%d vertices, %d triangles, %d boundary edges, %d components read from %s" % (fuse.mesh_counts(v, t) + (args.src,)))
    print("%d vertices, %d triangles, %d boundary edges, %d components written to %s" % (fuse.mesh_counts(out_v, out_t) + (args.out,)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
