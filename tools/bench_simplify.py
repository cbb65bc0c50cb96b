"""Cost of simplifying a fused mesh ("Simplified meshes"), and what the simplified mesh saves downstream.  The mesh
is the one tools/bench_fuse.py fuses (128^3 voxels of 2 mm, 32 frames: 193 368 triangles), simplified at cells of 2, 4 and 8
voxels.  The HIP path (utils/simplify.py) runs beside the same steps written with torch operations in this file (index_add_ in
float64, torch.linalg.eigh); the outputs are compared before anything is timed.  Then the stages of the HIP path one by one,
so that the share of torch.unique and torch.sort is visible, and render_frames and one align_poses call with the full and
with the simplified mesh in the same windows.  Device events around every iteration; warm-up first; min / median / max over
the iterations; the two versions of a step alternate.

    python tools/bench_simplify.py [--cells 2 4 8] [--iters 20] [--warmup 3] [--out FILE.json]

Prints one JSON line.  The traffic of the sums kernel is an estimate from its instructions, not from counters: per corner it
requests one list entry (4 B), the triangle's three indices (12 B), three ranks (12 B) and three vertices (36 B), per vertex
entry 4 + 4 + 12 B; `must` counts every array once (the lists, the triangles, the ranks, the vertices, the starts and the
output)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_fuse import box_mesh, look_at, timed, views  # noqa: E402


# ---- the torch restatement ---------------------------------------------------------------------------------------------------
def torch_simplify(v, t, cell, origin, dims, eps):
    """The steps of simplify_mesh with torch operations: the same triangles; the vertices from eigh instead of Jacobi."""
    dev = v.device
    V = int(v.shape[0])
    o = torch.tensor(origin, dtype=torch.float64, device=dev)
    p = v.to(torch.float64)
    g = torch.floor((p - o) / cell)
    n = torch.tensor(dims, dtype=torch.float64, device=dev)
    ok = ((g >= 0.0) & (g < n)).all(dim=1)
    gi = torch.where(ok.unsqueeze(1), g, torch.zeros_like(g)).to(torch.int64)
    key = torch.where(ok, (gi[:, 2] * dims[1] + gi[:, 1]) * dims[0] + gi[:, 0], torch.full((V,), -1, dtype=torch.int64, device=dev))
    cells, inverse = torch.unique(key, sorted=True, return_inverse=True)
    unused = (cells[:1] < 0).to(torch.int64)
    rank = inverse - unused
    C = int(cells.numel() - unused)
    cells = cells[int(cells.numel()) - C:]
    grid = torch.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], dim=1)
    z = o + (grid.to(torch.float64) + 0.5) * cell
    used = rank >= 0
    m = torch.zeros((C, 3), dtype=torch.float64, device=dev).index_add_(0, rank[used], p[used] - z[rank[used]])
    n_v = torch.zeros((C,), dtype=torch.float64, device=dev).index_add_(0, rank[used], torch.ones_like(p[used][:, 0]))
    idx = t.to(torch.int64)
    live = ((idx >= 0) & (idx < V)).all(dim=1)
    r = rank[idx.clamp(0, V - 1)]
    live &= (r >= 0).all(dim=1)
    idx, r = idx[live], r[live]
    A = torch.zeros((C, 3, 3), dtype=torch.float64, device=dev)
    b = torch.zeros((C, 3), dtype=torch.float64, device=dev)
    for k in range(3):
        zc = z[r[:, k]]
        q0, q1, q2 = p[idx[:, 0]] - zc, p[idx[:, 1]] - zc, p[idx[:, 2]] - zc
        nrm = torch.linalg.cross(q1 - q0, q2 - q0)
        d = -(nrm * q0).sum(dim=1)
        A.index_add_(0, r[:, k], nrm.unsqueeze(2) * nrm.unsqueeze(1))
        b.index_add_(0, r[:, k], nrm * d.unsqueeze(1))
    mean = m / n_v.unsqueeze(1)
    lam, vec = torch.linalg.eigh(A)
    lmax = lam[:, 2]
    usable = torch.isfinite(lam).all(dim=1) & (lmax > 0.0)
    res = -b - (A @ mean.unsqueeze(2)).squeeze(2)
    coef = (vec.transpose(1, 2) @ res.unsqueeze(2)).squeeze(2) / lam
    coef = torch.where((lam > eps * lmax.unsqueeze(1)) & usable.unsqueeze(1), coef, torch.zeros_like(coef))
    x = mean + (vec @ coef.unsqueeze(2)).squeeze(2)
    inside = (x.abs() <= cell / 2.0).all(dim=1)
    x = torch.where(inside.unsqueeze(1), x, mean)
    pos = z + x
    # the triangles
    r3 = rank[t.to(torch.int64).clamp(0, V - 1)]
    bad = ~(((t >= 0) & (t < V)).all(dim=1) & (r3 >= 0).all(dim=1)) | (r3[:, 0] == r3[:, 1]) | (r3[:, 1] == r3[:, 2]) | (r3[:, 2] == r3[:, 0])
    first = torch.argmin(r3, dim=1)
    rows = torch.arange(int(t.shape[0]), device=dev)
    ra, rb, rc = r3[rows, first], r3[rows, (first + 1) % 3], r3[rows, (first + 2) % 3]
    tri_key = torch.where(bad, torch.full_like(ra, -1), (((ra << 21) + rb) << 21) + rc)
    at = torch.nonzero(tri_key >= 0).reshape(-1)
    uniq, inv = torch.unique(tri_key[at], sorted=True, return_inverse=True)
    low = torch.full((int(uniq.numel()),), int(tri_key.numel()), dtype=torch.int64, device=dev)
    low.scatter_reduce_(0, inv, at, reduce='amin')
    k = tri_key[torch.sort(low).values]
    tri = torch.stack([k >> 42, (k >> 21) & ((1 << 21) - 1), k & ((1 << 21) - 1)], dim=1)
    keep = torch.unique(tri, sorted=True)
    cell_vertex = torch.full((C,), -1, dtype=torch.int64, device=dev)
    cell_vertex[keep] = torch.arange(int(keep.numel()), dtype=torch.int64, device=dev)
    return pos[keep].to(torch.float32), cell_vertex[tri].to(torch.int32)


def stages(simp, v, t, cell, iters, warmup):
    """The HIP path's stages one by one, each timed on the inputs the stage before it left.  -> (dict of timings, C, corners added, vertices added, the corners per cell: min, median, max)."""
    dev = v.device
    box = simp.mesh_box(v)
    o, dims = simp.default_grid(box, cell)
    key = simp.cluster_keys(v, o, cell, dims)

    def unique():
        cells, inverse = torch.unique(key, sorted=True, return_inverse=True)
        unused = (cells[:1] < 0).to(torch.int64)
        return cells, (inverse - unused).to(torch.int32).contiguous(), int(cells.numel() - unused)
    cells, rank, C = unique()
    cells = cells[int(cells.numel()) - C:]
    grid = torch.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], dim=1).to(torch.int32).contiguous()

    def group():
        return simp.grouped(rank, C) + simp.grouped(simp.corner_ranks(t, rank), C)
    orders = group()
    sums, counts = simp.cluster_sums(v, t, rank, grid, o, cell, *orders)
    pos, how, err = simp.cluster_place(sums, counts, grid, o, cell)
    tri_key = simp.cluster_triangles(t, rank, C)

    def assemble():
        at = torch.nonzero(tri_key >= 0).reshape(-1)
        uniq, inv = torch.unique(tri_key[at], sorted=True, return_inverse=True)
        low = torch.full((int(uniq.numel()),), int(tri_key.numel()), dtype=torch.int64, device=dev)
        low.scatter_reduce_(0, inv, at, reduce='amin')
        k = tri_key[torch.sort(low).values]
        tri = torch.stack([k >> 42, (k >> 21) & ((1 << 21) - 1), k & ((1 << 21) - 1)], dim=1)
        keep = torch.unique(tri, sorted=True)
        cell_vertex = torch.full((C,), -1, dtype=torch.int64, device=dev)
        cell_vertex[keep] = torch.arange(int(keep.numel()), dtype=torch.int64, device=dev)
        return pos[keep].to(torch.float32), cell_vertex[tri].to(torch.int32)
    names = ["box", "keys", "unique", "group", "sums", "place", "triangles", "assemble"]
    fns = [lambda: simp.mesh_box(v), lambda: simp.cluster_keys(v, o, cell, dims), unique, group,
           lambda: simp.cluster_sums(v, t, rank, grid, o, cell, *orders), lambda: simp.cluster_place(sums, counts, grid, o, cell),
           lambda: simp.cluster_triangles(t, rank, C), assemble]
    times = {}
    for name, fn in zip(names, fns):                                                    # one at a time: a stage's own steady state
        times[name] = timed([fn], iters, warmup)[0]
    per_cell = counts[:, 1].to(torch.float64)
    load = dict(corners_min=int(per_cell.min()), corners_median=float(per_cell.median()), corners_max=int(per_cell.max()))
    return times, C, int(counts[:, 1].sum()), int(counts[:, 0].sum()), load


def main(argv=None):
    parser = argparse.ArgumentParser(description="time mesh simplification against a torch restatement, and the simplified mesh downstream")
    parser.add_argument("--n", type=int, default=128, help="voxels per side of the fused volume")
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--cells", type=int, nargs="+", default=[2, 4, 8], help="cell sides in voxels")
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify needs a GPU: nothing is measured without one")
    from cloudaae_amd.utils import fuse, mesh_models, render, track
    from cloudaae_amd.utils import simplify as simp
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    n, F, H, W = args.n, args.frames, 480, 640
    s = 0.002
    mesh = box_mesh([0.16, 0.12, 0.09])
    poses = np.stack([look_at(d, 0.7) for d in views(F)])
    intr = np.tile(np.array([600.0, 600.0, (W - 1) / 2.0, (H - 1) / 2.0, 10000.0], np.float32), (F, 1))
    depth = render.render_frames([mesh], [[(0, 1, T)] for T in poses], intr, H, W)['depth']
    vol = fuse.Volume((-0.5 * n * s,) * 3, s, (n, n, n), dev)
    fuse.integrate(vol, depth, torch.from_numpy(intr).to(dev), torch.from_numpy(poses).to(dev))
    v, t = fuse.extract_mesh(vol)
    V, T = int(v.shape[0]), int(t.shape[0])
    out = dict(vertices=V, triangles=T, voxel=s, iters=args.iters, warmup=args.warmup, cells={})

    meshes = {}
    for k in args.cells:
        cell = k * s
        sv, st = simp.simplify_mesh(v, t, cell)
        o, dims = simp.default_grid(simp.mesh_box(v), cell)
        rv, rt = torch_simplify(v, t, cell, o, dims, simp.EPS)
        same_triangles = bool(torch.equal(st, rt))
        apart = float((sv.to(torch.float64) - rv.to(torch.float64)).abs().max() / cell) if same_triangles and sv.numel() else float('nan')
        whole = timed([lambda: simp.simplify_mesh(v, t, cell), lambda: torch_simplify(v, t, cell, o, dims, simp.EPS)], args.iters, args.warmup)
        times, C, corners, listed, load = stages(simp, v, t, cell, args.iters, args.warmup)
        requested = 64 * corners + 20 * listed
        must = 4 * (3 * T) + 4 * V + 12 * T + 4 * V + 12 * V + 2 * 8 * (C + 1) + 12 * C + (128 + 8) * C
        sec = times["sums"]["median"] * 1e-3
        counts = fuse.mesh_counts(sv, st)
        out["cells"][str(k)] = dict(cell=cell, occupied_cells=C, vertices=counts[0], triangles=counts[1], boundary_edges=counts[2],
                                    components=counts[3], same_triangles_as_torch=same_triangles, vertices_apart_in_cells=apart,
                                    simplify_ms=whole[0], simplify_torch_ms=whole[1], stages_ms=times, corner_load=load,
                                    sums_requested_bytes=requested, sums_must_bytes=must,
                                    sums_requested_gbytes_per_s=requested / sec / 1e9, sums_must_gbytes_per_s=must / sec / 1e9,
                                    sums_corners_per_s=corners / sec)
        meshes[k] = (sv, st)

    # downstream: the renderer and one align_poses call, the full mesh and the simplified ones in the same windows
    packed = mesh_models.pack_meshes([(v, t)] + [meshes[k] for k in args.cells], device=dev)
    frames = lambda i: [[(i, 1, T)] for T in poses]                                     # noqa: E731
    fns = [lambda i=i: render.render_frames(packed, frames(i), intr, H, W) for i in range(len(args.cells) + 1)]
    r = timed(fns, args.iters, args.warmup)
    out["render_frames_ms"] = dict(frames=F, image=[H, W], full=r[0], **{"cell_%d" % k: r[1 + j] for j, k in enumerate(args.cells)})
    shift = np.eye(4)
    shift[:3, 3] = [0.004, -0.003, 0.005]
    start = np.stack([shift @ T for T in poses[:8]])
    first = track.align_poses(depth[:8], intr[:8], packed, [0] * 8, list(range(8)), start)
    window = (first['origin'], first['wh'], first['ww'])
    fns = [lambda i=i: track.align_poses(depth[:8], intr[:8], packed, [i] * 8, list(range(8)), start, window=window)
           for i in range(len(args.cells) + 1)]
    r = timed(fns, args.iters, args.warmup)
    ends = [track.align_poses(depth[:8], intr[:8], packed, [i] * 8, list(range(8)), start, window=window)['poses'].cpu().numpy()
            for i in range(len(args.cells) + 1)]
    off = [float(np.abs(e - poses[:8]).max()) for e in ends]
    out["align_poses_ms"] = dict(tracks=8, window=[int(first['wh']), int(first['ww'])], full=r[0],
                                 **{"cell_%d" % k: r[1 + j] for j, k in enumerate(args.cells)})
    out["align_poses_largest_pose_entry_off"] = dict(full=off[0], **{"cell_%d" % k: off[1 + j] for j, k in enumerate(args.cells)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
