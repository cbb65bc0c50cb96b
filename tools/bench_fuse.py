"""Cost of fusing a model ("Fused models"): cloudaae_tsdf_integrate at 128^3 voxels x 32 frames of 480 x 640, and
count + emit + weld on the result, each beside a plain torch restatement of the same step on the same GPU.  Device events
around every iteration; warm-up first; min / median / max over the iterations; the two versions of a step alternate.  The
restatements' outputs are compared with the kernels' before anything is timed (integers and float64 bits: equal).

    python tools/bench_fuse.py [--n 128] [--frames 32] [--iters 20] [--warmup 3] [--out FILE.json]

Prints one JSON line.  bytes_per_voxel counts what the integrate kernel must move: the state once in and once out (32 B)
plus one uint16 depth sample per frame that reaches the image (an upper bound of 2 F B; the samples of neighbouring voxels
share cache lines)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_mesh(size):
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)], np.int32)
    return ((v - 0.5) * np.asarray(size)).astype(np.float32), t


def look_at(direction, distance):
    zc = np.asarray(direction, np.float64) / np.sqrt(np.sum(np.square(direction)))
    up = np.array([0.0, 0.0, 1.0]) if abs(zc[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    xc = np.cross(up, zc)
    xc /= np.sqrt((xc * xc).sum())
    T = np.eye(4)
    T[:3, :3] = np.stack([xc, np.cross(zc, xc), zc])
    T[:3, 3] = [0.0, 0.0, distance]
    return T


def views(n):
    """n directions on a spiral over the sphere."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


# ---- the torch restatements ------------------------------------------------------------------------------------------------
def torch_integrate(state, origin, s, depth, intr, poses, front, behind, z_near):
    nz, ny, nx, _ = state.shape
    dev = state.device
    F, H, W = depth.shape
    ax = [origin[a] + (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * s for a, n in enumerate((nx, ny, nz))]
    x, y, z = ax[0].view(1, 1, nx), ax[1].view(1, ny, 1), ax[2].view(nz, 1, 1)
    d16 = (depth.to(torch.int32) & 0xFFFF)
    k = intr.to(torch.float64).cpu().numpy()
    A = poses.cpu().numpy()
    for f in range(F):
        P = A[f]
        X = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
        Y = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
        Z = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
        up = ((k[f, 0] * X) / Z + k[f, 2]) + 0.5
        vp = ((k[f, 1] * Y) / Z + k[f, 3]) + 0.5
        ok = (Z > z_near) & (up >= 0.0) & (up < float(W)) & (vp >= 0.0) & (vp < float(H))
        pu = torch.where(ok, torch.floor(up), torch.zeros_like(up)).to(torch.int64)
        pv = torch.where(ok, torch.floor(vp), torch.zeros_like(vp)).to(torch.int64)
        d = d16[f][pv, pu]
        ok &= d != 0
        sdf = d.to(torch.float64) / k[f, 4] - Z
        q = torch.round((torch.where(sdf < front, sdf, torch.full_like(sdf, front)) / front) * 4096.0).to(torch.int32)
        near = ok & (sdf >= -behind)
        deep = ok & ~near & (sdf >= -front)
        zero = torch.zeros_like(q)
        state[..., 0] += torch.where(near, q, zero)
        state[..., 1] += near.to(torch.int32)
        state[..., 2] += torch.where(deep, q, zero)
        state[..., 3] += deep.to(torch.int32)
    return state


def torch_extract_mesh(state, origin, s, min_count=1):
    """count + emit + weld with torch operations: the same triangles, vertices in key order."""
    from tools import gen_tsdf_tables as G
    nz, ny, nx, _ = state.shape
    dev = state.device
    st = state.to(torch.float64)
    near = state[..., 1] >= min_count
    deep = ~near & (state[..., 3] >= 1)
    v = torch.where(near, st[..., 0] / st[..., 1], torch.where(deep, st[..., 2] / st[..., 3], torch.zeros_like(st[..., 0])))
    known = near | deep
    off = [((c >> 2), (c >> 1) & 1, c & 1) for c in range(8)]
    val = torch.stack([v[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].reshape(-1) for dz, dy, dx in off], dim=1)
    live = torch.stack([known[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].reshape(-1) for dz, dy, dx in off], dim=1).all(dim=1)
    inside = val < 0.0
    cell = torch.arange(val.shape[0], dtype=torch.int64, device=dev)
    I, J, K = cell % (nx - 1), (cell // (nx - 1)) % (ny - 1), cell // ((nx - 1) * (ny - 1))
    ax = [origin[a] + (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * s for a, n in enumerate((nx, ny, nz))]
    rows = []
    for ti, tet in enumerate(G.tetrahedra()):
        pat = sum(inside[:, c].to(torch.int64) << l for l, c in enumerate(tet))
        for p in range(1, 15):
            sel = torch.nonzero(live & (pat == p)).reshape(-1)
            if sel.numel() == 0:
                continue
            for k, tri in enumerate(G.triangles(p)):
                if G.swapped(tet, p):
                    tri = [tri[0], tri[2], tri[1]]
                pos = torch.zeros((sel.numel(), 3, 3), dtype=torch.float64, device=dev)
                key = torch.zeros((sel.numel(), 3), dtype=torch.int64, device=dev)
                for vi, (la, lb) in enumerate(tri):
                    lo, hi = tet[la], tet[lb]
                    t = val[sel, lo] / (val[sel, lo] - val[sel, hi])
                    il = [I[sel] + (lo & 1), J[sel] + ((lo >> 1) & 1), K[sel] + (lo >> 2)]
                    ih = [I[sel] + (hi & 1), J[sel] + ((hi >> 1) & 1), K[sel] + (hi >> 2)]
                    for a in range(3):
                        clo, chi = ax[a][il[a]], ax[a][ih[a]]
                        pos[:, vi, a] = clo + (chi - clo) * t
                    key[:, vi] = ((il[2] * ny + il[1]) * nx + il[0]) * 8 + (hi ^ lo)
                rows.append((sel * 12 + ti * 2 + k, pos, key))
    if not rows:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    order = torch.argsort(torch.cat([r[0] for r in rows]))
    pos, key = torch.cat([r[1] for r in rows])[order], torch.cat([r[2] for r in rows])[order]
    keys, inverse = torch.unique(key.reshape(-1), sorted=True, return_inverse=True)
    first = torch.zeros((keys.numel(),), dtype=torch.int64, device=dev)
    first.scatter_(0, inverse, torch.arange(inverse.numel(), dtype=torch.int64, device=dev))
    return pos.reshape(-1, 3)[first].to(torch.float32), inverse.reshape(-1, 3).to(torch.int32)


def timed(fns, iters, warmup):
    """The callables alternate; -> per callable (min, median, max) in milliseconds."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [dict(min=float(np.min(m)), median=float(np.median(m)), max=float(np.max(m))) for m in ms]


def main(argv=None):
    parser = argparse.ArgumentParser(description="time TSDF fusion and mesh extraction against torch restatements")
    parser.add_argument("--n", type=int, default=128, help="voxels per side")
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--height", type=int, default=480)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--iters", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse needs a GPU: nothing is measured without one")
    from cloudaae_amd.utils import fuse, render
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    n, F, H, W = args.n, args.frames, args.height, args.width
    s = 0.002
    mesh = box_mesh([0.16, 0.12, 0.09])
    poses = np.stack([look_at(d, 0.7) for d in views(F)])
    intr = np.tile(np.array([600.0, 600.0, (W - 1) / 2.0, (H - 1) / 2.0, 10000.0], np.float32), (F, 1))
    depth = render.render_frames([mesh], [[(0, 1, T)] for T in poses], intr, H, W)['depth']
    origin = (-0.5 * n * s,) * 3
    intr_d, poses_d = torch.from_numpy(intr).to(dev), torch.from_numpy(poses).to(dev)
    front, behind = fuse.FRONT_VOXELS * s, fuse.BEHIND_VOXELS * s

    vol = fuse.Volume(origin, s, (n, n, n), dev)
    fuse.integrate(vol, depth, intr_d, poses_d)
    ref = torch_integrate(torch.zeros_like(vol.state), origin, s, depth, intr_d, poses_d, front, behind, render.Z_NEAR)
    same_state = bool(torch.equal(vol.state, ref))
    v, t = fuse.extract_mesh(vol)
    rv, rt = torch_extract_mesh(vol.state, origin, s)
    same_mesh = bool(torch.equal(t, rt) and torch.equal(v.view(torch.int32), rv.view(torch.int32)))

    scratch = fuse.Volume(origin, s, (n, n, n), dev)
    scratch_ref = torch.zeros_like(vol.state)
    t_int = timed([lambda: fuse.integrate(scratch, depth, intr_d, poses_d),
                   lambda: torch_integrate(scratch_ref, origin, s, depth, intr_d, poses_d, front, behind, render.Z_NEAR)],
                  args.iters, args.warmup)
    t_ext = timed([lambda: fuse.extract_mesh(vol), lambda: torch_extract_mesh(vol.state, origin, s)], args.iters, args.warmup)
    t_parts = timed([lambda: fuse.extract_triangles(vol)], args.iters, args.warmup)
    voxels = n ** 3
    must = voxels * (32 + 2 * F) + F * H * W * 2
    out = dict(voxels=[n, n, n], frames=F, image=[H, W], triangles=int(t.shape[0]), vertices=int(v.shape[0]),
               same_state=same_state, same_mesh=same_mesh,
               integrate_ms=t_int[0], integrate_torch_ms=t_int[1], extract_mesh_ms=t_ext[0], extract_mesh_torch_ms=t_ext[1],
               count_emit_ms=t_parts[0], bytes_per_voxel=32 + 2 * F, integrate_bytes=must,
               integrate_gbytes_per_s=must / (t_int[0]['median'] * 1e-3) / 1e9,
               integrate_voxel_frames_per_s=voxels * F / (t_int[0]['median'] * 1e-3), iters=args.iters, warmup=args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
