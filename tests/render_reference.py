"""NumPy restatement of DESIGN.md, "Rendered frames": posed triangle meshes -> depth uint16, label uint8 and the winning
draw rank per pixel.  Written from the definition.  Screen coordinates, areas and edge values are int64 (exact: the guard
band keeps them below 2^52), the floating-point part is float64 on the widened float32 inputs in the order the definition
writes it (NumPy does not fuse a product into a sum), and the depth test is the minimum of an integer key -- so every
output is an integer and is expected to equal the kernel's bit for bit.  Triangles are drawn one after the other, in
rank order; the order does not matter.

`variant` (project, draw_triangle, render) names deliberate departures from the definition, one boundary each; the
default, no variant, is the definition.  tests/test_render_edges_host.py uses them to show that its boundary families
tell the definition from its neighbours."""
import numpy as np

FRAC = 256                       # 8 fractional bits
GUARD = float(1 << 24)           # |ix|, |iy| above: unusable
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
VARIANTS = ('exclusive_edges',       # coverage w > 0 for w >= 0
            'half_even_vertex',      # the vertex snap rounds an exact half to even, not up
            'half_even_depth',       # the depth quantisation likewise
            'du_gt_1',               # du > 1 for du >= 1
            'du_lt_65535',           # du < 65535 for du <= 65535
            'z_gt_near',             # Z > z_near for Z >= z_near
            'guard_lt',              # |ix|, |iy| < 2^24 for <= 2^24
            'owner_lt')              # rank -> instance: the last j with base[j] < rank for <= rank


def _variant(variant):
    v = frozenset([variant] if isinstance(variant, str) else variant or ())
    assert v <= frozenset(VARIANTS), v
    return v


def pose_matrix(rotvec, trans):
    """[Rodrigues(rotvec) | trans; 0 0 0 1] in float64: a helper for the tests' poses (any 4x4 would do)."""
    r = np.asarray(rotvec, np.float64)
    theta = float(np.sqrt((r * r).sum()))
    K = np.zeros((3, 3))
    if theta > 0:
        k = r / theta
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)
    T[:3, 3] = np.asarray(trans, np.float64)
    return T


def project(vertices, pose, intr, z_near, variant=None):
    """The vertex stage: (ix, iy int64, iz float64, usable bool) of one instance's vertices."""
    variant = _variant(variant)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    A = np.asarray(pose, np.float64).reshape(-1)
    fx, fy, cx, cy = (float(np.float32(k)) for k in np.asarray(intr).reshape(-1)[:4])
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all='ignore'):
        X = ((A[0] * x + A[1] * y) + A[2] * z) + A[3]
        Y = ((A[4] * x + A[5] * y) + A[6] * z) + A[7]
        Z = ((A[8] * x + A[9] * y) + A[10] * z) + A[11]
        sx = (fx * X) / Z + cx
        sy = (fy * Y) / Z + cy
        fxv = np.floor(sx * 256.0 + 0.5)
        fyv = np.floor(sy * 256.0 + 0.5)
        if 'half_even_vertex' in variant:
            fxv, fyv = np.rint(sx * 256.0), np.rint(sy * 256.0)
        ok = np.isfinite(Z) & (Z >= float(z_near)) & (np.abs(fxv) <= GUARD) & (np.abs(fyv) <= GUARD)      # a NaN fails
        if 'z_gt_near' in variant:
            ok &= Z > float(z_near)
        if 'guard_lt' in variant:
            ok &= (np.abs(fxv) < GUARD) & (np.abs(fyv) < GUARD)
        ix = np.where(ok, fxv, 0.0).astype(np.int64)
        iy = np.where(ok, fyv, 0.0).astype(np.int64)
        iz = np.where(ok, 1.0 / np.where(ok, Z, 1.0), 0.0)
    return ix, iy, iz, ok


def _ceil_div(a, b):
    return -((-a) // b)


def draw_triangle(zbuf, rank, xs, ys, zs, factor, variant=None):
    """One usable triangle with a non-zero area into zbuf [H,W] uint64.  xs, ys: Python ints; zs: 1 / Z.  Returns the
    number of samples in its clamped box."""
    variant = _variant(variant)
    H, W = zbuf.shape
    (ax, bx, cx), (ay, by, cy), (iza, izb, izc) = xs, ys, zs
    area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    assert area2 != 0
    if area2 < 0:
        bx, cx, by, cy, izb, izc, area2 = cx, bx, cy, by, izc, izb, -area2
    u0, u1 = max(_ceil_div(min(xs), FRAC), 0), min(max(xs) // FRAC, W - 1)
    v0, v1 = max(_ceil_div(min(ys), FRAC), 0), min(max(ys) // FRAC, H - 1)
    if u1 < u0 or v1 < v0:
        return 0
    px = (np.arange(u0, u1 + 1, dtype=np.int64) * FRAC)[None, :]
    py = (np.arange(v0, v1 + 1, dtype=np.int64) * FRAC)[:, None]
    wa = (cx - bx) * (py - by) - (cy - by) * (px - bx)
    wb = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    wc = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    assert np.all(wa + wb + wc == area2) and max(np.abs(wa).max(), np.abs(wb).max(), np.abs(wc).max()) < (1 << 52)
    covered = (wa >= 0) & (wb >= 0) & (wc >= 0)
    if 'exclusive_edges' in variant:
        covered = (wa > 0) & (wb > 0) & (wc > 0)
    if covered.any():
        with np.errstate(all='ignore'):
            q = (wa.astype(np.float64) * iza +wb.astype(np.float64) * izb) + wc.astype(np.float64) * izc
            z = float(area2) / q
            du = np.floor(z * factor + 0.5)
            if 'half_even_depth' in variant:
                du = np.rint(z * factor)
            keep = covered & (du >= 1.0) & (du <= 65535.0)
            if 'du_gt_1' in variant:
                keep &= du > 1.0
            if 'du_lt_65535' in variant:
                keep &= du < 65535.0
        key = (np.where(keep, du, 0.0).astype(np.uint64) << np.uint64(32)) | np.uint64(rank)
        cell = zbuf[v0:v1 + 1, u0:u1 + 1]
        cell[...] = np.where(keep, np.minimum(cell, key), cell)
    return (u1 - u0 + 1) * (v1 - v0 + 1)


def instance_bases(meshes, frames):
    """(inst_offsets [F+1], inst_mesh [J], inst_label [J], poses [J,16], vert_base [J+1], tri_base [J+1])."""
    flat = [inst for fr in frames for inst in fr]
    offs = np.cumsum([0] + [len(fr) for fr in frames]).astype(np.int32)
    mesh = np.array([i[0] for i in flat], np.int32).reshape(-1)
    lab = np.array([i[1] for i in flat], np.int32).reshape(-1)
    poses = np.array([np.asarray(i[2], np.float64).reshape(16) for i in flat], np.float64).reshape(-1, 16)
    vb = np.cumsum([0] + [len(meshes[m][0]) for m in mesh]).astype(np.int64)
    tb = np.cumsum([0] + [len(meshes[m][1]) for m in mesh]).astype(np.int64)
    return offs, mesh, lab, poses, vb, tb


def render(meshes, frames, intrinsics, height, width, z_near=0.05, variant=None):
    """meshes: [(vertices [V,3] float32, triangles [T,3] int, ...)]; frames: per frame a list of (mesh index, label,
    pose 4x4 float64); intrinsics [F,5] float32 (fx, fy, cx, cy, factor_depth).  -> dict(depth [F,H,W] uint16, label
    uint8, tri int32, dropped, degenerate [J] int32, box [R] int64: the samples in the clamped box of every draw rank,
    -1 for a rank that was not drawn)."""
    variant = _variant(variant)
    intr = np.asarray(intrinsics, np.float32).reshape(len(frames), 5)
    offs, mesh, lab, poses, vb, tb = instance_bases(meshes, frames)
    F, J = len(frames), len(mesh)
    assert int(tb[-1]) < (1 << 31)
    zbuf = np.full((F, height, width), EMPTY, np.uint64)
    dropped, degenerate = np.zeros(J, np.int32), np.zeros(J, np.int32)
    box = np.full(int(tb[-1]), -1, np.int64)
    for f in range(F):
        factor = float(intr[f, 4])
        for j in range(offs[f], offs[f + 1]):
            v, t = meshes[mesh[j]][0], np.asarray(meshes[mesh[j]][1], np.int64).reshape(-1, 3)
            ix, iy, iz, ok = project(v, poses[j], intr[f], z_near, variant)
            for k, ids in enumerate(t):
                if np.any(ids < 0) or np.any(ids >= len(ix)) or not np.all(ok[ids]):
                    dropped[j] += 1
                    continue
                xs, ys = [int(c) for c in ix[ids]], [int(c) for c in iy[ids]]
                if (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0]) == 0:
                    degenerate[j] += 1
                    continue
                box[tb[j] + k] = draw_triangle(zbuf[f], int(tb[j]) + k, xs, ys, iz[ids], factor, variant)
    hit = zbuf != EMPTY
    rank = np.where(hit, zbuf & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    owner = np.searchsorted(tb, rank, side='right') - 1           # the last j with base[j] <= rank
    if 'owner_lt' in variant:
        owner = np.searchsorted(tb, rank, side='left') - 1
    depth = np.where(hit, zbuf >> np.uint64(32), 0).astype(np.uint16)
    label = np.where(hit & (owner >= 0), lab[np.clip(owner, 0, max(J - 1, 0))] if J else 0, 0).astype(np.uint8)
    tri = np.where(hit, rank, -1).astype(np.int32)
    return dict(depth=depth, label=label, tri=tri, dropped=dropped, degenerate=degenerate, box=box)


def backproject(depth, intr):
    """"Frame segments": pixel (u, v) of depth d -> ((u - cx) dm / fx, (v - cy) dm / fy, dm), dm = d / factor, in
    float64 here (the tests compare geometry, not bits)."""
    fx, fy, cx, cy, factor = (float(k) for k in np.asarray(intr, np.float32))
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    dm = depth.astype(np.float64) / factor
    return np.stack([(u - cx) * dm / fx, (v - cy) * dm / fy, dm], axis=-1)
