"""NumPy restatement of DESIGN.md, "Fused models": posed depth frames -> an integer TSDF state -> marching tetrahedra on
the voxel centres -> a welded triangle mesh.  Written from the definition.  The sums are integers and the extraction is
float64 on exactly widened values in the order the definition writes it (NumPy does not fuse a product into a sum), so
every output is expected to equal the kernels' bit for bit.

The second half holds what the host and the GPU tests share: mesh bookkeeping (closedness, components, Euler
characteristic, signed volume), exact distances to the surface of a union of axis-aligned boxes, and the 14-view scenes."""
import functools
import itertools

import numpy as np

QUANT = 4096.0
MAX_DIM = 512
MAX_VOXELS = 1 << 27
MAX_FRAMES = 1 << 19
AXIS_ORDERS = list(itertools.permutations(range(3)))          # lexicographic: (x,y,z), (x,z,y), (y,x,z), ...


# ---- the volume ------------------------------------------------------------------------------------------------------------
def new_state(dims):
    nx, ny, nz = (int(n) for n in dims)
    assert all(2 <= n <= MAX_DIM for n in (nx, ny, nz)) and nx * ny * nz <= MAX_VOXELS
    return np.zeros((nz, ny, nx, 4), np.int32)


def centres(origin, voxel, n, axis):
    """o + (i + 0.5) s of one axis, float64."""
    return float(origin[axis]) + (np.arange(n, dtype=np.float64) + 0.5) * float(voxel)


def volume_for(aabb, voxel, margin=4):
    """(origin [3] float64, dims (nx, ny, nz)) of the volume around a box with `margin` voxels on every side."""
    lo, hi = np.asarray(aabb, np.float64)
    s = float(voxel)
    dims = tuple(int(n) for n in np.ceil((hi - lo) / s).astype(np.int64) + 2 * int(margin))
    return lo - margin * s, dims


# ---- integration -----------------------------------------------------------------------------------------------------------
def integrate(state, origin, voxel, depth, intr, poses, front, behind, z_near=0.05, label=None, want=None):
    """Adds F frames to state [nz,ny,nx,4] int32 in place (and returns it)."""
    nz, ny, nx, _ = state.shape
    depth = np.asarray(depth)
    F, H, W = depth.shape
    assert depth.dtype == np.uint16 and F <= MAX_FRAMES
    intr = np.asarray(intr, np.float32).reshape(F, 5).astype(np.float64)
    poses = np.asarray(poses, np.float64).reshape(F, 4, 4)
    front, behind, z_near = float(front), float(behind), float(z_near)
    assert front >= behind > 0 and z_near > 0 and np.isfinite(front)       # (the entry point refuses behind = front)
    x = centres(origin, voxel, nx, 0)[None, None, :]
    y = centres(origin, voxel, ny, 1)[None, :, None]
    z = centres(origin, voxel, nz, 2)[:, None, None]
    filt = label is not None and want is not None
    for f in range(F):
        A = poses[f]
        fx, fy, cx, cy, factor = intr[f]
        with np.errstate(all='ignore'):
            X = ((A[0, 0] * x + A[0, 1] * y) + A[0, 2] * z) + A[0, 3]
            Y = ((A[1, 0] * x + A[1, 1] * y) + A[1, 2] * z) + A[1, 3]
            Z = ((A[2, 0] * x + A[2, 1] * y) + A[2, 2] * z) + A[2, 3]
            ok = Z > z_near
            up = ((fx * X) / Z + cx) + 0.5
            vp = ((fy * Y) / Z + cy) + 0.5
            ok &= (up >= 0.0) & (up < float(W)) & (vp >= 0.0) & (vp < float(H))          # a NaN fails
            pu = np.where(ok, np.floor(up), 0.0).astype(np.int64)
            pv = np.where(ok, np.floor(vp), 0.0).astype(np.int64)
            d = depth[f][pv, pu]
            ok &= d != 0
            if filt and int(want[f]) != 0:
                ok &= np.asarray(label)[f][pv, pu] == int(want[f])
            sdf = d.astype(np.float64) / factor - Z
            q = np.rint((np.where(sdf < front, sdf, front) / front) * QUANT)
            near = ok & (sdf >= -behind)
            deep = ok & ~near & (sdf >= -front)
        state[..., 0] += np.where(near, q, 0.0).astype(np.int32)
        state[..., 1] += near.astype(np.int32)
        state[..., 2] += np.where(deep, q, 0.0).astype(np.int32)
        state[..., 3] += deep.astype(np.int32)
    return state


# ---- the case table, from the geometry -------------------------------------------------------------------------------------
def tetrahedra():
    """Six per cell, each its four corners 0, bit a1, bits a1 | a2, 7."""
    return [(0, 1 << a1, (1 << a1) | (1 << a2), 7) for a1, a2, _ in AXIS_ORDERS]


def pattern_triangles(p):
    """The triangles of sign pattern p (bit l: local vertex l is inside), before the swap: each three edges, an edge a
    pair of local vertices, smaller first."""
    ins = [l for l in range(4) if (p >> l) & 1]
    outs = [l for l in range(4) if not (p >> l) & 1]
    if not ins or not outs:
        return []
    if len(ins) == 1 or len(outs) == 1:
        s = ins[0] if len(ins) == 1 else outs[0]
        return [tuple(tuple(sorted((s, o))) for o in range(4) if o != s)]
    (a, b), (c, d) = ins, outs
    q = [tuple(sorted(e)) for e in ((a, c), (a, d), (b, d), (b, c))]
    return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, c >> 2], np.float64)


@functools.lru_cache(maxsize=None)
def swap_table():
    """[6][16] bool: the second and third vertices of the pattern's triangles are swapped.  From the geometry of the unit
    cell: the normal (p1 - p0) x (p2 - p0) must not point from the outside vertices' mean towards the inside vertices'
    mean.  The answer does not depend on where on its edge a vertex lies: asserted over random positions."""
    rng = np.random.default_rng(5)
    table = np.zeros((6, 16), bool)
    for ti, tet in enumerate(tetrahedra()):
        P = np.array([_corner_xyz(c) for c in tet])
        for p in range(1, 15):
            ins = [l for l in range(4) if (p >> l) & 1]
            outs = [l for l in range(4) if not (p >> l) & 1]
            toward = P[ins].mean(axis=0) - P[outs].mean(axis=0)
            seen = set()
            for _ in range(8):
                t = rng.uniform(0.05, 0.95, (4, 4))
                for tri in pattern_triangles(p):
                    pts = [P[a] + (P[b] - P[a]) * t[a, b] for a, b in tri]
                    n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                    dot = float(n @ toward)
                    assert abs(dot) > 1e-9
                    seen.add(dot > 0)
            assert len(seen) == 1, (ti, p)
            table[ti, p] = seen.pop()
    return table


# ---- extraction ------------------------------------------------------------------------------------------------------------
def corner_values(state, min_count=1):
    """-> (v [nz,ny,nx] float64, known bool).  v is 0 where unknown."""
    st = np.asarray(state, np.int32).astype(np.float64)
    cnt, cntd = np.asarray(state)[..., 1], np.asarray(state)[..., 3]
    near = cnt >= int(min_count)
    deep = ~near & (cntd >= 1)
    with np.errstate(all='ignore'):
        v = np.where(near, st[..., 0] / st[..., 1], np.where(deep, st[..., 2] / st[..., 3], 0.0))
    return v, near | deep


def extract_triangles(state, origin, voxel, min_count=1):
    """-> (tri_count [cells] uint8, tri_pos [T,3,3] float64, tri_key [T,3] int64), triangles in the order cell,
    tetrahedron, triangle."""
    assert int(min_count) >= 1
    nz, ny, nx, _ = state.shape
    v, known = corner_values(state, min_count)
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    K, J, I = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing='ij')
    K, J, I = K.ravel(), J.ravel(), I.ravel()                                    # cell linear order
    ncell = len(I)
    off = [((c >> 2), (c >> 1) & 1, c & 1) for c in range(8)]                   # (dz, dy, dx)
    val = np.stack([v[K + dz, J + dy, I + dx] for dz, dy, dx in off], axis=1)    # [cells, 8]
    live = np.all(np.stack([known[K + dz, J + dy, I + dx] for dz, dy, dx in off], axis=1), axis=1)
    inside = val < 0.0
    swaps = swap_table()
    axes = [centres(origin, voxel, n, a) for a, n in enumerate((nx, ny, nz))]
    rows = []                                                                    # (cell, tet, tri, pos [n,3,3], key [n,3])
    for ti, tet in enumerate(tetrahedra()):
        pat = sum(inside[:, c].astype(np.int64) << l for l, c in enumerate(tet))
        for p in range(1, 15):
            sel = np.nonzero(live & (pat == p))[0]
            if not len(sel):
                continue
            for k, tri in enumerate(pattern_triangles(p)):
                if swaps[ti, p]:
                    tri = (tri[0], tri[2], tri[1])
                pos = np.zeros((len(sel), 3, 3))
                key = np.zeros((len(sel), 3), np.int64)
                for vi, (la, lb) in enumerate(tri):
                    lo, hi = tet[la], tet[lb]                                    # lo is a subset of hi: the smaller linear index
                    assert lo & hi == lo and lo != hi
                    vlo, vhi = val[sel, lo], val[sel, hi]
                    t = vlo / (vlo - vhi)
                    idx_lo = [I[sel] + (lo & 1), J[sel] + ((lo >> 1) & 1), K[sel] + (lo >> 2)]
                    idx_hi = [I[sel] + (hi & 1), J[sel] + ((hi >> 1) & 1), K[sel] + (hi >> 2)]
                    for a in range(3):
                        clo, chi = axes[a][idx_lo[a]], axes[a][idx_hi[a]]
                        pos[:, vi, a] = clo + (chi - clo) * t
                    key[:, vi] = ((idx_lo[2] * ny + idx_lo[1]) * nx + idx_lo[0]) * 8 + (hi ^ lo)
                rows.append((sel, np.full(len(sel), ti), np.full(len(sel), k), pos, key))
    if not rows:
        return np.zeros(ncell, np.uint8), np.zeros((0, 3, 3)), np.zeros((0, 3), np.int64)
    cell = np.concatenate([r[0] for r in rows])
    order = np.lexsort((np.concatenate([r[2] for r in rows]), np.concatenate([r[1] for r in rows]), cell))
    count = np.bincount(cell, minlength=ncell)
    assert count.max() <= 12
    return count.astype(np.uint8), np.concatenate([r[3] for r in rows])[order], np.concatenate([r[4] for r in rows])[order]


def weld(tri_pos, tri_key):
    """-> (vertices [V,3] float32 in ascending key order, triangles [T,3] int32).  Every occurrence of a key must carry the
    same position bits."""
    keys, first, inverse = np.unique(tri_key.reshape(-1), return_index=True, return_inverse=True)
    flat = np.ascontiguousarray(tri_pos.reshape(-1, 3))
    assert flat[first][inverse.reshape(-1)].tobytes() == flat.tobytes(), "one edge, two positions"
    return flat[first].astype(np.float32), inverse.reshape(-1, 3).astype(np.int32)


def extract_mesh(state, origin, voxel, min_count=1):
    _, pos, key = extract_triangles(state, origin, voxel, min_count)
    return weld(pos, key)


# ---- mesh bookkeeping ------------------------------------------------------------------------------------------------------
def mesh_stats(vertices, triangles):
    """dict(V, T, E, boundary: undirected edges used by one triangle only, oriented: every directed edge occurs once and its
    reverse once, components, euler = V - E + T, volume: signed, positive for outward normals)."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    V = len(v)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    d = d[d[:, 0] != d[:, 1]]                                                     # (a zero-area triangle's collapsed edge)
    code = d[:, 0] * max(V, 1) + d[:, 1]
    rev = d[:, 1] * max(V, 1) + d[:, 0]
    uniq, cnt = np.unique(code, return_counts=True)
    oriented = bool(np.all(cnt == 1) and np.array_equal(np.unique(rev), uniq)) if len(code) else True
    und, ucnt = np.unique(np.minimum(code, rev), return_counts=True)
    parent = np.arange(V)
    while len(d):                                                                 # label propagation to a fixed point
        low = np.minimum(parent[d[:, 0]], parent[d[:, 1]])
        new = parent.copy()
        np.minimum.at(new, d[:, 0], low)
        np.minimum.at(new, d[:, 1], low)
        new = new[new]
        if np.array_equal(new, parent):
            break
        parent = new
    used = np.unique(t)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return dict(V=V, T=len(t), E=len(und), boundary=int((ucnt == 1).sum()), oriented=oriented,
                components=len(np.unique(parent[used])) if len(used) else 0, euler=V - len(und) + len(t),
                volume=float((a * np.cross(b, c)).sum() / 6.0))


# ---- the true surface of a union of axis-aligned boxes ---------------------------------------------------------------------
def _minus(rect, hole):
    """A closed 2-D rectangle (lo [2], hi [2]) minus an open one -> up to four closed rectangles."""
    (l0, l1), (h0, h1) = rect
    (a0, a1), (b0, b1) = hole
    a0, a1, b0, b1 = max(a0, l0), max(a1, l1), min(b0, h0), min(b1, h1)
    if a0 >= b0 or a1 >= b1:
        return [rect]
    out = [((l0, l1), (a0, h1)), ((b0, l1), (h0, h1)), ((a0, l1), (b0, a1)), ((a0, b1), (b0, h1))]
    return [r for r in out if r[0][0] <= r[1][0] and r[0][1] <= r[1][1] and (r[0][0] < r[1][0] or r[0][1] < r[1][1])]


def union_surface(boxes):
    """The surface of a union of axis-aligned boxes [(lo [3], hi [3])] as rectangles (axis, coordinate, lo [2], hi [2] over
    the two other axes in ascending order): every face of a box minus the open interiors of the others."""
    rects = []
    for bi, (lo, hi) in enumerate(boxes):
        for axis in range(3):
            o = [a for a in range(3) if a != axis]
            for c in (lo[axis], hi[axis]):
                parts = [((lo[o[0]], lo[o[1]]), (hi[o[0]], hi[o[1]]))]
                for bj, (l2, h2) in enumerate(boxes):
                    if bj != bi and l2[axis] < c < h2[axis]:
                        parts = [r for part in parts for r in _minus(part, ((l2[o[0]], l2[o[1]]), (h2[o[0]], h2[o[1]])))]
                rects += [(axis, float(c), np.array(r[0], np.float64), np.array(r[1], np.float64)) for r in parts]
    return rects


def surface_distance(points, rects):
    """The distance of every point to the nearest rectangle."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    best = np.full(len(p), np.inf)
    for axis, c, lo, hi in rects:
        o = [a for a in range(3) if a != axis]
        q = p[:, o]
        gap = np.maximum(np.maximum(lo - q, q - hi), 0.0)
        best = np.minimum(best, np.sqrt((p[:, axis] - c) ** 2 + (gap ** 2).sum(axis=1)))
    return best


def surface_samples(rects, per_side=15):
    """per_side x per_side points of every rectangle, its border included."""
    out = []
    for axis, c, lo, hi in rects:
        o = [a for a in range(3) if a != axis]
        g = np.linspace(0.0, 1.0, per_side)
        a, b = np.meshgrid(lo[0] + (hi[0] - lo[0]) * g, lo[1] + (hi[1] - lo[1]) * g, indexing='ij')
        pts = np.zeros((per_side * per_side, 3))
        pts[:, axis], pts[:, o[0]], pts[:, o[1]] = c, a.ravel(), b.ravel()
        out.append(pts)
    return np.concatenate(out)


def nearest_vertex_distance(points, vertices):
    v = np.asarray(vertices, np.float64)
    return np.array([np.sqrt(((v - p) ** 2).sum(axis=1).min()) for p in np.asarray(points, np.float64)])


# ---- the scenes ------------------------------------------------------------------------------------------------------------
SCENE_H, SCENE_W = 240, 320
SCENE_INTR = np.array([600.0, 600.0, 159.5, 119.5, 10000.0], np.float32)
SCENE_DISTANCE = 0.6
FRONT_VOXELS, BEHIND_VOXELS = 4.0, 1.5


def view_directions():
    """14: towards +-x, +-y, +-z and the eight diagonals (unit vectors, the camera's viewing direction)."""
    d = [np.eye(3)[a] * s for a in range(3) for s in (1.0, -1.0)]
    d += [np.array([sx, sy, sz]) / np.sqrt(3.0) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    return d


def look_at(direction, centre, distance=SCENE_DISTANCE):
    """model -> camera: the camera looks along `direction` at `centre` from `distance` away."""
    zc = np.asarray(direction, np.float64)
    up = np.array([0.0, 0.0, 1.0]) if abs(zc[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    xc = np.cross(up, zc)
    xc /= np.sqrt((xc * xc).sum())
    yc = np.cross(zc, xc)
    T = np.eye(4)
    T[:3, :3] = np.stack([xc, yc, zc])
    T[:3, 3] = np.array([0.0, 0.0, distance]) - T[:3, :3] @ np.asarray(centre, np.float64)
    return T


def cube_mesh(side=0.07):
    import mesh_models_reference as M
    v, t, _ = M.cube()
    return (v.astype(np.float64) * side).astype(np.float32), t


def prism_mesh():
    import pose_verify_reference as V
    return V.l_prism()


def mesh_boxes(name):
    """The axis-aligned boxes whose union the scene's mesh is."""
    if name == 'cube':
        v, _ = cube_mesh()
        return [(v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64))]
    v, _ = prism_mesh()
    return [(v[:8].min(axis=0).astype(np.float64), v[:8].max(axis=0).astype(np.float64)),
            (v[8:].min(axis=0).astype(np.float64), v[8:].max(axis=0).astype(np.float64))]


def scene_inputs(name, voxel, renderer=None):
    """dict(mesh, poses [14,4,4], intr [14,5], depth [14,H,W] uint16, origin, dims, voxel, aabb).  renderer(meshes, frames,
    intr, H, W) -> depth; default the NumPy one."""
    import render_reference as R
    mesh = cube_mesh() if name == 'cube' else prism_mesh()
    v = mesh[0].astype(np.float64)
    aabb = np.stack([v.min(axis=0), v.max(axis=0)])
    poses = np.stack([look_at(d, aabb.mean(axis=0)) for d in view_directions()])
    intr = np.tile(SCENE_INTR, (len(poses), 1))
    frames = [[(0, 1, T)] for T in poses]
    if renderer is None:
        depth = R.render([mesh], frames, intr, SCENE_H, SCENE_W)['depth']
    else:
        depth = renderer([mesh], frames, intr, SCENE_H, SCENE_W)
    origin, dims = volume_for(aabb, voxel)
    return dict(mesh=mesh, poses=poses, intr=intr, depth=depth, origin=origin, dims=dims, voxel=float(voxel), aabb=aabb)


@functools.lru_cache(maxsize=None)
def scene(name, voxel, behind_voxels=BEHIND_VOXELS):
    """The scene's inputs, its fused state and its mesh by this restatement (computed once per process; do not modify)."""
    s = scene_inputs(name, voxel)
    state = integrate(new_state(s['dims']), s['origin'], voxel, s['depth'], s['intr'], s['poses'], FRONT_VOXELS * voxel,
                      behind_voxels * voxel)
    count, pos, key = extract_triangles(state, s['origin'], voxel)
    vertices, triangles = weld(pos, key)
    s.update(state=state, tri_count=count, tri_pos=pos, tri_key=key, vertices=vertices, triangles=triangles)
    return s


def scene_distances(s, name):
    """(largest vertex-to-surface distance, largest surface-sample-to-vertex distance), in voxels."""
    rects = union_surface(mesh_boxes(name))
    a = surface_distance(s['vertices'], rects).max() / s['voxel']
    b = nearest_vertex_distance(surface_samples(rects), s['vertices']).max() / s['voxel']
    return float(a), float(b)


# ---- states written by hand ------------------------------------------------------------------------------------------------
def state_from_field(field, count=1):
    """A state whose near band holds round(field * 4096) with `count` votes (acc = count * that): v = the rounded field."""
    f = np.asarray(field, np.float64)
    st = np.zeros(f.shape + (4,), np.int32)
    st[..., 0] = np.rint(f * QUANT).astype(np.int32) * int(count)
    st[..., 1] = int(count)
    return st


def sphere_state(n=24, radius=8.3, front=4.0):
    """The sphere of `radius` voxels around the middle of n^3 voxels (s = 1, origin 0), its distance cut to +-front and
    quantised as a vote is."""
    c = np.arange(n) + 0.5 - n / 2.0
    r = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return state_from_field(np.clip(r - radius, -front, front) / front)


def random_field_state(n=12, seed=3):
    """A few sinusoids on n^3, the outer layer forced positive."""
    rng = np.random.default_rng(seed)
    g = (np.arange(n) + 0.5) / n
    z, y, x = g[:, None, None], g[None, :, None], g[None, None, :]
    f = np.zeros((n, n, n))
    for _ in range(4):
        k = rng.uniform(3.0, 9.0, 3)
        ph = rng.uniform(0.0, 6.28, 3)
        f = f + rng.uniform(0.3, 1.0) * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    f = np.clip(f, -1.0, 1.0)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (0.5,) * 6
    return state_from_field(f)


def pattern_state(mask, magnitudes=None):
    """2 x 2 x 2 voxels, corner c inside when bit c of mask is set."""
    m = np.ones(8) * 0.5 if magnitudes is None else np.asarray(magnitudes, np.float64)
    f = np.array([(-m[c] if (mask >> c) & 1 else m[c]) for c in range(8)]).reshape(2, 2, 2)      # [z,y,x]: c = x + 2y + 4z
    return state_from_field(f)


# ---- the hand cases of the integration -------------------------------------------------------------------------------------
def hand_cases():
    """Fronto-parallel depth under the identity pose; factor_depth = 8192 and s, origin powers of two, so every sdf is exact.
    -> list of (name, dict of integrate's arguments with dims).  fx = fy = 64, s = 1/64: voxel columns one pixel apart at
    Z = 1 ... the closed forms are asserted in tests/test_fuse_host.py."""
    s = 1.0 / 64.0
    F_ = 8192.0
    front, behind = 4 * s, 1.5 * s
    cases = []

    def case(name, depth, origin, dims, intr=None, poses=None, **kw):
        depth = np.asarray(depth, np.uint16)
        F = depth.shape[0]
        intr = np.tile(np.array([64.0, 64.0, 3.5, 3.5, F_], np.float32), (F, 1)) if intr is None else np.asarray(intr, np.float32)
        poses = np.tile(np.eye(4), (F, 1, 1)) if poses is None else np.asarray(poses, np.float64)
        args = dict(origin=np.asarray(origin, np.float64), voxel=s, depth=depth, intr=intr, poses=poses, front=front,
                    behind=behind, z_near=0.05)
        args.update(kw)
        cases.append((name, dict(dims=dims, **args)))

    # a column of voxels along z through pixel (4, 4): centres at Z = 1 + (k + 0.5) / 64 - 8 / 64, the surface at d / 8192
    flat = np.full((1, 8, 8), 8192, np.uint16)                                   # the plane Z = 1
    case("plane at 1 m", flat, [0.0, 0.0, 1.0 - 8 * s], (2, 2, 16))
    # sdf exactly at front, -behind, -front and on either side: depths one unit (1/8192 m) apart around each threshold
    rows = []
    for k, off in ((3, 4 * s), (12, -1.5 * s), (14, -4 * s)):                     # (voxel k's Z) + off = the surface
        zc = 1.0 - 8 * s + (k + 0.5) * s
        for du in (-1, 0, 1):
            rows.append(int(round((zc + off) * F_)) + du)
    case("thresholds", np.array(rows, np.uint16)[:, None, None] * np.ones((1, 8, 8), np.uint16), [0.0, 0.0, 1.0 - 8 * s], (2, 2, 16))
    # a tie of rint: sdf / front * 4096 = n + 0.5 needs sdf = (n + 0.5) / 65536: one eighth of a depth unit, so the centre
    # is moved instead (origin z shifted by 1 / 131072, a power of two)
    case("rint tie", flat, [0.0, 0.0, 1.0 - 8 * s - 1.0 / 131072.0], (2, 2, 16))
    # pixels at u + 0.5 = 0 and u + 0.5 = W: centres at x = (-4 + i) / 64 with cx = 3.5, Z = 1 give u + 0.5 = i exactly
    # for i = 0 .. 8
    case("image borders", flat, [-4.5 * s, -4.5 * s, 1.0 - 0.5 * s], (10, 10, 2))
    # Z = z_near exactly and one voxel beyond (z_near = 1/16, a power of two)
    case("z_near", np.full((1, 8, 8), 600, np.uint16), [0.0, 0.0, 1.0 / 16.0 - 1.5 * s], (2, 2, 4), z_near=1.0 / 16.0,
         intr=np.array([[1.0, 1.0, 3.5, 3.5, F_]], np.float32))
    # depth 0 in a quarter of the image
    holes = flat.copy()
    holes[0, :4, :4] = 0
    case("depth 0", holes, [-4.5 * s, -4.5 * s, 1.0 - 2 * s], (10, 10, 4))
    # labels: want 0, matching and not matching, over three frames
    lab = np.zeros((3, 8, 8), np.uint8)
    lab[:, :, :4], lab[:, :, 4:] = 2, 5
    case("labels", np.repeat(flat, 3, axis=0), [-4.5 * s, -4.5 * s, 1.0 - 2 * s], (10, 10, 4), label=lab,
         want=np.array([0, 2, 7], np.int32))
    return cases


def run_case(args):
    a = dict(args)
    return integrate(new_state(a.pop('dims')), **a)


def wavy_state(dims, seed=0, zeros=0, unknown=0, count=1):
    """A smooth random field on (nx, ny, nz) voxels written into the near band; `zeros` voxels get the value 0 exactly and
    `unknown` voxels no vote at all."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.arange(nz)[:, None, None], np.arange(ny)[None, :, None], np.arange(nx)[None, None, :]
    f = np.zeros((nz, ny, nx))
    for _ in range(3):
        k = rng.uniform(0.4, 1.3, 3)
        ph = rng.uniform(0.0, 6.28, 3)
        f = f + rng.uniform(0.2, 0.5) * np.sin(k[0] * x + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * z + ph[2])
    f = np.clip(f + 0.05 * rng.standard_normal(f.shape), -1.0, 1.0)
    st = state_from_field(f, count)
    flat = st.reshape(-1, 4)
    pick = rng.permutation(len(flat))
    flat[pick[:zeros], 0] = 0
    flat[pick[zeros:zeros + unknown]] = 0
    return st


# ---- 17 small frames of two labelled cubes, for the integration's volumes -------------------------------------------------
SMALL_H, SMALL_W = 48, 64
SMALL_INTR = np.array([120.0, 120.0, 31.5, 23.5, 10000.0], np.float32)


@functools.lru_cache(maxsize=None)
def small_frames():
    """dict(depth [17,48,64] uint16, label uint8, intr [17,5], poses [17,4,4], want [17] int32: 0, 1, 2 and a label no pixel
    has, mixed): the 7 cm cube (label 1) and a 3 cm cube beside it (label 2) from the 14 scene directions and three more."""
    import render_reference as R
    big = cube_mesh()
    small = ((big[0].astype(np.float64) * (3.0 / 7.0) + [0.09, 0.01, 0.02]).astype(np.float32), big[1])
    dirs = view_directions() + [np.array(d) / np.sqrt(np.sum(np.square(d))) for d in ([1.0, 2.0, 0.5], [-2.0, 1.0, 1.0], [0.3, -1.0, 2.0])]
    poses = np.stack([look_at(d, [0.05, 0.035, 0.035]) for d in dirs])
    intr = np.tile(SMALL_INTR, (len(poses), 1))
    out = R.render([big, small], [[(0, 1, T), (1, 2, T)] for T in poses], intr, SMALL_H, SMALL_W)
    want = np.array([0, 1, 2, 1, 7, 0, 2, 2, 1, 0, 1, 2, 7, 1, 0, 2, 1], np.int32)
    return dict(depth=out['depth'], label=out['label'], intr=intr, poses=poses, want=want)


def small_volumes():
    """(name, origin, voxel, dims): the shapes the integration kernel is held to."""
    return [("2 x 2 x 2", [0.015, 0.015, 0.015], 0.02, (2, 2, 2)),
            ("23 x 5 x 3", [-0.011, 0.025, 0.03], 0.004, (23, 5, 3)),
            ("65 x 2 x 2", [-0.03, 0.033, 0.068], 0.002, (65, 2, 2)),
            ("half outside the frustum", [0.0, 0.0, 0.0], 0.03, (20, 4, 4)),
            ("behind some cameras", [0.45, 0.015, 0.015], 0.01, (30, 4, 4))]
