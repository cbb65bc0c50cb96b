"""NumPy restatement of DESIGN.md, "Mesh sampling", with Python integers wherever the definition is integer arithmetic:
triangle weights, their cumulative sums, the draw of a triangle and of its barycentric coordinates, the sampled points,
colours and normals.  Written from the definition; the host Philox is the one of tests/pose_sampling_reference.py.
Also the meshes the tests are run on: a cube, an icosphere, a lattice of right triangles and a random soup."""
import numpy as np

from pose_sampling_reference import philox4x32, u01

STREAM_MESH = 20
TWO32 = float(1 << 32)


# ---- the definition ------------------------------------------------------------------------------------------------
def triangle_normals(vertices, triangles):
    """(n [T,3], A2 [T], valid [T]) in double on the widened coordinates: n = (b - a) x (c - a), each component
    (p q) - (r s); A2 = sqrt((nx^2 + ny^2) + nz^2).  valid: every index inside the mesh, A2 finite and not 0."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    inside = np.all((t >= 0) & (t < len(v)), axis=1)
    ts = np.where(inside[:, None], t, 0)
    a, b, c = (v[ts[:, k]] if len(v) else np.zeros((len(t), 3)) for k in range(3))
    e1, e2 = b - a, c - a
    with np.errstate(all='ignore'):
        n = np.stack([(e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1]),
                      (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2]),
                      (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])], axis=1)
        a2 = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    valid = inside & np.isfinite(a2) & (a2 > 0)
    return n, a2, valid


def mesh_weights(vertices, triangles):
    """One mesh -> dict(weights [T] uint64 = floor(A2 / A2max * 2^32), cum [T] uint64 (inclusive), W (Python int),
    invalid (int), a2max (float), a2 [T])."""
    _, a2, valid = triangle_normals(vertices, triangles)
    a2 = np.where(valid, a2, 0.0)
    # the maximum by the bit pattern of the non-negative doubles: the same value as the floating-point maximum
    a2max = float(a2.view(np.uint64).max().view(np.float64)) if len(a2) else 0.0
    w = [0] * len(a2)
    if a2max > 0.0:
        w = [int(np.floor((x / a2max) * TWO32)) for x in a2]
    cum, run = [], 0
    for x in w:
        run += x
        cum.append(run)
    return dict(weights=np.array(w, np.uint64), cum=np.array(cum, np.uint64), W=run, invalid=int((~valid).sum()),
                a2max=a2max, a2=a2)


def draw(cum, n, seed, first_index=0, mesh_id=0):
    """The integer part of n draws: (tri [n] int64 (-1 when W = 0), u [n], v [n] float64 after the reflection).
    cum: the mesh's cumulative weights (the restatement's or a kernel's)."""
    cum = np.asarray(cum, np.uint64)
    g = [int(first_index) + j for j in range(n)]
    assert all(x < (1 << 40) for x in g)
    ctr = np.array([(int(mesh_id) << 40) + x for x in g], np.uint64)
    r = philox4x32(seed, ctr, STREAM_MESH)
    W = int(cum[-1]) if len(cum) else 0
    u = u01(r[:, 2]).astype(np.float64)
    v = u01(r[:, 3]).astype(np.float64)
    flip = u + v > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    if W == 0:
        return np.full(n, -1, np.int64), u, v
    target = np.array([(((int(a) << 32) + int(b)) * W) >> 64 for a, b in zip(r[:, 0], r[:, 1])], np.uint64)
    tri = np.searchsorted(cum, target, side='right').astype(np.int64)          # the first t with cum[t] > target
    return tri, u, v


def sample_mesh(vertices, triangles, n, seed, first_index=0, mesh_id=0, colors=None, cum=None):
    """One mesh -> dict(xyzrgb [n,6] float32, tri [n] int64, normal [n,3] float64, bary [n,3] float64 (b0, u, v))."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if cum is None:
        cum = mesh_weights(v32, t)['cum']
    tri, u, v = draw(cum, n, seed, first_index, mesh_id)
    b0 = (1.0 - u) - v
    out = np.zeros((n, 6), np.float32)
    normal = np.zeros((n, 3), np.float64)
    ok = tri >= 0
    if ok.any():
        ids = t[np.where(ok, tri, 0)]
        ok &= np.all((ids >= 0) & (ids < len(v32)), axis=1)
        ids = np.where(ok[:, None], ids, 0)

        def mix(values):
            x = np.asarray(values, np.float32).astype(np.float64)
            a, b, c = x[ids[:, 0]], x[ids[:, 1]], x[ids[:, 2]]
            return ((b0[:, None] * a + u[:, None] * b) + v[:, None] * c).astype(np.float32)
        out[:, :3] = mix(v32)
        if colors is not None:
            out[:, 3:] = mix(np.asarray(colors, np.float32).reshape(-1, 3))
        nrm, a2, _ = triangle_normals(v32, ids)
        with np.errstate(all='ignore'):
            normal = np.where((np.isfinite(a2) & (a2 > 0))[:, None], nrm / a2[:, None], 0.0)
        out[~ok] = 0
        normal[~ok] = 0
        tri = np.where(ok, tri, -1)
    return dict(xyzrgb=out, tri=tri, normal=normal, bary=np.stack([b0, u, v], axis=1))


# ---- meshes ----------------------------------------------------------------------------------------------------------
def cube():
    """The unit cube [0,1]^3: 8 vertices, 12 triangles, outward winding; colours = the coordinates."""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)], np.int32)
    return v, t, v.copy()


def icosphere(subdivisions=3, radius=1.0):
    """An icosahedron subdivided `subdivisions` times (20 * 4^k faces: 1280 at k = 3), vertices on the sphere."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdivisions):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def lattice(num_triangles, seed=0):
    """num_triangles axis-aligned right triangles in the plane z = 0 with legs 1, 2 or 4 (chosen by a seeded draw), one
    per unit-spaced lattice cell of 8 x 8: every A2 is one of 1, 2, 4, 8, 16 and every weight ratio is exact."""
    rng = np.random.default_rng(seed)
    legs = np.array([1, 2, 4])
    a = legs[rng.integers(0, 3, num_triangles)].astype(np.float32)
    b = legs[rng.integers(0, 3, num_triangles)].astype(np.float32)
    i = np.arange(num_triangles)
    ox, oy = (8 * (i % 64)).astype(np.float32), (8 * (i // 64)).astype(np.float32)
    z = np.zeros(num_triangles, np.float32)
    v = np.stack([np.stack([ox, oy, z], 1), np.stack([ox + a, oy, z], 1), np.stack([ox, oy + b, z], 1)], axis=1)
    return v.reshape(-1, 3), np.arange(3 * num_triangles, dtype=np.int32).reshape(-1, 3)


def soup(num_triangles=200, seed=0, degenerate=False):
    """A random triangle soup on shared vertices, with colours.  degenerate: the first four triangles become a
    zero-area one (collinear corners), one with a repeated vertex, one with an out-of-range index and one 2^-40 the
    size of the mesh's largest (a scaled copy of it, on vertices of its own)."""
    rng = np.random.default_rng(seed)
    nv = max(num_triangles // 2, 8)
    v = rng.uniform(-1, 1, (nv, 3)).astype(np.float32)
    t = np.stack([rng.permutation(nv)[:3] for _ in range(num_triangles)]).astype(np.int32)
    if degenerate:
        a2 = mesh_weights(v, t[4:])['a2']
        big = t[4 + int(np.argmax(a2))]
        # exact powers of two: the small copy's A2 is 2^-40 of the largest's exactly (edges scale by 2^-20)
        small = (v[big].astype(np.float64) * 2.0 ** -20).astype(np.float32)
        assert np.array_equal(small.astype(np.float64), v[big].astype(np.float64) * 2.0 ** -20)
        line = np.array([[0, 0, 0], [0.25, 0.5, 0.75], [0.5, 1.0, 1.5]], np.float32)
        v = np.concatenate([v, small, line])
        t[0] = [nv + 3, nv + 4, nv + 5]
        t[1] = [t[1][0], t[1][1], t[1][0]]
        t[2] = [t[2][0], len(v), t[2][2]]
        t[3] = [nv, nv + 1, nv + 2]
    c = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    return v, t, c


def pack(meshes):
    """[(vertices, triangles[, colors])] -> (vert_offsets, tri_offsets int32 [S+1], vertices [V,3], triangles [T,3],
    colors [V,3] or None)."""
    vo = np.cumsum([0] + [len(m[0]) for m in meshes]).astype(np.int32)
    to = np.cumsum([0] + [len(m[1]) for m in meshes]).astype(np.int32)
    v = np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 3) for m in meshes])
    t = np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in meshes])
    has = [len(m) > 2 and m[2] is not None for m in meshes]
    c = np.concatenate([np.asarray(m[2], np.float32).reshape(-1, 3) for m in meshes]) if all(has) else None
    return vo, to, v, t, c
