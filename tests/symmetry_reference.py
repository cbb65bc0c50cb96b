"""NumPy restatement of DESIGN.md, "Object symmetries": the score of csrc/symmetry.hip with the definition's association,
the bookkeeping of cloudaae_amd/utils/symmetry.py, and the analytic solids the tests search.

The score (hausdorff_scores) is the definition, brute force.  hausdorff_scores_fast finds each query's nearest target
with scipy's cKDTree and then forms that pair's distance by the definition: the same number up to the last bit of the
tree's own tie between near-equal neighbours -- for the margins of the acceptance rule, never for a bit-exact check.

The procedure (find_symmetries) is restated WITHOUT the sharpening step (b): no ICP.  Its axes are those of the coarse
grid.  Scores are flat around a true axis, so two grid axes more than merge_deg apart can both stand for one true axis
and an element is then counted twice (measured: the box gives 4 or 5 members by the grid's orientation, the square prism
10 instead of 8, the triangular prism 8 instead of 6); the kind, the orders that occur, the L-shaped solid's 1 and the
cylinder's step count do not depend on the sharpening and are what the host tests use it for.
"""
import math

import numpy as np

ORDER_STEPS = 120
COARSE_ANGLES = (2.0 * math.pi / 2.0, 2.0 * math.pi / 3.0, 2.0 * math.pi / 5.0)


# ---- the score -------------------------------------------------------------------------------------------------------
def apply(T, p):
    """icp_apply of csrc/pose_math.h on points p [n,3] float64 under T [4,4]: ((A00 x + A01 y) + A02 z) + A03 row by row."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def squared_hausdorff(queries, targets, transforms):
    """H2 [c] float64: max_i min_j ((dx dx + dy dy) + dz dz), d = T_c x_i - y_j, on the float32 points widened exactly."""
    q = np.asarray(queries, np.float32)[:, :3].astype(np.float64)
    t = np.asarray(targets, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
    out = np.zeros(len(T))
    for c in range(len(T)):
        p = apply(T[c], q)
        best = np.full(len(p), np.inf)
        for lo in range(0, len(t), 2048):
            d = p[:, None, :] - t[None, lo:lo + 2048, :]
            best = np.minimum(best, ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1))
        out[c] = best.max()
    return out


def hausdorff_scores(queries, targets, transforms, limit2=np.inf):
    """out [c] float64 = sqrt(H2_c) where H2_c <= limit2, else +inf."""
    h2 = squared_hausdorff(queries, targets, transforms)
    return np.where(h2 <= limit2, np.sqrt(h2), np.inf)


def hausdorff_scores_fast(queries, targets, transforms, limit2=np.inf):
    """hausdorff_scores with the nearest target found by a k-d tree (see the module's docstring)."""
    from scipy.spatial import cKDTree
    q = np.asarray(queries, np.float32)[:, :3].astype(np.float64)
    t = np.asarray(targets, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
    tree = cKDTree(t)
    out = np.zeros(len(T))
    for lo in range(0, len(T), 256):
        p = np.stack([apply(Tc, q) for Tc in T[lo:lo + 256]])
        _, j = tree.query(p.reshape(-1, 3), workers=-1)
        d = p.reshape(-1, 3) - t[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[lo:lo + len(p)] = d2.reshape(len(p), -1).max(axis=1)
    return np.where(out <= limit2, np.sqrt(out), np.inf)


# ---- rotations ---------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """[3,3]: Rodrigues' rotation by `angle` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt(a @ a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def about(R, centre):
    """[4,4]: x -> R (x - centre) + centre."""
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(centre, np.float64) - R @ np.asarray(centre, np.float64)
    return T


def angle_deg(Ra, Rb):
    """The rotation distance of two rotation matrices in degrees."""
    return math.degrees(math.acos(min(1.0, max(-1.0, (float(np.trace(Ra.T @ Rb)) - 1.0) / 2.0))))


def angles_deg(Ra, Rb):
    """[a,b] rotation distances of Ra [a,3,3] and Rb [b,3,3]."""
    tr = np.einsum("aij,bij->ab", np.asarray(Ra), np.asarray(Rb))
    return np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


def fibonacci_hemisphere(k):
    i = np.arange(int(k), dtype=np.float64)
    z = (i + 0.5) / float(k)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def coarse_candidates(num_axes, centre):
    """([3 num_axes,4,4] transforms, [3 num_axes,3,3] rotations): every grid axis under the three coarse angles."""
    R = np.stack([rotation(a, th) for th in COARSE_ANGLES for a in fibonacci_hemisphere(num_axes)])
    return np.stack([about(r, centre) for r in R]), R


def order_from_mask(passed, steps=ORDER_STEPS):
    """The largest n dividing `steps` such that passed[k steps / n - 1] for every k = 1 .. n - 1; 1 when there is none."""
    best = 1
    for n in range(2, steps + 1):
        if steps % n == 0 and all(passed[k * (steps // n) - 1] for k in range(1, n)):
            best = n
    return best


def discretisation_count(r_max, diameter, disc_step=0.01):
    """The smallest n >= 2 with 2 r_max sin(pi / n) <= disc_step diameter, by counting up."""
    n = 2
    while 2.0 * r_max * math.sin(math.pi / n) > disc_step * diameter:
        n += 1
    return n


def diameter_of(points):
    p = np.asarray(points, np.float64)[:, :3]
    d = p[:, None, :] - p[None, :, :]
    return float(np.sqrt((d * d).sum(axis=2).max()))


def find_symmetries(targets, queries, diameter, tol=0.02, num_axes=2048, merge_deg=5.0, disc_step=0.01, scores=None):
    """The procedure without sharpening: dict(kind, count, orders, epsilon, h0).  `scores`: the scoring function
    (default hausdorff_scores_fast)."""
    scores = scores or hausdorff_scores_fast
    t = np.asarray(targets, np.float32)[:, :3].astype(np.float64)
    centre = t.mean(axis=0)
    h0 = float(scores(queries, targets, np.eye(4)[None])[0])
    eps = h0 + tol * diameter
    cand, R = coarse_candidates(num_axes, centre)
    s = scores(queries, targets, cand, eps * eps)
    axes = []
    grid = np.concatenate([fibonacci_hemisphere(num_axes)] * 3)
    for i in np.argsort(s, kind="stable"):
        if not np.isfinite(s[i]):
            break
        if all(math.degrees(math.acos(min(1.0, abs(float(grid[i] @ a))))) > merge_deg for a in axes):
            axes.append(grid[i])
    orders = []
    for a in axes:
        sweep = np.stack([about(rotation(a, 2.0 * math.pi * k / ORDER_STEPS), centre) for k in range(1, ORDER_STEPS)])
        orders.append(order_from_mask(np.isfinite(scores(queries, targets, sweep, eps * eps))))
    keep = [i for i, n in enumerate(orders) if n > 1]
    axes, orders = [axes[i] for i in keep], [orders[i] for i in keep]
    cont = [i for i, n in enumerate(orders) if n == ORDER_STEPS]
    out = dict(epsilon=eps, h0=h0, orders=orders, axes=axes)
    if not axes:
        out.update(kind="none", count=1)
    elif len(cont) >= 2:
        out.update(kind="spherical", count=1)
    elif len(cont) == 1:
        a = axes[cont[0]]
        r = t - centre[None]
        r_max = float(np.sqrt(((r - (r @ a)[:, None] * a[None]) ** 2).sum(axis=1)).max())
        n = discretisation_count(r_max, diameter, disc_step)
        flip = any(i != cont[0] and abs(float(axes[i] @ a)) <= math.sin(math.radians(merge_deg)) for i in range(len(axes)))
        out.update(kind="axial", count=n * (2 if flip else 1), steps=n)
    else:
        members = [np.eye(3)]
        for a, n in zip(axes, orders):
            for k in range(1, n):
                r = rotation(a, 2.0 * math.pi * k / n)
                if all(angle_deg(r, m) > merge_deg for m in members):
                    members.append(r)
        out.update(kind="finite", count=len(members))
    return out


# ---- the test solids -----------------------------------------------------------------------------------------------------
# a fixed, non-trivial rigid motion: no symmetry axis of a solid is a coordinate axis
MOTION_R = rotation((2.0, -1.0, 1.0), 1.0)
MOTION_T = np.array([0.031, -0.047, 0.62])

# the proportions (metres) and why: tests/test_symmetry_host.py, "margins"
BOX = (0.10, 0.075, 0.05)                  # half-edges, all different
SQUARE_PRISM = (0.10, 0.07)                # half-length along its axis, half-edge of the square
TRI_PRISM = (0.07, 0.08)                   # half-height, circumradius of the equilateral triangle
CYLINDER = (0.08, 0.05, 24)                # half-height, radius, sides
L_SOLID = (0.16, 0.10, 0.05, 0.06)         # long leg, short leg, leg width, thickness


def _moved(v):
    return (np.asarray(v, np.float64) @ MOTION_R.T + MOTION_T[None]).astype(np.float32)


def _prism(poly, h):
    """A right prism over the convex-or-not polygon poly [k,2] (counter-clockwise, a fan from vertex 0 must triangulate
    it) between z = -h and z = +h: (vertices [2k,3], triangles [4k-4,3])."""
    k = len(poly)
    v = np.array([[x, y, -h] for x, y in poly] + [[x, y, h] for x, y in poly], np.float64)
    t = []
    for i in range(1, k - 1):
        t.append([0, i + 1, i])
        t.append([k, k + i, k + i + 1])
    for i in range(k):
        j = (i + 1) % k
        t.append([i, j, k + j])
        t.append([i, k + j, k + i])
    return v, np.array(t, np.int32)


def _group(elements):
    """Local rotations -> the same in the moved frame."""
    return np.stack([MOTION_R @ r @ MOTION_R.T for r in elements])


def solid(name):
    """(vertices [V,3] float32 under the fixed motion, triangles [T,3] int32, group [g,3,3]: the solid's proper rotations
    in the moved frame with the identity first (for the cylinder a spread of them), centre [3], axis or None)."""
    ex, ey, ez = np.eye(3)
    if name == "box":
        a, b, c = BOX
        v, t = _prism([(-a, -b), (a, -b), (a, b), (-a, b)], c)
        g = [np.eye(3)] + [rotation(e, math.pi) for e in (ex, ey, ez)]
    elif name == "square_prism":
        h, s = SQUARE_PRISM
        v, t = _prism([(-s, -s), (s, -s), (s, s), (-s, s)], h)
        g = [np.eye(3)] + [rotation(ez, k * math.pi / 2.0) for k in (1, 2, 3)] + \
            [rotation(e, math.pi) for e in (ex, ey, ex + ey, ex - ey)]
    elif name == "tri_prism":
        h, r = TRI_PRISM
        corners = [(r * math.cos(2.0 * math.pi * k / 3.0), r * math.sin(2.0 * math.pi * k / 3.0)) for k in range(3)]
        v, t = _prism(corners, h)
        g = [np.eye(3)] + [rotation(ez, k * 2.0 * math.pi / 3.0) for k in (1, 2)] + \
            [rotation((c[0], c[1], 0.0), math.pi) for c in corners]
    elif name == "cylinder":
        h, r, k = CYLINDER
        v, t = _prism([(r * math.cos(2.0 * math.pi * i / k), r * math.sin(2.0 * math.pi * i / k)) for i in range(k)], h)
        g = [np.eye(3)] + [rotation(ez, 2.0 * math.pi * i / ORDER_STEPS) for i in range(7, ORDER_STEPS, 7)] + \
            [rotation((math.cos(u), math.sin(u), 0.0), math.pi) for u in np.arange(12) * 0.2618 + 0.1]
    elif name == "l_solid":
        p, q, w, h = L_SOLID
        v, t = _prism([(0.0, 0.0), (p, 0.0), (p, w), (w, w)], h)             # the long leg, then the rest of the short one
        v2, t2 = _prism([(0.0, 0.0), (w, w), (w, q), (0.0, q)], h)
        t = np.concatenate([t, t2 + len(v)])
        v = np.concatenate([v, v2])
        # the two prisms share the diagonal wall from (0, 0) to (w, w): its four triangles are inside the solid
        keep = [i for i, tri in enumerate(t) if not _on_diagonal(v[tri])]
        t = t[keep]
        g = [np.eye(3)]
    else:
        raise ValueError(name)
    local_centre = surface_centroid(v, t)
    v = v - local_centre[None]
    axis = MOTION_R @ ez if name in ("cylinder", "square_prism", "tri_prism") else None
    return _moved(v), t.astype(np.int32), _group(g), MOTION_T.copy(), axis


def _on_diagonal(tri):
    return bool(np.all(np.abs(tri[:, 0] - tri[:, 1]) < 1e-12))


def surface_centroid(v, t):
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1))
    return ((a + b + c) / 3.0 * area[:, None]).sum(axis=0) / area.sum()


SOLIDS = ("box", "square_prism", "tri_prism", "cylinder", "l_solid")
EXPECTED_COUNT = {"box": 4, "square_prism": 8, "tri_prism": 6, "l_solid": 1}


def sample_surface(vertices, triangles, n, seed):
    """n points uniform by area on the mesh from numpy's default_rng(seed): [n,3] float32."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1))
    tri = rng.choice(len(triangles), size=n, p=area / area.sum())
    u, w = rng.random(n), rng.random(n)
    flip = u + w > 1.0
    u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
    return (a[tri] + u[:, None] * (b[tri] - a[tri]) + w[:, None] * (c[tri] - a[tri])).astype(np.float32)
