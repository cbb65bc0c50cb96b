"""Scenes that put cloudaae_render_frames (csrc/render.hip) on its boundaries: samples on edges and vertices, boxes at
the lane/wave threshold, a queue longer than its grid of waves, the ends of the depth range, the near plane and the
guard band, launch sizes around a block, and thousands of triangles racing for one cell.  No GPU here:
tests/test_render_edges_host.py proves on the CPU that every scene has the property it is named for, and
tests/test_40_render_edges_gpu.py holds the kernel to tests/render_reference.py on them, bit for bit.

Everything is dyadic.  A piece is given in PIXELS: the vertex (px Z, py Z, Z) under fx = fy = 1, cx = cy = 0 and the
identity pose projects to (px, py) exactly when Z is a power of two (or a small multiple of 1/64) and px, py are
multiples of 1/512, so fixed-point vertices, edge values and du are what the builder writes down.

scene(family, case) -> (meshes, frames, intr, H, W, z_near), the form render_reference.render and test_25's launch take;
CASES[family] lists the cases."""
import functools
import os
import re

import numpy as np

import render_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "cloudaae_amd", "csrc", "render.hip")).read()
RN_SMALL = int(re.search(r"#define CLOUDAAE_RN_SMALL (\d+)", SRC).group(1))
RN_BLOCK = int(re.search(r"constexpr int RN_BLOCK = (\d+);", SRC).group(1))
RN_QUEUE_BLOCKS = int(re.search(r"constexpr int RN_QUEUE_BLOCKS = (\d+);", SRC).group(1))
WAVES = RN_QUEUE_BLOCKS * RN_BLOCK // 64          # the queue kernel's grid, in waves
S = RN_SMALL

EYE = np.eye(4)
UNIT = [1.0, 1.0, 0.0, 0.0]                        # fx, fy, cx, cy: screen = (X / Z, Y / Z)
EMPTY_MESH = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))


def mesh_of(tris):
    """[((px, py, Z), (px, py, Z), (px, py, Z))] -> (vertices [3T,3] float32, triangles [T,3]): unshared vertices."""
    p = np.asarray(tris, np.float64).reshape(-1, 3)
    v = np.stack([p[:, 0] * p[:, 2], p[:, 1] * p[:, 2], p[:, 2]], axis=1)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "not exact in float32"
    return v32, np.arange(len(p), dtype=np.int32).reshape(-1, 3)


def flat(points, z=1.0):
    """A triangle of pixel points at one depth."""
    return tuple((x, y, z) for x, y in points)


def intr_rows(n, factor=1000.0, k=UNIT):
    return np.array([list(k) + [factor]] * n, np.float32)


def scaled(s, shift=(0.0, 0.0)):
    """A pose that takes the vertex (px, py, 1) to ((px + sx) s, (py + sy) s, s): the pixel (px + sx, py + sy) at depth s."""
    T = np.diag([float(s), float(s), float(s), 1.0])
    T[:3, 3] = [shift[0] * s, shift[1] * s, 0.0]
    return T


def right_triangle(x0, y0, w, h, mirror=False, z=1.0):
    """A right triangle whose box is exactly the w x h samples from (x0, y0): its corners lie half a pixel outside
    them.  mirror: the right angle at the far corner, so that the box's last column and row are covered."""
    xa, xb, ya, yb = x0 - 0.5, x0 + w - 0.5, y0 - 0.5, y0 + h - 0.5
    if mirror:
        return flat([(xb, yb), (xa, yb), (xb, ya)], z)
    return flat([(xa, ya), (xb, ya), (xa, yb)], z)


# ---- on_edge ---------------------------------------------------------------------------------------------------------------
HALF_VERTEX = (10 + 1.0 / 512, 2.0)     # sx 256 = 2560.5: half-up 2561, half-even 2560
HALF_FACTOR = 1000.5                     # z = 1: z factor = 1000.5: half-up 1001, half-even 1000


def _on_edge(case):
    H = W = 48
    if case == 'slopes':
        # vertices on samples; edges along rows, columns, the diagonal and slopes 1/2, 2, -1/3; every triangle in both
        # windings, the second copy in a frame of its own
        t = [flat([(2, 2), (18, 2), (2, 18)]), flat([(20, 2), (40, 12), (20, 12)]), flat([(2, 22), (12, 42), (2, 42)]),
             flat([(20, 30), (44, 22), (44, 30)]), flat([(20, 14), (30, 14), (30, 19)]), flat([(16, 34), (30, 34), (23, 46)])]
        back = [(a, c, b) for a, b, c in t]
        return [mesh_of(t), mesh_of(back)], [[(0, 1, EYE)], [(1, 2, EYE)]], intr_rows(2), H, W, 0.05
    if case == 'shared':
        # pairs sharing an edge: (far, near) and (near, far) in draw order, a pair at one depth, and each with the other
        # winding; the shared edges are a diagonal, a slope of 1/2 and a row
        def pair(x, y, za, zb, flip):
            a = ((x, y, za), (x + 12, y, za), (x, y + 12, za))
            b = ((x + 12, y, zb), (x + 12, y + 12, zb), (x, y + 12, zb))
            return [a, (b[0], b[2], b[1]) if flip else b]
        t = pair(2, 2, 1.0, 0.5, False) + pair(18, 2, 0.5, 1.0, True) + pair(34, 2, 1.0, 1.0, False)
        t += [((2, 20, 1.0), (22, 30, 1.0), (2, 30, 1.0)), ((2, 20, 0.25), (22, 20, 0.25), (22, 30, 0.25))]      # slope 1/2
        t += [((26, 20, 0.5), (46, 20, 0.5), (36, 28, 0.5)), ((46, 20, 2.0), (26, 20, 2.0), (36, 16, 2.0))]       # a row
        return [mesh_of(t)], [[(0, 3, EYE)]], intr_rows(1, 1024.0), H, W, 0.05
    if case == 'slivers':
        t = [flat([(2.5, 2.75), (10.5, 10.75), (2.5, 3.0)]),               # 8 x 8 samples in the box, none covered
             flat([(14.25, 2.5), (17.75, 5.75), (14.25, 2.75)]),           # 3 x 3 (the lane path), none covered
             flat([(2.25, 20.25), (2.75, 20.5), (2.5, 20.75)]),            # no sample in the box
             flat([(20.25, 20.0), (20.75, 30.0), (20.5, 40.0)]),           # no column in the box, rows in plenty
             flat([(30.0, 20.0), (30.0, 40.0), (30 + 1.0 / 256, 30.0)]),   # one column, covered along the edge x = 30
             flat([(2, 30), (16, 30 + 1.0 / 256), (2, 30 + 2.0 / 256)])]   # one row, covered at its first sample only
        return [mesh_of(t)], [[(0, 4, EYE)]], intr_rows(1), H, W, 0.05
    if case == 'negative':
        e = 1.0 / 256
        t = [flat([(-3, -2), (5, -2), (-3, 6)]),                           # integral minima below zero
             flat([(-3 + e, 10 + e), (4 + e, 10 + e), (-3 + e, 17 + e)]),  # k + 1/256 minima and maxima
             flat([(-8, 20), (-e, 20), (-8, 30)]),                         # the largest x is -1/256: nothing
             flat([(-8, 32), (0, 32), (-8, 44)]),                          # the largest x is 0: the vertex sample alone
             flat([(20, -6), (30, -e), (40, -6)]),                         # the largest y is -1/256: nothing
             flat([(20, -6), (30, 0), (40, -6)], 0.5),                     # the largest y is 0
             flat([(40 + e, 40 + e), (47 + e, 40 + e), (40 + e, 47 + e)])]
        return [mesh_of(t)], [[(0, 5, EYE)]], intr_rows(1), H, W, 0.05
    if case == 'half_vertex':
        # the edge from HALF_VERTEX to (2559 / 256, 4) passes through the sample (10, 3) when the half rounds up and to
        # its left when it rounds to even; the triangle lies to the left
        t = [flat([HALF_VERTEX, (2559.0 / 256, 4.0), (2.0, 3.0)])]
        return [mesh_of(t)], [[(0, 6, EYE)]], intr_rows(1), H, W, 0.05
    if case == 'half_depth':
        t = [flat([(2, 2), (18, 2), (2, 18)]), flat([(20, 4), (40, 4), (30, 30)], 0.5)]
        return [mesh_of(t)], [[(0, 7, EYE)]], intr_rows(1, HALF_FACTOR), H, W, 0.05
    raise KeyError(case)


# ---- box_threshold ---------------------------------------------------------------------------------------------------------
BOXES = dict([('lane_1x%d' % (S - 1), (1, S - 1)), ('lane_1x%d' % S, (1, S)), ('wave_1x%d' % (S + 1), (1, S + 1)),
              ('lane_%dx1' % (S - 1), (S - 1, 1)), ('lane_%dx1' % S, (S, 1)), ('wave_%dx1' % (S + 1), (S + 1, 1)),
              ('lane_4x4', (4, 4)), ('lane_2x8', (2, 8)), ('wave_3x6', (3, 6)), ('wave_8x8', (8, 8)), ('wave_9x9', (9, 9)),
              ('wave_1x65', (1, 65)), ('wave_65x1', (65, 1)), ('wave_7x64', (7, 64)), ('wave_7x65', (7, 65)),
              ('wave_15x17', (15, 17))])
assert S % 4 == 0 and 4 <= S <= 60
CORNERS = {'corner_%d' % S: (4, S // 4), 'corner_%d' % (S + 1): (1, S + 1)}


def _box_threshold(case):
    H = W = 72
    if case in BOXES:
        w, h = BOXES[case]
        t = [[right_triangle(3, 4, w, h)], [right_triangle(3, 4, w, h, mirror=True)]]
    else:
        # a triangle of hundreds of pixels that the image's far corner clamps to w x h samples
        w, h = CORNERS[case]
        x, y = W - w - 0.5, H - h - 0.5
        t = [[flat([(x, y), (x + 300, y), (x, y + 300)])], [flat([(x, y), (x, y + 300), (x + 300, y)])]]      # both windings
    return [mesh_of(t[0]), mesh_of(t[1])], [[(0, 1, EYE)], [(1, 2, EYE)]], intr_rows(2), H, W, 0.05


# ---- queue_stride ----------------------------------------------------------------------------------------------------------
def _grid_cells():
    """The number of cells per side: the smallest even n whose 3/4 of 2 n^2 triangles (the cells of 3 x 4, 4 x 3 and 4 x 4
    pixels) exceed two trips of the queue's grid by a wave or more."""
    n = 2
    while 3 * n * n // 2 <= 2 * WAVES + 64:
        n += 2
    return n


def _queue_stride(case):
    n = _grid_cells()
    lines = np.cumsum([0] + [3 if i % 2 == 0 else 4 for i in range(n)])
    H = W = int(lines[-1]) + 1
    grid = []
    for r in range(n):
        for c in range(n):
            x0, x1, y0, y1 = lines[c], lines[c + 1], lines[r], lines[r + 1]
            grid += [flat([(x0, y0), (x1, y0), (x1, y1)]), flat([(x0, y0), (x1, y1), (x0, y1)])]
    # the second instance, frame 1: `pad` small triangles so that its pattern starts a wave, then 64 large, 64 small, a wave
    # whose lane 0 alone is large and a wave whose lane 63 alone is large
    pad = (-len(grid)) % 64
    kinds = [0] * pad + [1] * 64 + [0] * 64 + [1] + [0] * 63 + [0] * 63 + [1]
    cols = W // 8
    assert (len(kinds) + cols - 1) // cols * 8 <= H
    ballots = [right_triangle(1 + 8 * (i % cols), 1 + 8 * (i // cols), 5 if k else 3, 5 if k else 3, mirror=i % 2 == 1)
               for i, k in enumerate(kinds)]
    return [mesh_of(grid), mesh_of(ballots)], [[(0, 1, EYE)], [(1, 2, EYE)]], intr_rows(2), H, W, 0.05


def ballot_start():
    """The rank at which the second instance's pattern starts (a multiple of 64)."""
    n = _grid_cells()
    return (2 * n * n + 63) // 64 * 64


# ---- depth_range -----------------------------------------------------------------------------------------------------------
RANGE_Z = 2.0 ** -4
_below = lambda x: float(np.nextafter(np.float32(x), np.float32(0)))
RANGE_FACTORS = {'du_1': 8.0, 'du_0': _below(8.0), 'du_65535': 65535.0 * 16, 'du_65535_high': _below(65535.5 * 16),
                 'du_65536': 65535.5 * 16}
RANGE_VALUES = {'du_1': {0, 1}, 'du_0': {0}, 'du_65535': {0, 65535}, 'du_65535_high': {0, 65535}, 'du_65536': {0}}


def _depth_range(case):
    H = W = 48
    if case in RANGE_FACTORS:
        sq = [flat([(4, 4), (20, 4), (20, 20)], RANGE_Z), flat([(4, 4), (20, 20), (4, 20)], RANGE_Z),
              right_triangle(30, 6, 3, 3, z=RANGE_Z)]
        return [mesh_of(sq)], [[(0, 1, EYE)]], intr_rows(1, RANGE_FACTORS[case]), H, W, 2.0 ** -6
    if case == 'tilted':
        # 1 / z runs from 2^14 to 2^-5 across the box: du is 0 near the first vertex and 65536 on the far edge (factor 2048)
        t = [((4, 4, 2.0 ** -14), (44, 4, 32.0), (44, 44, 32.0)), ((4, 10, 2.0 ** -14), (4, 46, 32.0), (40, 46, 32.0)),
             ((2, 2, 2.0 ** -13), (5, 2, 2.0 ** -11), (2, 5, 2.0 ** -11))]      # the lane path: du 0 at (2, 2), 1 at the others
        # frame 1, the far end alone at a finer grain: du from 32768 to 131072, the cut two thirds along
        far = [((4, 4, 16.0), (44, 4, 64.0), (4, 44, 64.0))]
        return [mesh_of(t), mesh_of(far)], [[(0, 1, EYE)], [(1, 2, EYE)]], intr_rows(2, 2048.0), H, W, 2.0 ** -16
    raise KeyError(case)


# ---- near_and_guard --------------------------------------------------------------------------------------------------------
NEAR_Z = 0.25
GUARD_FACTOR = 1234.0


def _near_and_guard(case):
    H = W = 64
    if case in ('near_equal', 'near_above'):
        # one vertex at Z = z_near, shared by both triangles; the other three deeper
        v = np.array([[4 * NEAR_Z, 4 * NEAR_Z, NEAR_Z], [40 * 0.5, 4 * 0.5, 0.5], [40 * 0.5, 40 * 0.5, 0.5], [4 * 0.5, 40 * 0.5, 0.5],
                      [50, 50, 1], [60, 50, 1], [50, 60, 1]], np.float32)
        t = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
        z_near = NEAR_Z if case == 'near_equal' else float(np.nextafter(NEAR_Z, 1.0))
        return [(v, t)], [[(0, 1, EYE)]], intr_rows(1), H, W, z_near
    if case in ('guard_on', 'guard_past'):
        # fixed-point vertices (-2^24, -2^24), (2^24, -2^24), (0, 2^24); with cx = 1/256 the second becomes 2^24 + 1.  A
        # small neighbour in a frame of its own draws either way.
        v = np.array([[-65536, -65536, 1], [65536, -65536, 1], [0, 65536, 1]], np.float32)
        k = [1.0, 1.0, 0.0 if case == 'guard_on' else 1.0 / 256, 0.0]
        near = mesh_of([flat([(2, 2), (9, 2), (2, 9)], 0.5)])
        return ([(v, np.array([[0, 1, 2]], np.int32)), near], [[(0, 1, EYE)], [(1, 2, EYE)]], intr_rows(2, GUARD_FACTOR, k),
                H, W, 0.05)
    if case == 'bad_vertices':
        # a row of 14 triangles on 16 shared vertices: vertex 2 lies behind the camera, vertex 7 at Z = +0, vertex 12 has
        # a NaN; each spoils the three triangles that use it
        v = np.array([[2 + 4 * i, 4 + 10 * (i % 2), 1] for i in range(16)], np.float32)
        v[2, 2], v[7, 2], v[12, 1] = -1.0, 0.0, np.nan
        t = np.array([[i, i + 1, i + 2] for i in range(14)], np.int32)
        good = mesh_of([flat([(2, 2), (20, 2), (2, 12)])])
        inf_x, inf_z, nan_pose = EYE.copy(), EYE.copy(), EYE.copy()
        inf_x[0, 3], inf_z[2, 3], nan_pose[1, 0] = np.inf, np.inf, np.nan
        frames = [[(0, 1, EYE), (1, 2, scaled(1.0, (0, 20))), (1, 3, inf_x), (1, 4, scaled(1.0, (20, 20))), (1, 5, inf_z),
                   (1, 6, nan_pose), (1, 7, scaled(0.5, (0, 34)))]]
        return [(v, t), good], frames, intr_rows(1), H, W, 0.05
    raise KeyError(case)


# ---- launch_bounds ---------------------------------------------------------------------------------------------------------
SUMS = {'sums_255': (100, 100, 55), 'sums_256': (100, 100, 56), 'sums_257': (1, 128, 128), 'sums_513': (256, 1, 256)}
IMAGES = {'image_1x1': (1, 1, 1), 'image_1x97': (1, 1, 97), 'image_97x1': (1, 97, 1), 'pixels_255': (3, 5, 17),
          'pixels_256': (4, 8, 8), 'pixels_257': (1, 1, 257)}
MANY_FRAMES = 300
MANY_EMPTY = (0, 1, 150, 299)
LABELS = (1, 255, 256, 263, 0)


def strip(n):
    """A zigzag strip of n vertices and as many triangles (triangle k on vertices k, k + 1, k + 2 modulo n - 2, so the
    first two are drawn twice); n = 1: one vertex and a triangle that names it three times (degenerate)."""
    if n < 3:
        return (np.array([[1, 1, 1]] * n, np.float32), np.zeros((n, 3), np.int32))
    v = np.array([[1 + 0.25 * (i // 2), 1 + 5 * (i % 2) + (i % 4) * 0.25, 1] for i in range(n)], np.float32)
    t = np.array([[k % (n - 2) + d for d in range(3)] for k in range(n)], np.int32)
    return v, t


def _many_frames():
    one = mesh_of([flat([(0.5, 0.5), (5.5, 0.5), (0.5, 4.5)])])
    two = mesh_of([flat([(0, 0), (6, 0), (6, 4)]), flat([(0, 0), (6, 4), (0, 4)], 2.0)])
    no_tri = (np.array([[1, 1, 1], [2, 1, 1]], np.float32), np.zeros((0, 3), np.int32))
    meshes = [one, two, no_tri, EMPTY_MESH]
    order = [2, 3, 0, 1, 0, 2, 2, 1, 1, 3]            # zero-triangle meshes first and twice in a row
    frames, intr, k = [], [], 0
    for f in range(MANY_FRAMES):
        intr.append([1.0 + 0.25 * (f % 3), 1.0 + 0.5 * (f % 2), (f % 4) * 0.25, (f % 5) * 0.125, 100.0 + f])
        if f in MANY_EMPTY:
            frames.append([])
            continue
        m = 2 if f == MANY_FRAMES - 2 else order[k % len(order)]     # ... and last
        frames.append([(m, 1 + f % 255, EYE)])
        k += 1
    return meshes, frames, np.array(intr, np.float32), 5, 7, 0.05


def _launch_bounds(case):
    if case in SUMS:
        sizes = SUMS[case]
        meshes = [strip(n) for n in sizes]
        frames = [[(i, i + 1, scaled(1.0, (0, 8 * i))) for i in range(len(sizes))]]
        return meshes, frames, intr_rows(1), 8 * len(sizes), 72, 0.05
    if case in IMAGES:
        F, H, W = IMAGES[case]
        big = mesh_of([flat([(-3, -3), (600, -3), (-3, 600)]), flat([(0, 0), (2, 0), (0, 2)], 0.5)])
        frames = [[(0, f + 1, scaled(2.0 ** -f))] for f in range(F)]
        return [big], frames, intr_rows(F), H, W, 0.05
    if case == 'many_frames':
        return _many_frames()
    if case == 'labels':
        patch = mesh_of([flat([(0, 0), (6, 0), (0, 6)])])
        frames = [[(0, lab, scaled(1.0, (1 + 8 * i, 1))) for i, lab in enumerate(LABELS)]]
        return [patch], frames, intr_rows(1), 9, 8 * len(LABELS), 0.05
    raise KeyError(case)


# ---- contention ------------------------------------------------------------------------------------------------------------
RACERS = 3000
PATCH = flat([(1.5, 1.5), (16.5, 1.5), (1.5, 16.5)])       # covers the 7 x 7 samples 2 .. 8 whole
CHIP = flat([(1.5, 1.5), (5.5, 1.5), (1.5, 5.5)])          # a 4 x 4 box: the lane path


def _contention(case):
    H = W = 12
    if case == 'decreasing':
        # 3000 instances of one triangle; the depth 1 - k / 64 of instance j, k = j // 100: 6400 - 100 k units
        frames = [[(0, 1 + j % 250, scaled(1.0 - (j // 100) / 64.0)) for j in range(RACERS)]]
        return [mesh_of([PATCH])], frames, intr_rows(1, 6400.0), H, W, 0.05
    if case == 'same_depth':
        return [mesh_of([PATCH] * RACERS)], [[(0, 9, EYE)]], intr_rows(1, 6400.0), H, W, 0.05
    if case == 'lane_and_wave':
        # the same race with every even instance a small triangle rasterised by its setup lane: it wins its samples, the
        # next rank the others
        frames = [[((j + 1) % 2, 1 + j % 250, scaled(1.0 - (j // 100) / 64.0)) for j in range(RACERS)]]
        return [mesh_of([PATCH]), mesh_of([CHIP])], frames, intr_rows(1, 6400.0), H, W, 0.05
    raise KeyError(case)


_BUILDERS = dict(on_edge=_on_edge, box_threshold=_box_threshold, queue_stride=_queue_stride, depth_range=_depth_range,
                 near_and_guard=_near_and_guard, launch_bounds=_launch_bounds, contention=_contention)
CASES = dict(on_edge=['slopes', 'shared', 'slivers', 'negative', 'half_vertex', 'half_depth'],
             box_threshold=list(BOXES) + list(CORNERS),
             queue_stride=['grid_and_ballots'],
             depth_range=list(RANGE_FACTORS) + ['tilted'],
             near_and_guard=['near_equal', 'near_above', 'guard_on', 'guard_past', 'bad_vertices'],
             launch_bounds=list(SUMS) + list(IMAGES) + ['many_frames', 'labels'],
             contention=['decreasing', 'same_depth', 'lane_and_wave'])
ALL = [(family, case) for family in CASES for case in CASES[family]]


@functools.lru_cache(maxsize=None)
def scene(family, case):
    return _BUILDERS[family](case)


@functools.lru_cache(maxsize=None)
def reference(family, case, variant=None):
    """render_reference.render of the scene, computed once per process; the arrays are shared: do not write to them."""
    meshes, frames, intr, H, W, z_near = scene(family, case)
    out = R.render(meshes, frames, intr, H, W, z_near, variant=variant)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- what the host test measures ---------------------------------------------------------------------------------------------
def setups(family, case):
    """Per draw rank of the scene: None (dropped or degenerate) or dict(frame, xs, ys (fixed point, b and c swapped to a
    positive area), box (u0, u1, v0, v1), area2)."""
    meshes, frames, intr, H, W, z_near = scene(family, case)
    offs, mesh, lab, poses, vb, tb = R.instance_bases(meshes, frames)
    out = []
    for f in range(len(frames)):
        for j in range(offs[f], offs[f + 1]):
            v, t = meshes[mesh[j]][0], np.asarray(meshes[mesh[j]][1], np.int64).reshape(-1, 3)
            ix, iy, iz, ok = R.project(v, poses[j], intr[f], z_near)
            for ids in t:
                if np.any(ids < 0) or np.any(ids >= len(ix)) or not np.all(ok[ids]):
                    out.append(None)
                    continue
                xs, ys = [int(c) for c in ix[ids]], [int(c) for c in iy[ids]]
                area2 = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
                if area2 == 0:
                    out.append(None)
                    continue
                if area2 < 0:
                    xs, ys, area2 = [xs[0], xs[2], xs[1]], [ys[0], ys[2], ys[1]], -area2
                u0, u1 = max(-((-min(xs)) // 256), 0), min(max(xs) // 256, W - 1)
                v0, v1 = max(-((-min(ys)) // 256), 0), min(max(ys) // 256, H - 1)
                out.append(dict(frame=f, xs=xs, ys=ys, box=(u0, u1, v0, v1), area2=area2))
    return out


def edge_values(s):
    """(wa, wb, wc) int64 arrays over the clamped box of one setups() entry (rows v0 .. v1, columns u0 .. u1)."""
    (ax, bx, cx), (ay, by, cy) = s['xs'], s['ys']
    u0, u1, v0, v1 = s['box']
    px = (np.arange(u0, u1 + 1, dtype=np.int64) * 256)[None, :]
    py = (np.arange(v0, v1 + 1, dtype=np.int64) * 256)[:, None]
    wa = (cx - bx) * (py - by) - (cy - by) * (px - bx)
    wb = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    wc = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return wa, wb, wc


def box_dims(s):
    u0, u1, v0, v1 = s['box']
    return max(u1 - u0 + 1, 0), max(v1 - v0 + 1, 0)
