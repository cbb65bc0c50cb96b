"""NumPy restatement of what oracle/synth_oracle.py leaves out of csrc/synth.hip -- the two random parts (occluder_kernel,
the padded rows of hpr_gather_kernel), both counter-based Philox and therefore exact functions of (seed, counter, stream) --
and the table of hull-vertex cases that tests/test_synth_reference_host.py (the inputs' conditions, on the CPU) and
tests/test_50_synth_paths_gpu.py (the kernels) both read, so that the two see identical arrays.  Import-only.

The transform, the flip and qhull come from oracle/synth_oracle.py; philox4x32, u01 and normal2 from
tests/pose_sampling_reference.py.  `dtype` is float32 (the kernel's arithmetic) or float64 (the same formula evaluated
wider: how far fp32 rounding can move a result, which sizes the occluder test's tolerance)."""
import collections
import functools
import math
import os

import numpy as np
from scipy.spatial import ConvexHull

import pose_sampling_reference as P
from oracle import synth_oracle as SO

STREAM_CENTRE_XY, STREAM_CENTRE_Z, STREAM_POINT_A, STREAM_POINT_B, STREAM_PADDING = 1, 2, 3, 4, 7
MARGIN_BOUND = 1e-10        # of the bounding-box diagonal: two orders above the kernel's HPR_EPS = 1e-12


# ---- occluder_kernel ----------------------------------------------------------------------------------------------------
def spherical_occluder(trans, per, wnear, hnear, near, sigma, seed, dtype=np.float32):
    """occluder_kernel line by line: [b, 2 * per, 3].  Streams 1 and 2 at counter `cloud` give the two blob centres (x from
    words 0, 1 of stream 1, y from words 2, 3 of stream 1, z from words 0, 1 of stream 2); streams 3 and 4 at counter
    (cloud << 32) | j give the six normals of pair j; rows 2j and 2j + 1 are blob 0 and blob 1.  The four scalars reach the
    kernel as floats, so they are rounded to fp32 first whatever `dtype` is."""
    f = dtype
    z = np.asarray(trans, np.float32)[:, 2].astype(f)
    b = z.shape[0]
    wnear, hnear, near, sigma = (f(np.float32(v)) for v in (wnear, hnear, near, sigma))
    cloud = np.arange(b, dtype=np.uint64)
    r1, r2 = P.philox4x32(seed, cloud, STREAM_CENTRE_XY), P.philox4x32(seed, cloud, STREAM_CENTRE_Z)
    x0, x1 = P.normal2(r1[:, 0], r1[:, 1], f)
    y0, y1 = P.normal2(r1[:, 2], r1[:, 3], f)
    z0, z1 = P.normal2(r2[:, 0], r2[:, 1], f)
    sx, sy, sz = wnear / f(10.0), hnear / f(10.0), (z - near) / f(6.0)
    mid = (near + z) / f(2.0)
    centre = np.stack([np.stack([x0 * sx, y0 * sy, mid + z0 * sz], axis=1),
                       np.stack([x1 * sx, y1 * sy, mid + z1 * sz], axis=1)], axis=1).astype(f)          # [b, blob, 3]
    ctr = ((cloud[:, None] << np.uint64(32)) | np.arange(per, dtype=np.uint64)[None, :]).reshape(-1)
    r3, r4 = P.philox4x32(seed, ctr, STREAM_POINT_A), P.philox4x32(seed, ctr, STREAM_POINT_B)
    g0, g1 = P.normal2(r3[:, 0], r3[:, 1], f)
    g2, g3 = P.normal2(r3[:, 2], r3[:, 3], f)
    g4, g5 = P.normal2(r4[:, 0], r4[:, 1], f)
    g = np.stack([g0, g1, g2, g3, g4, g5], axis=1).astype(f).reshape(b, per, 2, 3)                      # [b, j, blob, 3]
    occ = centre[:, None, :, :] + sigma * g
    return occ.reshape(b, 2 * per, 3).astype(f)


def occluder_tolerance(trans, per, wnear, hnear, near, sigma, seed):
    """(fp32 restatement, absolute tolerance): 10 x the largest change that evaluating the restatement in float64 makes,
    with a floor of 4 ulp of fp32 at the largest magnitude -- formed as pose_sampling_reference.float_tolerances forms its
    own, from the restatement alone."""
    o32 = spherical_occluder(trans, per, wnear, hnear, near, sigma, seed)
    o64 = spherical_occluder(trans, per, wnear, hnear, near, sigma, seed, dtype=np.float64)
    change = float(np.abs(o32.astype(np.float64) - o64).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(o32).max())))
    return o32, max(10.0 * change, floor)


# ---- spherical_flip_kernel ----------------------------------------------------------------------------------------------
def flip(a, b, center, param):
    """One cloud: concat(a, b) - center in fp32, then SO.spherical_flip.  Returns (flipped, org), the zero row appended."""
    a = np.asarray(a, np.float32).reshape(-1, 3)
    pts = a if b is None or len(b) == 0 else np.concatenate([a, np.asarray(b, np.float32).reshape(-1, 3)], 0)
    if center is not None:
        pts = pts - np.asarray(center, np.float32)[None, :]
    return SO.spherical_flip(pts, param)


# ---- hpr_gather_kernel --------------------------------------------------------------------------------------------------
def gather(vertex_ids, org, seed, h, rows):
    """hpr_gather_kernel in integers, for cloud h of a launch: (visible [rows, 3], num_vis, visible_id [rows], row_src
    [rows]).  ids ascending, nv = max(0, len(ids) - 2); rows below nv copy org[ids[r]], the others draw
    row = philox4x32(seed, (h << 32) | r, 7)[0] % nv; with nv == 0 rows are zeros, ids -1 and row_src -1."""
    ids = np.sort(np.asarray(vertex_ids, np.int64))
    org = np.asarray(org, np.float32)
    nv = max(0, len(ids) - 2)
    visible = np.zeros((rows, 3), np.float32)
    visible_id = np.full(rows, -1, np.int32)
    row_src = np.full(rows, -1, np.int32)
    if nv > 0:
        r = np.arange(rows, dtype=np.uint64)
        words = P.philox4x32(seed, (np.uint64(h) << np.uint64(32)) | r, STREAM_PADDING)[:, 0]
        row = np.where(r < np.uint64(nv), r.astype(np.int64), (words % np.uint32(nv)).astype(np.int64))
        visible = org[ids[row]]
        keep = min(nv, rows)
        visible_id[:keep] = ids[:keep]
        row_src = row.astype(np.int32)
    return visible, nv, visible_id, row_src


# ---- hull-vertex cases --------------------------------------------------------------------------------------------------
# points: what the hull test sees (fp32, the viewpoint is the last row); org: what the gather copies from; kind: 'gauss',
# 'flipped' or 'lattice'; corners: for a lattice, the ids its vertex set must be (the corners and the viewpoint)
HullCase = collections.namedtuple("HullCase", "name kind points org corners")

GAUSS_N1 = (5, 6, 7, 8, 9, 63, 64, 65, 66, 128, 129, 192, 193, 194, 195)
FLIPPED_N1 = (65, 193, 194, 1025, 4096, 4097, 4161) + tuple(range(5800, 6601, 100))


def gauss_cloud(n1, seed):
    """n1 - 1 standard normal points and the zero viewpoint row."""
    rng = np.random.default_rng([seed, n1])
    p = np.concatenate([rng.standard_normal((n1 - 1, 3)), np.zeros((1, 3))], 0).astype(np.float32)
    return HullCase("gauss_%d_s%d" % (n1, seed), "gauss", p, p, None)


def flipped_cloud(n1, seed):
    """A synthetic object model of n1 - 1 points (train_cloudAAE_ycbv.synthetic_object_models, on the CPU) under a random
    pose in front of the camera, flipped: what hidden point removal sees in training."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    model = T.synthetic_object_models(1, n1 - 1, seed=1000 + seed)[0, :, :3].numpy()
    rng = np.random.default_rng([seed, n1])
    ax = rng.standard_normal(3)
    ax = (ax / np.linalg.norm(ax) * rng.uniform(0, np.pi)).astype(np.float32)
    t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)], np.float32)
    f, o = SO.spherical_flip(SO.transform_object_model(model, ax, t))
    return HullCase("flipped_%d_s%d" % (n1, seed), "flipped", f, o, None)


def conforming_flipped_cloud(n1, first_seed=0, tries=8):
    """flipped_cloud(n1, seed) of the first seed from first_seed on that meets the host conditions (for a size known only
    on the GPU: the largest cloud the entry point accepts).  The choice looks at the inputs and qhull alone."""
    for seed in range(first_seed, first_seed + tries):
        case = flipped_cloud(n1, seed)
        if not conditions(case):
            return case
    raise AssertionError("no seed in %d..%d gives a %d-point flipped cloud inside the contract" % (first_seed, first_seed + tries - 1, n1))


def lattice_cube():
    """5 x 5 x 5 integer lattice at offset (3, -2, 7) and the zero viewpoint: 8 corners + the viewpoint are the vertices,
    every other point lies in a face, on an edge or inside."""
    i = np.arange(5)
    g = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3) + np.array([3, -2, 7])
    p = np.concatenate([g, np.zeros((1, 3))], 0).astype(np.float32)
    corners = [k for k in range(125) if all(c in (0, 4) for c in np.unravel_index(k, (5, 5, 5)))] + [125]
    return HullCase("lattice_5x5x5", "lattice", p, p, tuple(corners))


def lattice_plane():
    """7 x 7 integer grid in the plane z = 4 and the zero viewpoint: a pyramid over 4 corners, 45 more base points coplanar
    with them; the bounding box of the base has no extent in z."""
    i = np.arange(7)
    g = np.stack(np.meshgrid(i, i, indexing="ij"), -1).reshape(-1, 2) + np.array([-3, 1])
    p = np.concatenate([np.concatenate([g, np.full((49, 1), 4)], 1), np.zeros((1, 3))], 0).astype(np.float32)
    corners = [k for k in range(49) if all(c in (0, 6) for c in np.unravel_index(k, (7, 7)))] + [49]
    return HullCase("lattice_7x7_plane", "lattice", p, p, tuple(corners))


@functools.lru_cache(maxsize=None)
def hull_cases():
    """Every single-cloud case of the hull-vertex test, by name."""
    cases = [gauss_cloud(n1, 0) for n1 in GAUSS_N1] + [flipped_cloud(n1, 0) for n1 in FLIPPED_N1] + [lattice_cube(), lattice_plane()]
    return collections.OrderedDict((c.name, c) for c in cases)


HULL_CASE_NAMES = tuple(["gauss_%d_s0" % n for n in GAUSS_N1] + ["flipped_%d_s0" % n for n in FLIPPED_N1] +
                        ["lattice_5x5x5", "lattice_7x7_plane"])


@functools.lru_cache(maxsize=None)
def batch_cases():
    """Launches of several clouds, by name: a list of cases of one size each."""
    return collections.OrderedDict([
        ("b513_n9", [gauss_cloud(9, 100 + s) for s in range(513)]),
        ("b3_n9", [gauss_cloud(9, 1 + s) for s in range(3)]),
        ("b3_n194", [gauss_cloud(194, 1 + s) for s in range(3)]),
        # (seed 3 is left out: its cloud has a non-vertex 2.4e-12 of the diagonal below the hull, outside the contract)
        ("b3_n4097", [flipped_cloud(4097, s) for s in (1, 2, 4)]),
    ])


def golden_batch(golden_dir, b=3):
    """b clouds of 2449 points: the reference's own object model under its own pose records (tests/golden) with an explicit
    occluder blob between camera and object, flipped -- the shape of a training batch."""
    from cloudaae_amd import tfrecord_io as T
    models, _ = T.read_and_decode_obj_model(os.path.join(golden_dir, "obj_model_first1.tfrecords"))
    recs = T.PoseRecords([os.path.join(golden_dir, "pose_records_cls0_first4.tfrecords")])
    rng = np.random.default_rng(50)
    out = []
    for i in range(b):
        pts = SO.transform_object_model(models[0][:, :3], recs.axisangle[i], recs.translation[i])
        z = recs.translation[i][2]
        occ = (rng.standard_normal((400, 3)) * 0.01 + [0.01 * i, -0.01, (0.5 + z) / 2]).astype(np.float32)
        f, o = SO.spherical_flip(np.concatenate([pts, occ], 0))
        out.append(HullCase("golden_2449_%d" % i, "flipped", f, o, None))
    return out


_hulls = {}


def hull_of(case):
    """qhull on the case's points in double (cached by name: computed once, shared, never changed)."""
    if case.name not in _hulls:
        _hulls[case.name] = ConvexHull(case.points.astype(np.float64))
    return _hulls[case.name]


def visible_ids(case):
    """What visible_id[:num] must be: np.sort(hull.vertices)[:-2]."""
    return np.sort(hull_of(case).vertices)[:-2]


def margin(points, hull, ids):
    """For the given point ids, the signed depth below the hull (from hull.equations: > 0 inside, 0 on a facet's plane)
    divided by the bounding-box diagonal."""
    p = np.asarray(points, np.float64)
    ids = np.asarray(ids, np.int64).reshape(-1)
    diag = float(np.linalg.norm(p.max(0) - p.min(0)))
    if len(ids) == 0:
        return np.zeros(0)
    eq = hull.equations
    return -(p[ids] @ eq[:, :3].T + eq[:, 3]).max(axis=1) / diag


def smallest_margin(case):
    """The smallest margin of a non-vertex (inf if every point is a vertex)."""
    hull = hull_of(case)
    rest = np.setdiff1d(np.arange(len(case.points)), hull.vertices)
    return float(margin(case.points, hull, rest).min()) if len(rest) else math.inf


def conditions(case):
    """The conditions on a case's inputs under which the kernel's vertex set is qhull's (csrc/synth.hip's contract):
    returns the list of those it misses (empty: inside the contract)."""
    missed = []
    if len(np.unique(case.points, axis=0)) != len(case.points):
        missed.append("a row repeats exactly")
    hull = hull_of(case)
    n1 = len(case.points)
    if case.kind == "flipped" and (n1 - 1) not in hull.vertices:
        missed.append("the viewpoint is no hull vertex")
    if case.kind == "lattice":
        if sorted(hull.vertices.tolist()) != sorted(case.corners):
            missed.append("the vertex set is not corners + viewpoint")
    elif smallest_margin(case) < MARGIN_BOUND:
        missed.append("a non-vertex lies %.3g of the diagonal below the hull (< %g)" % (smallest_margin(case), MARGIN_BOUND))
    return missed


def describe_difference(case, got):
    """For an assertion message: the ids on which `got` and qhull's visible set differ, each with its margin."""
    want = visible_ids(case)
    hull = hull_of(case)
    extra, missing = np.setdiff1d(got, want), np.setdiff1d(want, got)
    return "%s: %d ids, qhull %d; only here %s (margin %s); only qhull %s (margin %s)" % (
        case.name, len(got), len(want), extra.tolist(), margin(case.points, hull, extra).tolist(), missing.tolist(),
        margin(case.points, hull, missing).tolist())
