"""Test infrastructure of tests/test_49_point_op_variants_gpu.py and tests/test_point_op_variants_host.py.

1. farthest_point_sample: farthest point sampling restated in plain NumPy -- running minima, the un-fused fp32 distance
   (dx*dx + dy*dy) + dz*dz, and among the points that hold the maximum the one with the lowest k mod 512, then the lowest
   k (what the reference's 512-thread strided scan and left-biased tree produce, tf_sampling_g.cu:130-165).  Two WRONG
   tie-break rules come with it; the host test shows that the inputs of the GPU test tell them from the right one.
2. The case tables of the GPU test -- farthest point sampling, kNN and the Chamfer search, each case with the kernel
   variant it is meant to reach -- and the inputs of every case, so that the host test examines exactly what the GPU runs.
3. The names of the values of cloudaae_farthest_point_sample_variant / cloudaae_knn_variant /
   cloudaae_nn_distance_variant, decoded with the constants of include/cloudaae_hip.h (read from the header, not copied).
"""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LANES = 512     # threads of the reference's kernel: point k belongs to thread k mod 512

# ---- 1. farthest point sampling in NumPy ---------------------------------------------------------------------------------
RULES = ("reference", "lowest_k", "highest_k_of_lane")


def _pick(run, rule):
    """the index the round returns: `run` = the running minima after this round's update"""
    k = np.flatnonzero(run == run.max())
    if rule == "lowest_k":                   # WRONG: a plain first-maximum scan
        return int(k[0])
    lane = k % LANES
    k = k[lane == lane.min()]
    if rule == "reference":                  # lowest k mod 512, then lowest k
        return int(k[0])
    if rule == "highest_k_of_lane":          # WRONG: the right thread, its LAST point (a `>=` in the strided scan)
        return int(k[-1])
    raise ValueError(rule)


def farthest_point_sample(m, points, rule="reference"):
    """points [b, n, 3] float32 -> indices [b, m] int32; out[:, 0] = 0 (tf_sampling_g.cu:105-170)"""
    points = np.ascontiguousarray(points, dtype=F32)
    b, n, _ = points.shape
    out = np.zeros((b, m), np.int32)
    for c in range(b):
        x, y, z = points[c, :, 0], points[c, :, 1], points[c, :, 2]
        run = np.full(n, F32(1e38), F32)
        last = 0
        for j in range(1, m):
            dx, dy, dz = x - x[last], y - y[last], z - z[last]
            d = (dx * dx + dy * dy) + dz * dz           # fp32 arrays: one rounding per operation
            run = np.minimum(run, d)
            last = _pick(run, rule)
            out[c, j] = last
    return out


def first_divergence(a, b):
    """the first round at which two index lists [m] differ, or None"""
    diff = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return int(diff[0]) if diff.size else None


# ---- 2. the cases -----------------------------------------------------------------------------------------------------
FpsCase = collections.namedtuple("FpsCase", "b n m variant")
# variant: "ppt<P>" = P points per thread, the winner's coordinates from LDS; "ppt32-memory" = from memory; "big"
FPS_BOUNDARY_N = (512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385)
_FPS_AT = {512: "ppt1", 513: "ppt2", 1024: "ppt2", 1025: "ppt4", 2048: "ppt4", 2049: "ppt8", 4096: "ppt8", 4097: "ppt16",
           8192: "ppt16", 8193: "ppt32", 12288: "ppt32", 12289: "ppt32-memory", 16384: "ppt32-memory", 16385: "big"}
FPS_ROUNDS = 96
FPS_CASES = [FpsCase(2, n, FPS_ROUNDS, _FPS_AT[n]) for n in FPS_BOUNDARY_N] + [
    FpsCase(2, 8192, 400, "ppt16"),             # 343 distinct lattice points: every later round is an n-way tie at 0
    FpsCase(2, 16384, 400, "ppt32-memory"),
    FpsCase(2, 16384, 4096, "ppt32-memory"),    # the call of evaluation at N = 4096 (xyz_recon [B, 4N, 3])
    FpsCase(33, 16385, 48, "big"),              # the big kernel's loop over clouds: a second cloud through a temp row ...
    FpsCase(70, 16500, 24, "big"),              # ... and a third
    FpsCase(3, 16385, 1, "big"),                # no rounds
    FpsCase(2, 700, 900, "ppt2"),               # more rounds than points
]


def fps_id(c):
    return "%dx%d-to-%d-%s" % (c.b, c.n, c.m, c.variant)


def fps_cloud(c):
    """integer lattice clouds: exact fp32 distances, ties in every round"""
    rng = np.random.default_rng(c.n * 7 + c.m + c.b)
    return rng.integers(-3, 4, (c.b, c.n, 3)).astype(F32)


KnnCase = collections.namedtuple("KnnCase", "b n c ld k wide misaligned variant")
# wide: the value of the knob CLOUDAAE_KNN3_WIDE (None = unset).  misaligned: x starts one float past a 16-byte boundary.
# variant: what cloudaae_knn_variant must answer, as knn_variant_name() spells it.
KNN_CASES = [
    KnnCase(256, 200, 3, 24, 10, None, False, "c3 scan CS2"),       # b a multiple of 8: the remapped (cloud, tile)
    KnnCase(257, 200, 3, 24, 10, None, False, "c3 scan CS2"),
    KnnCase(512, 200, 3, 24, 20, None, False, "c3 scan CS1"),       # b a multiple of 8
    KnnCase(515, 200, 3, 24, 10, None, False, "c3 scan CS1"),
    KnnCase(64, 1000, 3, 24, 10, 0, False, "c3 scan CS2"),          # two ranges of 500 candidates: no multiple of the step 8
    KnnCase(128, 1000, 3, 24, 20, 0, False, "c3 scan CS1"),
    KnnCase(24, 6144, 3, 24, 10, 0, False, "c3 scan CS1"),          # the largest cloud of the scan kernel
    KnnCase(1, 6145, 3, 24, 10, None, False, "generic"),            # c3 generic by size
    KnnCase(3, 255, 3, 24, 10, None, False, "c3 scan CS4"),
    KnnCase(3, 256, 3, 24, 10, None, False, "c3 wide"),
    KnnCase(2, 300, 64, 65, 10, None, False, "generic"),            # c64 generic by stride
    KnnCase(2, 300, 64, 64, 10, None, True, "generic"),             # c64 generic by alignment
]
# (the largest cloud of the c3 wide kernel and the next size are found by bisection on the query: knn_wide_limit_cases)


def knn_id(c):
    return "%dx%dx%d-ld%d-k%d%s%s-%s" % (c.b, c.n, c.c, c.ld, c.k, "" if c.wide is None else "-wide%d" % c.wide,
                                         "-misaligned" if c.misaligned else "", c.variant.replace(" ", "-"))


def knn_cloud(c):
    """Gaussian rows, thirty of them twice: exact ties, the lower index must win"""
    rng = np.random.default_rng(c.n * 7 + c.c + c.k + c.b)
    x = rng.standard_normal((c.b, c.n, c.ld)).astype(F32)
    x[:, c.n // 2:c.n // 2 + 30] = x[:, :30]
    return x


def knn_wide_limit_cases(query, k):
    """[largest n that `query(b, n, c, ld, k, aligned)` still calls c3 wide, that n + 1], b = 1: bisection on the query alone"""
    is_wide = lambda n: knn_variant_name(query(1, n, 3, 24, k, 1))[0] == "c3 wide"
    lo, hi = 256, 6145              # wide at 256 (the smallest cloud it takes), never above 6144
    assert is_wide(lo) and not is_wide(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if is_wide(mid) else (lo, mid)
    after = knn_variant_name(query(1, hi, 3, 24, k, 1))[0]
    return [KnnCase(1, lo, 3, 24, k, None, False, "c3 wide"), KnnCase(1, hi, 3, 24, k, None, False, after)]


NnCase = collections.namedtuple("NnCase", "b n m filter prefix variant")
# filter: the value of the knob CLOUDAAE_NN_FILTER (None = unset: the launcher's own choice).  prefix: through
# cloudaae_nn_distance_prefix, targets = distinct rows followed by copies.  variant: "Q1" / "Q2" / "Q4" / "filter".
NN_CASES = [
    NnCase(257, 511, 511, None, False, "Q2"),
    NnCase(600, 430, 7, None, False, "Q2"),         # fewer candidates than one 16-candidate tile
    NnCase(2052, 256, 256, None, False, "Q4"),
    NnCase(256, 512, 512, 0, False, "Q2"),          # b (n + m) = 256 * 1024 exactly
    NnCase(256, 512, 511, 0, False, "Q1"),
    NnCase(1024, 512, 512, 0, False, "Q4"),         # b (n + m) = 4 * 256 * 1024 exactly
    NnCase(1024, 512, 511, 0, False, "Q2"),
    # (a lane's query slot q holds queries 256 q ... 256 q + 255 of a workgroup's 256 Q: the Q4 cases above fill slots 0 and 1
    #  only.  Here all four hold queries, with a tail in slot 0 of a second workgroup (n) and in slot 3 (m))
    NnCase(512, 1030, 1018, 0, False, "Q4"),
    NnCase(300, 500, 400, 0, True, "Q2"),
]


def nn_id(c):
    return "%dx%dx%d%s%s-%s" % (c.b, c.n, c.m, "" if c.filter is None else "-filter%d" % c.filter,
                                "-prefix" if c.prefix else "", c.variant)


def nn_prefix_counts(c):
    """count2 of a prefix case: below m, equal to m, and values the entry point must ignore (0, above m), in turn"""
    return [[max(1, c.m // 4), c.m, max(2, c.m // 3), 0, c.m + 5, 37][i % 6] for i in range(c.b)]


def nn_clouds(c):
    """(xyz1 [b, n, 3], xyz2 [b, m, 3], row_src2 [b, m] or None): the clouds of test_nn_distance_vs_oracle with duplicated
    candidates in both directions (the first copy must win); a prefix case has padded targets instead -- count distinct rows,
    then re-draws of them, as test_nn_distance_prefix_equals_full_search builds them"""
    rng = np.random.default_rng(c.b * 1000 + c.n + c.m)
    a = (rng.standard_normal((c.b, c.n, 3)) * 0.05 + [0.1, -0.2, 0.9]).astype(F32)
    t = (rng.standard_normal((c.b, c.m, 3)) * 0.05 + [0.1, -0.2, 0.9]).astype(F32)
    src = None
    if c.prefix:
        src = np.empty((c.b, c.m), np.int32)
        for i, count in enumerate(nn_prefix_counts(c)):
            k = count if 0 < count <= c.m else c.m
            pick = rng.integers(0, k, c.m - k)
            t[i, k:] = t[i, pick]
            src[i, :k] = np.arange(k)
            src[i, k:] = pick
        a[:, :40] = t[:, 10:50]                 # exact hits
    else:
        dup = min(20, c.m // 2)
        t[:, c.m // 2:c.m // 2 + dup] = t[:, :dup]
    dup = c.n // 4                              # (many: the other direction may have only a handful of queries)
    a[:, c.n // 2:c.n // 2 + dup] = a[:, :dup]
    return a, t, src


def nn_tied_queries(queries, candidates):
    """how many queries [nq, 3] of ONE cloud have their minimum (un-fused fp32) at two or more candidates [nc, 3]"""
    d = queries[:, None, :] - candidates[None, :, :]
    D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return int(((D == D.min(1, keepdims=True)).sum(1) >= 2).sum())


# ---- 3. the names of the variants -------------------------------------------------------------------------------------
def header_constants():
    text = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    found = re.findall(r"#define\s+(CLOUDAAE_(?:FPS|KNN|NN)_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)\b", text)
    return {name: int(value, 0) for name, value in found}


def fps_variant_name(v):
    H = header_constants()
    if v == H["CLOUDAAE_FPS_BIG"]:
        return "big"
    ppt = v & H["CLOUDAAE_FPS_PPT_MASK"]
    assert v >= 0 and ppt in (1, 2, 4, 8, 16, 32) and v & ~(H["CLOUDAAE_FPS_PPT_MASK"] | H["CLOUDAAE_FPS_XYZ_FROM_MEMORY"]) == 0, v
    return "ppt%d%s" % (ppt, "-memory" if v & H["CLOUDAAE_FPS_XYZ_FROM_MEMORY"] else "")


def knn_variant_name(v):
    """(kernel, list length K)"""
    H = header_constants()
    names = {H["CLOUDAAE_KNN_C3_WIDE"]: "c3 wide", H["CLOUDAAE_KNN_C3_SCAN_1"]: "c3 scan CS1",
             H["CLOUDAAE_KNN_C3_SCAN_2"]: "c3 scan CS2", H["CLOUDAAE_KNN_C3_SCAN_4"]: "c3 scan CS4",
             H["CLOUDAAE_KNN_C64_WIDE"]: "c64 wide", H["CLOUDAAE_KNN_C64_SCAN_1"]: "c64 scan 1 wave",
             H["CLOUDAAE_KNN_C64_SCAN_2"]: "c64 scan 2 waves", H["CLOUDAAE_KNN_GENERIC"]: "generic"}
    assert len(names) == 8 and v >= 0 and (v >> 8) in (10, 20, 32), v
    return names[v & 0xff], v >> 8


def nn_variant_name(v):
    H = header_constants()
    assert v in (H["CLOUDAAE_NN_FILTER_KERNEL"], 1, 2, 4), v
    return "filter" if v == H["CLOUDAAE_NN_FILTER_KERNEL"] else "Q%d" % v
