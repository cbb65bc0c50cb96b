"""GPU: every path of the on-line synthesis kernels (csrc/synth.hip) against a restatement -- the transform, the flip and
qhull of oracle/synth_oracle.py, the Philox-driven occluder and padding rows of tests/synth_reference.py -- at the sizes where
the kernels change path: the class gather and its clamp, both branches of the exponential map, workgroup and stride
boundaries of the flip, the neighbourhood switch, group and group-batch boundaries and both workgroup sizes of the hull-vertex
test, the largest cloud LDS admits, one workgroup per cloud, exactly coplanar points, and every refusal of the entry points.
The hull-vertex inputs come from synth_reference.hull_cases(), which tests/test_synth_reference_host.py holds to the
kernel's stated contract on the CPU."""
import math

import numpy as np
import pytest
import torch

import synth_reference as S

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOBS = (1, 0, 2)       # CLOUDAAE_HPR_CULL: the default, the full strided scan, every first-pass violation through the fallback


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


# ---- transform_model_kernel ---------------------------------------------------------------------------------------------
AXIS_ANGLES = np.array([[0.0, 0.0, 0.0],                                   # the identity: out = p + t exactly
                        [0.05, -0.03, 0.04],                              # |a|^2 = 5e-3 < 1e-2: the Taylor branch
                        np.array([2.0, -1.0, 2.0]) / 3.0 * (math.pi - 5e-4),   # within 1e-3 of pi
                        [0.7, -1.1, 0.4],
                        [-2.0, 0.3, 1.2]], np.float64).astype(np.float32)      # (records hold fp32 axis-angles)


@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("npts", [1, 255, 257, 2048])
def test_transform_gathers_clamps_and_rotates(hip, npts, b):
    """Three distinct models; class ids mix 0, 1, 2; ids -1 and 3 read models 0 and 2 (the kernel's clamp); bit equality
    with the restatement for the zero, the Taylor-branch, the near-pi and two general axis-angles.  b * npts = 1, 255, 257,
    1275, 1285, ...: last workgroups of 1, 255, 1, 251, 5 threads."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from oracle import synth_oracle as SO
    rng = np.random.default_rng([50, npts, b])
    models = (rng.standard_normal((3, npts, 6)) * 0.05).astype(F32)
    assert not np.array_equal(models[0], models[1]) and not np.array_equal(models[1], models[2])
    a64 = AXIS_ANGLES.astype(np.float64)
    assert 0 < (a64[1] ** 2).sum() < 1e-2 and 0 < math.pi - np.linalg.norm(a64[2]) < 1e-3

    def run(ids, axag, trans):
        x = {"axisangle": _dev(axag), "translation": _dev(trans), "class_id": _dev(ids, np.int64)}
        x = T.transform_object_model(T.get_rotation_matrix(T.get_object_model(x, _dev(models))))
        return x["model_xyz_rot_trans"].cpu().numpy()

    launches = [np.arange(5)] if b == 5 else [np.array([k]) for k in range(4)]
    for which in launches:
        axag = AXIS_ANGLES[which]
        trans = (rng.uniform(-0.3, 0.3, (b, 3)) + [0, 0, 0.9]).astype(F32)
        for base in (np.array([2, 0, 1, 2, 0])[:b], np.array([0, 2, 1, 0, 2])[:b]):
            got = run(base, axag, trans)
            assert got.shape == (b, npts, 3)
            for i in range(b):
                want = SO.transform_object_model(models[base[i]][:, :3], axag[i], trans[i])
                assert np.array_equal(got[i], want), (which[i], base[i])
                if not axag[i].any():
                    assert np.array_equal(got[i], models[base[i]][:, :3] + trans[i][None, :])
            clamped = np.where(base == 0, -1, np.where(base == 2, 3, base))
            assert np.array_equal(run(clamped, axag, trans), got)
            far = np.where(base == 0, -(1 << 40), np.where(base == 2, 1 << 40, base))
            assert np.array_equal(run(far, axag, trans), got)


# ---- occluder_kernel ----------------------------------------------------------------------------------------------------
def _occluder(hip, trans, per, wnear, hnear, near, sigma, seed):
    b = trans.shape[0]
    t = _dev(trans, F32)
    occ = torch.full((b, 2 * per, 3), float("nan"), dtype=torch.float32, device="cuda")
    hip.check(hip.lib().cloudaae_random_spherical_occluder(b, per, hip.ptr(t), float(wnear), float(hnear), float(near),
                                                           float(sigma), int(seed), hip.ptr(occ), hip.stream()),
              "cloudaae_random_spherical_occluder")
    return occ.cpu().numpy()


def _occluder_trans(b, near, rng):
    """z spread over 0.6 .. 1.6; one sample of every batch (the only one of a batch of one: chosen by the caller) sits on
    the near plane, where the centres have no spread along z."""
    t = rng.uniform(-0.3, 0.3, (b, 3)).astype(F32)
    t[:, 2] = np.linspace(0.6, 1.6, b, dtype=F32) if b > 1 else F32(1.1)
    t[b // 2, 2] = F32(near) if b > 1 else t[0, 2]
    return t


@pytest.mark.parametrize("near", [0.4, 0.5])
@pytest.mark.parametrize("b,per", [(1, 1), (1, 200), (3, 85), (1, 257), (513, 1), (4, 200)])
def test_occluder_equals_the_restatement(hip, b, per, near):
    """Every row of both blobs against the fp32 restatement: a swapped pair of Philox words, a wrong stream or counter, a
    wrong row interleave moves a row by ~sigma or more, four orders above the tolerance (which comes from the restatement
    alone: 10 x its own fp32-to-fp64 change, at least 4 ulp).  b * per = 1, 200, 255, 257, 513, 800."""
    from oracle import synth_oracle as SO
    hnear, wnear = SO.get_frustum_near(near=near, ratio=(57.5 if near == 0.4 else 58.0) / 45.0)
    rng = np.random.default_rng([51, b, per])
    variants = [_occluder_trans(b, near, rng)]
    if b == 1:                      # a batch of one: the near-plane sample is a launch of its own
        variants.append(np.array([[0.1, -0.2, near]], F32))
    for trans in variants:
        for seed in (0, 2 ** 40 + 3):
            want, tol = S.occluder_tolerance(trans, per, wnear, hnear, near, 0.01, seed)
            got = _occluder(hip, trans, per, wnear, hnear, near, 0.01, seed)
            err = float(np.abs(got.astype(np.float64) - want).max())
            print("SYNTHPATHS occluder b %d per %d near %.1f seed %d: tolerance %.3g, largest difference %.3g" % (b, per, near, seed, tol, err))
            assert got.shape == (b, 2 * per, 3) and np.isfinite(got).all()
            assert err <= tol
    # every shape saw one sample on the near plane (z - near == 0 in fp32: the centres have no spread along z)
    assert sum(int((t[:, 2] == F32(near)).sum()) for t in variants) == 1


def test_occluder_rows_do_not_depend_on_the_batch(hip):
    from oracle import synth_oracle as SO
    hnear, wnear = SO.get_frustum_near()
    trans = _occluder_trans(4, 0.5, np.random.default_rng(52))
    four = _occluder(hip, trans, 200, wnear, hnear, 0.5, 0.01, 11)
    three = _occluder(hip, trans[:3], 200, wnear, hnear, 0.5, 0.01, 11)
    assert np.array_equal(four[2], three[2]) and np.array_equal(four[:3], three)
    assert not np.array_equal(four, _occluder(hip, trans, 200, wnear, hnear, 0.5, 0.01, 12))


# ---- spherical_flip_kernel ----------------------------------------------------------------------------------------------
def _flip(hip, a, bpts, center, param):
    """The entry point itself (utils.hidden_point_removal._flip cannot express na = 0)."""
    b, na, nb = a.shape[0], a.shape[1], 0 if bpts is None else bpts.shape[1]
    ad = _dev(a, F32) if na else None
    bd = _dev(bpts, F32) if nb else None
    cd = _dev(center, F32) if center is not None else None
    flipped = torch.full((b, na + nb + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
    org = torch.full_like(flipped, float("nan"))
    hip.check(hip.lib().cloudaae_spherical_flip(b, na, hip.ptr(ad) if na else None, nb, hip.ptr(bd) if nb else None,
                                                hip.ptr(cd) if cd is not None else None, float(param), hip.ptr(flipped),
                                                hip.ptr(org), hip.stream()), "cloudaae_spherical_flip")
    return flipped.cpu().numpy(), org.cpu().numpy()


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("na,nb", [(1, 0), (4, 0), (255, 0), (256, 0), (257, 0), (200, 56), (0, 5), (2048, 400)])
def test_flip_shapes_centres_and_params(hip, na, nb, b):
    """Clouds shorter than a workgroup, counts around its 256 threads (the viewpoint row is thread 255's, thread 0's second
    and thread 1's second), no first or no second part, with and without a per-cloud centre; param = 0 makes R the largest
    norm itself, so the farthest point flips onto itself."""
    rng = np.random.default_rng([53, na, nb, b])
    a = (rng.standard_normal((b, na, 3)) * 0.05 + [0.05, -0.1, 0.9]).astype(F32)
    bpts = (rng.standard_normal((b, nb, 3)) * 0.02 + [0.0, 0.0, 0.6]).astype(F32) if nb else None
    centres = (np.array([0.02, -0.03, 0.01]) * (1 + np.arange(b))[:, None]).astype(F32)
    for center in (None, centres):
        for param in (0.8 * math.pi, 0.0):
            flipped, org = _flip(hip, a, bpts, center, param)
            assert flipped.shape == org.shape == (b, na + nb + 1, 3)
            for h in range(b):
                f, o = S.flip(a[h], None if bpts is None else bpts[h], None if center is None else center[h], param)
                assert np.array_equal(org[h], o), (h, param)
                np.testing.assert_allclose(flipped[h], f, rtol=2e-7, atol=0)
                assert (flipped[h, -1] == 0).all() and (org[h, -1] == 0).all()
                if param == 0.0:
                    x, y, z = o[:-1, 0], o[:-1, 1], o[:-1, 2]
                    far = int(np.argmax(np.sqrt((x * x + y * y) + z * z)))
                    assert np.array_equal(flipped[h, far], org[h, far]), (h, far)


# ---- hull_vertex_kernel -------------------------------------------------------------------------------------------------
def _hull_ids(knobs, cases, knob, seed=0):
    """One launch over `cases` (same size): per cloud the ids the library calls visible; checks the gather's fixed rows too."""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    knobs("CLOUDAAE_HPR_CULL", knob)
    F, O = _dev(np.stack([c.points for c in cases])), _dev(np.stack([c.org for c in cases]))
    vis, num, ids = hpr.convexHull(F, O, seed=seed, return_ids=True)
    vis, num, ids = vis.cpu().numpy(), num.cpu().numpy(), ids.cpu().numpy()
    out = []
    for h, c in enumerate(cases):
        n = int(num[h])
        assert 0 <= n <= len(c.points) and (ids[h, n:] == -1).all()
        assert np.array_equal(vis[h, :n], c.org[ids[h, :n]])
        out.append(ids[h, :n])
    return out


def _assert_visible_sets(knobs, cases, quiet=False):
    for knob in KNOBS:
        for c, got in zip(cases, _hull_ids(knobs, cases, knob)):
            if not quiet:
                print("SYNTHPATHS hpr %-22s n1 %5d knob %d vertices %5d" % (c.name, len(c.points), knob, len(got) + 2))
            assert np.array_equal(got, S.visible_ids(c)), (knob, S.describe_difference(c, got))


@pytest.mark.parametrize("name", S.HULL_CASE_NAMES)
def test_visible_set_equals_qhull(hip, knobs, name):
    """visible_id[:num] is np.sort(hull.vertices)[:-2], identically, under the default, the full strided scan and the
    forced fallback.  Gaussian clouds from the entry's minimum of 5 points over one and two groups of 64 with a short last
    group to both sides of hpr_near_of's switch at 193 / 194; flipped object models up to 64 and 65 groups (the second trip
    of the 64-group loop) and across 5 800 .. 6 600 points, where the 8-wave kernel gives way to the 16-wave one (which side
    a size takes is NOT observed: the switch depends on the kernels' static LDS, and the nine sizes straddle it for any
    static LDS between about 2.7 KB and 12 KB); a cube lattice and a flat grid, where 116 and 45 points lie exactly in a
    face of the hull and must not be reported."""
    _assert_visible_sets(knobs, [S.hull_cases()[name]])


@pytest.fixture(scope="module")
def largest_n1(hip):
    """The largest cloud the entry point accepts, by bisection with b = 0 calls: they pass the size checks and return
    before any launch."""
    L = hip.lib()
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def accepted(n1):
        return L.cloudaae_hidden_point_removal_rows(0, n1, None, None, 0, n1, None, None, None, None, hip.ptr(ws), hip.stream()) == 0
    lo, hi = 5, 160 * 1024 // 12 + 1          # 12 bytes a point: 13 654 points alone are more than a CU's 160 KB
    assert accepted(lo) and not accepted(hi)
    assert b"too large" in L.cloudaae_last_error()
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    print("SYNTHPATHS hpr largest accepted n1 = %d" % lo)
    return lo


def test_largest_cloud_lds_admits(hip, knobs, largest_n1):
    """One cloud of the largest accepted size equals qhull's set; one point more is refused as too large.  (The size is
    known only here, so the case is made here -- by the same rule as the table's, from the first seed that meets the host
    conditions, which look at the inputs and qhull alone.)"""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    assert 12000 < largest_n1 <= 12800
    case = S.conforming_flipped_cloud(largest_n1)
    print("SYNTHPATHS hpr %s: smallest non-vertex margin %.3g" % (case.name, S.smallest_margin(case)))
    _assert_visible_sets(knobs, [case])
    more = torch.zeros((1, largest_n1 + 1, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="too large"):
        hpr.convexHull(more, more)


def test_one_workgroup_per_cloud(hip, knobs):
    """513 clouds of 9 points: more clouds than resident workgroups, so the grid is one workgroup per cloud."""
    _assert_visible_sets(knobs, S.batch_cases()["b513_n9"], quiet=True)


def test_batch_equals_single_clouds_and_repeats(hip, knobs):
    """Three clouds of 4097 points: each alone gives what it gives in the batch, and a second run of the same launch gives
    the same bits in every output."""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    cases = S.batch_cases()["b3_n4097"]
    together = _hull_ids(knobs, cases, 1)
    for c, got in zip(cases, together):
        assert np.array_equal(got, S.visible_ids(c)), S.describe_difference(c, got)
        alone = _hull_ids(knobs, [c], 1)[0]
        assert np.array_equal(alone, got)
    F, O = _dev(np.stack([c.points for c in cases])), _dev(np.stack([c.org for c in cases]))
    one = hpr.convexHull(F, O, seed=9, return_ids=True, rows=5000, return_src=True)
    two = hpr.convexHull(F, O, seed=9, return_ids=True, rows=5000, return_src=True)
    for x, y in zip(one, two):
        assert torch.equal(x, y)


# ---- hpr_gather_kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b3_n9", "b3_n194", "golden_2449", "b3_n4097"])
def test_gather_equals_the_restatement(hip, golden_dir, name):
    """visible, num_vis, visible_id and row_src, all four bit for bit, from qhull's vertex ids: for two seeds (one with a
    high half), for fewer rows than visible points, exactly as many, one more, n1 and 3 n1, and for every sample of a batch
    of three (the Philox counter carries the sample)."""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    cases = S.golden_batch(golden_dir) if name == "golden_2449" else S.batch_cases()[name]
    n1 = len(cases[0].points)
    vertices = [S.hull_of(c).vertices for c in cases]
    nvs = [len(v) - 2 for v in vertices]
    assert min(nvs) >= 2
    F, O = _dev(np.stack([c.points for c in cases])), _dev(np.stack([c.org for c in cases]))
    rows_list = sorted({1, n1, 3 * n1} | {nv + d for nv in nvs for d in (-1, 0, 1)})
    for seed in (0, 2 ** 40 + 3):
        for rows in rows_list:
            vis, num, ids, src = (t.cpu().numpy() for t in hpr.convexHull(F, O, seed=seed, return_ids=True, rows=rows, return_src=True))
            assert vis.shape == (3, rows, 3) and ids.shape == src.shape == (3, rows) and ids.dtype == src.dtype == np.int32
            for h, c in enumerate(cases):
                w_vis, w_num, w_ids, w_src = S.gather(vertices[h], c.org, seed, h, rows)
                assert int(num[h]) == w_num == nvs[h], (h, S.describe_difference(c, ids[h, :int(num[h])]))
                assert np.array_equal(ids[h], w_ids), (seed, rows, h)
                assert np.array_equal(src[h], w_src), (seed, rows, h)
                assert np.array_equal(vis[h], w_vis), (seed, rows, h)


def test_gather_of_a_collinear_cloud_has_no_visible_point(hip):
    """(i, 0, 0), i = 1 .. 8, and the viewpoint at the origin: by the kernel's own rule only the two ends of the segment
    separate strictly, two flags leave nv = 0 -- zero rows, ids and row_src of -1 (qhull refuses such a cloud)."""
    from cloudaae_amd.utils import hidden_point_removal as hpr
    p = np.zeros((1, 9, 3), F32)
    p[0, :8, 0] = np.arange(1, 9)
    P = _dev(p)
    vis, num, ids, src = hpr.convexHull(P, P, seed=4, return_ids=True, rows=20, return_src=True)
    assert int(num[0]) == 0 and bool((ids == -1).all()) and bool((src == -1).all()) and bool((vis == 0).all())
    want = S.gather([7, 8], p[0], 4, 0, 20)
    assert want[1] == 0 and np.array_equal(vis[0].cpu().numpy(), want[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------
CANARY = 0x5A


def _canary(nbytes):
    return torch.full((max(int(nbytes), 16),), CANARY, dtype=torch.uint8, device="cuda")


def test_flip_refuses_bad_sizes(hip):
    L = hip.lib()
    src = _canary(65536 * 3 * 3 * 4)
    out_f, out_o = _canary(65536 * 4 * 3 * 4), _canary(65536 * 4 * 3 * 4)

    def call(b=2, na=2, nb=1):
        return L.cloudaae_spherical_flip(b, na, hip.ptr(src), nb, hip.ptr(src), None, 2.5, hip.ptr(out_f), hip.ptr(out_o), hip.stream())
    for kw in (dict(b=65536), dict(na=0, nb=0), dict(b=-1), dict(na=-1), dict(nb=-1), dict(na=-3, nb=5)):
        assert call(**kw) != 0, kw
        assert b"cloudaae_spherical_flip" in L.cloudaae_last_error(), kw
    torch.cuda.synchronize()
    for buf in (src, out_f, out_o):
        assert bool((buf == CANARY).all())
    assert call(b=0) == 0                                               # nothing to do is no error
    torch.cuda.synchronize()
    assert bool((out_f == CANARY).all()) and bool((out_o == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out_f == CANARY).all())


def test_hidden_point_removal_refuses_bad_arguments(hip, largest_n1):
    L = hip.lib()
    big = 65536 * 5
    pts = _canary(max(big, largest_n1 + 1) * 12)
    vis, num, ids, src = _canary(big * 12), _canary(65536 * 8), _canary(big * 4), _canary(big * 4)
    ws = _canary(L.cloudaae_hpr_workspace_bytes(65536, 5))

    def call(b=2, n1=5, rows=5, w=hip.ptr(ws)):
        return L.cloudaae_hidden_point_removal_rows(b, n1, hip.ptr(pts), hip.ptr(pts), 0, rows, hip.ptr(vis), hip.ptr(num),
                                                    hip.ptr(ids), hip.ptr(src), w, hip.stream())
    for kw, words in ((dict(n1=4), b"bad size"), (dict(rows=0), b"output rows"), (dict(b=65536), b"bad size"), (dict(b=-1), b"bad size"),
                      (dict(w=None), b"bad size"), (dict(b=1, n1=largest_n1 + 1, rows=1), b"too large")):
        assert call(**kw) != 0, kw
        err = L.cloudaae_last_error()
        assert b"cloudaae_hidden_point_removal" in err and words in err, (kw, err)
    # the plain entry (rows = n1) goes through the same checks
    assert L.cloudaae_hidden_point_removal(2, 4, hip.ptr(pts), hip.ptr(pts), 0, hip.ptr(vis), hip.ptr(num), hip.ptr(ids), hip.ptr(ws),
                                           hip.stream()) != 0
    assert b"cloudaae_hidden_point_removal" in L.cloudaae_last_error()
    torch.cuda.synchronize()
    for buf in (pts, vis, num, ids, src, ws):
        assert bool((buf == CANARY).all())
    assert call(b=0) == 0
    torch.cuda.synchronize()
    for buf in (vis, num, ids, src, ws):
        assert bool((buf == CANARY).all())


def test_workspace_bytes_follow_the_stated_layout(hip):
    """flags [b, n1] bytes padded to 16; sorted points [b, n1, 3] floats; their permutation [b, n1] ints; a queue counter
    per cloud."""
    L = hip.lib()
    for b, n1 in ((1, 5), (3, 4097)):
        want = (b * n1 + 15) // 16 * 16 + 12 * b * n1 + 4 * b * n1 + 4 * b
        assert int(L.cloudaae_hpr_workspace_bytes(b, n1)) == want, (b, n1)
    assert int(L.cloudaae_hpr_workspace_bytes(1, 5)) == 100 and int(L.cloudaae_hpr_workspace_bytes(3, 4097)) == 208972
