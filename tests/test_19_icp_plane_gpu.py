"""GPU: surface normals (cloudaae_estimate_normals, utils/normals.py) and point-to-plane ICP
(cloudaae_icp_point_to_plane, utils/icp.py) against the float64 NumPy restatements of their definitions
(tests/normals_reference.py, tests/icp_plane_reference.py), and the plane refinement inside evaluate_batch.

Tolerances.  Normals: eps = 100 x max(d, 1e-12), d = what reversing the order of the restatement's own sums changes
(measured in the test: 3e-16 in 1 - |n . n'|, 1.4e-15 in the eigenvalues relative to the largest, so eps = 1e-10).
ICP: those of tests/test_14_icp_gpu.py (iterations equal, fitness equal as a count, T to 1e-9, rmse to 1e-9 relative);
the float64 restatement differs from its numpy.longdouble run by at most 4e-13 in T on these scenes
(profiles/notes_icp_plane.md), so the 6x6 solve needs no looser bound."""
import os
import warnings

import numpy as np
import pytest
import torch

import icp_plane_reference as PL
import icp_reference as R
import normals_reference as NR
from test_14_icp_gpu import _batch, _graph_and_element

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 0.015


@pytest.fixture(scope="module")
def model():
    from cloudaae_amd import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    return models[0]                                  # [2048, 6] float32: xyz | rgb


@pytest.fixture(scope="module")
def model_normals(model):
    return NR.estimate_normals(model, RADIUS)         # (normals, eigenvalues, count) of the restatement


@pytest.fixture(scope="module")
def eps(model, model_normals):
    n0, e0, _ = model_normals
    n1, e1, _ = NR.estimate_normals(model, RADIUS, reverse=True)
    d = max((1.0 - np.abs((n0 * n1).sum(axis=1))).max(), (np.abs(e0 - e1) / e0[:, 2:3]).max())
    print("order-of-sums difference of the restatement: %.3e" % d)
    return 100.0 * max(d, 1e-12)


def _normals_gpu(xyz, radius, **kw):
    from cloudaae_amd.utils.normals import estimate_normals
    out = estimate_normals(torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), radius, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _compare_normals(got, ref, eps, signed=None):
    (n, e, c), (nr, er, cr) = got, ref
    assert np.array_equal(c, cr)
    few = cr < 3
    assert np.all(n[few] == [0.0, 0.0, 1.0]) and np.all(e[few] == 0.0)
    gap = NR.relative_gap(er)
    ok = ~few & (gap >= 0.1)
    assert (~few & ~ok).sum() <= 0.01 * len(cr)           # the share the gap rule leaves out: a condition
    dot = (n[ok] * nr[ok]).sum(axis=1)
    print("normals: %d compared, max 1 - |dot| %.3e, max eigenvalue difference / largest %.3e"
          % (ok.sum(), (1.0 - np.abs(dot)).max(), (np.abs(e[ok] - er[ok]) / er[ok][:, 2:3]).max()))
    assert np.all(np.abs(dot) >= 1.0 - eps)
    assert np.all(np.abs(e[ok] - er[ok]) <= eps * er[ok][:, 2:3])
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-14
    assert np.all(np.diff(e, axis=1) >= 0.0)
    if signed is not None:
        sel = ok & signed
        assert np.all((n[sel] * nr[sel]).sum(axis=1) >= 1.0 - eps)
    return ok


def test_normals_vs_restatement(hip, model, model_normals, eps):
    assert eps <= 1e-9
    assert model_normals[2].min() == 19 and (NR.relative_gap(model_normals[1]) < 0.1).sum() == 0
    got = _normals_gpu(model[None], RADIUS)
    assert got[0].shape == (1, 2048, 3) and got[0].dtype == np.float64 and got[2].dtype == np.int32
    ok = _compare_normals([g[0] for g in got], model_normals, eps)
    assert ok.all()
    # S = 3: the model and two permutations of it, each against the restatement on that set
    rng = np.random.default_rng(4)
    sets = np.stack([model, model[rng.permutation(2048)], model[rng.permutation(2048)]])
    got3 = _normals_gpu(sets, RADIUS)
    for s in range(3):
        ref = model_normals if s == 0 else NR.estimate_normals(sets[s], RADIUS)
        _compare_normals([g[s] for g in got3], ref, eps)
    # a set's result does not depend on S; two runs give the same bits
    for a, b in zip(got, got3):
        assert a[0].tobytes() == b[0].tobytes()
    again = _normals_gpu(sets, RADIUS)
    for a, b in zip(got3, again):
        assert a.tobytes() == b.tobytes()


def test_normals_with_too_few_neighbours(hip, model, eps):
    ref = NR.estimate_normals(model, 0.005)
    assert (ref[2] < 3).sum() == 1290
    got = _normals_gpu(model[None], 0.005)
    assert np.array_equal(got[2][0], ref[2])
    few = ref[2] < 3
    assert np.all(got[0][0][few] == [0.0, 0.0, 1.0]) and np.all(got[1][0][few] == 0.0)
    # a larger min_neighbors moves the rule with it
    got8 = _normals_gpu(model[None], 0.005, min_neighbors=8)
    assert np.array_equal(got8[2][0], ref[2])
    assert np.all(got8[0][0][ref[2] < 8] == [0.0, 0.0, 1.0]) and np.all(got8[1][0][ref[2] < 8] == 0.0)
    assert got8[0][0][ref[2] >= 8].tobytes() == got[0][0][ref[2] >= 8].tobytes()


def test_normals_viewpoint_queries_and_packed_sets(hip, model, eps):
    from cloudaae_amd.utils.normals import estimate_normals
    v = np.array([0.3, -0.2, 0.5])
    rng = np.random.default_rng(6)
    q = (model[rng.permutation(2048)[:500], :3] + rng.standard_normal((500, 3)).astype(np.float32) * 2e-3)
    ref = NR.estimate_normals(model, RADIUS, queries=q, viewpoint=v)
    got = _normals_gpu(model[None], RADIUS, queries=torch.from_numpy(q[None]).cuda(), viewpoint=v)
    side = np.abs((ref[0] * (q.astype(np.float64) - v)).sum(axis=1)) > 1e-6
    _compare_normals([g[0] for g in got], ref, eps, signed=side)
    assert np.all((got[0][0] * (q.astype(np.float64) - v)).sum(axis=1)[side & (ref[2] >= 3)] <= 0.0)
    # ragged packed sets with offsets: 2048 + 1500 points (the second set: a denser, smaller copy), the queries of
    # the second set padded with far points that have no neighbour
    second = (model[rng.permutation(2048)[:1500], :3] * np.float32(0.75)).astype(np.float32)
    packed = torch.from_numpy(np.concatenate([model[:, :3], second])).cuda()
    offsets = torch.tensor([0, 2048, 3548], dtype=torch.int32).cuda()
    queries = np.full((2, 2048, 3), 10.0, np.float32)
    queries[0] = model[:, :3]
    queries[1, :1500] = second
    out = estimate_normals(packed, RADIUS, queries=torch.from_numpy(queries).cuda(), offsets=offsets)
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in out]
    _compare_normals([o[0] for o in out], NR.estimate_normals(model, RADIUS), eps)
    _compare_normals([o[1][:1500] for o in out], NR.estimate_normals(second, RADIUS), eps)
    assert np.all(out[2][1][1500:] == 0) and np.all(out[0][1][1500:] == [0.0, 0.0, 1.0])
    assert np.all(out[1][1][1500:] == 0.0)


def _gpu(src, dst, normals, rot, trans, **kw):
    from cloudaae_amd.utils.icp import refine_pose_icp
    out = refine_pose_icp(torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(dst).cuda(),
                          torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda(), estimation="point_to_plane",
                          normals=torch.from_numpy(np.ascontiguousarray(normals)).cuda(), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_rotations(out):
    """R orthonormal, Rodrigues(rot_axag) = R to 1e-12, angle in [0, pi]; trans = T's translation.  T is a product of
    one rotation per update (T <- U T, never re-orthonormalised, by definition), each orthonormal to a few units of
    2^-52 and multiplied in with a few more: the bound is 8 x 2^-52 per factor (300 updates: 5e-13)."""
    for c in range(len(out["transformation"])):
        T = out["transformation"][c]
        Rm = T[:3, :3]
        bound = 8.0 * 2.0 ** -52 * (int(out["iterations"][c].sum()) + 2)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= bound
        assert abs(np.linalg.det(Rm) - 1.0) <= bound
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        assert np.abs(R.rodrigues(out["rot_axag"][c]) - Rm).max() < 1e-12
        assert np.linalg.norm(out["rot_axag"][c]) <= np.pi + 1e-12
        assert np.array_equal(out["trans"][c], T[:3, 3].astype(np.float32))


def _agree(got, c, T, fit, rmse, its, M):
    assert np.array_equal(got["iterations"][c], its), (c, got["iterations"][c], its)
    assert round(got["fitness"][c] * M) == round(fit * M), c
    print("cloud %d: updates %d, max |T - T_ref| %.3e, rmse %.6e vs %.6e"
          % (c, its.sum(), np.abs(got["transformation"][c] - T).max(), got["inlier_rmse"][c], rmse))
    assert np.abs(got["transformation"][c] - T).max() <= 1e-9, c
    assert abs(got["inlier_rmse"][c] - rmse) <= 1e-9 * rmse, c


@pytest.mark.parametrize("B,N", [(1, 256), (1, 1024), (8, 256), (8, 1024)])
def test_plane_icp_vs_restatement(hip, model, model_normals, B, N):
    """Scenes as in test_14: a half-space cut of N points, 1 mm noise, a start 2-4 deg and 3-5 mm off.  The scene is
    the source, the model with the restatement's normals the target, the poses model -> camera."""
    obj, scene, rot, trans, _ = _batch(model, B, N, seed=1900 + 10 * B + N)
    nrm = np.repeat(model_normals[0][None], B, axis=0)
    got = _gpu(scene, obj, nrm, rot, trans, pose_maps_target_to_source=True)
    assert got["iterations"].shape == (B, 10) and got["iterations"].dtype == np.int32
    for c in range(B):
        T, fit, rmse, its = PL.refine(scene[c], obj[c], nrm[c], rot[c], trans[c], pose_maps_target_to_source=True)
        _agree(got, c, T, fit, rmse, its, N)
    _check_rotations(got)


def test_plane_icp_target_to_source_flag(hip, model, model_normals):
    """The flagged call = the unflagged call on the inverted start pose, its output inverted on the host.  The start
    translation is zero and the inverse of an axis-angle is its negative, so both starts are exact in float32 and
    the two runs see the same numbers; the true translation is 3-5 mm."""
    rng = np.random.default_rng(23)
    B, N = 3, 512
    scenes, rots = [], []
    for _ in range(B):
        rot = R.log_map(R.rodrigues(rng.standard_normal(3)))
        t = rng.standard_normal(3)
        t *= rng.uniform(3e-3, 5e-3) / np.linalg.norm(t)
        sc, r0, _ = R.scene(model[:, :3], rot, t, N, 1e-3, rng, rng.uniform(2, 4), 0.0)
        scenes.append(sc)
        rots.append(r0)
    scene, rot, zero = np.stack(scenes), np.stack(rots), np.zeros((B, 3), np.float32)
    obj = np.repeat(model[None], B, axis=0)
    nrm = np.repeat(model_normals[0][None], B, axis=0)
    a = _gpu(scene, obj, nrm, rot, zero, pose_maps_target_to_source=True)
    b = _gpu(scene, obj, nrm, -rot, zero)
    assert np.array_equal(a["iterations"], b["iterations"])
    assert np.array_equal(a["fitness"], b["fitness"])
    assert np.all(np.abs(a["inlier_rmse"] - b["inlier_rmse"]) <= 1e-9 * b["inlier_rmse"])
    for c in range(B):
        assert np.abs(a["transformation"][c] - PL.invert(b["transformation"][c])).max() <= 1e-9
        assert np.abs(R.rodrigues(a["rot_axag"][c]) @ R.rodrigues(b["rot_axag"][c]) - np.eye(3)).max() < 1e-9
    _check_rotations(a)
    _check_rotations(b)


def _pose_error(T, truth):
    dR = T[:3, :3] @ truth[:3, :3].T
    return (np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))),
            np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def test_plane_icp_recovers_the_pose(hip, model, model_normals):
    """Noise-free half-space views, the start 2-4 deg and 3-5 mm off: the refined errors lie strictly below the
    start's and at the restatement's own (on the CPU beforehand: 1.7e-6 deg and about 1e-9 m after 20 and 23
    updates, profiles/notes_icp_plane.md)."""
    B, N = 2, 1024
    obj, scene, rot, trans, truth = _batch(model, B, N, seed=77, noise=0.0)
    nrm = np.repeat(model_normals[0][None], B, axis=0)
    got = _gpu(scene, obj, nrm, rot, trans, pose_maps_target_to_source=True)
    for c in range(B):
        T, fit, rmse, its = PL.refine(scene[c], obj[c], nrm[c], rot[c], trans[c], pose_maps_target_to_source=True)
        _agree(got, c, T, fit, rmse, its, N)
        deg0, m0 = _pose_error(R.initial_transform(rot[c], trans[c]), truth[c])
        deg, m = _pose_error(got["transformation"][c], truth[c])
        deg_r, m_r = _pose_error(T, truth[c])
        print("cloud %d: start %.3f deg %.3e m, refined %.3e deg %.3e m, restated %.3e deg %.3e m"
              % (c, deg0, m0, deg, m, deg_r, m_r))
        assert deg < deg0 and m < m0
        assert abs(m - m_r) <= 1e-9 and abs(np.radians(deg) - np.radians(deg_r)) <= 1e-7
        assert got["fitness"][c] == 1.0
    _check_rotations(got)


def test_plane_icp_degenerate_systems(hip, model, model_normals):
    obj, scene, rot, trans, _ = _batch(model, 3, 256, seed=41)
    # every target normal the same: a system of rank three
    for n in ([0.0, 0.0, 1.0], [0.6, 0.0, 0.8]):
        flat = np.tile(np.array(n), (3, 2048, 1))
        got = _gpu(scene, obj, flat, rot, trans, pose_maps_target_to_source=True)
        for k in ("transformation", "rot_axag", "trans", "fitness", "inlier_rmse"):
            assert np.all(np.isfinite(got[k])), k
    # fewer than six correspondences: the pose stays as it is
    nrm = np.repeat(model_normals[0][None], 3, axis=0)
    far = scene + np.float32(1.0)
    far[:, :4] = scene[:, :4]                               # four points of each cloud may still find a partner
    got = _gpu(far, obj, nrm, rot, trans, pose_maps_target_to_source=True)
    t0 = _gpu(far, obj, nrm, rot, trans, pose_maps_target_to_source=True, rounds=0)
    assert np.array_equal(got["transformation"].view(np.int64), t0["transformation"].view(np.int64))
    assert np.all(got["fitness"] <= 4.0 / 256) and np.all(np.isfinite(got["inlier_rmse"]))
    assert np.all(got["iterations"] == 1)
    tiny = _gpu(scene, obj, nrm, rot, trans, pose_maps_target_to_source=True, radius=1e-7)
    assert np.all(np.isfinite(tiny["transformation"])) and np.all(tiny["fitness"] < 6.0 / 256)
    for c in range(3):
        assert np.abs(tiny["transformation"][c] - R.initial_transform(rot[c], trans[c])).max() <= 1e-14


def test_plane_icp_is_deterministic_and_batch_independent(hip, model, model_normals):
    obj, scene, rot, trans, _ = _batch(model, 5, 1024, seed=13)
    nrm = np.repeat(model_normals[0][None], 5, axis=0)
    a = _gpu(scene, obj, nrm, rot, trans, pose_maps_target_to_source=True)
    b = _gpu(scene, obj, nrm, rot, trans, pose_maps_target_to_source=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    one = _gpu(scene[3:4], obj[3:4], nrm[3:4], rot[3:4], trans[3:4], pose_maps_target_to_source=True)
    for k in a:
        assert one[k][0].tobytes() == a[k][3].tobytes(), k


def test_evaluate_batch_plane_icp(hip, model):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils.icp import refine_pose_icp
    from cloudaae_amd.utils.normals import estimate_normals
    B, N = 4, 256
    graph, el = _graph_and_element(model, B, N)
    plane = {"estimation": "point_to_plane"}
    plain = E.evaluate_batch(graph, el)
    out = E.evaluate_batch(graph, el, icp=plane)
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(out[k], v), k
    normals = estimate_normals(el["obj_batch"], 0.015)[0]
    direct = refine_pose_icp(el["xyz_inlier"][:, :N], el["obj_batch"], out["rot_pred"], out["trans_pred"],
                             estimation="point_to_plane", normals=normals, pose_maps_target_to_source=True)
    names = dict(transformation="transformation_icp", rot_axag="rot_icp", trans="trans_icp", fitness="fitness_icp",
                 inlier_rmse="inlier_rmse_icp", iterations="iterations_icp")
    for k, name in names.items():
        assert torch.equal(out[name], direct[k]), name
        assert bool(torch.isfinite(out[name].double()).all()), name
    for k in ("trans_loss_icp", "axag_loss_icp", "trans_loss_perSample_icp", "axag_loss_perSample_icp"):
        assert bool(torch.isfinite(out[k]).all()), k
    # given normals are used as they are
    given = E.evaluate_batch(graph, dict(el, obj_normals=normals), icp=plane)
    for name in names.values():
        assert torch.equal(given[name], out[name]), name
    scored = E.evaluate_batch(graph, el, icp=plane, score=True)
    for k in ("add_pred", "adds_pred", "add_icp", "adds_icp"):
        assert scored[k].shape == (B,) and bool(torch.isfinite(scored[k]).all()), k
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(scored[k], v), k
    # recorded and replayed: the same bits, no torch kernel inside the plan
    for kw, want in ((dict(icp=plane), out), (dict(icp=plane, score=True), scored)):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            r1 = E.evaluate_batch(graph, el, replay=True, **kw)
            r2 = E.evaluate_batch(graph, el, replay=True, **kw)
        for r in (r1, r2):
            for k, v in want.items():
                if isinstance(v, torch.Tensor):
                    assert torch.equal(r[k], v), k
    plans = graph.__dict__["_eval_plans"]
    assert any(p[0] is not None and not p[0].foreign_ops for p in plans.values())
    # icp=True is still the point-to-point schedule, to the bit
    p2p = E.evaluate_batch(graph, el, icp=True)
    ref = refine_pose_icp(el["obj_batch"], el["xyz_inlier"][:, :N], out["rot_pred"], out["trans_pred"])
    for k, name in names.items():
        assert torch.equal(p2p[name], ref[k]), name
    with pytest.raises(ValueError):
        E.evaluate_batch(graph, el, icp={"estimation": "point_to_line"})
