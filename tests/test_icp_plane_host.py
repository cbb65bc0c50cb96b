"""CPU: the point-to-plane ICP and the normal estimation entry points are exported and reject bad arguments before
they touch memory; the two NumPy restatements (tests/normals_reference.py, tests/icp_plane_reference.py) behave as
their definitions say on analytic inputs."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_exports_and_abi_revision(cdll):
    from cloudaae_amd import _lib
    for name in ("cloudaae_estimate_normals", "cloudaae_estimate_normals_workspace_bytes",
                 "cloudaae_icp_point_to_plane"):
        assert hasattr(cdll, name), name
        assert name in _lib._SIGNATURES or name.endswith("_bytes")
    assert _lib.ABI_VERSION == 602 and cdll.cloudaae_version() == 602
    assert cdll.cloudaae_estimate_normals_workspace_bytes(1, 2048) > 0
    assert cdll.cloudaae_estimate_normals_workspace_bytes(0, 2048) == -1
    assert cdll.cloudaae_estimate_normals_workspace_bytes(1, 0) == -1
    assert cdll.cloudaae_estimate_normals_workspace_bytes(1, (1 << 28) + 1) == -1


# a fake, never dereferenced address: every call below must fail in validation, before any HIP runtime call
_X = 0x1000


def _icp_args(**kw):
    a = dict(b=1, m=1024, src=_X, sps=3, scs=1024 * 3, n=2048, dst=_X, dps=6, dcs=2048 * 6, normals=_X, inverse=1,
             rot=_X, trans=_X, radius=0.01, decay=0.9, rounds=10, max_it=30, rf=1e-6, rr=1e-6, T=_X, rot_out=_X,
             trans_out=_X, fit=_X, rmse=_X, its=_X)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("bad, needle", [
    (dict(b=0), "b, m and n"), (dict(m=0), "b, m and n"), (dict(n=0), "b, m and n"),
    (dict(n=4097), "limit"), (dict(m=4097), "limit"),
    (dict(rounds=-1), "rounds"), (dict(max_it=-1), "max_iteration"),
    (dict(radius=0.0), "radius"), (dict(radius=-0.01), "radius"), (dict(radius=float("inf")), "radius"),
    (dict(decay=0.0), "decay"), (dict(decay=1.5), "decay"), (dict(decay=-0.9), "decay"),
    (dict(sps=2), "stride"), (dict(dps=2), "stride"),
    (dict(src=None), "null"), (dict(dst=None), "null"), (dict(normals=None), "null"), (dict(rot=None), "null"),
    (dict(trans=None), "null"), (dict(T=None), "null"), (dict(rot_out=None), "null"), (dict(trans_out=None), "null"),
    (dict(fit=None), "null"), (dict(rmse=None), "null"), (dict(its=None), "null"),
])
def test_point_to_plane_rejects_invalid_arguments(cdll, bad, needle):
    rc = cdll.cloudaae_icp_point_to_plane(*_icp_args(**bad))
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_icp_point_to_plane" in msg and needle in msg, msg


def _normals_args(**kw):
    a = dict(s=1, offsets=_X, xyz=_X, ps=3, max_points=2048, k=2048, queries=_X, qps=3, qss=2048 * 3, radius=0.015,
             min_neighbors=3, viewpoint=None, normals=_X, eig=_X, count=_X, ws=_X, ws_bytes=1 << 30)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("bad, needle", [
    (dict(s=0), "s must"), (dict(k=0), "k must"), (dict(max_points=0), "max_points"),
    (dict(max_points=(1 << 28) + 1), "max_points"),
    (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
    (dict(min_neighbors=2), "min_neighbors"), (dict(min_neighbors=0), "min_neighbors"),
    (dict(ps=2), "stride"), (dict(qps=2), "stride"), (dict(s=2, qss=3), "overlap"),
    (dict(offsets=None), "null"), (dict(xyz=None), "null"), (dict(queries=None), "null"), (dict(normals=None), "null"),
    (dict(eig=None), "null"), (dict(count=None), "null"), (dict(ws=None), "null"),
    (dict(ws_bytes=16), "workspace"),
])
def test_estimate_normals_rejects_invalid_arguments(cdll, bad, needle):
    rc = cdll.cloudaae_estimate_normals(*_normals_args(**bad))
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_estimate_normals" in msg and needle in msg, msg


def _sphere(n, radius, rng):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * radius).astype(np.float32)


def test_restated_normals_of_a_sphere_point_along_the_radius():
    """6000 points on a sphere of 0.1 m, neighbourhood 0.02 m: the cap a query sees is symmetric about its radius up to
    the sampling, so the normal lies along it (the cap's own sag, r^2 / 2R = 2 mm, does not tilt it)."""
    import normals_reference as NR
    rng = np.random.default_rng(3)
    pts = _sphere(6000, 0.1, rng)
    q = pts[:200]
    n, eig, count = NR.estimate_normals(pts, 0.02, queries=q, viewpoint=(0.0, 0.0, 0.0))
    assert count.min() >= 20
    radial = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    cos = (n * radial).sum(axis=1)
    assert np.all(cos < 0.0)                                   # flipped to face the centre
    assert np.degrees(np.arccos(np.abs(cos))).max() < 5.0
    assert np.all(np.diff(eig, axis=1) >= 0.0) and np.all(NR.relative_gap(eig) >= 0.1)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-14
    # too few neighbours: (0, 0, 1), zeros, the count
    n2, eig2, count2 = NR.estimate_normals(pts, 1e-4, queries=q, viewpoint=(0.0, 0.0, 0.0))
    assert np.all(count2 == 1) and np.all(n2 == [0.0, 0.0, 1.0]) and np.all(eig2 == 0.0)
    # the order of the sums changes the last bits only
    n3, eig3, count3 = NR.estimate_normals(pts, 0.02, queries=q, reverse=True)
    assert np.array_equal(count3, count)
    assert (1.0 - np.abs((n * n3).sum(axis=1))).max() < 1e-12


def test_restated_plane_update_removes_the_residual_of_a_plane():
    """Targets on the three coordinate planes through the origin (a corner; one plane alone leaves three of the six
    unknowns free, which the definition answers with no update -- asserted below), sources = the targets shifted by
    4 mm.  The residual r = (p - q) . n is then linear in the update with the exact solution x = (0, 0, 0, -shift):
    ONE update brings sum r^2 from 1e-2 down to rounding level.  With a small rotation on top the first update
    leaves the second-order term, and the second one removes it."""
    import icp_plane_reference as PL
    import icp_reference as R
    rng = np.random.default_rng(8)
    uv = rng.uniform(0.0, 0.1, (600, 2))
    Q = np.zeros((600, 3))
    Nq = np.zeros((600, 3))
    for k in range(3):                                   # plane k: coordinate k is 0, normal e_k
        rows = slice(200 * k, 200 * (k + 1))
        Q[rows, (k + 1) % 3] = uv[rows, 0]
        Q[rows, (k + 2) % 3] = uv[rows, 1]
        Nq[rows, k] = 1.0
    shift = np.array([0.004, -0.002, 0.003])
    P = Q + shift
    _, _, r0 = PL.system(P, Q, Nq)
    U = PL.plane_update(P, Q, Nq)
    assert U is not None
    _, _, r1 = PL.system(R.apply(U, P), Q, Nq)
    assert (r0 * r0).sum() > 1e-3
    assert (r1 * r1).sum() < 1e-28
    assert np.abs(U[:3, 3] + shift).max() < 1e-15 and np.abs(U[:3, :3] - np.eye(3)).max() < 1e-13
    # rotation and shift: second order after one update, rounding after three
    T = R.initial_transform(np.array([0.01, -0.02, 0.015]), shift)
    P = R.apply(T, Q)
    sq = [(PL.system(P, Q, Nq)[2] ** 2).sum()]
    for _ in range(3):
        U = PL.plane_update(P, Q, Nq)
        assert U is not None and np.abs(U[:3, :3] @ U[:3, :3].T - np.eye(3)).max() < 1e-15
        P = R.apply(U, P)
        sq.append((PL.system(P, Q, Nq)[2] ** 2).sum())
    assert sq[1] < 1e-4 * sq[0] and sq[3] < 1e-24 * sq[0], sq
    # one plane alone, fewer than six correspondences, a zero system: no update
    one = slice(0, 200)
    assert PL.plane_update(Q[one] + shift, Q[one], Nq[one]) is None
    assert PL.plane_update(P[:5], Q[:5], Nq[:5]) is None
    assert PL.ldl_solve(np.zeros((6, 6)), np.zeros(6)) is None
    # inversion of a rigid transform
    assert np.abs(PL.compose(PL.invert(T), T) - np.eye(4)).max() < 1e-15
