"""CPU: the pose-score entry points of the C ABI (additions under revision 602) are exported and reject bad arguments
before they touch the GPU; the NumPy restatement (tests/pose_score_reference.py) and the host summary of
utils/pose_score.py give the known answers of DESIGN.md "Pose scores"."""
import os

import numpy as np
import pytest

import pose_score_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_abi_revision_and_export(cdll):
    from cloudaae_amd import _lib
    assert _lib.ABI_VERSION == 602 == cdll.cloudaae_version()
    for name in ("cloudaae_pose_score", "cloudaae_pose_matrix", "cloudaae_cloud_diameter", "cloudaae_pose_stack",
                 "cloudaae_pose_score_workspace_bytes", "cloudaae_cloud_diameter_workspace_bytes"):
        assert hasattr(cdll, name), name
    for name in ("cloudaae_pose_score", "cloudaae_pose_matrix", "cloudaae_cloud_diameter", "cloudaae_pose_stack"):
        assert name in _lib._SIGNATURES
    # two sums per (sample, pose, block of 64 points); one maximum per (cloud, block)
    assert cdll.cloudaae_pose_score_workspace_bytes(1, 1, 2048) == 8 * 2 * 32
    assert cdll.cloudaae_pose_score_workspace_bytes(3, 2, 65) == 8 * 2 * 3 * 2 * 2
    assert cdll.cloudaae_cloud_diameter_workspace_bytes(21, 2048) == 8 * 21 * 32
    assert cdll.cloudaae_pose_score_workspace_bytes(0, 1, 1) == -1
    assert cdll.cloudaae_cloud_diameter_workspace_bytes(1, 0) == -1


# a fake, never dereferenced address: every call below must fail in validation, before any HIP runtime call
_X = 0x1000


def _score_args(**kw):
    a = dict(b=2, p=2, m=2048, model=_X, ps=6, cs=2048 * 6, est=_X, gt=_X, add=_X, adds=_X, nn=_X, ws=_X)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("bad, needle", [
    (dict(b=0), "b, p and m"), (dict(p=0), "b, p and m"), (dict(m=0), "b, p and m"), (dict(b=-1), "b, p and m"),
    (dict(ps=2), "stride"), (dict(cs=2047 * 6 + 2), "overlap"),
    (dict(model=None), "null"), (dict(est=None), "null"), (dict(gt=None), "null"), (dict(add=None), "null"),
    (dict(adds=None), "null"), (dict(ws=None), "null"),
    (dict(b=1 << 20, p=1 << 10, m=1 << 20, cs=1 << 40), "grid"),
])
def test_pose_score_rejects_bad_arguments(cdll, bad, needle):
    assert cdll.cloudaae_pose_score(*_score_args(**bad)) != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_pose_score" in msg and needle in msg, msg


@pytest.mark.parametrize("bad, needle", [
    (dict(b=0), "b must"), (dict(rot=None), "null"), (dict(trans=None), "null"), (dict(out=None), "null"),
    (dict(f64=2), "rot_is_f64"),
])
def test_pose_matrix_rejects_bad_arguments(cdll, bad, needle):
    a = dict(b=4, rot=_X, f64=0, trans=_X, out=_X)
    a.update(bad)
    assert cdll.cloudaae_pose_matrix(*(list(a.values()) + [None])) != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_pose_matrix" in msg and needle in msg, msg


@pytest.mark.parametrize("bad, needle", [
    (dict(c=0), "c and m"), (dict(m=0), "c and m"), (dict(ps=2), "stride"), (dict(cs=10), "overlap"),
    (dict(model=None), "null"), (dict(diam=None), "null"), (dict(ws=None), "null"),
])
def test_cloud_diameter_rejects_bad_arguments(cdll, bad, needle):
    a = dict(c=21, m=2048, model=_X, ps=6, cs=2048 * 6, diam=_X, ws=_X)
    a.update(bad)
    assert cdll.cloudaae_cloud_diameter(*(list(a.values()) + [None])) != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_cloud_diameter" in msg and needle in msg, msg


@pytest.mark.parametrize("bad", [dict(b=0), dict(first=None), dict(second=None), dict(out=None)])
def test_pose_stack_rejects_bad_arguments(cdll, bad):
    a = dict(b=4, first=_X, second=_X, out=_X)
    a.update(bad)
    assert cdll.cloudaae_pose_stack(*(list(a.values()) + [None])) != 0
    assert "cloudaae_pose_stack" in cdll.cloudaae_last_error().decode()


# ---- the restatement on known answers ---------------------------------------------------------------------------------

def _pose(seed, trans=(0.05, -0.1, 0.9)):
    rng = np.random.default_rng(seed)
    return R.pose_matrix(rng.standard_normal(3), np.array(trans, np.float32))


def test_equal_poses_score_zero():
    model = np.random.default_rng(0).standard_normal((300, 3)).astype(np.float32) * 0.05
    G = _pose(1)
    add, adds, nn = R.score(model, G, G)
    assert add == 0.0 and adds == 0.0 and (nn == 0.0).all()


def test_pure_translation():
    """delta = (3, -4, 12) / 1024 on float32 points below 0.25 m: every x + delta is exact in float64, so each point's
    distance is |delta| = 13 / 1024 up to the roundings of one norm, and the mean adds a few more."""
    model = (np.random.default_rng(2).random((512, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(0.5)
    G = np.eye(4)
    delta = np.array([3.0, -4.0, 12.0]) / 1024.0
    E = G.copy()
    E[:3, 3] = delta
    add, adds, nn = R.score(model, E, G)
    assert abs(add - 13.0 / 1024.0) <= 1e-15 * (13.0 / 1024.0)
    assert adds <= add and (nn <= (13.0 / 1024.0) ** 2).all()


def test_lattice_symmetry_gives_zero_adds():
    lat = R.lattice(4, 0.0078125)                                  # centred on 0: a quarter turn about z maps it to itself
    G = _pose(3)
    Rz = np.eye(4)
    Rz[:3, :3] = R.initial_transform(np.array([0.0, 0.0, np.pi / 2]), np.zeros(3))[:3, :3]
    E = G @ Rz
    add, adds, nn = R.score(lat, E, G)
    assert adds <= 1e-12 and add > 1e-3
    far2 = 3 * (3 * 0.0078125) ** 2                                # exact in binary
    assert R.diameter(lat) == np.sqrt(far2)
    assert R.diameter(lat[:1]) == 0.0


def test_block_sum_is_the_stated_order():
    v = np.random.default_rng(4).random(130)
    blocks = []
    for s in range(0, 130, 64):
        b = np.zeros(64)
        b[:len(v[s:s + 64])] = v[s:s + 64]
        for h in (32, 16, 8, 4, 2, 1):
            b = b[:h] + b[h:2 * h]
        blocks.append(b[0])
    assert R.block_sum(v) == (blocks[0] + blocks[1]) + blocks[2]
    assert abs(R.block_sum(v) - v.sum()) < 1e-12


# ---- the summary on closed forms (worked by hand from the definition) -------------------------------------------------

CLOSED = [([0.0] * 7, 1.0), ([0.11, 0.2, 5.0], 0.0), ([0.05], 1.0), ([0.05, 0.2], 0.5), ([0.0, 0.2], 0.5),
          ([0.02, 0.02, 0.06, 0.3], 0.65), ([], 0.0)]


@pytest.mark.parametrize("d, want", CLOSED)
def test_auc_closed_forms(d, want):
    from cloudaae_amd.utils import pose_score as S
    assert abs(R.auc(d) - want) < 1e-15
    assert abs(S.auc(d) - want) < 1e-15
    assert abs(S.auc(d[::-1]) - want) < 1e-15                      # the order of the samples does not matter


def test_auc_of_many_evenly_spaced_distances():
    from cloudaae_amd.utils import pose_score as S
    d = np.linspace(0.0, 0.1, 100001)
    assert abs(S.auc(d) - 0.50001) < 1e-8 and abs(R.auc(d) - S.auc(d)) < 1e-12
    assert abs(S.auc(d * 2, limit=0.2) - S.auc(d)) < 1e-12          # the limit is a parameter


def test_accuracy_thresholds_are_strict():
    from cloudaae_amd.utils import pose_score as S
    below = np.nextafter(0.02, 0.0)
    s = S.summarize([below, 0.02, np.nextafter(0.02, 1.0), 0.0])
    assert s["acc_2cm"] == 0.5 and s["acc_0.1d"] is None and s["n"] == 4
    diam = 0.25
    edge = 0.1 * diam
    s = S.summarize([np.nextafter(edge, 0.0), edge, np.nextafter(edge, 1.0)], diameter=diam)
    assert s["acc_0.1d"] == 1.0 / 3.0
    s = S.summarize([0.01, 0.01], diameter=np.array([0.05, 0.2]))    # per-sample diameters: 0.005 and 0.02
    assert s["acc_0.1d"] == 0.5
    r = R.summarize([0.01, 0.01], diameter=np.array([0.05, 0.2]))
    assert r["acc_0.1d"] == 0.5 and r["acc_2cm"] == 1.0


def test_log_picks_adds_for_symmetric_classes():
    import torch
    from cloudaae_amd.utils import pose_score as S
    assert tuple(S.SYMMETRIC_CLASSES) == (12, 15, 18, 19, 20) == R.SYMMETRIC_CLASSES
    diam = np.full(21, 0.2)
    log = S.PoseScoreLog(("pred", "icp"), diameters=diam)
    cls = torch.tensor([0, 12, 12, 3])
    add = torch.tensor([[0.01, 0.005], [0.09, 0.08], [0.2, 0.15], [0.03, 0.001]], dtype=torch.float64)
    adds = torch.tensor([[0.004, 0.002], [0.01, 0.005], [0.03, 0.012], [0.02, 0.0005]], dtype=torch.float64)
    log.append(cls[:2], add[:2], adds[:2], seq=[48, 48], frame=[1, 2])
    log.append(cls[2:], add[2:], adds[2:])
    rows = log.rows()
    assert rows["class_id"].tolist() == [0, 12, 12, 3] and rows["seq"].tolist() == [48, 48, -1, -1]
    s = log.summary()
    assert sorted(s["classes"]) == [0, 3, 12]
    for k, pose in enumerate(("pred", "icp")):
        a, sdist = add[:, k].numpy(), adds[:, k].numpy()
        pick = R.add_s_pick(cls.numpy(), a, sdist)
        assert pick.tolist() == [a[0], sdist[1], sdist[2], a[3]]
        for metric, d in (("add", a), ("adds", sdist), ("add(-s)", pick)):
            got, want = s["all"][pose][metric], R.summarize(d, diameter=0.2)
            assert got["n"] == 4
            for key in ("auc", "acc_2cm", "acc_0.1d"):
                assert abs(got[key] - want[key]) < 1e-15, (pose, metric, key)
        got = s["classes"][12][pose]["add(-s)"]
        want = R.summarize(sdist[1:3], diameter=0.2)
        assert got["n"] == 2 and abs(got["auc"] - want["auc"]) < 1e-15
    other = S.PoseScoreLog(("pred", "icp"), diameters=diam, symmetric=())       # a parameter
    other.append(cls, add, adds)
    assert other.summary()["all"]["pred"]["add(-s)"] == other.summary()["all"]["pred"]["add"]
    lines = log.lines()
    assert len(lines) == 4 * 2 * 3 and lines[-1].startswith("score all icp add(-s) n 4 ")
    assert all(" auc " in l and " acc_2cm " in l and " acc_0.1d " in l for l in lines)
