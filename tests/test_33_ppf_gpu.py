"""GPU: cloudaae_ppf_model_pairs, cloudaae_ppf_vote and cloudaae_ppf_cluster through the C ABI against the NumPy
restatement of DESIGN.md "Pose proposals" (tests/ppf_reference.py), then utils/ppf.py through the renderer,
evaluate_batch(propose=...) and the evaluation's command line.

Keys, reference indices, votes, bins and scores are integers and are compared for equality, no cell left out; stored
directions and poses are compared bit for bit.  Outputs sit between guard rows that are filled with a byte pattern, so
every call starts on garbage."""
import os

import numpy as np
import pytest
import torch

import mesh_models_reference as MR
import pose_verify_reference as V
import ppf_reference as P
import render_reference as R
import test_ppf_host as H

pytestmark = pytest.mark.gpu

GUARD = 4
FILL = 0xA5


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_32_pose_verify_gpu.py)."""

    def __init__(self, rows, cols, dtype, dev):
        item = torch.empty((), dtype=dtype).element_size()
        self.rb = cols * item
        self.full = torch.full(((rows + 2 * GUARD) * self.rb,), FILL, dtype=torch.uint8, device=dev)
        self.view = self.full[GUARD * self.rb:(GUARD + rows) * self.rb].view(dtype).view(rows, cols)
        self.rows = rows

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        full = self.full.cpu().numpy()
        edge = GUARD * self.rb
        assert np.all(full[:edge] == FILL) and np.all(full[edge + self.rows * self.rb:] == FILL), "guard rows were written"
        return self.view.cpu().numpy()


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _d(a, ty, dev):
    return torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def flat_patch(rows, cols, step):
    g = (np.stack(np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"), -1).reshape(-1, 2) * step).astype(np.float32)
    return np.concatenate([g, np.zeros((rows * cols, 1), np.float32)], axis=1)


_cache = {}


def two_sets():
    """S = 2 ragged sets, neither a multiple of 64: 48 oriented points of the L prism and a flat patch of 7 x 10 points
    1 cm apart, all normals +z, so every cosine sits on 0 or 1 and the buckets are few and long; a diameter of 40 cm is
    claimed for it, so that a distance bin of 2 cm holds many pairs of one reference point."""
    if "sets" not in _cache:
        xyz, nrm, diam = H.prism_model(48, seed=7)
        flat = flat_patch(7, 10, 0.01)
        _cache["sets"] = ([(xyz, nrm), (flat, np.tile([0.0, 0.0, 1.0], (70, 1)))], [diam, 0.4])
    return _cache["sets"]


def reference_model(n_alpha):
    if ("model", n_alpha) not in _cache:
        sets, diam = two_sets()
        _cache[("model", n_alpha)] = P.make_model(sets, diam, n_alpha=n_alpha)
    return _cache[("model", n_alpha)]


def product_model(dev, n_alpha):
    from cloudaae_amd.utils import ppf
    if ("product", n_alpha) not in _cache:
        sets, diam = two_sets()
        _cache[("product", n_alpha)] = ppf.PPFModels.from_points([s[0] for s in sets], [s[1] for s in sets], diam, n_alpha=n_alpha,
                                                                 device=dev)
    return _cache[("product", n_alpha)]


# ---- cloudaae_ppf_model_pairs ------------------------------------------------------------------------------------------------
def test_model_pairs_equal_the_restatement(hip, dev):
    sets, diam = two_sets()
    ref = reference_model(30)
    sizes = np.array([len(s[0]) for s in sets])
    assert sizes.tolist() == [48, 70]
    off, poff = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(sizes * sizes)])
    n_pairs = int(poff[-1])
    key, rf, dr = Guarded(n_pairs, 1, torch.int32, dev), Guarded(n_pairs, 1, torch.int32, dev), Guarded(n_pairs, 2, torch.float32, dev)
    g = [_d(off, np.int32, dev), _d(poff, np.int64, dev), _d(ref["xyz"], np.float32, dev), _d(ref["normals"], np.float64, dev),
         _d(ref["dist_step"], np.float64, dev), _d(ref["cos_edges"], np.float64, dev)]
    hip.check(hip.lib().cloudaae_ppf_model_pairs(2, g[0].data_ptr(), g[1].data_ptr(), int(off[-1]), n_pairs, g[2].data_ptr(),
                                                 g[3].data_ptr(), g[4].data_ptr(), 20, 15, g[5].data_ptr(), key.ptr(), rf.ptr(),
                                                 dr.ptr(), hip.stream()), "cloudaae_ppf_model_pairs")
    torch.cuda.synchronize()
    want_key = np.concatenate([p[0].reshape(-1) for p in ref["pairs"]])
    want_ref = np.concatenate([p[1].reshape(-1) for p in ref["pairs"]])
    want_dir = np.concatenate([p[2].reshape(-1, 2) for p in ref["pairs"]])
    got_key, got_ref, got_dir = key.numpy().ravel(), rf.numpy().ravel(), dr.numpy()
    print("pairs %d: key differs in %d, ref in %d, dir in %d; kept %d, skipped %d" % (
        n_pairs, (got_key != want_key).sum(), (got_ref != want_ref).sum(), (_bits(got_dir) != _bits(want_dir)).sum(),
        (want_key >= 0).sum(), (want_key < 0).sum()))
    assert np.array_equal(got_key, want_key) and np.array_equal(got_ref, want_ref)
    assert np.array_equal(_bits(got_dir), _bits(want_dir))
    assert (want_key[poff[1]:] >= 0).sum() > 1000 and len(np.unique(want_key[poff[1]:])) < 40      # few, long buckets
    # the CSR of the product: the same table, sorted by (set, key), pair order inside a bucket
    m = product_model(dev, 30)
    assert np.array_equal(m.pair_key.cpu().numpy(), want_key)
    assert m.bucket_start.dtype == torch.int32 and np.array_equal(m.bucket_start.cpu().numpy(), ref["bucket_start"])
    assert np.array_equal(m.entry_ref.cpu().numpy(), ref["entry_ref"]) and m.n_entries == len(ref["entry_ref"])
    assert np.array_equal(_bits(m.entry_dir.cpu().numpy()), _bits(ref["entry_dir"]))
    for a, b in zip(m.tables, (ref["cos_edges"], ref["alpha_edges"], ref["alpha_cs"])):
        assert np.array_equal(_bits(a), _bits(b))
    # a class without a model in front of and between the sets: the same entries under the other class ids
    from cloudaae_amd.utils import ppf
    moved = ppf.PPFModels.from_points([s[0] for s in sets], [s[1] for s in sets], diam, classes=[3, 1], num_class=5, device=dev)
    assert moved.offsets.tolist() == [0, 0, 70, 70, 118, 118]
    bs = moved.bucket_start.cpu().numpy()
    assert np.array_equal(bs[1] - bs[1, 0], ref["bucket_start"][1] - ref["bucket_start"][1, 0])
    assert np.array_equal(bs[3] - bs[3, 0], ref["bucket_start"][0]) and bs[0].max() == 0 and np.all(bs[4] == moved.n_entries)


# ---- cloudaae_ppf_vote ---------------------------------------------------------------------------------------------------------
def vote_scene():
    """B = 3, N = 70.  Sample 0: class 0, the prism's 48 points under a pose and 22 clutter points, four points masked,
    among them point 0, the would-be first reference; the clutter is spread over more than the prism's diameter, so pairs
    fall past the last distance bin.  Sample 1: class 5, outside the table.  Sample 2: class 1, the flat patch facing the
    camera: hundreds of votes meet in one cell."""
    if "scene" not in _cache:
        sets, _ = two_sets()
        xyz, nrm = sets[0]
        gt = R.pose_matrix([0.5, -0.4, 0.3], [-0.02, 0.01, 0.5])
        rng = np.random.default_rng(33)
        p = xyz.astype(np.float64) @ gt[:3, :3].T + gt[:3, 3]
        n = nrm @ gt[:3, :3].T
        cp = p.mean(axis=0) + rng.uniform(-0.1, 0.1, (22, 3))
        cn = rng.standard_normal((22, 3))
        cn /= np.sqrt((cn * cn).sum(axis=1, keepdims=True))
        order = rng.permutation(70)
        s0, n0 = np.concatenate([p, cp])[order].astype(np.float32), np.concatenate([n, cn])[order]
        s2 = flat_patch(7, 10, 0.01) + np.array([-0.05, -0.08, 0.5], np.float32)
        n2 = np.tile([0.0, 0.0, -1.0], (70, 1))
        scene, normals = np.stack([s0, s0[::-1], s2]), np.stack([n0, n0[::-1], n2])
        mask = np.ones((3, 70), np.uint8)
        mask[0, [0, 3, 10, 69]] = 0
        mask[2, 5] = 0
        _cache["scene"] = (scene, normals, mask, np.array([0, 5, 1], np.int64), gt)
    return _cache["scene"]


@pytest.mark.parametrize("ref_step,n_alpha,peaks", [(3, 30, 2), (1, 6, 4), (3, 6, 1), (1, 30, 1)])
def test_votes_peaks_and_poses_equal_the_restatement(hip, dev, ref_step, n_alpha, peaks):
    scene, normals, mask, cls, _ = vote_scene()
    ref = reference_model(n_alpha)
    m = product_model(dev, n_alpha)
    key = ("votes", ref_step, n_alpha, peaks)
    want = P.vote(scene, normals, mask, cls, ref, ref_step, peaks)
    B, N = mask.shape
    Rn = -(-N // ref_step)
    cells = m.m_max * n_alpha
    assert m.m_max == 70 and want["acc"].shape == (B, Rn, 70, n_alpha)
    acc = Guarded(B * Rn, cells, torch.int32, dev)
    votes, mi, bn = (Guarded(B * Rn, peaks, torch.int32, dev) for _ in range(3))
    pose = Guarded(B * Rn * peaks, 16, torch.float64, dev)
    g = [_d(scene, np.float32, dev), _d(normals, np.float64, dev), _d(mask, np.uint8, dev), _d(cls, np.int64, dev)]
    hip.check(hip.lib().cloudaae_ppf_vote(
        B, N, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), ref_step, peaks, m.num_class,
        m.offsets.data_ptr(), m.m_total, m.m_max, m.xyz.data_ptr(), m.normals.data_ptr(), m.dist_step.data_ptr(), m.n_dist,
        m.n_angle, m.n_alpha, m.cos_edges.data_ptr(), m.alpha_edges.data_ptr(), m.alpha_cs.data_ptr(), m.bucket_start.data_ptr(),
        m.n_entries, m.entry_ref.data_ptr(), m.entry_dir.data_ptr(), votes.ptr(), mi.ptr(), bn.ptr(), pose.ptr(), acc.ptr(),
        hip.stream()), "cloudaae_ppf_vote")
    torch.cuda.synchronize()
    got_acc = acc.numpy().reshape(B, Rn, 70, n_alpha)
    got_pose = pose.numpy().reshape(B, Rn, peaks, 4, 4)
    print("%s: accumulator differs in %d of %d cells (sum %d, largest cell %d); votes in %d, bins in %d, poses in %d of %d numbers"
          % (key, (got_acc != want["acc"]).sum(), got_acc.size, want["acc"].sum(), want["acc"].max(),
             (votes.numpy().reshape(B, Rn, peaks) != want["votes"]).sum(), (bn.numpy().reshape(B, Rn, peaks) != want["bin"]).sum(),
             (_bits(got_pose) != _bits(want["pose"])).sum(), got_pose.size))
    assert np.array_equal(got_acc, want["acc"])
    assert np.array_equal(votes.numpy().reshape(B, Rn, peaks), want["votes"])
    assert np.array_equal(mi.numpy().reshape(B, Rn, peaks), want["model_index"])
    assert np.array_equal(bn.numpy().reshape(B, Rn, peaks), want["bin"])
    assert np.array_equal(_bits(got_pose), _bits(want["pose"]))
    # what the case is there for
    assert want["acc"][0].sum() > 0 and want["acc"][2].max() >= 100 and not want["acc"][1].any()
    assert not want["votes"][1].any() and (want["model_index"][1] == -1).all()
    n_ref0 = -(-66 // ref_step)
    assert want["votes"][0, :n_ref0, 0].max() > 0 and not want["acc"][0, n_ref0:].any()      # 66 usable points: the last slots are empty
    assert want["acc"][0][:, 48:].sum() == 0                                                 # the prism has 48 points of the 70 rows
    # the product's wrapper gives the same without the accumulator
    from cloudaae_amd.utils import ppf
    v = ppf.vote(m, g[0], g[1], g[2], g[3], ref_step, peaks)
    assert np.array_equal(v["votes"].cpu().numpy(), want["votes"]) and np.array_equal(_bits(v["pose"].cpu().numpy()), _bits(want["pose"]))


def test_the_cluttered_scene_has_pairs_past_the_last_bin_and_the_prism_is_found(hip, dev):
    scene, normals, mask, cls, gt = vote_scene()
    ref = reference_model(30)
    # the q_d >= n_dist skip: the far pairs of the cluttered scene have no key
    key = np.stack([P.pair_key(scene[0, r], normals[0, r], scene[0], normals[0], ref["dist_step"][0], 20, 15, ref["cos_edges"])[0]
                    for r in range(70)])
    assert (key < 0).sum() > 70 + 10 and (key >= 0).sum() > 1000
    from cloudaae_amd.utils import ppf
    m = product_model(dev, 30)
    r = ppf.propose_poses(m, _d(scene, np.float32, dev), _d(normals, np.float64, dev), _d(mask, np.uint8, dev), _d(cls, np.int64, dev),
                          top=3, ref_step=3, peaks=2)
    want = P.propose(ref, scene, normals, mask, cls, top=3, ref_step=3, peaks=2)
    assert np.array_equal(r["score"].cpu().numpy(), want["score"]) and np.array_equal(r["valid"].cpu().numpy(), want["valid"])
    assert np.array_equal(_bits(r["pose"].cpu().numpy()), _bits(want["pose"]))
    tt2, rot_bound = P.thresholds(ref["diameters"])
    dist, trace = P.pose_errors(want["pose"][0, 0], gt)
    print("prism: %.4f m and trace %.4f from the truth (%.4f, %.4f); scores %s" % (dist, trace, np.sqrt(tt2[0]), rot_bound,
                                                                                   want["score"].tolist()))
    assert dist * dist <= tt2[0] and trace >= rot_bound and not want["valid"][1].any()


# ---- cloudaae_ppf_cluster ------------------------------------------------------------------------------------------------------
def cluster_case():
    """B = 3, C = 70 candidates (no multiple of 64).  Sample 0: candidate 0 has the most votes and founds the first cluster at
    the identity; candidates exactly on, just inside and just outside the rotation bound and the translation threshold
    follow with equal votes, then random poses; the last ten have no votes.  Sample 1: two candidates close to each other
    and nothing else -- one cluster, fewer than top.  Sample 2: a class outside the table."""
    rng = np.random.default_rng(70)
    C = 70
    theta, x0 = 2.0 * np.pi / 30, 0.0185

    def rz(t, x=0.0):
        c, s = np.cos(t), np.sin(t)
        T = np.eye(4)
        T[:2, :2] = [[c, -s], [s, c]]
        T[0, 3] = x
        return T
    pose = np.stack([R.pose_matrix(rng.standard_normal(3) * 0.8, rng.standard_normal(3) * 0.05) for _ in range(3 * C)]).reshape(3, C, 4, 4)
    votes = np.full((3, C), 7, np.int32)
    pose[0, 0] = np.eye(4)
    votes[0, 0] = 50
    pose[0, 1:7] = [rz(theta), rz(theta + 1e-9), rz(theta - 1e-9), rz(0.0, x0), rz(0.0, np.nextafter(x0, 1.0)), rz(0.0, np.nextafter(x0, 0.0))]
    votes[0, 20:30] = rng.integers(1, 30, 10)
    votes[0, 60:] = 0
    votes[1] = 0
    votes[1, [13, 66]] = [4, 9]
    pose[1, 66] = pose[1, 13]
    pose[1, 66, 0, 3] += 0.001
    c0 = np.cos(theta)
    return votes, pose, np.array([0, 1, 2], np.int64), np.array([x0 * x0, 1.0]), (c0 + c0) + 1.0


@pytest.mark.parametrize("top", [4, 1, 64])
def test_clusters_equal_the_restatement(hip, dev, top):
    votes, pose, cls, tt2, rot_bound = cluster_case()
    want = P.cluster(votes, pose, cls, tt2, rot_bound, top)
    if top == 4:
        first = want["members"][0][0]
        print("first cluster: %s; clusters of sample 0: %d" % (first, len(P.cluster(votes, pose, cls, tt2, rot_bound, 64)["members"][0])))
        # on the bound and inside it join; outside it does not
        assert first[0] == 0 and {1, 3, 4, 6} <= set(first[1]) and not {2, 5} & set(first[1])
        assert want["valid"].tolist() == [[1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0]] and want["score"][1, 0] == 13
        assert np.array_equal(want["pose"][1, 0], pose[1, 66])
    B, C = votes.shape
    out, rot = Guarded(B * top, 16, torch.float64, dev), Guarded(B * top, 3, torch.float64, dev)
    trans, score, valid = Guarded(B * top, 3, torch.float32, dev), Guarded(B, top, torch.int32, dev), Guarded(B, top, torch.int32, dev)
    g = [_d(votes, np.int32, dev), _d(pose, np.float64, dev), _d(cls, np.int64, dev), _d(tt2, np.float64, dev)]
    hip.check(hip.lib().cloudaae_ppf_cluster(B, C, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), 2, g[3].data_ptr(),
                                             float(rot_bound), top, out.ptr(), rot.ptr(), trans.ptr(), score.ptr(), valid.ptr(),
                                             hip.stream()), "cloudaae_ppf_cluster")
    torch.cuda.synchronize()
    assert np.array_equal(score.numpy(), want["score"]) and np.array_equal(valid.numpy(), want["valid"])
    got = out.numpy().reshape(B, top, 4, 4)
    assert np.array_equal(_bits(got), _bits(want["pose"]))
    assert np.array_equal(trans.numpy().reshape(B, top, 3), want["trans"])
    ax = rot.numpy().reshape(B, top, 3)
    worst = max(np.abs(R.pose_matrix(ax[b, t], [0, 0, 0])[:3, :3] - got[b, t, :3, :3]).max() for b in range(B) for t in range(top))
    print("top %d: rodrigues(rot_axag) against the pose, worst %.3g" % (top, worst))
    assert worst <= 1e-12 and np.sqrt((ax * ax).sum(axis=2)).max() <= np.pi + 1e-15


def test_limits_are_refused_without_a_launch(hip, dev):
    from cloudaae_amd.utils import ppf
    L = hip.lib()
    # a table that does not fit the LDS: 1400 points x 30 bins x 4 bytes > 158 KiB -- on the host, before anything is built
    rng = np.random.default_rng(1)
    big = rng.random((1400, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="LDS"):
        ppf.PPFModels.from_points([big], [np.tile([0.0, 0.0, 1.0], (1400, 1))], [1.0], device=dev)
    m = product_model(dev, 30)
    scene, normals, mask, cls, _ = vote_scene()
    g = [_d(scene, np.float32, dev), _d(normals, np.float64, dev), _d(mask, np.uint8, dev), _d(cls, np.int64, dev)]
    votes, mi, bn = (Guarded(3 * 14, 2, torch.int32, dev) for _ in range(3))
    pose = Guarded(3 * 14 * 2, 16, torch.float64, dev)

    def call(b=3, n=70, ref_step=5, peaks=2, m_max=m.m_max, m_total=m.m_total, n_alpha=30, n_entries=m.n_entries, out=votes.ptr(),
             sc=g[0].data_ptr()):
        return L.cloudaae_ppf_vote(b, n, sc, g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), ref_step, peaks, m.num_class,
                                   m.offsets.data_ptr(), m_total, m_max, m.xyz.data_ptr(), m.normals.data_ptr(),
                                   m.dist_step.data_ptr(), m.n_dist, m.n_angle, n_alpha, m.cos_edges.data_ptr(),
                                   m.alpha_edges.data_ptr(), m.alpha_cs.data_ptr(), m.bucket_start.data_ptr(), n_entries,
                                   m.entry_ref.data_ptr(), m.entry_dir.data_ptr(), out, mi.ptr(), bn.ptr(), pose.ptr(), None,
                                   hip.stream())
    assert call(m_max=1400, m_total=1400) != 0
    err = L.cloudaae_last_error()
    assert b"cloudaae_ppf_vote" in err and b"LDS" in err
    assert call(b=0) != 0 and call(n=1) != 0 and call(ref_step=0) != 0 and call(ref_step=71) != 0 and call(peaks=0) != 0
    assert call(peaks=5) != 0 and call(n_alpha=7) != 0 and call(n_alpha=0) != 0 and call(n_entries=-1) != 0
    assert call(out=None) != 0 and call(sc=None) != 0 and call(m_max=0) != 0
    torch.cuda.synchronize()
    for buf in (votes, mi, bn, pose):
        assert np.all(buf.numpy().view(np.uint8) == FILL)
    assert call() == 0
    torch.cuda.synchronize()
    assert votes.numpy().max() > 0
    tt2 = _d([1.0, 1.0], np.float64, dev)
    cv, cp = _d(np.ones((1, 5)), np.int32, dev), _d(np.tile(np.eye(4).reshape(16), (5, 1)), np.float64, dev)
    out, rot, trans = Guarded(2, 16, torch.float64, dev), Guarded(2, 3, torch.float64, dev), Guarded(2, 3, torch.float32, dev)
    score, valid = Guarded(1, 2, torch.int32, dev), Guarded(1, 2, torch.int32, dev)

    def clu(b=1, c=5, top=2, nclass=2, bound=2.9, o=out.ptr(), v=cv.data_ptr()):
        return L.cloudaae_ppf_cluster(b, c, v, cp.data_ptr(), g[3].data_ptr(), nclass, tt2.data_ptr(), bound, top, o, rot.ptr(),
                                      trans.ptr(), score.ptr(), valid.ptr(), hip.stream())
    assert clu(c=4097) != 0
    assert b"cloudaae_ppf_cluster" in L.cloudaae_last_error()
    assert clu(b=0) != 0 and clu(c=0) != 0 and clu(top=0) != 0 and clu(top=65) != 0 and clu(nclass=0) != 0
    assert clu(bound=float("nan")) != 0 and clu(o=None) != 0 and clu(v=None) != 0
    torch.cuda.synchronize()
    for buf in (out, rot, trans, score, valid):
        assert np.all(buf.numpy().view(np.uint8) == FILL)
    assert clu() == 0
    torch.cuda.synchronize()
    assert score.numpy().tolist() == [[5, 0]] and valid.numpy().tolist() == [[1, 0]]       # five identical candidates: one cluster
    key = Guarded(4, 1, torch.int32, dev)

    def pairs(s=1, m_total=2, n_pairs=4, n_dist=20, n_angle=15, k=key.ptr()):
        return L.cloudaae_ppf_model_pairs(s, m.offsets.data_ptr(), m.pair_offsets.data_ptr(), m_total, n_pairs, m.xyz.data_ptr(),
                                          m.normals.data_ptr(), m.dist_step.data_ptr(), n_dist, n_angle, m.cos_edges.data_ptr(), k,
                                          key.ptr(), key.ptr(), hip.stream())
    assert pairs(s=0) != 0
    assert b"cloudaae_ppf_model_pairs" in L.cloudaae_last_error()
    assert pairs(m_total=0) != 0 and pairs(n_pairs=0) != 0 and pairs(n_dist=0) != 0 and pairs(n_angle=65) != 0 and pairs(k=None) != 0
    assert pairs(n_dist=1 << 20, n_angle=64) != 0
    torch.cuda.synchronize()
    assert np.all(key.numpy().view(np.uint8) == FILL)


# ---- through the renderer ---------------------------------------------------------------------------------------------------------
def test_a_rendered_prism_is_proposed_near_its_pose_as_the_restatement_does(hip, dev):
    from cloudaae_amd.utils import ppf, render
    lv, lt = V.l_prism()
    gt = R.pose_matrix([0.5, -0.4, 0.3], [-0.02, 0.01, 0.5])
    intr = np.array([[150.0, 150.0, 79.5, 59.5, 10000.0]], np.float32)
    fr = render.render_frames([(lv, lt)], [[(0, 1, gt)]], intr, 120, 160, device=dev)
    depth = fr["depth"][0].cpu().numpy().view(np.uint16).astype(np.float64) / 10000.0
    v, u = np.nonzero((fr["label"][0].cpu().numpy() == 1) & (depth > 0))            # the segment
    z = depth[v, u]
    pts = np.stack([(u - 79.5) * z / 150.0, (v - 59.5) * z / 150.0, z], axis=1)[::3].astype(np.float32)
    assert 150 <= len(pts) <= 1024, len(pts)
    models = ppf.PPFModels.from_meshes([(lv, lt)], num_point=256, device=dev)
    scene = _d(pts[None], np.float32, dev)
    normals, mask = ppf.scene_normals(scene, 0.012)
    assert mask.dtype == torch.uint8 and int(mask.sum()) >= 0.9 * len(pts)
    cls = torch.zeros(1, dtype=torch.int64, device=dev)
    got = ppf.propose_poses(models, scene, normals, mask, cls, top=4)
    ref = dict(offsets=models.offsets.cpu().numpy(), xyz=models.xyz.cpu().numpy(), normals=models.normals.cpu().numpy(),
               dist_step=models.dist_step.cpu().numpy(), n_dist=20, n_angle=15, n_alpha=30, cos_edges=models.tables[0],
               alpha_edges=models.tables[1], alpha_cs=models.tables[2], bucket_start=models.bucket_start.cpu().numpy(),
               entry_ref=models.entry_ref.cpu().numpy(), entry_dir=models.entry_dir.cpu().numpy(), m_max=256,
               diameters=models.diameters)
    # the table itself against the restatement, then the proposals on the same inputs
    key, rf, dr = P.model_pairs(ref["xyz"], ref["normals"], ref["dist_step"][0], 20, 15, ref["cos_edges"])
    assert np.array_equal(models.pair_key.cpu().numpy(), key.reshape(-1))
    assert np.array_equal(_bits(models.pair_dir.cpu().numpy()), _bits(dr.reshape(-1, 2)))
    want = P.propose(ref, pts[None], normals.cpu().numpy(), mask.cpu().numpy(), [0], top=4)
    assert np.array_equal(got["score"].cpu().numpy(), want["score"]) and np.array_equal(got["valid"].cpu().numpy(), want["valid"])
    assert np.array_equal(_bits(got["pose"].cpu().numpy()), _bits(want["pose"]))
    assert np.array_equal(_bits(models.trans_thresh2.cpu().numpy()), _bits(P.thresholds(models.diameters)[0]))
    tt2, rot_bound = P.thresholds(models.diameters)
    errs = [P.pose_errors(want["pose"][0, t], gt) for t in range(4) if want["valid"][0, t]]
    print("rendered prism, %d points: scores %s, (metres, trace) from the truth %s; thresholds %.4f m, trace %.4f"
          % (len(pts), want["score"][0].tolist(), errs, np.sqrt(tt2[0]), rot_bound))
    assert any(d * d <= tt2[0] and tr >= rot_bound for d, tr in errs)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def records(hip, dev, tmp_path_factory):
    """The two made-up meshes, four rendered frames of 160 x 120, the element of class 0 with its frames and labels and
    a randomly initialised graph, as tests/test_32_pose_verify_gpu.py builds them; and the prism's pair table."""
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import ppf, render
    tmp = tmp_path_factory.mktemp("propose")
    os.makedirs(str(tmp / "meshes"))
    lv, lt = V.l_prism()
    cv, ct, _ = MR.cube()
    _write_ply(str(tmp / "meshes" / "obj_000001.ply"), lv * np.float32(1500.0), lt)
    _write_ply(str(tmp / "meshes" / "obj_000002.ply"), (cv - np.float32(0.5)) * np.array([240.0, 240.0, 30.0], np.float32), ct)
    render.main(["--meshes", str(tmp / "meshes"), "--out", str(tmp / "data"), "--frames", "4", "--objects", "2", "--seq", "48",
                 "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    path = str(tmp / "data" / "0048_pcnn.tfrecord")
    files = mm.mesh_files(str(tmp / "meshes"))
    models = mm.models_from_meshes(files, scale=0.001, oversample=2, device=dev)
    packed = mm.pack_meshes(files, 0.001, dev)
    frames = tfrecord_io.read_frames(path, verify=True)
    N = 128
    el = E.element_from_frames(frames, 0, N, models, seed=4, device=dev, keep_frames=True, keep_labels=True)
    assert el is not None
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": len(el['class_id'])})
    table = ppf.PPFModels.from_meshes(files[:1], num_point=128, scale=0.001, classes=[0], num_class=2, device=dev)
    return dict(tmp=tmp, path=path, models=models, packed=packed, el=el, graph=graph, N=N, ppf=table)


def test_evaluate_batch_appends_the_proposals_to_the_candidates(hip, dev, records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import pose_verify as PV
    el, graph, packed, models = records['el'], records['graph'], records['packed'], records['models']
    tensors = {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}
    B = len(el['class_id'])
    table = PV.HypothesisTable.from_models(models[:1], classes=[0], num_class=2)
    verify = dict(meshes=packed, mesh_index=None, hypotheses=table, tau=0.01, mode=0)
    propose = dict(models=records['ppf'], top=3)
    for icp in (True, None):
        base = E.evaluate_batch(graph, tensors, icp=icp, score=True, verify=verify)
        same = E.evaluate_batch(graph, tensors, icp=icp, score=True, verify=verify, propose=None)
        assert set(same) == set(base)
        for k, v in base.items():                                     # propose=None: every output is today's
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, same[k]), k
        out = E.evaluate_batch(graph, tensors, icp=icp, score=True, verify=verify, propose=propose)
        assert set(out) - set(base) == {"proposed_poses", "proposed_score", "proposed_valid"}
        assert tuple(out['proposed_poses'].shape) == (B, 3, 4, 4) and out['proposed_poses'].dtype == torch.float64
        assert out['proposed_score'].dtype == torch.int32 and tuple(out['proposed_valid'].shape) == (B, 3)
        cand = out['verify_candidates']
        assert tuple(cand.shape) == (B, 7, 4, 4) and tuple(out['verify_counts'].shape) == (B, 7, 6)
        # the first P_h candidates are those of the call without proposals, bit for bit
        assert torch.equal(cand[:, :4], base['verify_candidates'])
        assert torch.equal(out['verify_counts'][:, :4], base['verify_counts'])
        assert torch.equal(out['verify_score'][:, :4], base['verify_score'])
        for k, v in base.items():                                     # what does not depend on the winner is unchanged
            if isinstance(v, torch.Tensor) and not (k.startswith('verify_') or k.endswith('_ver')):
                assert torch.equal(v, out[k]), k
        ok = out['proposed_valid'] != 0
        print("icp %s: proposal scores %s valid %s best %s verify_score %s" % (icp, out['proposed_score'].tolist(), ok.tolist(),
                                                                               out['verify_best'].tolist(), out['verify_score'].tolist()))
        assert bool(ok[:, 0].all())                                   # every segment of 128 points yields a cluster
        if icp is None:
            assert torch.equal(cand[:, 4:][ok], out['proposed_poses'][ok])
            assert torch.equal(cand[:, 4:][~ok], cand[:, 0:1].expand(B, 3, 4, 4)[~ok])
        best = out['verify_best'].to(torch.int64)
        assert torch.equal(out['transformation_ver'], cand[torch.arange(B, device=dev), best])
        assert float(out['verify_score'][:, 4:][~ok].sum()) == 0.0   # an invalid proposal cannot win
    # without verify the proposals are reported alone
    plain = E.evaluate_batch(graph, tensors)
    alone = E.evaluate_batch(graph, tensors, propose=propose)
    assert set(alone) - set(plain) == {"proposed_poses", "proposed_score", "proposed_valid"}
    assert torch.equal(alone['proposed_poses'], out['proposed_poses'])
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, alone[k]), k
    with pytest.raises(ValueError, match="replay"):
        E.evaluate_batch(graph, tensors, replay=True, propose=propose)
    with pytest.raises(ValueError, match="PPFModels"):
        E.evaluate_batch(graph, tensors, propose=dict(top=3))


def test_command_line_prints_the_propose_line(hip, dev, records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    tmp, path = records['tmp'], records['path']
    obj = str(tmp / "obj_models.tfrecords")
    mm.main(["--meshes", str(tmp / "meshes"), "--out", obj, "--scale", "0.001", "--oversample", "2"])
    graph = T.TrainGraph({"num_point": 128, "gpu": 0}, {}, {"batch_size": 1})
    ckpt = graph.save(str(tmp / "model.ckpt"))
    common = ["--files", path, "--object_model", obj, "--trained_model", ckpt[:-len(".npz")], "--target_cls", "0",
              "--num_point", "128", "--batch_size", "1"]
    capsys.readouterr()
    assert E.main(common + ["--verify", "--icp", "--meshes", str(tmp / "meshes"), "--mesh_scale", "0.001", "--propose", "ppf",
                            "--propose_top", "2", "--propose_points", "128"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    n = int([ln for ln in lines if ln.startswith("batch size ")][0].split()[-1])
    prop = [ln for ln in lines if ln.startswith("propose ")]
    assert n >= 1 and len(prop) == 1 and lines[-1] == prop[0], lines[-6:]
    tok = prop[0].split()
    assert tok[:4] == ["propose", "class", "0", "n"] and int(tok[4]) == n
    assert [tok[i] for i in (5, 7, 9)] == ["from_prediction", "from_flip", "from_proposal"]
    assert sum(int(tok[i]) for i in (6, 8, 10)) == n
    assert lines[-2].startswith("verify class 0 ")
    for bad in (["--propose", "ppf"], ["--propose", "ppf", "--verify"]):
        with pytest.raises(SystemExit) as err:
            E.main(common + bad)
        assert err.value.code == 2 and "--propose" in capsys.readouterr().err
