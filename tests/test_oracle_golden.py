"""CPU: the oracle against the committed golden vectors and its own properties."""
import glob
import os

import numpy as np
import pytest


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


CHAMFER = ["chamfer_seed0_1x5x6", "chamfer_rand_2x256x256", "chamfer_dup_ties_2x64x64",
           "chamfer_ragged_3x77x1031"]


@pytest.mark.parametrize("name", CHAMFER)
def test_chamfer_oracle_matches_reference_lines(oracle, golden_dir, name):
    # expected outputs were produced by the reference's own C++ lines (oracle/_ref)
    g = _load(golden_dir, name)
    d1, i1, d2, i2 = oracle.nn_distance(g["xyz1"], g["xyz2"])
    assert np.array_equal(i1, g["idx1"]) and np.array_equal(i2, g["idx2"])
    assert np.array_equal(d1, g["dist1"]) and np.array_equal(d2, g["dist2"])
    gx1, gx2 = oracle.nn_distance_grad(g["xyz1"], g["xyz2"], g["grad_dist1"], i1, g["grad_dist2"], i2)
    assert np.array_equal(gx1, g["grad_xyz1"]) and np.array_equal(gx2, g["grad_xyz2"])


def test_chamfer_seed0_known_answer(oracle, golden_dir):
    # the reference's only seeded input (tf_nndistance_cpu.py:28-46) and its brute-force matrix
    g = _load(golden_dir, "chamfer_seed0_1x5x6")
    np.random.seed(0)
    assert np.array_equal(np.random.random((1, 5, 3)), g["pc1_f64"])
    assert np.array_equal(np.random.random((1, 6, 3)), g["pc2_f64"])
    D = g["brute_f64"]
    d1, i1, d2, i2 = oracle.nn_distance(g["xyz1"], g["xyz2"])
    assert np.array_equal(i1[0], D.argmin(1)) and np.array_equal(i2[0], D.argmin(0))
    np.testing.assert_allclose(d1[0], D.min(1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(d2[0], D.min(0), rtol=0, atol=1e-6)


def test_chamfer_against_live_reference_lines(oracle, golden_dir):
    # the reference lines' outputs for these inputs are stored (oracle/make_golden.py: chamfer_live_case); where oracle/_ref
    # was built, the live lines must still give them
    g = _load(golden_dir, "chamfer_live_3x130x513")
    a, b, g1, g2 = g["xyz1"], g["xyz2"], g["grad_dist1"], g["grad_dist2"]
    ref = (g["dist1"], g["idx1"], g["dist2"], g["idx2"])
    rg = (g["grad_xyz1"], g["grad_xyz2"])
    if oracle.have_ref():
        for x, y in zip(oracle.ref_nn_distance(a, b), ref):
            assert np.array_equal(x, y)
        live = oracle.ref_nn_distance_grad(a, b, g1, ref[1], g2, ref[3])
        assert np.array_equal(live[0], rg[0]) and np.array_equal(live[1], rg[1])
    ours = oracle.nn_distance(a, b)
    for x, y in zip(ours, ref):
        assert np.array_equal(x, y)
    og = oracle.nn_distance_grad(a, b, g1, ours[1], g2, ours[3])
    assert np.array_equal(og[0], rg[0]) and np.array_equal(og[1], rg[1])
    # OpenMP over the batch must not change the per-cloud order
    og8 = oracle.nn_distance_grad(a, b, g1, ours[1], g2, ours[3], threads=4)
    assert np.array_equal(og[0], og8[0]) and np.array_equal(og[1], og8[1])


def test_chamfer_brute_force_semantics(oracle):
    # tf_nndistance.py:77-85: squared L2 min / argmin
    rng = np.random.default_rng(7)
    a = rng.standard_normal((2, 50, 3)).astype(np.float32)
    b = rng.standard_normal((2, 70, 3)).astype(np.float32)
    d1, i1, d2, i2 = oracle.nn_distance(a, b)
    D = ((a[:, :, None, :].astype(np.float64) - b[:, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(i1, D.argmin(2)) and np.array_equal(i2, D.argmin(1))
    np.testing.assert_allclose(d1, D.min(2), atol=1e-5)


def test_chamfer_empty_other_cloud(oracle):
    a = np.ones((2, 4, 3), np.float32)
    b = np.zeros((2, 0, 3), np.float32)
    d1, i1, d2, i2 = oracle.nn_distance(a, b)
    assert (d1 == 0).all() and (i1 == 0).all() and d2.shape == (2, 0)


@pytest.mark.parametrize("name", ["fps_rand_2x1024_to_256", "fps_dup_2x700_to_128",
                                  "fps_lattice_1x1500_to_300"])
def test_fps_golden_and_property(oracle, golden_dir, name):
    g = _load(golden_dir, name)
    out = oracle.farthest_point_sample(int(g["npoint"]), g["inp"])
    assert np.array_equal(out, g["out"])
    # property: pick j is an arg-max of the running min distance to picks < j
    P = g["inp"]
    for c in range(P.shape[0]):
        run = np.full(P.shape[1], 1e38, np.float32)
        assert out[c, 0] == 0
        for j in range(1, out.shape[1]):
            d = P[c] - P[c, out[c, j - 1]]
            d = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            run = np.minimum(run, d.astype(np.float32))
            assert run[out[c, j]] == run.max()
            # tie-break of tf_sampling_g.cu:130-165: lowest k mod 512, then lowest k
            ties = np.flatnonzero(run == run.max())
            want = min(ties, key=lambda k: (k % 512, k))
            assert out[c, j] == want


@pytest.mark.parametrize("name", ["knn_xyz_dup_2x300_k10", "knn_feat64_2x257_k10",
                                  "knn_feat64_2x257_k20"])
def test_knn_golden_and_stable_argsort(oracle, golden_dir, name):
    g = _load(golden_dir, name)
    k, c = int(g["k"]), int(g["channels"])
    idx = oracle.knn(g["x"], k, channels=c)
    assert np.array_equal(idx, g["nn_idx"])
    for cl in range(g["x"].shape[0]):
        D = oracle.pairwise_distance(g["x"][cl], channels=c)
        assert np.array_equal(idx[cl], np.argsort(D, axis=1, kind="stable")[:, :k])


def test_knn_formula_order(oracle):
    # D = (sq_i + (-2*inner)) + sq_j with fp32 fma-chain inner (tf_util.py:613-618)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 8)).astype(np.float32)
    D = oracle.pairwise_distance(x)
    sq = np.zeros(40, np.float32)
    for ch in range(8):
        sq = sq + x[:, ch] * x[:, ch]
    inner = np.zeros((40, 40), np.float64)
    for ch in range(8):  # fmaf = exact product + one rounding
        inner = (x[:, None, ch].astype(np.float64) * x[None, :, ch].astype(np.float64) + inner
                 ).astype(np.float32).astype(np.float64)
    want = (sq[:, None] + (-2 * inner).astype(np.float32)).astype(np.float32) + sq[None, :]
    assert np.array_equal(D, want.astype(np.float32))


def test_gather_and_grad(oracle):
    rng = np.random.default_rng(4)
    inp = rng.standard_normal((2, 30, 3)).astype(np.float32)
    idx = rng.integers(0, 30, (2, 12)).astype(np.int32)
    out = oracle.gather_point(inp, idx)
    assert np.array_equal(out, np.take_along_axis(inp, idx[:, :, None].astype(np.int64), 1))
    og = rng.standard_normal((2, 12, 3)).astype(np.float32)
    ig = oracle.gather_point_grad(inp.shape, idx, og)
    want = np.zeros_like(inp)
    for c in range(2):
        for j in range(12):
            want[c, idx[c, j]] += og[c, j]
    assert np.array_equal(ig, want)


def test_prob_sample_golden_and_semantics(oracle, golden_dir):
    """tf_sampling_g.cu:7-104: fixture replay, prefix sums close to a float64 cumsum, every index the
    first one whose prefix sum reaches draw * total."""
    g = np.load(os.path.join(golden_dir, "probsample_2x8227_400.npz"))
    out, cum = oracle.prob_sample(g["inp"], g["inpr"], return_cumsum=True)
    assert np.array_equal(out, g["out"]) and np.array_equal(cum, g["cumsum"])
    ref = np.cumsum(g["inp"].astype(np.float64), axis=1)
    assert np.abs(cum - ref).max() <= 1e-6 * ref.max()
    key = g["inpr"] * cum[:, -1:]
    for b in range(out.shape[0]):
        i = out[b]
        assert (cum[b, i] >= key[b]).all()
        prev = np.where(i > 0, cum[b, np.maximum(i - 1, 0)], -np.inf)
        assert (prev < key[b]).all()
    # quad order on a hand case: a, a+b, c+(a+b), (d+c)+(a+b)
    p = np.array([[0.1, 0.2, 0.3, 0.4, 0.5]], np.float32)
    _, c = oracle.prob_sample(p, np.zeros((1, 1), np.float32), return_cumsum=True)
    a, b_, cc, d, e = (np.float32(v) for v in p[0])
    q3 = (d + cc) + (b_ + a)
    assert np.array_equal(c[0], np.array([a, b_ + a, cc + (b_ + a), q3, e + q3], np.float32))


def test_golden_files_present(golden_dir):
    assert len(glob.glob(os.path.join(golden_dir, "*.npz"))) >= 10


# ---- independent cross-pins of oracle pieces the reference itself cannot pin (TensorFlow is absent).
# They stay labelled "parity unpinned by the reference": these checks only show that the restatement implements the
# documented formula, via a second, independently written implementation.
def test_oracle_batch_norm_equals_torch_functional():
    import torch
    from oracle import model_oracle as MO
    g = torch.Generator().manual_seed(2)
    x = torch.randn(6, 50, 1, 16, generator=g) * 3 + 1
    V = MO.Vars(seed=0)
    V.p["s/gamma"] = (torch.rand(16, generator=g) + 0.5).requires_grad_(True)
    V.p["s/beta"] = torch.randn(16, generator=g).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = MO.batch_norm(xr, "s", V, True, 0.9)
    y.square().sum().backward()
    x2 = x.clone().requires_grad_(True)
    w, b = V.p["s/gamma"].detach().clone().requires_grad_(True), V.p["s/beta"].detach().clone().requires_grad_(True)
    rm, rv = torch.zeros(16), torch.zeros(16)
    # torch's momentum is (1 - decay); its running_var update uses the UNBIASED variance, TF's EMA the biased one
    y2 = torch.nn.functional.batch_norm(x2.reshape(-1, 16), rm, rv, w, b, True, 0.1, MO.BN_EPS).reshape(x.shape)
    y2.square().sum().backward()
    assert torch.allclose(y, y2, rtol=1e-5, atol=1e-5)
    assert torch.allclose(xr.grad, x2.grad, rtol=1e-4, atol=1e-4)
    assert torch.allclose(V.p["s/gamma"].grad, w.grad, rtol=1e-4, atol=1e-3)
    flat = x.reshape(-1, 16)
    assert torch.allclose(V.s["s/moments/Squeeze/ExponentialMovingAverage"], 0.1 * flat.mean(0), rtol=1e-5, atol=1e-6)
    assert torch.allclose(V.s["s/moments/Squeeze_1/ExponentialMovingAverage"], 0.1 * flat.var(0, unbiased=False), rtol=1e-5)
    ye = MO.batch_norm(x, "s", V, False, None)                        # inference: the shadows
    want = (x - V.s["s/moments/Squeeze/ExponentialMovingAverage"]) / torch.sqrt(
        V.s["s/moments/Squeeze_1/ExponentialMovingAverage"] + 1e-3) * V.p["s/gamma"] + V.p["s/beta"]
    assert torch.allclose(ye, want, rtol=1e-5, atol=1e-5)


def test_oracle_adam_equals_the_closed_form_of_tf_apply_adam():
    import torch
    from oracle import model_oracle as MO
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(1000)
    params = {"w": torch.tensor(p0, dtype=torch.float32)}
    opt = MO.AdamTF()
    p, m, v = p0.astype(np.float64), np.zeros(1000), np.zeros(1000)
    for t in range(1, 6):
        g = rng.standard_normal(1000) * 10.0 ** (t - 3)
        opt.apply(params, {"w": torch.tensor(g, dtype=torch.float32)})
        # tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); m, v EMAs; var -= lr_t m / (sqrt(v) + eps)
        gf = g.astype(np.float32).astype(np.float64)
        m = 0.9 * m + 0.1 * gf
        v = 0.999 * v + 0.001 * gf * gf
        p = p - 0.0008 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-8)
        assert np.abs(params["w"].numpy() - p).max() < 5e-6, t
    assert abs(float(opt.b1p) - 0.9 ** 6) < 1e-6 and abs(float(opt.b2p) - 0.999 ** 6) < 1e-6


def test_oracle_fps_equals_naive_argmax_on_tie_free_clouds(oracle):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 500, 3)).astype(np.float32)          # continuous coordinates: no distance ties
    got = oracle.farthest_point_sample(40, x)
    for b in range(3):
        d = np.full(500, 1e38, np.float32)
        idx, last = [0], 0
        for _ in range(39):
            diff = x[b] - x[b, last]
            dist = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
            d = np.minimum(d, dist.astype(np.float32))
            last = int(np.argmax(d))
            idx.append(last)
        assert np.array_equal(got[b], np.array(idx, np.int32)), b
