"""CPU: what tests/test_49_point_op_variants_gpu.py relies on, shown where no GPU is needed.

- the NumPy farthest point sampling of tests/sampling_reference.py is the oracle's, at every size of the GPU test;
- the lattice clouds of the GPU test DISCRIMINATE: a kernel with a wrong tie-break (lowest k among the maxima; or the right
  thread, k mod 512 lowest, but its highest k) returns another index list within the rounds the GPU test runs;
- every Chamfer case has queries whose minimum sits at two candidates, every kNN case a query with a tie at the k-th distance;
- every case reaches the kernel variant it is named after (the variant queries launch nothing), and together the cases
  reach every variant the GPU test promises;
- the bare GatherPointGrad op refuses tensors its kernel would misread, before anything is launched.
"""
import numpy as np
import pytest
import torch

import sampling_reference as R


@pytest.fixture(scope="module")
def lib():
    from cloudaae_amd import _lib
    return _lib


@pytest.fixture
def host_knobs(lib):
    touched = []

    def set_(name, value):
        touched.append(name)
        lib.set_knob(name, value)
    yield set_
    for name in touched:
        lib.set_knob(name, None)


def _knn_query(lib):
    return lambda *args: int(lib.lib().cloudaae_knn_variant(*args))


@pytest.mark.parametrize("case", R.FPS_CASES, ids=R.fps_id)
def test_numpy_fps_is_the_oracle(oracle, case):
    p = R.fps_cloud(case)
    assert np.array_equal(R.farthest_point_sample(case.m, p), oracle.farthest_point_sample(case.m, p, threads=8))


def test_numpy_fps_on_continuous_and_duplicated_clouds(oracle):
    rng = np.random.default_rng(5)
    p = rng.standard_normal((2, 1300, 3)).astype(np.float32)
    p[:, 650:750] = p[:, :100]
    assert np.array_equal(R.farthest_point_sample(200, p), oracle.farthest_point_sample(200, p))
    one = np.repeat(p[:, :1], 700, axis=1)             # one point 700 times: every round an n-way tie, index 0 wins
    assert not R.farthest_point_sample(30, one).any()


@pytest.mark.parametrize("case", [c for c in R.FPS_CASES if c.n >= 513 and c.m >= R.FPS_ROUNDS and c.m <= c.n], ids=R.fps_id)
def test_lattice_clouds_tell_wrong_tie_breaks_apart(case):
    p = R.fps_cloud(case)[:2]
    m = R.FPS_ROUNDS                                    # (within the rounds every such case runs)
    right = R.farthest_point_sample(m, p)
    first = R.farthest_point_sample(m, p, rule="lowest_k")
    last = R.farthest_point_sample(m, p, rule="highest_k_of_lane")
    for cloud in range(p.shape[0]):
        assert len(set(right[cloud].tolist())) == m, "a repeated pick: the cloud ran out of distinct points"
        d1, d2 = R.first_divergence(right[cloud], first[cloud]), R.first_divergence(right[cloud], last[cloud])
        print("n = %5d cloud %d: 'lowest k' diverges at round %s, 'lowest k mod 512, highest k' at round %s" % (case.n, cloud, d1, d2))
        assert d1 is not None
        if case.n >= 1024:
            assert d2 is not None


def test_fps_cases_reach_their_variants(lib):
    q = lib.lib().cloudaae_farthest_point_sample_variant
    for c in R.FPS_CASES:
        assert R.fps_variant_name(int(q(c.n))) == c.variant, c
    assert {c.variant for c in R.FPS_CASES} == {"ppt1", "ppt2", "ppt4", "ppt8", "ppt16", "ppt32", "ppt32-memory", "big"}
    assert int(q(0)) == -1 and R.fps_variant_name(int(q(1))) == "ppt1"
    # each boundary of the dispatch has a case on either side
    for lo in (512, 1024, 2048, 4096, 8192, 12288, 16384):
        assert R.fps_variant_name(int(q(lo))) != R.fps_variant_name(int(q(lo + 1)))
        assert {lo, lo + 1} <= {c.n for c in R.FPS_CASES}


@pytest.mark.parametrize("case", R.KNN_CASES, ids=R.knn_id)
def test_knn_cases_reach_their_variants_and_have_ties(lib, host_knobs, oracle, case):
    if case.wide is not None:
        host_knobs("CLOUDAAE_KNN3_WIDE", case.wide)
    name, K = R.knn_variant_name(_knn_query(lib)(case.b, case.n, case.c, case.ld, case.k, 0 if case.misaligned else 1))
    assert name == case.variant and K == (10 if case.k <= 10 else 20)
    # a tie at the k-th distance: some query's k-th and (k+1)-th neighbours are equally far (one cloud is enough)
    x = R.knn_cloud(case)[:1]
    _, d = oracle.knn(x, case.k + 1, channels=case.c, threads=8, return_dist=True)
    assert (d[0, :, case.k - 1] == d[0, :, case.k]).any()


def test_knn_cases_reach_every_promised_variant(lib):
    query = _knn_query(lib)
    limits = R.knn_wide_limit_cases(query, 10) + R.knn_wide_limit_cases(query, 20)
    assert [c.variant for c in limits] == ["c3 wide", "c3 scan CS4"] * 2
    assert limits[0].n > limits[2].n > 2048          # (the longer lists leave less LDS for the cloud)
    reached = {c.variant for c in R.KNN_CASES + limits}
    assert {"c3 wide", "c3 scan CS1", "c3 scan CS2", "c3 scan CS4", "generic"} <= reached
    generic = [c for c in R.KNN_CASES if c.variant == "generic"]
    assert any(c.c == 64 and c.ld % 4 for c in generic) and any(c.c == 64 and c.misaligned for c in generic)
    assert any(c.c == 3 and c.n > 6144 for c in generic)
    # the same arguments, aligned and with a whole stride, are NOT generic: stride and alignment alone decide
    assert R.knn_variant_name(query(2, 300, 64, 64, 10, 1))[0] == "c64 wide"
    # b a multiple of 8 (the remapped workgroup order) with each of the scan kernel's merges
    for cs in ("c3 scan CS1", "c3 scan CS2"):
        assert any(c.variant == cs and c.b % 8 == 0 for c in R.KNN_CASES), cs
    assert query(0, 10, 3, 3, 5, 1) == -1 and query(1, 10, 3, 3, 11, 1) == -1 and query(1, 10, 3, 2, 5, 1) == -1


@pytest.mark.parametrize("case", R.NN_CASES, ids=R.nn_id)
def test_chamfer_cases_reach_their_variants_and_have_ties(lib, host_knobs, case):
    if case.filter is not None:
        host_knobs("CLOUDAAE_NN_FILTER", case.filter)
    assert R.nn_variant_name(int(lib.lib().cloudaae_nn_distance_variant(case.b, case.n, case.m))) == case.variant
    a, t, src = R.nn_clouds(case)
    clouds = range(min(4, case.b))                  # (a few clouds are enough)
    assert sum(R.nn_tied_queries(a[i], t[i]) for i in clouds) >= 1 and sum(R.nn_tied_queries(t[i], a[i]) for i in clouds) >= 1
    if case.prefix:
        counts = R.nn_prefix_counts(case)
        assert any(0 < k < case.m for k in counts) and case.m in counts and 0 in counts and any(k > case.m for k in counts)
        for i, k in enumerate(counts):
            k = k if 0 < k <= case.m else case.m
            assert (src[i, :k] == np.arange(k)).all() and (src[i, k:] < k).all()
            assert np.array_equal(t[i, k:], t[i, src[i, k:]])


def test_chamfer_cases_reach_every_plain_variant(lib, host_knobs):
    own = {c.variant for c in R.NN_CASES if c.filter is None}
    assert own == {"Q2", "Q4"}, "Q = 2 and Q = 4 by the launcher's own choice"
    assert {c.variant for c in R.NN_CASES} == {"Q1", "Q2", "Q4"}
    assert any(c.prefix and c.variant == "Q2" for c in R.NN_CASES)
    q = lambda *s: R.nn_variant_name(int(lib.lib().cloudaae_nn_distance_variant(*s)))
    assert q(32, 4096, 4096) == "filter" and q(1, 5, 6) == "Q1"
    assert int(lib.lib().cloudaae_nn_distance_variant(0, 5, 6)) == -1
    host_knobs("CLOUDAAE_NN_FILTER", 0)
    assert q(32, 4096, 4096) == "Q2"
    host_knobs("CLOUDAAE_NN_FILTER", 1)
    assert q(1, 5, 6) == "filter"


def test_gather_point_grad_refuses_what_its_kernel_would_misread(lib, monkeypatch):
    """tf_sampling.gather_point_grad, the bare op: an int64 index tensor would be read as pairs of int32, a float64
    gradient as pairs of float32.  Refused like _GatherPoint.forward refuses them -- before the library is asked for
    anything (so nothing is launched and nothing allocated)."""
    from cloudaae_amd.tf_ops.sampling import tf_sampling
    calls = []
    monkeypatch.setattr(tf_sampling._lib, "lib", lambda: calls.append("lib") or pytest.fail("the library was reached"))
    monkeypatch.setattr(tf_sampling._lib, "empty", lambda *a, **k: calls.append("empty") or pytest.fail("an output was allocated"))
    inp, out_g = torch.zeros((2, 9, 3)), torch.zeros((2, 4, 3))
    idx = torch.zeros((2, 4), dtype=torch.int32)
    for bad in ((inp, idx.long(), out_g), (inp, idx.short(), out_g), (inp.double(), idx, out_g), (inp, idx, out_g.double()),
                (inp, idx, out_g.half())):
        with pytest.raises(ValueError, match="GatherPointGrad"):
            tf_sampling.gather_point_grad(*bad)
    assert calls == []
