"""GPU: every size-dispatched kernel variant of farthest point sampling, kNN and the Chamfer search against the oracle.

The launchers of these three ops pick a kernel instantiation from b, n, m, the row stride and the pointer's alignment.
Every case here first ASKS the library which variant its call takes (cloudaae_farthest_point_sample_variant,
cloudaae_knn_variant, cloudaae_nn_distance_variant: the decision functions the launchers themselves call) and asserts that
it is the one the case is named after, prints it, then runs the op.  Every comparison is equality of integers or of float
bits with oracle.*; there is no tolerance.  The cases, their inputs and the reasons why those inputs would expose a wrong
tie-break or a wrong tail are in tests/sampling_reference.py and tests/test_point_op_variants_host.py.

Reached (the -s output names them): farthest point sampling with 1, 2, 4, 8, 16, 32 points per thread, 32 with the
winner's coordinates from memory, and the big kernel (also with more clouds than workgroups); kNN c3 wide (up to the largest
cloud it takes), c3 scan with 1, 2, 4 candidate ranges, c64 generic by stride and by alignment, c3 generic by size; the
Chamfer search with 1, 2, 4 queries per lane (2 and 4 also by the launcher's own choice, 2 also through the prefix entry).
"""
import numpy as np
import pytest
import torch

import sampling_reference as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- farthest point sampling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FPS_CASES, ids=R.fps_id)
def test_fps_variant_vs_oracle(hip, oracle, case):
    from cloudaae_amd.tf_ops.sampling import tf_sampling
    variant = R.fps_variant_name(int(hip.lib().cloudaae_farthest_point_sample_variant(case.n)))
    assert variant == case.variant
    print("farthest point sampling (b, n, m) = (%d, %d, %d): %s" % (case.b, case.n, case.m, variant))
    p = R.fps_cloud(case)
    want = oracle.farthest_point_sample(case.m, p, threads=8)
    got = tf_sampling.farthest_point_sample(case.m, _dev(p)).cpu().numpy()
    assert np.array_equal(want, got)


# ---- kNN -----------------------------------------------------------------------------------------------------------------
def _run_knn(hip, oracle, knobs, case):
    if case.wide is not None:
        knobs("CLOUDAAE_KNN3_WIDE", case.wide)
    x = R.knn_cloud(case)
    if case.misaligned:             # the same rows one float past a 16-byte boundary
        buf = torch.empty(x.size + 4, device="cuda")
        assert buf.data_ptr() % 16 == 0
        xd = buf[1:1 + x.size].view(x.shape)
        xd.copy_(torch.from_numpy(x))
    else:
        xd = _dev(x)
    aligned = int(xd.data_ptr() % 16 == 0)
    assert aligned == (0 if case.misaligned else 1)
    name, K = R.knn_variant_name(int(hip.lib().cloudaae_knn_variant(case.b, case.n, case.c, case.ld, case.k, aligned)))
    assert name == case.variant
    print("kNN (b, n, c, ld, k) = (%d, %d, %d, %d, %d)%s%s: %s, lists of %d" % (
        case.b, case.n, case.c, case.ld, case.k, "" if case.wide is None else ", CLOUDAAE_KNN3_WIDE=%d" % case.wide,
        ", x misaligned" if case.misaligned else "", name, K))
    want = oracle.knn(x, case.k, channels=case.c, threads=8)
    got = torch.full((case.b, case.n, case.k), -1, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().cloudaae_knn(case.b, case.n, case.c, case.ld, case.k, xd.data_ptr(), hip.ptr(got), hip.stream()), "knn")
    assert np.array_equal(want, got.cpu().numpy())


@pytest.mark.parametrize("case", R.KNN_CASES, ids=R.knn_id)
def test_knn_variant_vs_oracle(hip, oracle, knobs, case):
    _run_knn(hip, oracle, knobs, case)


@pytest.mark.parametrize("k", [10, 20])
def test_knn_c3_wide_at_its_largest_cloud_and_the_next(hip, oracle, knobs, k):
    """the largest n the query still calls c3 wide (found by bisection on the query alone) and n + 1 (the scan kernel)"""
    last, after = R.knn_wide_limit_cases(lambda *a: int(hip.lib().cloudaae_knn_variant(*a)), k)
    assert after.n == last.n + 1 and after.variant == "c3 scan CS4"
    _run_knn(hip, oracle, knobs, last)
    _run_knn(hip, oracle, knobs, after)


# ---- the Chamfer search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.NN_CASES, ids=R.nn_id)
def test_chamfer_search_variant_vs_oracle(hip, oracle, knobs, case):
    from cloudaae_amd.tf_ops.nn_distance import tf_nndistance
    if case.filter is not None:
        knobs("CLOUDAAE_NN_FILTER", case.filter)
    variant = R.nn_variant_name(int(hip.lib().cloudaae_nn_distance_variant(case.b, case.n, case.m)))
    assert variant == case.variant
    print("Chamfer search (b, n, m) = (%d, %d, %d)%s%s: %s" % (
        case.b, case.n, case.m, "" if case.filter is None else ", CLOUDAAE_NN_FILTER=%d" % case.filter,
        ", prefix entry" if case.prefix else "", variant))
    a, t, src = R.nn_clouds(case)
    want = oracle.nn_distance(a, t, threads=8)
    distinct2 = None
    if case.prefix:
        distinct2 = (torch.tensor(R.nn_prefix_counts(case), dtype=torch.int64, device="cuda"), _dev(src))
    got = tf_nndistance.nn_distance(_dev(a), _dev(t), distinct2=distinct2)
    for w, g in zip(want, got):             # dist1, idx1, dist2, idx2: float bits and integers
        assert w.dtype == g.cpu().numpy().dtype and np.array_equal(w, g.cpu().numpy())


# ---- GatherPointGrad, the bare op ----------------------------------------------------------------------------------------
def test_gather_point_grad_refuses_other_dtypes(hip, monkeypatch):
    """an int64 index tensor would be read as pairs of int32: refused before the library is called (nothing launched)"""
    from cloudaae_amd.tf_ops.sampling import tf_sampling
    inp, out_g = torch.zeros((2, 9, 3), device="cuda"), torch.ones((2, 4, 3), device="cuda")
    idx = torch.tensor([[0, 3, 5, 8], [1, 2, 4, 7]], dtype=torch.int32, device="cuda")
    good = tf_sampling.gather_point_grad(inp, idx, out_g)
    assert float(good.sum()) == 24.0
    calls = []
    entry = hip.lib().cloudaae_gather_point_grad
    monkeypatch.setattr(hip.lib(), "cloudaae_gather_point_grad", lambda *a: calls.append(a) or entry(*a))
    for bad in ((inp, idx.long(), out_g), (inp.double(), idx, out_g), (inp, idx, out_g.double())):
        with pytest.raises(ValueError, match="GatherPointGrad"):
            tf_sampling.gather_point_grad(*bad)
    assert calls == []
    assert torch.equal(tf_sampling.gather_point_grad(inp, idx, out_g), good) and len(calls) == 1
