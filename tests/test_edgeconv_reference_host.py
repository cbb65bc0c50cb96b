"""CPU: tests/edgeconv_reference.py is anchored before any kernel is judged by it (tests/test_22_edge_conv_paths_gpu.py).

  * at float64 the three stages, chained, agree with torch.autograd on a float64 evaluation of the edge-tensor
    definition (index_select, cat, matmul, batch norm, relu, mean / amax over k) to 1e-12: output, shadows, every gradient;
  * every case of the table is conditioned with its stored seed (no edge whose ReLU mask or maximum fp32 cannot decide),
    found within 16 redraws, and on the lattice y from the edge tensor equals fl32(U + Q) exactly;
  * every case takes the launcher branch it is there for (edgeconv_reference.launcher_paths: the launcher's predicates
    evaluated for the case), and every kernel instantiation appears;
  * the constants of the GPU file's bounds are four times what the float32 restatement reaches against float64 over the
    case table, rounded up to a power of two;
  * every mutant of the reference exceeds an allowed bound on a named case."""
import functools

import numpy as np
import pytest
import torch

import edgeconv_reference as R

F32, F64 = np.float32, np.float64


def _torch_edgeconv(x, idx, W, b, gamma, beta, training, sm, sv, decay, pool, B, N, k):
    nb = torch.from_numpy(R.neighbours(idx, B, N, k).ravel())
    centre = x.repeat_interleave(k, 0)
    e = torch.cat([centre, x.index_select(0, nb) - centre], 1)
    y = e @ W + b
    if training:
        mean = y.mean(0)
        var = ((y - mean.detach()) ** 2).mean(0)
        om = float(F32(1.0) - F32(decay))
        with torch.no_grad():
            sm -= (sm - mean.detach()) * om
            sv -= (sv - var.detach()) * om
    else:
        mean, var = sm, sv
    inv = gamma * torch.rsqrt(var + 1e-3)
    z = torch.relu(y * inv + (beta - mean * inv)).view(B * N, k, -1)
    return z.mean(1) if pool == 1 else z.amax(1)


@pytest.mark.parametrize("pool,training,ties", [(1, 1, 0), (2, 1, 1), (1, 0, 0), (2, 0, 1)])
def test_float64_reference_equals_torch_autograd(pool, training, ties):
    B, N, k, cin, C = 2, 9, 4, 3, 5
    rng = np.random.default_rng(10 * pool + training)
    P = B * N
    x = rng.standard_normal((P, cin)).astype(F32)
    W = rng.standard_normal((2 * cin, C)).astype(F32)
    b = rng.standard_normal(C).astype(F32)
    idx = rng.integers(0, N, (B, N, k)).astype(np.int32)
    if ties:
        idx[0, 2, :] = (1, 1, 7, 1)       # the same neighbour three times: three equal edges
        idx[1, 3, :] = 3                  # four self edges
    gamma = np.abs(1 + 0.2 * rng.standard_normal(C)).astype(F32)
    beta = (0.3 * rng.standard_normal(C)).astype(F32)
    sm, sv = (0.5 * rng.standard_normal(C)).astype(F32), (2 + np.abs(rng.standard_normal(C))).astype(F32)
    dout = rng.standard_normal((P, C)).astype(F32)
    dx0 = rng.standard_normal((P, cin)).astype(F32)

    a = R.stage_a(x, W, b)
    y_def = R.edge_preactivation(x, idx, W, b, B, N, k)
    nb = R.neighbours(idx, B, N, k)
    np.testing.assert_allclose((a.pq[:, None, :C] + a.pq[:, C:][nb]).reshape(-1, C), y_def, rtol=0, atol=1e-13)
    # the chain A -> B -> C at float64 (stage B takes fp32 rows: feed it the float64 ones through a lossless detour)
    import bn_reference as BN
    bw = BN.backward(y_def, gamma, beta, training, sm, sv, 1, None, k, pool, dout)
    ref = R.stage_b(a.pq.astype(F32), idx, B, N, k, gamma, beta, training, sm, sv, 0.9, pool, dout)
    # stage_b on the rounded pq against its own definition on the same rows
    y32 = R.edge_rows(a.pq.astype(F32), idx, B, N, k)
    bw32 = BN.backward(y32, gamma, beta, training, sm, sv, 1, None, k, pool, dout)
    T = np.zeros((P, C))
    np.add.at(T, nb.ravel(), bw32.dy)
    np.testing.assert_allclose(ref.dpq[:, :C], bw32.dy.reshape(P, k, C).sum(1), rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref.dpq[:, C:], T - ref.dpq[:, :C], rtol=0, atol=1e-13)
    # ... and the float64 chain against autograd
    S = bw.dy.reshape(P, k, C).sum(1)
    T = np.zeros((P, C))
    np.add.at(T, nb.ravel(), bw.dy)
    dpq = np.concatenate([S, T - S], 1)
    cc = _stage_c64(dpq, x, W, dx0)

    t = lambda v, g=False: torch.tensor(np.asarray(v, F64), requires_grad=g)
    tx, tW, tb, tg, tbe = t(x, True), t(W, True), t(b, True), t(gamma, True), t(beta, True)
    tsm, tsv = t(sm), t(sv)
    out = _torch_edgeconv(tx, idx, tW, tb, tg, tbe, training, tsm, tsv, 0.9, pool, B, N, k)
    (out * t(dout)).sum().backward()
    close = lambda p, q: np.testing.assert_allclose(np.asarray(p, F64), q.detach().numpy(), rtol=1e-12, atol=1e-12)
    close(bw.fw.pooled, out)
    fwd = BN.forward(y_def, gamma, beta, training, sm, sv, 0.9, 1, k, pool)
    close(fwd.ema_mean, tsm)
    close(fwd.ema_var, tsv)
    close(cc[0] - dx0.astype(F64), tx.grad)
    close(cc[1], tW.grad)
    close(bw.dbias, tb.grad)
    close(bw.dgamma, tg.grad)
    close(bw.dbeta, tbe.grad)
    if ties and pool == 2:
        assert (bw.fw.ties[2] >= 1).all() and (bw.fw.ties[N + 3] == k).all() and bw.fw.ties[2].max() >= 3


def _stage_c64(dpq, x, W, dx0):
    """stage C on a float64 dpq (R.stage_c rounds its dpq to fp32, as the kernel's is)"""
    cin, C = x.shape[1], W.shape[1]
    Wf = np.concatenate([W[:cin], W[cin:]], 1).astype(F64)
    dwf = x.astype(F64).T @ dpq
    got = R.stage_c(dpq.astype(F32), x, W, 0, dx0)
    np.testing.assert_allclose(got.dx, dpq @ Wf.T + dx0, rtol=1e-6, atol=1e-6)
    return dpq @ Wf.T + dx0, np.concatenate([dwf[:, :C], dwf[:, C:]], 0)


def test_bf16_rounding_is_to_nearest_even():
    a = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e-5, 65280.0], F32)
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.rne_bf16(a), want)
    r = np.random.default_rng(0).standard_normal(4096).astype(F32)
    assert np.array_equal(R.rne_bf16(r), torch.from_numpy(r).to(torch.bfloat16).to(torch.float32).numpy())
    assert np.array_equal(R.bf16_bits(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


DATA_CASES = sorted(R._DATA.values(), key=lambda c: c.data)


@pytest.mark.parametrize("data", [c.data for c in DATA_CASES])
def test_every_case_is_conditioned_with_its_stored_seed(data):
    c = R._DATA[data]
    assert c.base_seed <= c.seed <= c.base_seed + R.MAX_REDRAWS
    x = R.make_inputs(c)
    assert x.seed == c.seed and x.ambiguous == 0
    if c.family == "lattice":
        y_def = R.edge_preactivation(x.x, x.idx, x.W, x.b, c.B, c.N, c.k)
        assert np.array_equal(R.edge_rows(x.pq, x.idx, c.B, c.N, c.k).astype(F64), y_def)       # exact, whatever the order
        assert np.abs(y_def).max() < 512 and np.array_equal(y_def * 128, np.round(y_def * 128))
        for bf in (x.x, x.W):
            assert np.array_equal(R.rne_bf16(bf), bf)
        if c.B * c.N * c.k >= 1000:       # the ReLU has not been conditioned away
            assert 0.2 < R.reference(c).passing < 0.8


def test_constructed_lists_hold_what_they_claim():
    for c in DATA_CASES:
        if c.hub is None or c.N < 140:
            continue
        idx = R.make_inputs(c).idx
        for b in range(c.B):
            deg = np.bincount(idx[b].ravel(), minlength=c.N)
            if c.k > 1:
                assert deg[R.P64] == 64 and deg[R.P65] == 65 and deg[R.P21] == 21 and deg[R.P21] % 8 != 0, c.data
                assert deg[R.HUB] >= (c.N if c.hub == "all" else c.hub), c.data
                assert (idx[b, :, 0] == R.HUB).all() or c.hub != "all"
            else:
                assert deg[R.P64] == 64 and deg[R.P65] == 65, c.data
            assert deg[R.NOBODY] == 0 and (idx[b, R.SELF] == R.SELF).any() and (idx[b, R.SAME] == R.HUB).all(), c.data
            assert deg.max() <= 2000


@pytest.mark.parametrize("name", [c.name for c in R.ALL_CASES])
def test_case_takes_the_branch_it_is_there_for(name):
    c = R.ALL_BY_NAME[name]
    p = R.launcher_paths(c)
    for key, want in c.why.items():
        assert p[key] == want, (name, key, p[key], want)


def test_every_instantiation_appears():
    seen = set()
    for c in R.CASES:
        seen |= R.instantiations_of(c)
    missing = R.required_instantiations() - seen
    assert not missing, sorted(missing)
    products = {R.launcher_paths(c)["product"] for c in R.CASES}
    assert {"stream128", "stream256", "general", "bf16"} <= products
    for key in ("stat_grid_capped", "apply_grid_capped", "lds_over_48k", "xcd_wraps", "fewer_points_than_waves"):
        assert any(R.launcher_paths(c)[key] for c in R.CASES), key
    # hubs past two chunks of sources reach both apply kernels, in both pools
    hubs = {R.launcher_paths(c)["bwd_apply"][0:1] + (c.pool,) for c in R.CASES if c.hub == "all" and c.N > 128 and c.k > 1}
    assert {("ec_bwd_apply_mean4", 1), ("ec_bwd_apply", 1), ("ec_bwd_apply", 2)} <= hubs


# ---- constants ----------------------------------------------------------------------------------------------------------
def _outputs(r):
    return {"save_mean": r.save_mean, "save_var": r.save_var, "out": r.out, "ties": r.ties, "edge_stats": r.edge_stats,
            "dgamma": r.dgamma, "dbeta": r.dbeta, "dbias": r.dbias, "dpq": r.dpq}


@functools.lru_cache(maxsize=None)
def _measured(data):
    """normalised errors of the float32 restatement against float64 on one data set: stage B (lattice), A and C (all)"""
    c = R._DATA[data]
    x = R.make_inputs(c)
    e = {}
    if c.family == "lattice":
        ref = R.reference(c)
        e.update(R.stage_b_errors(_outputs(R.reference(c, F32)), ref))
        dpq = ref.dpq.astype(F32)
    else:
        dpq = np.random.default_rng(c.seed).standard_normal((c.B * c.N, 2 * c.cout)).astype(F32)
    for bf16 in (0, 1):
        a64, a32 = R.stage_a(x.x, x.W, x.b, bf16), R.stage_a(x.x, x.W, x.b, bf16, F32)
        e["pq"] = max(e.get("pq", 0.0), R.product_errors(a32.pq, a64.pq, a64.t, "pq")["pq"])
        start = x.dout[:, :1] * np.ones((1, c.cin), F32)
        c64, c32 = R.stage_c(dpq, x.x, x.W, bf16, start), R.stage_c(dpq, x.x, x.W, bf16, start, F32)
        e["dx"] = max(e.get("dx", 0.0), R.product_errors(c32.dx, c64.dx, c64.tdx, "dx")["dx"])
        e["dw"] = max(e.get("dw", 0.0), R.product_errors(c32.dw, c64.dw, c64.tdw, "dw")["dw"])
    return e


def test_constants_are_four_times_the_restatement():
    worst, where = {k: 0.0 for k in R.ALLOWED}, {}
    for c in DATA_CASES:
        for k, v in _measured(c.data).items():
            if k in R.CONSTANT_OF:
                assert np.isfinite(v), (c.data, k)
                if v > worst[R.CONSTANT_OF[k]]:
                    worst[R.CONSTANT_OF[k]], where[R.CONSTANT_OF[k]] = v, c.data
            elif k in R.FIXED:
                assert v <= 0.5 if k.startswith("save") else v == 0.0, (c.data, k, v)
    for k in sorted(worst):
        print("EDGECONV constant %-9s measured %8.3f allowed %6g  (%s)" % (k, worst[k], R.ALLOWED[k], where.get(k)))
    for k, v in worst.items():
        assert R.ALLOWED[k] >= 4.0 * v and R.ALLOWED[k] < 16.0 * v, (k, v, R.ALLOWED[k])
        assert R.ALLOWED[k] == R.pow2_ceil(4.0 * v), (k, v)


# ---- mutants --------------------------------------------------------------------------------------------------------------
# every mutant must exceed an allowed bound on the case named here
KILLED_BY = {"first_64_sources_only": "arg_base", "tail_source_dropped": "arg_base", "k_plus_one": "arg_base",
             "unshared_ties": "inst_o64_k10_max", "m2_zero": "arg_base", "centre_not_subtracted": "arg_base",
             "odd_last_point_counted_twice": "odd_tail_N33", "drop_last_edge": "three_points"}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_catch_the_mutant(mutant):
    c = R.CASE_BY_NAME[KILLED_BY[mutant]]
    x = R.make_inputs(c)
    ref = R.reference(c)
    if mutant == "centre_not_subtracted":
        got = R.stage_a(x.x, x.W, x.b, 0, F64, mutant).pq
        assert not np.array_equal(got, x.pq64)                                  # lattice: stage A is bit for bit
        g = R.make_inputs(R.CASE_BY_NAME["gauss_general"])
        gx = R.stage_a(g.x, g.W, g.b)
        over = R.product_errors(R.stage_a(g.x, g.W, g.b, 0, F64, mutant).pq, gx.pq, gx.t, "pq")["pq"] / R.allowed_of("pq")
        assert over > 100, over
        return
    e = R.stage_b_errors(_outputs(R.reference(c, F64, mutant)), ref)
    over = {k: v / max(R.allowed_of(k), 0.5) for k, v in e.items()}
    print("EDGECONV mutant %s on %s: %s" % (mutant, c.name, {k: round(v, 2) for k, v in over.items() if v > 1}))
    assert max(over.values()) > 1.0, (mutant, c.name, e)
    if mutant in ("first_64_sources_only", "tail_source_dropped"):
        # only the reverse-list sums move, and only at the points the mutant touches: hubs, the 65-entry list / every list
        assert over["dT"] > 100 and all(v <= 1.0 for k, v in over.items() if k != "dT"), over
        d = np.abs(R.reference(c, F64, mutant).dpq - ref.dpq)[:, c.cout:].max(1).reshape(c.B, c.N)
        if mutant == "first_64_sources_only":
            assert (d[:, R.HUB] > 0).all() and (d[:, R.P65] > 0).all() and (d[:, R.P64] == 0).all() and (d[:, R.P21] == 0).all()
        else:
            assert (d[:, R.P64] > 0).all() and (d[:, R.NOBODY] == 0).all()


def test_hub_mutants_survive_without_the_hub_cases():
    """first_64_sources_only is invisible on lists of random clouds' size: it is the planted lists that catch it"""
    c = R.CASE_BY_NAME["odd_tail_N33"]
    assert R.reference(c).deg.max() <= 64
    e = R.stage_b_errors(_outputs(R.reference(c, F64, "first_64_sources_only")), R.reference(c))
    assert max(e.values()) <= 0.5


def test_unmutated_reference_has_no_error():
    c = R.CASE_BY_NAME["inst_o64_k10_max"]
    ref = R.reference(c)
    e = R.stage_b_errors(_outputs(ref), ref)
    assert e.pop("save_mean") <= 0.5 and e.pop("save_var") <= 0.5
    assert max(e.values()) == 0.0
