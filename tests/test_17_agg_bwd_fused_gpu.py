"""GPU: cloudaae_bn_backward_dx_bf16x3 -- the batch-norm backward of the mean-pooled dgcnn_agg layer with its apply pass
formed inside the input-gradient product -- against the two calls it replaces (cloudaae_bn_backward, then
cloudaae_gemm_bf16x3p on the dy that one wrote): dy, dX and the parameter gradients must be the same BITS, because the
fused kernel applies the same fp32 operations in the same order (bn_common.h: bn_bwd_dy_hoisted, shared by both)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C, NOUT = 1024, 320       # the layer: [M x 320] x [320 x 1024], 1024 channels normalised and mean-pooled per cloud
GUARD = 64                # floats in front of and behind dy / dX
SENTINEL = -12345.5


def _guarded(rows, cols, dev):
    buf = torch.full((rows * cols + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + rows * cols].view(rows, cols)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _layer(hip, M, rows, relu, with_forward, seed):
    """inputs of the backward pass: y and the saved statistics (from the library's own forward pass when with_forward -- then
    the backward takes the per-group counts of the forward, as the train step does --, else free-standing tensors with channels
    whose normalised value is EXACTLY zero for many rows: the edge of the ReLU mask)"""
    L = hip.lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    y = (rnd(M, C) * 1.5 + rnd(1, C)).to(dev)
    gamma = (1.0 + 0.2 * rnd(C)).to(dev)
    beta = (0.3 * rnd(C)).to(dev)
    groups = M // rows
    pstats = None
    ws = torch.zeros(int(L.cloudaae_bn_workspace_bytes(C)) // 8, dtype=torch.float64, device=dev)
    if with_forward:
        save_mean, save_var = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ema_m, ema_v = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        decay = torch.full((1,), 0.9, device=dev)
        pooled = torch.empty(groups, C, device=dev)
        if relu:
            pstats = torch.empty(groups * 3 * C, dtype=torch.float64, device=dev)
        hip.check(L.cloudaae_bn_forward(M, C, y.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), 1, decay.data_ptr(),
                                        ema_m.data_ptr(), ema_v.data_ptr(), save_mean.data_ptr(), save_var.data_ptr(), int(relu),
                                        None, C, rows, 1, pooled.data_ptr(), None, hip.ptr(pstats), ws.data_ptr(), hip.stream()),
                  "cloudaae_bn_forward")
    else:
        save_mean = (0.5 * rnd(C)).to(dev)
        save_var = (0.5 + rnd(C).abs()).to(dev)
        # channels 0, 8, 16, ...: beta = 0 and mean = 0, so z = y * sc + 0 and every y == 0 sits exactly on the edge (z == +-0);
        # a third of their rows get y = +0 or -0, and a tenth of ALL elements elsewhere are exact zeros too
        beta[::8] = 0.0
        save_mean[::8] = 0.0
        edge = torch.rand(M, C // 8, generator=g).to(dev)
        ych = y[:, ::8]
        ych[edge < 0.33] = 0.0
        ych[edge < 0.16] = -0.0
        y[:, ::8] = ych
        y[torch.rand(M, C, generator=g).to(dev) < 0.1] = 0.0
    dpooled = rnd(groups, C).to(dev)
    W = (0.05 * rnd(NOUT, C)).to(dev)
    nbytes = int(L.cloudaae_x3_planes_bytes(C, NOUT))
    planes_fwd = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=dev)
    planes_bwd = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=dev)
    hip.check(L.cloudaae_x3_split_weight(NOUT, C, W.data_ptr(), C, planes_fwd.data_ptr(), planes_bwd.data_ptr(), hip.stream()),
              "cloudaae_x3_split_weight")
    return dict(y=y, gamma=gamma, beta=beta, save_mean=save_mean, save_var=save_var, dpooled=dpooled, planes=planes_bwd,
                pstats=pstats, ws=ws)


@pytest.mark.parametrize("with_forward", [False, True], ids=["edge_zeros", "after_forward"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("M,rows", [(128, 128), (1024, 1024), (1024, 256), (32768, 1024)])
def test_fused_equals_the_two_calls(hip, M, rows, relu, with_forward):
    L = hip.lib()
    dev = torch.device("cuda")
    assert L.cloudaae_bn_backward_dx_bf16x3_supported(M, C, NOUT, rows) == 1
    a = _layer(hip, M, rows, relu, with_forward, seed=M + rows + 2 * relu + with_forward)
    y = a["y"]
    out = {}
    for fused in (False, True):
        dybuf, dy = _guarded(M, C, dev)
        dxbuf, dx = _guarded(M, NOUT, dev)
        dgamma, dbeta, dbias = (torch.full((C,), SENTINEL, device=dev) for _ in range(3))
        a["ws"].zero_()
        common = (M, C, y.data_ptr(), C, a["gamma"].data_ptr(), a["beta"].data_ptr(), a["save_mean"].data_ptr(),
                  a["save_var"].data_ptr(), 1, relu)
        grads = (dy.data_ptr(), C, dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(), 0, hip.ptr(a["pstats"]),
                 a["ws"].data_ptr())
        if fused:
            consts = torch.empty(int(L.cloudaae_bn_backward_dx_bf16x3_consts_bytes(M, C, rows)) // 4, device=dev)
            hip.check(L.cloudaae_bn_backward_dx_bf16x3(*common, rows, a["dpooled"].data_ptr(), *grads, consts.data_ptr(), NOUT,
                                                       a["planes"].data_ptr(), dx.data_ptr(), NOUT, hip.stream()),
                      "cloudaae_bn_backward_dx_bf16x3")
        else:
            hip.check(L.cloudaae_bn_backward(*common, None, C, rows, 1, a["dpooled"].data_ptr(), None, None, *grads,
                                             hip.stream()), "cloudaae_bn_backward")
            hip.check(L.cloudaae_gemm_bf16x3p(M, NOUT, C, dy.data_ptr(), C, a["planes"].data_ptr(), dx.data_ptr(), NOUT, None, 0,
                                              None, hip.stream()), "cloudaae_gemm_bf16x3p")
        torch.cuda.synchronize()
        assert _guards_intact(dybuf) and _guards_intact(dxbuf), fused
        out[fused] = (dy.clone(), dx.clone(), dgamma, dbeta, dbias)
    for name, r, f in zip(("dy", "dx", "dgamma", "dbeta", "dbias"), out[False], out[True]):
        assert bool(torch.isfinite(r).all()), name
        assert torch.equal(r, f), (name, int((r != f).sum()), float((r - f).abs().max()))
    if not with_forward:       # the edge was really there: y == 0 in channels whose shift is zero
        edge = (y[:, ::8] == 0.0).float().mean()
        assert 0.3 < float(edge) < 0.6


@pytest.mark.parametrize("M,nout,rows", [(1024, 256, 256),      # 128-column tiles
                                         (1024, 320, 64),       # a row tile would straddle clouds
                                         (1024, 320, 192),      # ... also when the group is larger than the tile
                                         (320, 320, 160),       # rows not in whole 128-row tiles
                                         (1024, 320, 0)])
def test_unsupported_shapes_are_refused(hip, M, nout, rows):
    L = hip.lib()
    dev = torch.device("cuda")
    assert L.cloudaae_bn_backward_dx_bf16x3_supported(M, C, nout, rows) == 0
    t = torch.zeros(max(M, 1) * C, device=dev)
    v = torch.ones(C, device=dev)
    ws = torch.zeros(int(L.cloudaae_bn_workspace_bytes(C)) // 8, dtype=torch.float64, device=dev)
    planes = torch.zeros(C * nout * 3, dtype=torch.bfloat16, device=dev)
    rc = L.cloudaae_bn_backward_dx_bf16x3(M, C, t.data_ptr(), C, v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), 1, 1, rows,
                                          t.data_ptr(), t.data_ptr(), C, v.data_ptr(), v.data_ptr(), None, 0, None, ws.data_ptr(),
                                          t.data_ptr(), nout, planes.data_ptr(), t.data_ptr(), nout, hip.stream())
    assert rc != 0 and b"not served" in L.cloudaae_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0          # nothing was launched


def _state(g):
    return [t.clone() for t in (g.store.flat_params, g.adam_m, g.adam_v, g.store.flat_state)]


def _count_fused_calls(hip, monkeypatch):
    lib = hip.lib()
    entry = lib.cloudaae_bn_backward_dx_bf16x3
    calls = []

    def counting(*args):
        calls.append(1)
        return entry(*args)
    monkeypatch.setattr(lib, "cloudaae_bn_backward_dx_bf16x3", counting)
    return calls


def test_deterministic_graph_ends_identical_with_and_without(hip, monkeypatch):
    """TrainGraph(deterministic=True) stepped three times with the fused path allowed and with it switched off: identical
    weights, Adam slots and moving averages.  (Deterministic mode keeps dgcnn_agg on the fp32 products, so what this pins is
    that the switch and the link between the two autograd functions leave that mode alone.)"""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import _functions as F
    B, N = 4, 256
    mk = lambda: T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=False, deterministic=True)
    a, b = mk(), mk()
    assert torch.equal(a.store.flat_params, b.store.flat_params)
    els = [T.synthetic_element(B, N, a.device, seed=170 + i) for i in range(3)]
    for el in els:
        el["noise"] = torch.randn((B, N, 3), device="cuda") * 0.001
    try:
        for el in els:
            monkeypatch.setattr(F, "AGG_BWD_FUSED", True)
            a.train_step(el)
            monkeypatch.setattr(F, "AGG_BWD_FUSED", False)
            b.train_step(el)
            torch.cuda.synchronize()
            for x, y in zip(_state(a), _state(b)):
                assert torch.equal(x, y)
    finally:
        T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=False)._set_mode()


@pytest.mark.parametrize("replay", [False, True])
def test_split_product_step_takes_the_fused_path_and_keeps_its_gradients(hip, monkeypatch, replay):
    """The ordinary (bf16x3) step: with the switch on the layer goes through the new entry, with it off through the two calls;
    from the same state both give the same losses, and gradients that agree as two runs of ONE configuration do (the
    weight-gradient products and the fully connected stack add with fp32 atomics: tests/test_10_replay_gpu.py)."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import _functions as F
    B, N = 4, 256
    calls = _count_fused_calls(hip, monkeypatch)
    mk = lambda: T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=replay)
    monkeypatch.setattr(F, "AGG_BWD_FUSED", True)
    on = mk()
    monkeypatch.setattr(F, "AGG_BWD_FUSED", False)
    off = mk()
    assert torch.equal(on.store.flat_params, off.store.flat_params)
    el = T.synthetic_element(B, N, on.device, seed=180)
    el["noise"] = torch.randn((B, N, 3), device="cuda") * 0.001
    calls.clear()
    o_off = off.train_step(el)
    assert not calls
    monkeypatch.setattr(F, "AGG_BWD_FUSED", True)
    o_on = on.train_step(el)
    torch.cuda.synchronize()
    assert len(calls) == 1
    for k in ("xyz_loss", "trans_loss", "axag_loss", "total_loss"):
        assert float(o_on[k]) == float(o_off[k]), k
    g1, g2 = on.store.flat_grads, off.store.flat_grads
    assert bool(torch.isfinite(g1).all())
    assert float((g1 - g2).abs().max()) <= 5e-3 * float(g1.abs().max())
