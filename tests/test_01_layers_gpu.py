"""GPU: dense layers, batch norm, fused edge-conv, losses and optimiser through the C-ABI,
against the CPU oracle (oracle/model_oracle.py) on the same seeded inputs.
Tolerances: these are fp32 computations whose summation ORDER differs from the oracle's
(MFMA k-order vs BLAS, fp64 two-level column sums vs torch), so they are compared to
fp32 round-off, not bitwise; index-producing ops are bit-exact (test_00_ops_gpu.py)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _rel(got, want):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    return np.abs(got - want).max() / (np.abs(want).max() + 1e-30)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (32, 1024, 1024), (2, 3, 256), (200, 130, 70), (4096, 64, 24),
                                   (4096, 128, 64), (320, 1024, 8192), (64, 64, 20000), (129, 257, 33),
                                   (2, 12288, 1024), (128, 1024, 1024), (100, 300, 500), (128, 12288, 1024)])
def test_gemm(hip, ta, tb, M, N, K):
    rng = np.random.default_rng(M * 7 + N * 3 + K + ta * 2 + tb)
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    want = (A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64) + bias
    dA, dB, dbias = _dev(A), _dev(B), _dev(bias)
    C = torch.full((M, N), float("nan"), device="cuda")
    L = hip.lib()
    hip.check(L.cloudaae_gemm_f32(ta, tb, M, N, K, hip.ptr(dA), A.shape[1], hip.ptr(dB), B.shape[1], hip.ptr(C), N,
                                  hip.ptr(dbias), 0, hip.stream()), "gemm")
    scale = np.sqrt(K) + 1
    assert np.abs(C.cpu().numpy() - want).max() / scale < 2e-5
    # accumulate on top, no bias
    hip.check(L.cloudaae_gemm_f32(ta, tb, M, N, K, hip.ptr(dA), A.shape[1], hip.ptr(dB), B.shape[1], hip.ptr(C), N,
                                  None, 1, hip.stream()), "gemm")
    assert np.abs(C.cpu().numpy() - (2 * want - bias)).max() / scale < 4e-5


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (32, 1024, 1024), (2, 3, 256), (200, 130, 70), (4096, 64, 24),
                                   (4096, 128, 64), (320, 1024, 8192), (64, 64, 20000), (129, 257, 33),
                                   (2, 12288, 1024), (32768, 1024, 320)])
def test_gemm_bf16(hip, ta, tb, M, N, K):
    """bf16 operands (round to nearest even), fp32 accumulate: equals the float64 product of the
    bf16-rounded operands up to fp32 accumulation round-off -- the rounding itself is exact."""
    if M * N * K > 2 ** 31 and (ta or tb):
        pytest.skip("largest shape once")
    rng = np.random.default_rng(M * 7 + N * 3 + K + ta * 2 + tb)
    A = torch.from_numpy(rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32))
    B = torch.from_numpy(rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    Ar, Br = A.cuda().bfloat16().double(), B.cuda().bfloat16().double()      # torch rounds RNE too
    want = ((Ar.T if ta else Ar) @ (Br.T if tb else Br) + bias.cuda().double())
    dA, dB, dbias = A.cuda(), B.cuda(), bias.cuda()
    C = torch.full((M, N), float("nan"), device="cuda")
    L = hip.lib()
    hip.check(L.cloudaae_gemm_bf16(ta, tb, M, N, K, hip.ptr(dA), A.shape[1], hip.ptr(dB), B.shape[1], hip.ptr(C), N,
                                   hip.ptr(dbias), 0, hip.stream()), "gemm_bf16")
    scale = np.sqrt(K) + 1
    assert float((C.double() - want).abs().max()) / scale < 2e-5
    hip.check(L.cloudaae_gemm_bf16(ta, tb, M, N, K, hip.ptr(dA), A.shape[1], hip.ptr(dB), B.shape[1], hip.ptr(C), N,
                                   None, 1, hip.stream()), "gemm_bf16")
    assert float((C.double() - (2 * want - bias.cuda().double())).abs().max()) / scale < 4e-5
    # and it is a bf16 product, not an fp32 one
    if K >= 256:
        full = (A.cuda().double().T if ta else A.cuda().double()) @ (B.cuda().double().T if tb else B.cuda().double())
        assert float((want - bias.cuda().double() - full).abs().max()) / scale > 1e-4


@pytest.mark.parametrize("M,N,K", [(2048, 320, 512), (16384, 320, 512), (1024, 160, 512), (4096, 320, 1024)])
def test_gemm_160_wide_tiles_stay_inside(hip, M, N, K):
    """N a multiple of 160 but not of 128 takes 128 x 160 tiles; the tall / short-K rule (64-row tiles below K = 512) must
    not apply to them (it once launched a 64-row grid over 128-row tiles: half the workgroups started past the end of A
    and C).  Guard rows before and after C must survive; result against float64."""
    rng = np.random.default_rng(M + N + K)
    A = _dev(rng.standard_normal((M, K)).astype(np.float32))
    B = _dev(rng.standard_normal((K, N)).astype(np.float32))
    guard = 64
    buf = torch.full((guard + M + guard, N), 777.0, device="cuda")
    C = buf[guard:guard + M]
    L = hip.lib()
    hip.check(L.cloudaae_gemm_f32(0, 0, M, N, K, hip.ptr(A), K, hip.ptr(B), N, C.data_ptr(), N, None, 0, hip.stream()),
              "gemm")
    torch.cuda.synchronize()
    assert float((buf[:guard] - 777.0).abs().max()) == 0.0 and float((buf[guard + M:] - 777.0).abs().max()) == 0.0
    assert _rel(C, A.double() @ B.double()) < 1e-5


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M,N,K", [(128, 1024, 1024), (1024, 1024, 320), (256, 12288, 1024), (100, 300, 500), (4096, 64, 24),
                                   (33, 3, 256)])
def test_gemm_ordered_is_bit_reproducible(hip, M, N, K, bf16):
    """cloudaae_gemm_*_ordered: a product cut over K keeps its slices apart and sums them in slice order -- the same
    bits launch after launch (the plain call adds the slices with fp32 atomics), equal to the plain call to round-off,
    C not cleared beforehand, bias added once."""
    rng = np.random.default_rng(M + N + K)
    A = _dev(rng.standard_normal((M, K)).astype(np.float32))
    B = _dev(rng.standard_normal((K, N)).astype(np.float32))
    bias = _dev(rng.standard_normal(N).astype(np.float32))
    L = hip.lib()
    nm = "bf16" if bf16 else "f32"
    n = int(getattr(L, "cloudaae_gemm_%s_ordered_workspace" % nm)(M, N, K))
    splits = int(getattr(L, "cloudaae_gemm_%s_splits" % nm)(M, N, K))
    assert (n > 0) == (splits > 1) and n == (splits * M * N if splits > 1 else 0)
    ws = torch.full((max(n, 1),), float("nan"), device="cuda")
    runs = []
    for _ in range(8):
        C = torch.full((M, N), float("nan"), device="cuda")
        hip.check(getattr(L, "cloudaae_gemm_%s_ordered" % nm)(0, 0, M, N, K, hip.ptr(A), K, hip.ptr(B), N, hip.ptr(C), N,
                                                               hip.ptr(bias), ws.data_ptr() if n else None, n, hip.stream()),
                  "gemm_ordered")
        runs.append(C)
    torch.cuda.synchronize()
    for C in runs[1:]:
        assert torch.equal(C, runs[0])
    plain = torch.empty((M, N), device="cuda")
    hip.check(getattr(L, "cloudaae_gemm_%s" % nm)(0, 0, M, N, K, hip.ptr(A), K, hip.ptr(B), N, hip.ptr(plain), N,
                                                   hip.ptr(bias), 0, hip.stream()), "gemm")
    assert _rel(runs[0], plain) < 1e-5
    if n:       # a cut product without its workspace, or with one that is too small for the cut, is refused
        for wsp, size in ((None, 0), (ws.data_ptr(), n - 1)):
            rc = getattr(L, "cloudaae_gemm_%s_ordered" % nm)(0, 0, M, N, K, hip.ptr(A), K, hip.ptr(B), N, hip.ptr(plain), N,
                                                              None, wsp, size, hip.stream())
            assert rc != 0 and "workspace" in L.cloudaae_last_error().decode()


def test_gemm_strided_views(hip):
    # column slices of wider buffers as A and C (what the fused encoder uses)
    rng = np.random.default_rng(0)
    big = _dev(rng.standard_normal((512, 320)).astype(np.float32))
    W = _dev(rng.standard_normal((64, 128)).astype(np.float32))
    out = torch.zeros((512, 256), device="cuda")
    L = hip.lib()
    hip.check(L.cloudaae_gemm_f32(0, 0, 512, 128, 64, big.data_ptr() + 4 * 64, 320, hip.ptr(W), 128,
                                  out.data_ptr() + 4 * 128, 256, None, 0, hip.stream()), "gemm")
    want = big[:, 64:128].double() @ W.double()
    assert _rel(out[:, 128:], want) < 1e-5 and float(out[:, :128].abs().max()) == 0.0


def _oracle_bn(x, gamma, beta, training, sm, sv, decay, relu):
    from oracle import model_oracle as MO
    V = MO.Vars()
    V.p["s/beta"], V.p["s/gamma"] = beta, gamma
    V.s["s/moments/Squeeze/ExponentialMovingAverage"] = sm
    V.s["s/moments/Squeeze_1/ExponentialMovingAverage"] = sv
    y = MO.batch_norm(x, "s", V, training, decay)
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("M,C,relu,training", [(32, 1024, True, True), (2, 256, True, True), (1000, 70, False, True),
                                               (4096, 64, True, True), (64, 512, True, False)])
def test_batch_norm_fwd_bwd(hip, M, C, relu, training):
    from cloudaae_amd.utils import _functions as F
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).requires_grad_(True)
    sm, sv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    w = torch.randn(M, C, generator=g)
    want = _oracle_bn(x, gamma, beta, training, sm.clone(), sv.clone(), 0.9, relu)
    (want * w).sum().backward()
    xd = x.detach().cuda().requires_grad_(True)
    gd, bd = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
    smd, svd = sm.cuda(), sv.cuda()
    decay = torch.full((1,), 0.9, device="cuda")
    out, mean, var = F.BatchNormFn.apply(xd, gd, bd, smd, svd, decay, training, relu, 0, 0, True)
    (out * w.cuda()).sum().backward()
    assert _rel(out, want) < 2e-5
    assert _rel(xd.grad, x.grad) < 2e-4
    assert _rel(gd.grad, gamma.grad) < 2e-4 and _rel(bd.grad, beta.grad) < 2e-4
    if training:   # EMA shadows: s -= (s - stat) * (1 - decay)
        ref_sm, ref_sv = sm.clone(), sv.clone()
        _oracle_bn(x.detach(), gamma.detach(), beta.detach(), True, ref_sm, ref_sv, 0.9, relu)
        assert _rel(smd, ref_sm) < 1e-5 and _rel(svd, ref_sv) < 1e-5


@pytest.mark.parametrize("pool", ["mean", "max"])
def test_batch_norm_pool(hip, pool):
    from cloudaae_amd.utils import _functions as F
    B, N, C = 3, 200, 130
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * N, C, generator=g)
    if pool == "max":
        x[N:N + 50] = x[:50]          # duplicated rows in another cloud; and ties inside one cloud:
        x[10] = x[3]
    x.requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).requires_grad_(True)
    w = torch.randn(B, C, generator=g)
    z = _oracle_bn(x, gamma, beta, True, torch.zeros(C), torch.zeros(C), 0.5, True).reshape(B, N, C)
    want = z.mean(1) if pool == "mean" else z.amax(1)     # amax shares the gradient among ties, like tf.reduce_max
    (want * w).sum().backward()
    xd = x.detach().cuda().requires_grad_(True)
    gd, bd = gamma.detach().cuda().requires_grad_(True), beta.detach().cuda().requires_grad_(True)
    decay = torch.full((1,), 0.5, device="cuda")
    pooled, mean, var = F.BatchNormFn.apply(xd, gd, bd, torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"),
                                            decay, True, True, N, 1 if pool == "mean" else 2, False)
    (pooled * w.cuda()).sum().backward()
    assert _rel(pooled, want) < 2e-5
    assert _rel(xd.grad, x.grad) < 3e-4
    assert _rel(gd.grad, gamma.grad) < 3e-4 and _rel(bd.grad, beta.grad) < 3e-4


@pytest.mark.parametrize("B,N,cin,cout,k,pool", [(2, 256, 24, 64, 10, "mean"), (2, 200, 64, 64, 10, "mean"),
                                                 (3, 128, 64, 128, 10, "mean"), (2, 130, 64, 64, 20, "max"),
                                                 (2, 100, 24, 128, 5, "max"), (1, 64, 64, 64, 32, "mean"),
                                                 # (clouds on every XCD / the model's N and k = 20; much larger cases put
                                                 # single edges on the ReLU corner, where the two sides may differ by a
                                                 # whole edge's gradient: tools/dev/chk_edgeconv_shapes.py counts them)
                                                 (8, 512, 64, 64, 20, "mean"), (1, 1024, 64, 128, 20, "mean")])
def test_edge_conv_fwd_bwd(hip, oracle, B, N, cin, cout, k, pool):
    from cloudaae_amd.utils import _functions as F
    from oracle import model_oracle as MO
    g = torch.Generator().manual_seed(B * N + cin + cout + k)
    x = (torch.randn(B, N, cin, generator=g) * 0.5)
    if pool == "max":
        x[:, 7] = x[:, 3]             # duplicate points -> tied maxima
    x.requires_grad_(True)
    nn_idx = torch.from_numpy(oracle.knn(x.detach().numpy(), k, channels=min(cin, 64))).long()
    V = MO.Vars(seed=3)
    edge = MO.get_edge_feature(x, nn_idx, k)
    y = MO.conv2d_1x1(edge, cout, "ec", V, True, True, 0.5)
    V.p["ec/biases"].data.normal_(0, 0.1, generator=g)
    V.p["ec/bn/gamma"].data.uniform_(0.5, 1.5, generator=g)
    V.p["ec/bn/beta"].data.normal_(0, 0.1, generator=g)
    for s in V.s.values():
        s.zero_()
    y = MO.conv2d_1x1(edge, cout, "ec", V, True, True, 0.5)
    want = y.mean(2) if pool == "mean" else y.amax(2)
    w = torch.randn(B, N, cout, generator=g)
    (want * w).sum().backward()

    xd = x.detach().cuda().requires_grad_(True)
    P = {n: p.detach().cuda().requires_grad_(True) for n, p in V.p.items()}
    sm, sv = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
    decay = torch.full((1,), 0.5, device="cuda")
    out = F.EdgeConvFn.apply(xd, nn_idx.int().cuda(), P["ec/weights"].reshape(2 * cin, cout), P["ec/biases"],
                             P["ec/bn/gamma"], P["ec/bn/beta"], sm, sv, decay, True, 1 if pool == "mean" else 2, None)
    (out * w.cuda()).sum().backward()
    assert _rel(out, want) < 3e-5
    assert _rel(xd.grad, x.grad) < 5e-4
    for n in ("ec/weights", "ec/bn/gamma", "ec/bn/beta"):
        assert _rel(P[n].grad, V.p[n].grad) < 5e-4, n
    # the conv bias feeds a batch norm: its gradient is analytically zero; both sides are round-off
    scale = float(V.p["ec/weights"].grad.abs().max())
    assert float(P["ec/biases"].grad.abs().max()) < 1e-3 * scale + 1e-4
    for got, name in ((sm, "ec/bn/moments/Squeeze/ExponentialMovingAverage"),
                      (sv, "ec/bn/moments/Squeeze_1/ExponentialMovingAverage")):
        assert _rel(got, V.s[name]) < 2e-5


def test_edge_conv_into_slot_and_eval_mode(hip, oracle):
    from cloudaae_amd.utils import tf_util
    from oracle import model_oracle as MO
    tf_util.reset_default_store(device="cuda")
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 96, 24, generator=g)
    nn_idx = torch.from_numpy(oracle.knn(x.numpy(), 10, channels=3))
    buf = torch.zeros((2, 96, 320), device="cuda")
    out = tf_util.edge_conv(x.cuda(), nn_idx.cuda(), 64, scope="dgcnn2", pool="mean", bn_decay=0.5, is_training=False,
                            out_slot=(buf, 64))
    assert out.shape == (2, 96, 1, 64) and out.data_ptr() == buf.data_ptr() + 4 * 64
    V = MO.Vars()
    sd = tf_util.default_store().state_dict()
    y = MO.conv2d_1x1(MO.get_edge_feature(x, nn_idx.long(), 10), 64, "dgcnn2", V, True, False, 0.5)
    V.p["dgcnn2/weights"].data.copy_(sd["dgcnn2/weights"].cpu())
    y = MO.conv2d_1x1(MO.get_edge_feature(x, nn_idx.long(), 10), 64, "dgcnn2", V, True, False, 0.5).mean(2)
    assert _rel(buf[:, :, 64:128], y) < 3e-5
    assert float(buf[:, :, :64].abs().max()) == 0 and float(buf[:, :, 128:].abs().max()) == 0


def test_division_by_the_neighbour_count_is_the_division(hip):
    """the mean-pool gradient pass divides by k once per gathered element with the IEEE sequence's k-only part taken out of
    the loop (edgeconv.hip: ec_div_by): the quotient of EVERY float -- all 2^32 numerators, subnormal quotients, zeros,
    infinities, NaN -- equals `x / k` in its bits.  Two correction steps: for every k a layer can have and a few other
    divisors; one step: for the k the launcher uses it with (10 and 20) -- and not for every k, which is why there are two."""
    from cloudaae_amd import _lib
    count = torch.zeros(2, dtype=torch.int64, device="cuda")

    def differing(d, corrections):
        _lib.check(_lib.lib()._cdll.cloudaae_selftest_div_by(float(d), corrections, count.data_ptr(), _lib.stream()), "cloudaae_selftest_div_by")
        return tuple(int(v) for v in count.cpu())
    for d in list(range(1, 65)) + [100.0, 1000.0, 7.5, 123.456, 1.0000001, 1.9999999, 999999.0, 1048576.0]:
        assert differing(d, 2) == (0, 0), d
        assert differing(d, 0) == (0, 0), d          # the launcher's choice for k = d
    assert differing(10, 1) == (0, 0) and differing(20, 1) == (0, 0)
    bad, largest = differing(26, 1)
    assert bad > 0 and largest < 0x01000000          # (only quotients in the subnormal range)


@pytest.mark.parametrize("cout", [64, 128])
def test_edge_conv_streamed_product_equals_the_general_one(hip, cout):
    """[P' | Q] = X [W_c | W_n] at 64 input channels goes through ec_pq_stream_kernel (weights in registers, rows streamed);
    rows that are not 16-byte aligned take the general fp32 product.  Same k order in both: the same bits."""
    from cloudaae_amd.utils import _functions as F
    B, N, c, k = 2, 512, 64, 10
    g = torch.Generator(device="cuda").manual_seed(cout)
    wide = torch.randn((B, N, c + 1), generator=g, device="cuda")
    x_odd = wide[:, :, :c]                                   # row stride 65 floats: the general product
    x = x_odd.contiguous()                                   # row stride 64: the streamed one
    W = torch.randn((2 * c, cout), generator=g, device="cuda") * 0.1
    idx = torch.randint(0, N, (B, N, k), generator=g, device="cuda", dtype=torch.int32)
    gamma, beta = torch.rand(cout, generator=g, device="cuda") + 0.5, torch.randn(cout, generator=g, device="cuda") * 0.1

    def fwd(xx):
        return F.EdgeConvFn.apply(xx, idx, W, torch.zeros(cout, device="cuda"), gamma, beta, torch.zeros(cout, device="cuda"),
                                  torch.ones(cout, device="cuda"), torch.full((1,), 0.5, device="cuda"), True, 1, None)
    assert x_odd.stride(1) == c + 1 and x.stride(1) == c
    assert torch.equal(fwd(x), fwd(x_odd))


def test_losses_vs_oracle(hip):
    from cloudaae_amd.losses import angular_distance_taylor, chamfer_loss, trans_distance
    from oracle import model_oracle as MO
    g = torch.Generator().manual_seed(3)
    B = 37
    pred = torch.randn(B, 3, generator=g).requires_grad_(True)
    label = torch.randn(B, 3, generator=g)
    want, wper = MO.translation_error(pred, label)
    want.backward()
    pd = pred.detach().cuda().requires_grad_(True)
    got, gper = trans_distance.get_translation_error(pd, label.cuda())
    got.backward()
    assert _rel(got, want) < 1e-6 and _rel(gper, wper) < 1e-6 and _rel(pd.grad, pred.grad) < 1e-5

    # rotation: generic, small-angle Taylor branch (theta^2 < 1e-2) on either side, clipped acos
    ax = torch.randn(B, 3, generator=g, dtype=torch.float64)
    lab = torch.randn(B, 3, generator=g, dtype=torch.float64)
    ax[0] *= 1e-2; lab[1] *= 1e-2; ax[2] = lab[2].float().double(); ax[3] *= 3.0; lab[4] = ax[4] * -1
    p32 = ax.float().requires_grad_(True)
    want, wper = MO.rotation_error(p32.double(), lab)
    want.float().backward()
    pd = p32.detach().cuda().requires_grad_(True)
    got, gper = angular_distance_taylor.get_rotation_error(pd, lab.cuda())
    got.backward()
    assert got.dtype == torch.float32 and gper.dtype == torch.float64
    assert abs(float(got) - float(want)) < 1e-6
    # every row by itself against the 50-digit reference, with the bounds of tests/test_34_step_paths_gpu.py: the rows that
    # nearly coincide with their label (clipped) and the opposite ones are tiny next to a maximum set by angles near 1
    import step_reference as SR
    ref = SR.rotation(p32.detach().numpy(), lab.numpy(), SR.MP)
    assert ref.clipped[2] == 1 and (np.abs(np.abs(ref.t) - SR.LIM) > 1e-9).all()
    errs = SR.rotation_errors({"theta": gper.cpu().numpy(), "rot_loss": np.float32(float(got)), "drot": pd.grad.cpu().numpy(),
                               "drot_scale": 1.0 / B}, ref)
    assert all(v <= SR.allowed_of(k) for k, v in errs.items()), errs
    # (the oracle itself, float64 torch, holds these bounds only on the well-conditioned rows)
    easy = (ref.clipped == 0) & (np.abs(ref.t) < 0.99)
    assert _rel(gper.cpu()[easy], wper.detach()[easy]) < 1e-12 and _rel(pd.grad.cpu()[easy], p32.grad[easy]) < 1e-5
    R = angular_distance_taylor.exponential_map(lab.cuda())
    assert _rel(R, MO.exponential_map(lab)) < 1e-14

    # chamfer loss + gradient of the mean
    a = torch.randn(3, 200, 3, generator=g).requires_grad_(True)
    b = torch.randn(3, 200, 3, generator=g)
    want, wper = MO.chamfer_loss(a, b)
    want.backward()
    ad = a.detach().cuda().requires_grad_(True)
    got, gper = chamfer_loss.get_loss(ad, b.cuda())
    got.backward()
    assert abs(float(got) - float(want)) < 1e-6 and _rel(gper, wper) == 0
    assert _rel(ad.grad, a.grad) < 1e-5


def test_step_kernels(hip):
    from oracle import model_oracle as MO
    L = hip.lib()
    # bn_decay schedule, train_cloudAAE_ycbv.py:194-202
    step = torch.zeros(1, device="cuda")
    out = torch.zeros(1, device="cuda")
    for s_, bsz in [(0, 128), (1, 128), (2, 128), (3, 32), (100, 2), (7, 40)]:
        step.fill_(float(s_))
        hip.check(L.cloudaae_bn_decay_schedule(hip.ptr(step), float(bsz), 0.5, 40.0, 0.5, 0.99, hip.ptr(out),
                                               hip.stream()), "decay")
        assert float(out) == pytest.approx(MO.bn_decay_schedule(s_, bsz), abs=1e-7)
    # input assembly, :206-226
    b = MO.synthetic_batch(5, 100, seed=2)
    dpc = torch.empty((5, 64, 24), device="cuda")
    dmean = torch.empty((5, 3), device="cuda")
    dnoisy = torch.empty((5, 64, 3), device="cuda")
    noise64 = b["noise"][:, :64].contiguous()
    pc, mean, noisy = MO.assemble_input(b["visiblePoints"], noise64, b["class_id"], 64)
    dvis, dnoise, dcls = b["visiblePoints"].cuda(), noise64.cuda(), b["class_id"].cuda()
    hip.check(L.cloudaae_input_assemble(5, 100, 64, 21, hip.ptr(dvis), hip.ptr(dnoise), hip.ptr(dcls), hip.ptr(dpc),
                                        hip.ptr(dmean), hip.ptr(dnoisy), hip.stream()), "assemble")
    assert _rel(dmean, mean) < 1e-6 and torch.equal(dnoisy.cpu(), noisy)
    assert float((dpc.cpu() - pc).abs().max()) < 1e-6 and torch.equal(dpc.cpu()[:, :, 3:], pc[:, :, 3:])
    # the same rows at other shapes of the kernel: rows that are not whole 16-byte pieces (C = 3 + 2), more than one point
    # per thread (N = 1500), and a cloud above the 4096 points whose rows go through LDS (the per-point row stores)
    for nb, P, N, ncls in [(3, 1600, 1500, 2), (2, 5000, 4200, 21), (2, 4096, 4096, 21)]:
        gg = torch.Generator().manual_seed(N)
        vis = torch.randn((nb, P, 3), generator=gg)
        nz = torch.randn((nb, N, 3), generator=gg) * 0.01
        cls = torch.randint(0, ncls, (nb,), generator=gg)
        dpc2 = torch.empty((nb, N, 3 + ncls), device="cuda")
        dmean2, dnoisy2 = torch.empty((nb, 3), device="cuda"), torch.empty((nb, N, 3), device="cuda")
        dvis2, dnz2, dcls2 = vis.cuda(), nz.cuda(), cls.cuda()       # (held: the call only sees their addresses)
        hip.check(L.cloudaae_input_assemble(nb, P, N, ncls, hip.ptr(dvis2), hip.ptr(dnz2), hip.ptr(dcls2),
                                            hip.ptr(dpc2), hip.ptr(dmean2), hip.ptr(dnoisy2), hip.stream()), "assemble")
        torch.cuda.synchronize()
        want_noisy = vis[:, :N] + nz
        assert torch.equal(dnoisy2.cpu(), want_noisy)
        # (the kernel's mean is a fixed-order fp32 tree: compare the rows with ITS mean, the mean itself to round-off)
        assert float((dmean2.cpu() - want_noisy.double().mean(dim=1).float()).abs().max()) < 1e-6
        assert torch.equal(dpc2.cpu()[:, :, :3], want_noisy - dmean2.cpu()[:, None, :])
        assert torch.equal(dpc2.cpu()[:, :, 3:], torch.nn.functional.one_hot(cls, ncls).float()[:, None, :].expand(nb, N, ncls))
    # Adam (TF ApplyAdam form) over 3 steps on a ragged length
    g = torch.Generator().manual_seed(1)
    n = 1003
    p0 = torch.randn(n, generator=g)
    params = {"w": p0.clone()}
    opt = MO.AdamTF()
    dp = torch.zeros(1004, device="cuda"); dp[:n] = p0.cuda()
    dm, dv = torch.zeros(1004, device="cuda"), torch.zeros(1004, device="cuda")
    b1p, b2p = torch.full((1,), 0.9, device="cuda"), torch.full((1,), 0.999, device="cuda")
    for it in range(3):
        grad = torch.randn(n, generator=g) * (10.0 ** (it - 1))
        opt.apply(params, {"w": grad})
        dg = torch.zeros(1004, device="cuda"); dg[:n] = grad.cuda() * 4
        hip.check(L.cloudaae_adam_tf(n, hip.ptr(dp), hip.ptr(dg), hip.ptr(dm), hip.ptr(dv), 0.0008, 0.9, 0.999, 1e-8,
                                     hip.ptr(b1p), hip.ptr(b2p), 0.25, 1, hip.stream()), "adam")
        assert float((dp[:n].cpu() - params["w"]).abs().max()) < 2e-7
    assert float(b1p) == pytest.approx(0.9 ** 4, rel=1e-6)


def test_input_assemble_draws_its_own_noise(hip):
    """cloudaae_input_assemble_noise: the tf.random.normal(stddev=0.004/3) of train_cloudAAE_ycbv.py:217 drawn inside
    the assembly kernel -- a pure function of (seed, step counter, cloud, point): N(0, stddev) per coordinate,
    identical when repeated, different for another step / seed, and the rest of the assembly (:206-226) unchanged
    (centroid of the noisy points, centred coordinates, one-hot class)."""
    from oracle import model_oracle as MO
    L = hip.lib()
    B, P, N, std = 6, 3000, 2048, 0.004 / 3
    b = MO.synthetic_batch(B, P, seed=4)
    vis, cls = b["visiblePoints"].cuda(), b["class_id"].cuda()
    draws = torch.zeros(2, dtype=torch.int64, device="cuda")     # {draw counter, ticket}

    def run(seed, s_):
        draws[0] = s_
        pc, mean = torch.empty((B, N, 24), device="cuda"), torch.empty((B, 3), device="cuda")
        noisy = torch.empty((B, N, 3), device="cuda")
        hip.check(L.cloudaae_input_assemble_noise(B, P, N, 21, hip.ptr(vis), hip.ptr(cls), hip.ptr(pc), hip.ptr(mean),
                                                  hip.ptr(noisy), std, seed, hip.ptr(draws), hip.stream()), "assemble")
        assert draws.tolist() == [s_ + 1, 0]                     # the launch advanced its counter, the ticket is back at 0
        return pc, mean, noisy
    pc, mean, noisy = run(77, 3)
    z = (noisy - vis[:, :N]).double()
    assert abs(float(z.mean())) < 5 * std / (B * N * 3) ** 0.5
    assert abs(float(z.std()) / std - 1.0) < 0.02
    assert abs(float((z ** 4).mean()) / std ** 4 - 3.0) < 0.15             # kurtosis of a normal
    for a in range(3):                                                       # coordinates are independent draws
        for c in range(a + 1, 3):
            assert abs(float((z[..., a] * z[..., c]).mean())) / std ** 2 < 0.03
    want_pc, want_mean, _ = MO.assemble_input(vis.cpu(), z.float().cpu(), b["class_id"], N)
    assert _rel(mean, want_mean) < 1e-6 and float((pc.cpu() - want_pc).abs().max()) < 1e-6
    again = run(77, 3)
    assert all(torch.equal(x, y) for x, y in zip(again, (pc, mean, noisy)))
    assert not torch.equal(run(77, 4)[2], noisy) and not torch.equal(run(78, 3)[2], noisy)
    # a counter beyond 2^32 (and beyond 2^24, where a float step counter stops changing) still gives a new stream
    big = run(77, (1 << 32) + 3)[2]
    assert not torch.equal(big, noisy) and not torch.equal(big, run(77, (1 << 32) + 4)[2])
    # back-to-back launches with the same arguments (a replayed step) draw fresh noise each time
    draws[0] = 3
    seq = []
    for _ in range(3):
        hip.check(L.cloudaae_input_assemble_noise(B, P, N, 21, hip.ptr(vis), hip.ptr(cls), hip.ptr(pc), hip.ptr(mean),
                                                  hip.ptr(noisy), std, 77, hip.ptr(draws), hip.stream()), "assemble")
        seq.append(noisy.clone())
    assert torch.equal(seq[0], again[2]) and torch.equal(seq[1], run(77, 4)[2]) and not torch.equal(seq[1], seq[2])
    # no noise at all (stddev 0): the plain assembly, and nothing is drawn
    draws[0] = 3
    hip.check(L.cloudaae_input_assemble_noise(B, P, N, 21, hip.ptr(vis), hip.ptr(cls), hip.ptr(pc), hip.ptr(mean),
                                              hip.ptr(noisy), 0.0, 77, hip.ptr(draws), hip.stream()), "assemble")
    assert torch.equal(noisy, vis[:, :N]) and draws.tolist() == [3, 0]


def test_loss_tail_equals_its_parts(hip):
    """cloudaae_loss_tail (per = dist1 + dist2, its mean, pose losses, total and the gradients for a known upstream
    d(total) in ONE launch; the last workgroup to arrive finishes) = cloudaae_add_mean_f32 + cloudaae_pose_losses +
    cloudaae_pose_losses_grad, bit for bit, launch after launch, the arrival counter left at zero."""
    L = hip.lib()
    g = torch.Generator().manual_seed(5)
    for B, n in ((32, 4096), (3, 100), (200, 1024)):
        d1, d2 = torch.rand(B, n, generator=g).cuda(), torch.rand(B, n, generator=g).cuda()
        tp, tl = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, 3, generator=g).cuda()
        rp = torch.randn(B, 3, generator=g).cuda()
        rl = torch.randn(B, 3, generator=g, dtype=torch.float64).cuda()
        up = torch.full((), 0.7, device="cuda")
        f32 = lambda *shape: torch.full(shape, float("nan"), device="cuda")      # noqa: E731
        f64 = lambda *shape: torch.full(shape, float("nan"), device="cuda", dtype=torch.float64)   # noqa: E731
        ws = torch.empty(int(L.cloudaae_mean_workspace_bytes()) // 8 + 1, dtype=torch.float64, device="cuda")
        per0, xyz0 = f32(B, n), f32()
        hip.check(L.cloudaae_add_mean_f32(B * n, hip.ptr(d1), hip.ptr(d2), hip.ptr(per0), hip.ptr(xyz0), hip.ptr(ws),
                                          hip.stream()), "add_mean")
        tper0, tloss0, rper0, jac0, rloss0, tot0 = f32(B), f32(), f64(B), f64(B, 3), f32(), f32()
        hip.check(L.cloudaae_pose_losses(B, hip.ptr(tp), hip.ptr(tl), hip.ptr(rp), hip.ptr(rl), hip.ptr(xyz0), 1000.0, 10.0,
                                         1.0, hip.ptr(tper0), hip.ptr(tloss0), hip.ptr(rper0), hip.ptr(jac0),
                                         hip.ptr(rloss0), hip.ptr(tot0), hip.stream()), "pose_losses")
        dx0, dt0, dr0 = f32(), f32(B, 3), f32(B, 3)
        hip.check(L.cloudaae_pose_losses_grad(B, hip.ptr(tp), hip.ptr(tl), hip.ptr(tper0), hip.ptr(jac0), hip.ptr(up), 1000.0,
                                              10.0, 1.0, hip.ptr(dx0), hip.ptr(dt0), hip.ptr(dr0), hip.stream()), "grad")
        ws2 = torch.full((int(L.cloudaae_loss_tail_workspace_bytes()) // 8 + 1,), float("nan"), dtype=torch.float64,
                         device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        for it in range(20):
            per, xyz = f32(B, n), f32()
            tper, tloss, rper, jac, rloss, tot = f32(B), f32(), f64(B), f64(B, 3), f32(), f32()
            dx, dt, dr = f32(), f32(B, 3), f32(B, 3)
            hip.check(L.cloudaae_loss_tail(B * n, hip.ptr(d1), hip.ptr(d2), hip.ptr(per), hip.ptr(xyz), B, hip.ptr(tp),
                                           hip.ptr(tl), hip.ptr(rp), hip.ptr(rl), 1000.0, 10.0, 1.0, hip.ptr(tper),
                                           hip.ptr(tloss), hip.ptr(rper), hip.ptr(jac), hip.ptr(rloss), hip.ptr(tot),
                                           hip.ptr(up), hip.ptr(dx), hip.ptr(dt), hip.ptr(dr), hip.ptr(ws2),
                                           hip.ptr(ticket), hip.stream()), "loss_tail")
            for a, c in ((per, per0), (xyz, xyz0), (tper, tper0), (tloss, tloss0), (rper, rper0), (jac, jac0),
                         (rloss, rloss0), (tot, tot0), (dx, dx0), (dt, dt0), (dr, dr0)):
                assert torch.equal(a, c), (B, n, it)
        assert int(ticket) == 0
        # without an upstream gradient the three gradient outputs may be NULL
        hip.check(L.cloudaae_loss_tail(B * n, hip.ptr(d1), hip.ptr(d2), hip.ptr(per), hip.ptr(xyz), B, hip.ptr(tp),
                                       hip.ptr(tl), hip.ptr(rp), hip.ptr(rl), 1000.0, 10.0, 1.0, hip.ptr(tper),
                                       hip.ptr(tloss), hip.ptr(rper), hip.ptr(jac), hip.ptr(rloss), hip.ptr(tot), None, None,
                                       None, None, hip.ptr(ws2), hip.ptr(ticket), hip.stream()), "loss_tail")
        assert torch.equal(tot, tot0)


def test_zero_buffers(hip):
    """cloudaae_zero_buffers: any number of buffers cleared by one launch per eight; guards untouched."""
    import ctypes
    L = hip.lib()
    sizes = [16, 4096, 1 << 20, 48, 0, 1 << 16, 32, 1024, 16, 160, 2048]
    big = torch.full((sum(sizes) // 4 + 64 * len(sizes),), 5.0, device="cuda")
    ptrs, nbytes, spans, off = [], [], [], 16
    for sz in sizes:
        ptrs.append(big.data_ptr() + 4 * off)
        nbytes.append(sz)
        spans.append((off, off + sz // 4))
        off += sz // 4 + 64
    hip.check(L._cdll.cloudaae_zero_buffers(len(sizes), (ctypes.c_void_p * len(sizes))(*ptrs),
                                           (ctypes.c_longlong * len(sizes))(*nbytes), hip.stream()), "zero_buffers")
    want = torch.full_like(big, 5.0)
    for a, c in spans:
        want[a:c] = 0.0
    assert torch.equal(big, want)
    rc = L._cdll.cloudaae_zero_buffers(1, (ctypes.c_void_p * 1)(big.data_ptr() + 4), (ctypes.c_longlong * 1)(16),
                                       hip.stream())
    assert rc != 0 and "aligned" in L.cloudaae_last_error().decode()


def test_recorded_step_is_short(hip):
    """The recorded B = 32-style step keeps its launch count down: the loss tail is one launch (no separate mean /
    pose-loss / pose-gradient kernels), "+ element_mean" rides in the output layers (no add_rowvec), the input noise is
    drawn by the assembly kernel and the gradient slots are cleared with the zero zones (no fill in the plan)."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    g = T.TrainGraph({"num_point": 256, "gpu": 0}, {}, {"batch_size": 8}, replay=True)
    el = T.synthetic_element(8, 256, g.device, seed=1)
    g.train_step(el)
    g.train_step(el)
    assert g.replay and g._plan is not None and not g._plan.foreign_ops
    names = [name for _, _, name in g._plan.entries if name is not None]
    for gone in ("cloudaae_add_rowvec", "cloudaae_add_mean_f32", "cloudaae_pose_losses", "cloudaae_pose_losses_grad",
                 "cloudaae_fill_scaled", "cloudaae_input_assemble"):
        assert gone not in names, gone
    assert names.count("cloudaae_loss_tail") == 1 and names.count("cloudaae_input_assemble_noise") == 1
    assert len(g._plan.zextra) == 1
    print("\nrecorded step: %d C-ABI calls: %s" % (len(names), " ".join(n.replace("cloudaae_", "") for n in names)))


def _make_graph(B, N, model_fn="get_model_dgcnn_mean_6d"):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    return T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, model_fn=model_fn)


MODEL_OF = {"get_model_dgcnn_mean_6d": "dgcnn_mean_6d", "get_model_dgcnn_max_6d": "dgcnn_max_6d",
            "get_model_pn": "pn"}


@pytest.mark.parametrize("B,N,model_fn", [(2, 256, "get_model_dgcnn_mean_6d"), (4, 128, "get_model_dgcnn_mean_6d"),
                                          (3, 128, "get_model_dgcnn_max_6d"), (4, 128, "get_model_pn")])
def test_train_step_vs_oracle(hip, B, N, model_fn):
    """BASELINE config 1 (single class, B=2, N=256) and small variants: one full step --
    forward, three losses, backward, gradients of every variable -- vs the CPU restatement."""
    from oracle import model_oracle as MO
    graph = _make_graph(B, N, model_fn)
    V = MO.Vars(seed=11)
    batch = MO.synthetic_batch(B, N, seed=5, single_class=0 if B == 2 else None)
    with torch.no_grad():
        MO.forward_losses(batch, V, N, is_training=False, model=MODEL_OF[model_fn])
    graph.store.load_state_dict(V.state_dict())
    assert graph.store.num_params == sum(p.numel() for p in V.p.values())
    dev_batch = {k: v.cuda() for k, v in batch.items()}
    out = graph.train_step(dev_batch)
    ref, grads = MO.train_step(batch, V, MO.AdamTF(), 0, N, B, model=MODEL_OF[model_fn])
    # north-star tolerance: fp32 Chamfer / pose losses within 1e-5 (measured: <= 1e-7 for B >= 4).
    # At B = 2 the FC batch norms normalise over two samples (x_hat = +-d / sqrt(d^2 + 4e-3)), which
    # amplifies the 1e-6 round-off of the embedding ~10x in the pose heads: 5e-5 there.
    ltol = 5e-5 if B == 2 else 1e-5
    for key in ("xyz_loss", "trans_loss", "axag_loss"):
        assert abs(float(out[key]) - float(ref[key])) <= ltol * max(1.0, abs(float(ref[key]))), key
    assert abs(float(out["total_loss"]) - float(ref["total_loss"])) <= ltol * abs(float(ref["total_loss"]))
    assert _rel(out["xyz_recon"], ref["xyz_recon"]) < 1e-4
    if "nn_idx1" in ref["end_points"]:
        pass
    # gradients of every trainable (conv biases in front of a batch norm are analytically zero)
    gmax = max(float(g.abs().max()) for g in grads.values())
    for name, g in grads.items():
        got = graph.store.vars[name].grad.cpu()
        if name.endswith("/biases") and (name.rsplit("/", 1)[0] + "/bn/beta") in grads:
            assert float(got.abs().max()) < 1e-3 * gmax + 1e-4, name
            continue
        # encoder gradients pass through kNN-grouped, BN-coupled layers; with max pooling a
        # round-off-level near-tie can move a gradient to a different arg-max element
        tol = 1e-3
        if "dgcnn" in name or "pn_conv" in name:
            tol = 1e-2 if "max" in model_fn or "pn" in model_fn else 2e-3
        if B == 2:      # batch-of-2 batch norm is ill-conditioned: round-off is amplified
            tol = 5e-2
        assert _rel(got, g) < tol, (name, _rel(got, g))
    # EMA shadows after the step
    for name, s in V.s.items():
        assert _rel(graph.store.vars[name].data, s) < 1e-4, name


@pytest.mark.parametrize("B,N,k", [(4, 256, 20), (4, 4096, 20)])
def test_train_step_k20_vs_oracle(hip, B, N, k):
    """BASELINE configs[4]'s shape (the fifth configuration): DGCNN with k=20 edge-conv, up to N=4096 points (LDS-tiled kNN
    stress), one full step vs the CPU restatement.

    The kNN op itself is bit-exact on identical inputs (test_00_ops_gpu.py).  Inside the network the
    grouping inputs of the two implementations agree to ~1e-7 relative only (layer 1: the centroid
    subtracted at train...:226 is a sum over N points; layers 2-4: features), so a k-th/(k+1)-th
    near-tie can pick a different neighbour (measured: 0.05-0.7 % of the entries at k=20), and every
    such swap moves losses and gradients by far more than round-off.  So: (1) free-running, the
    neighbour sets must agree on > 95 % of the points; (2) with the oracle grouping on the GPU's
    indices, the north-star tolerances apply unchanged."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from oracle import model_oracle as MO
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, k_neighbor=k)
    V = MO.Vars(seed=13)
    batch = MO.synthetic_batch(B, N, seed=17)
    with torch.no_grad():
        MO.forward_losses(batch, V, N, is_training=False, k=k)
    graph.store.load_state_dict(V.state_dict())
    out = graph.train_step({kk: v.cuda() for kk, v in batch.items()})
    gpu_idx = [out["end_points"]["nn_idx%d" % i].cpu() for i in (1, 2, 3, 4)]
    if N <= 256:
        with torch.no_grad():
            free = MO.forward_losses(batch, V, N, True, MO.bn_decay_schedule(0, B), k)
        for i in range(4):
            a = gpu_idx[i].long().sort(-1).values
            b = free["end_points"]["nn_idx%d" % (i + 1)].long().sort(-1).values
            assert float((a != b).any(-1).float().mean()) < 0.05, i
    ref, grads = MO.train_step(batch, V, MO.AdamTF(), 0, N, B, k=k, nn_override=gpu_idx)
    for key in ("xyz_loss", "trans_loss", "axag_loss"):
        assert abs(float(out[key].detach()) - float(ref[key])) <= 1e-5 * max(1.0, abs(float(ref[key]))), key
    assert _rel(out["xyz_recon"], ref["xyz_recon"]) < 1e-4
    gmax = max(float(g.abs().max()) for g in grads.values())
    for name, g in grads.items():
        got = graph.store.vars[name].grad.cpu()
        if name.endswith("/biases") and (name.rsplit("/", 1)[0] + "/bn/beta") in grads:
            assert float(got.abs().max()) < 1e-3 * gmax + 1e-4, name
            continue
        if N > 1024 and name.startswith("dgcnn_output"):
            # 16384 x 16384 Chamfer pairs: a handful of nearest-neighbour assignments sit on 1e-7
            # near-ties and flip, which moves one point's whole gradient to another column of this
            # layer -- a discrete change for those columns, invisible in the norm
            err = float((got - g).norm() / g.norm())
            assert err < 1e-2, (name, err)
            continue
        assert _rel(got, g) < (5e-3 if "dgcnn" in name else 1e-3), (name, _rel(got, g))


@pytest.mark.parametrize("B,N", [(8, 256), (8, 1024)])
def test_train_step_bf16_gemms_vs_oracle(hip, B, N):
    """BASELINE configs[2]'s arithmetic: the per-point conv1x1 products and their gradient products with bf16
    operands (round to nearest even) and fp32 accumulate, everything else fp32 -- against the
    restatement with the same rounding (oracle/model_oracle.py: GEMM_BF16), grouped on the GPU's
    neighbour indices.  A value on a bf16 rounding boundary rounds differently when the two
    implementations differ by an fp32 ulp, so agreement is ~1e-4, not round-off; and the bf16 step
    must differ from the fp32 step by far more than that.  (Batches of 8: with 4 clouds the batch norms of the
    fully connected heads subtract nearly equal numbers in their backward pass, and the ~1e-6 differences of the
    embedding that a bfloat16-stored y brings grow to 10 % of the smallest head gradient; measured 0.2 % at 8.)"""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from oracle import model_oracle as MO
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, gemm_dtype="bf16")
    f32 = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    V = MO.Vars(seed=21)
    batch = MO.synthetic_batch(B, N, seed=23)
    with torch.no_grad():
        MO.forward_losses(batch, V, N, is_training=False)
    graph.store.load_state_dict(V.state_dict())
    f32.store.load_state_dict(V.state_dict())
    dev = {k: v.cuda() for k, v in batch.items()}
    out = graph.train_step(dev)
    ref32 = f32.train_step(dev)
    gpu_idx = [out["end_points"]["nn_idx%d" % i].cpu() for i in (1, 2, 3, 4)]
    from cloudaae_amd.utils import _functions as F
    MO.GEMM_BF16, MO.ACT_BF16 = True, F.ACT_BF16      # (the graph keeps dgcnn_agg's y as bfloat16: same rounding point)
    try:
        ref, grads = MO.train_step(batch, V, MO.AdamTF(), 0, N, B, nn_override=gpu_idx)
    finally:
        MO.GEMM_BF16 = MO.ACT_BF16 = False
    for key in ("xyz_loss", "trans_loss", "axag_loss"):
        a, b = float(out[key].detach()), float(ref[key])
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (key, a, b)
    assert _rel(out["xyz_recon"], ref["xyz_recon"]) < 5e-3
    # it really is the bf16 arithmetic
    assert _rel(out["xyz_recon"].detach(), ref32["xyz_recon"].detach()) > 1e-4
    gmax = max(float(g.abs().max()) for g in grads.values())
    for name, g in grads.items():
        got = graph.store.vars[name].grad.cpu()
        if name.endswith("/biases") and (name.rsplit("/", 1)[0] + "/bn/beta") in grads:
            assert float(got.abs().max()) < 1e-2 * gmax + 1e-3, name
            continue
        err = float((got - g).norm() / (g.norm() + 1e-12))
        assert err < 1e-1, (name, err)


def test_eval_path_fps_gather(hip):
    """evaluate_cloudAAE_ycbv.py:442-452: eval-mode forward, FPS 4N->N on the reconstruction,
    gather, Chamfer against the first N target points."""
    from cloudaae_amd.losses import chamfer_loss
    from cloudaae_amd.tf_ops.sampling import tf_sampling
    from cloudaae_amd import train_cloudAAE_ycbv as T
    graph = _make_graph(4, 128)
    el = T.synthetic_element(4, 128, graph.device, seed=3)
    graph.train_step(el)                      # moves the EMA shadows off zero
    out = graph.eval_step(el)
    recon = out["xyz_recon"]
    sub = tf_sampling.gather_point(recon, tf_sampling.farthest_point_sample(128, recon))
    loss, per = chamfer_loss.get_loss(sub, el["visiblePoints_org"][:, :128].contiguous())
    assert sub.shape == (4, 128, 3) and per.shape == (4, 128) and math.isfinite(float(loss))
    before = out["end_points"]["layer_before_embedding"].tensor()
    assert before.shape == (4, 128, 1, 1024)
    assert _rel(before.reshape(4, 128, 1024).mean(1), out["end_points"]["embedding"]) < 1e-5


def test_training_reduces_loss(hip):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    graph = _make_graph(8, 128)
    el = T.synthetic_element(8, 128, graph.device, seed=1)
    first = None
    for i in range(30):
        out = graph.train_step(el)
        if first is None:
            first = float(out["total_loss"])
    last = float(out["total_loss"])
    assert math.isfinite(last) and last < 0.7 * first
    assert float(graph.batch) == 30.0


@pytest.mark.parametrize("M,N,K", [(4096, 1024, 320), (1000, 130, 70), (32768, 1024, 320)])
def test_gemm_colstats_feed_batch_norm(hip, M, N, K):
    """The product that leaves the column sums of its tiles (cloudaae_gemm_f32_colstats) + the batch norm
    that starts from them (cloudaae_bn_forward_colstats) = the plain product + cloudaae_bn_forward."""
    L = hip.lib()
    parts = L.cloudaae_gemm_f32_colstats_parts(M, N, K)
    assert parts > 0
    assert L.cloudaae_gemm_f32_colstats_parts(262144, 1024, 320) == 2048      # B = 256 per GPU
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).cuda()
    B = (torch.randn(K, N, generator=g) / math.sqrt(K)).cuda()
    bias = torch.randn(N, generator=g).cuda()
    gamma, beta = (torch.rand(N, generator=g) + 0.5).cuda(), torch.randn(N, generator=g).cuda()
    decay = torch.full((1,), 0.9, device="cuda")
    rows = 64 if M % 64 == 0 else 0
    res = []
    for fused in (False, True):
        C = torch.empty(M, N, device="cuda")
        ws = torch.zeros(int(L.cloudaae_bn_workspace_bytes(N)) // 8 + 1, dtype=torch.float64, device="cuda")
        cs = torch.zeros(parts * 2 * N, dtype=torch.float64, device="cuda")
        sm, sv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
        mean, var = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
        out = torch.empty(M, N, device="cuda")
        pooled = torch.empty(M // rows, N, device="cuda") if rows else None
        P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        s = hip.stream()
        if fused:
            hip.check(L.cloudaae_gemm_f32_colstats(0, 0, M, N, K, P(A), K, P(B), N, P(C), N, P(bias), P(cs), s), "g")
            hip.check(L.cloudaae_bn_forward_colstats(M, N, P(C), N, P(gamma), P(beta), 1, P(decay), P(sm), P(sv), P(mean),
                                                     P(var), 1, P(out), N, rows, 1 if rows else 0, P(pooled), None,
                                                     None, P(ws), P(cs), parts, s), "bn")
            stats = cs.reshape(parts, 2, N).sum(0)
            Cd = C.double()
            assert _rel(stats[0], Cd.sum(0)) < 1e-9 and _rel(stats[1], (Cd * Cd).sum(0)) < 1e-9
        else:
            hip.check(L.cloudaae_gemm_f32(0, 0, M, N, K, P(A), K, P(B), N, P(C), N, P(bias), 0, s), "g")
            hip.check(L.cloudaae_bn_forward(M, N, P(C), N, P(gamma), P(beta), 1, P(decay), P(sm), P(sv), P(mean), P(var),
                                            1, P(out), N, rows, 1 if rows else 0, P(pooled), None, None, P(ws), s), "bn")
        torch.cuda.synchronize()
        res.append((C, mean, var, sm, sv, out, pooled))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        if a is not None:
            assert _rel(a, b) < 1e-6


@pytest.mark.parametrize("M,N,K", [(4096, 1024, 320), (1000, 130, 70), (32768, 1024, 320)])
def test_gemm_bf16_colstats(hip, M, N, K):
    """cloudaae_gemm_bf16_colstats: the same C as cloudaae_gemm_bf16, and per tile row the fp64 column sums / sums of
    squares of exactly those stored values (what cloudaae_bn_forward_colstats starts from)."""
    L = hip.lib()
    parts = L.cloudaae_gemm_bf16_colstats_parts(M, N, K)
    assert parts > 0
    g = torch.Generator().manual_seed(M + N + 1)
    A = torch.randn(M, K, generator=g).cuda()
    B = (torch.randn(K, N, generator=g) / math.sqrt(K)).cuda()
    bias = torch.randn(N, generator=g).cuda()
    C0, C1 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    cs = torch.zeros(parts * 2 * N, dtype=torch.float64, device="cuda")
    P = lambda t: t.data_ptr()  # noqa: E731
    hip.check(L.cloudaae_gemm_bf16(0, 0, M, N, K, P(A), K, P(B), N, P(C0), N, P(bias), 0, hip.stream()), "g")
    hip.check(L.cloudaae_gemm_bf16_colstats(0, 0, M, N, K, P(A), K, P(B), N, P(C1), N, P(bias), P(cs), hip.stream()), "g")
    assert torch.equal(C0, C1)
    stats = cs.reshape(parts, 2, N).sum(0)
    Cd = C1.double()
    assert _rel(stats[0], Cd.sum(0)) < 1e-9 and _rel(stats[1], (Cd * Cd).sum(0)) < 1e-9


@pytest.mark.parametrize("ta,tb,M,N,K", [(0, 0, 4096, 1024, 320), (0, 0, 128, 256, 64), (0, 1, 4096, 320, 1024),
                                         (0, 1, 256, 128, 192), (1, 0, 320, 1024, 8192), (1, 0, 128, 256, 640),
                                         (1, 0, 320, 1024, 32768)])
def test_gemm_b16(hip, ta, tb, M, N, K):
    """cloudaae_gemm_b16: operands that ARE bfloat16 in memory, fp32 accumulate -- the float64 product of those values
    up to fp32 accumulation round-off; with a bfloat16 output, that result rounded once (one bf16 ulp at most from the
    rounding of the float64 product); column sums of the fp32 values; accumulation onto an fp32 C."""
    L = hip.lib()
    assert L.cloudaae_gemm_b16_supported(ta, tb, M, N, K) == 1
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + ta)
    A = torch.randn((K, M) if ta else (M, K), generator=g).cuda().bfloat16()
    B = (torch.randn((N, K) if tb else (K, N), generator=g) / math.sqrt(K)).cuda().bfloat16()
    bias = torch.randn(N, generator=g).cuda()
    Ad, Bd = A.double(), B.double()
    want = (Ad.T if ta else Ad) @ (Bd.T if tb else Bd) + bias.double()
    P = lambda t: t.data_ptr()  # noqa: E731
    C = torch.full((M, N), float("nan"), device="cuda")
    hip.check(L.cloudaae_gemm_b16(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C), N, 0, P(bias), 0, None,
                                  hip.stream()), "gemm_b16")
    scale = 2.0            # (B is scaled by 1 / sqrt(K): entries of C are O(1))
    assert float((C.double() - want).abs().max()) / scale < 2e-5
    hip.check(L.cloudaae_gemm_b16(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C), N, 0, None, 1, None,
                                  hip.stream()), "gemm_b16")
    assert float((C.double() - (2 * want - bias.double())).abs().max()) / scale < 4e-5
    parts = L.cloudaae_gemm_b16_colstats_parts(M, N, K) if not (ta or tb) else 0
    if True:
        # bfloat16 output: products that stay whole over K (one that is cut adds fp32 slices and refuses it)
        C16 = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
        cs = torch.zeros(max(parts, 1) * 2 * N, dtype=torch.float64, device="cuda")
        rc = L.cloudaae_gemm_b16(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C16), N, 1, P(bias), 0,
                                 P(cs) if parts else None, hip.stream())
        if rc != 0:      # cut over K: fp32 slices are added, a bf16 output is refused
            assert "cut over K" in L.cloudaae_last_error().decode() and (ta or tb) and K >= 512
        else:
            hip.check(rc, "gemm_b16")
            C32 = torch.empty((M, N), device="cuda")
            hip.check(L.cloudaae_gemm_b16(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C32), N, 0, P(bias), 0,
                                          None, hip.stream()), "gemm_b16")
            assert torch.equal(C16, C32.bfloat16())         # the fp32 result, rounded to nearest even
            if parts:
                stats = cs.reshape(parts, 2, N).sum(0)
                Cd = C32.double()
                assert _rel(stats[0], Cd.sum(0)) < 1e-9 and _rel(stats[1], (Cd * Cd).sum(0)) < 1e-9


@pytest.mark.parametrize("ta,tb,M,N,K", [(0, 0, 4096, 1024, 320), (0, 0, 128, 128, 32), (0, 1, 4096, 320, 1024),
                                         (0, 1, 256, 128, 96), (1, 0, 320, 1024, 32768), (1, 0, 128, 256, 640)])
def test_gemm_bf16x3(hip, ta, tb, M, N, K):
    """cloudaae_gemm_bf16x3: fp32 operands split exactly into three bfloat16 pieces, six piece products, fp32
    accumulate.  Against the float64 product of the fp32 operands it must be as close as the fp32 MFMA kernel is (the
    same 2e-5 / sqrt(K) bound as test_gemm, and within 2 x of cloudaae_gemm_f32's own error) -- NOT a bf16 product,
    whose error on the same data is three orders larger; column sums and accumulation as the fp32 entry points."""
    L = hip.lib()
    assert L.cloudaae_gemm_bf16x3_supported(ta, tb, M, N, K) == 1
    rng = np.random.default_rng(M * 7 + N * 3 + K + ta * 2 + tb)
    A = torch.from_numpy(rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)).cuda()
    B = torch.from_numpy(rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    Ad, Bd = A.double(), B.double()
    want = (Ad.T if ta else Ad) @ (Bd.T if tb else Bd) + bias.double()
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    C3, C32, Cb = (torch.full((M, N), float("nan"), device="cuda") for _ in range(3))
    parts = L.cloudaae_gemm_bf16x3_colstats_parts(M, N, K) if not (ta or tb) else 0
    cs = torch.zeros(max(parts, 1) * 2 * N, dtype=torch.float64, device="cuda")
    hip.check(L.cloudaae_gemm_bf16x3(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C3), N, P(bias), 0,
                                     P(cs) if parts else None, hip.stream()), "gemm_bf16x3")
    hip.check(L.cloudaae_gemm_f32(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C32), N, P(bias), 0, hip.stream()),
              "gemm_f32")
    hip.check(L.cloudaae_gemm_bf16(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(Cb), N, P(bias), 0, hip.stream()),
              "gemm_bf16")
    scale = np.sqrt(K) + 1
    e3 = float((C3.double() - want).abs().max())
    e32 = float((C32.double() - want).abs().max())
    eb = float((Cb.double() - want).abs().max())
    assert e3 / scale < 2e-5 and e3 <= 2.0 * e32 + 1e-6, (e3, e32)
    if K >= 96:
        assert eb > 100 * e3, (eb, e3)                  # a bf16 product is a different thing altogether
    if parts:
        stats = cs.reshape(parts, 2, N).sum(0)
        Cd = C3.double()
        assert _rel(stats[0], Cd.sum(0)) < 1e-9 and _rel(stats[1], (Cd * Cd).sum(0)) < 1e-9
    hip.check(L.cloudaae_gemm_bf16x3(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C3), N, None, 1, None,
                                     hip.stream()), "gemm_bf16x3")
    assert float((C3.double() - (2 * want - bias.double())).abs().max()) / scale < 4e-5


@pytest.mark.parametrize("ta,tb,M,N,K", [(0, 0, 4096, 1024, 320), (0, 1, 32768, 320, 1024), (1, 0, 320, 1024, 4096)])
def test_gemm_bf16x3_operands_the_split_treats_differently(hip, ta, tb, M, N, K):
    """The split product on operands a bfloat16 split could mishandle (both kernel generations: the streamed kernels for
    the first two shapes, the K-sliced one for the third):
      * |v| up to FLT_MAX, where bf16(v) would round to infinity: the leading piece saturates, the split stays exact, the
        results are the fp32 kernel's;
      * denormal operands (pieces are denormal bfloat16s): no NaN / inf, results within a few denormal ulps;
      * +-inf and NaN: every output the fp32 kernel makes non-finite is non-finite here too (NaN: the split does not tell
        inf from NaN), every other output is untouched."""
    L = hip.lib()
    assert L.cloudaae_gemm_bf16x3_supported(ta, tb, M, N, K) == 1
    rng = np.random.default_rng(5 * M + N + K)
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    FLT_MAX = float(np.finfo(np.float32).max)

    def run(A, B):
        C3 = torch.full((M, N), float("nan"), device="cuda")
        C32 = torch.full((M, N), float("nan"), device="cuda")
        hip.check(L.cloudaae_gemm_bf16x3(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C3), N, None, 0, None,
                                         hip.stream()), "gemm_bf16x3")
        hip.check(L.cloudaae_gemm_f32(ta, tb, M, N, K, P(A), A.shape[1], P(B), B.shape[1], P(C32), N, None, 0, hip.stream()),
                  "gemm_f32")
        Ad, Bd = A.double(), B.double()
        return C3, C32, (Ad.T if ta else Ad) @ (Bd.T if tb else Bd)

    a_shape, b_shape = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    # (1) magnitudes up to FLT_MAX in A (signs mixed), B scaled so that the sums stay finite
    a = rng.uniform(0.5, 1.0, a_shape).astype(np.float32) * np.float32(FLT_MAX)
    a *= rng.choice([-1.0, 1.0], a_shape).astype(np.float32)
    a.flat[:: 7] = np.float32(FLT_MAX)
    a.flat[3:: 11] = -np.float32(FLT_MAX)
    a.flat[5:: 13] = np.float32(3.3961775e38)         # just below / at the bfloat16 rounding boundary
    a.flat[6:: 17] = np.frombuffer(np.uint32(0x7f7f8000).tobytes(), dtype=np.float32)[0]
    b = (rng.standard_normal(b_shape) * 2.0 ** -110).astype(np.float32)
    C3, C32, want = run(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert bool(torch.isfinite(C3).all()) and bool(torch.isfinite(C32).all())
    scale = float(want.abs().max())
    e3, e32 = float((C3.double() - want).abs().max()) / scale, float((C32.double() - want).abs().max()) / scale
    assert e3 < 2e-5 / np.sqrt(K) * 30 and e3 <= 2.0 * e32 + 1e-7, (e3, e32)
    # ... and the same with the roles swapped (the big magnitudes in the operand that is split once / staged through LDS)
    C3, C32, want = run(torch.from_numpy((rng.standard_normal(a_shape) * 2.0 ** -110).astype(np.float32)).cuda(),
                        torch.from_numpy((rng.uniform(0.5, 1.0, b_shape) * FLT_MAX * rng.choice([-1.0, 1.0], b_shape))
                                         .astype(np.float32)).cuda())
    scale = float(want.abs().max())
    assert bool(torch.isfinite(C3).all())
    assert float((C3.double() - want).abs().max()) / scale <= 2.0 * float((C32.double() - want).abs().max()) / scale + 1e-7
    # (2) denormals
    a = (rng.standard_normal(a_shape) * 1e-40).astype(np.float32)
    b = rng.standard_normal(b_shape).astype(np.float32)
    C3, C32, want = run(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert bool(torch.isfinite(C3).all())
    assert float((C3.double() - want).abs().max()) < 1e-37       # (either kernel may flush: results are ~1e-39)
    # (3) +-inf and NaN in either operand
    a = rng.standard_normal(a_shape).astype(np.float32)
    b = rng.standard_normal(b_shape).astype(np.float32)
    a[3, 5], a[7, 2], a[64, 33] = np.inf, np.nan, -np.inf
    b[9, 4], b[40, 77] = -np.inf, np.nan
    b[5, :] = 0.5                                      # (exactly representable rows: their lower pieces are zero)
    C3, C32, want = run(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    bad32, bad3 = ~torch.isfinite(C32), ~torch.isfinite(C3)
    assert bool(bad32.any()) and torch.equal(bad32, bad3)
    ok = ~bad32
    good = torch.isfinite(want)
    assert torch.equal(ok, good.cuda() if not good.is_cuda else good)
    scale = float(want[good].abs().max())
    assert float((C3.double() - want)[ok].abs().max()) / scale < 2e-6


def test_gemm_bf16x3p_planes_entry_points(hip):
    """cloudaae_x3_split_weight + cloudaae_gemm_bf16x3p (what the dgcnn_agg layer calls: the weight split once per step)
    give bit for bit what cloudaae_gemm_bf16x3 gives with the split inside the call, column sums included."""
    L = hip.lib()
    M, K, N = 16384, 320, 1024           # (enough row tiles that cloudaae_gemm_bf16x3 takes the streamed route for both products)
    rng = np.random.default_rng(11)
    X = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda()
    W = torch.from_numpy((rng.standard_normal((K, N)) / 18).astype(np.float32)).cuda()
    dY = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    assert L.cloudaae_gemm_bf16x3p_supported(M, N, K) == 1 and L.cloudaae_gemm_bf16x3p_supported(M, K, N) == 1
    assert L.cloudaae_x3_planes_bytes(N, K) == 6 * N * K
    pf = torch.empty(3 * N * K, dtype=torch.bfloat16, device="cuda")
    pb = torch.empty(3 * N * K, dtype=torch.bfloat16, device="cuda")
    hip.check(L.cloudaae_x3_split_weight(K, N, P(W), N, P(pf), P(pb), hip.stream()), "x3_split_weight")
    # the two single-job splits write the same planes
    pf1, pb1 = torch.empty_like(pf), torch.empty_like(pb)
    hip.check(L.cloudaae_x3_split(N, K, P(W), N, 1, P(pf1), hip.stream()), "x3_split")
    hip.check(L.cloudaae_x3_split(K, N, P(W), N, 0, P(pb1), hip.stream()), "x3_split")
    assert torch.equal(pf.view(torch.int16), pf1.view(torch.int16)) and torch.equal(pb.view(torch.int16), pb1.view(torch.int16))
    # the planes add up to W exactly: h + m + l == w for every element
    planes = pb.float().reshape(N // 16, 3, K, 2, 8)               # [step][plane][row][unit][8]
    rows = torch.arange(K, device="cuda")
    swap = ((rows >> 3) & 1).bool()
    planes = torch.where(swap[None, None, :, None, None], planes.flip(3), planes)
    back = planes.sum(1).permute(1, 0, 2, 3).reshape(K, N)
    assert torch.equal(back, W)
    parts = L.cloudaae_gemm_bf16x3p_colstats_parts(M, N, K)
    assert parts == L.cloudaae_gemm_bf16x3_colstats_parts(M, N, K) and parts > 0
    Y, Y0 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    cs, cs0 = (torch.zeros(parts * 2 * N, dtype=torch.float64, device="cuda") for _ in range(2))
    hip.check(L.cloudaae_gemm_bf16x3p(M, N, K, P(X), K, P(pf), P(Y), N, P(bias), 0, P(cs), hip.stream()), "gemm_bf16x3p")
    hip.check(L.cloudaae_gemm_bf16x3(0, 0, M, N, K, P(X), K, P(W), N, P(Y0), N, P(bias), 0, P(cs0), hip.stream()), "gemm_bf16x3")
    assert torch.equal(Y, Y0) and torch.equal(cs, cs0)
    dX, dX0 = torch.empty(M, K, device="cuda"), torch.empty(M, K, device="cuda")
    hip.check(L.cloudaae_gemm_bf16x3p(M, K, N, P(dY), N, P(pb), P(dX), K, None, 0, None, hip.stream()), "gemm_bf16x3p")
    hip.check(L.cloudaae_gemm_bf16x3(0, 1, M, K, N, P(dY), N, P(W), N, P(dX0), K, None, 0, None, hip.stream()), "gemm_bf16x3")
    assert torch.equal(dX, dX0)
    want = X.double() @ W.double() + bias.double()
    assert float((Y.double() - want).abs().max()) / (np.sqrt(K) + 1) < 2e-5
    # refusals
    assert L.cloudaae_gemm_bf16x3p_supported(100, 128, 32) == 0 and L.cloudaae_gemm_bf16x3p_supported(128, 96, 32) == 0
    rc = L.cloudaae_gemm_bf16x3p(100, 128, 32, P(X), K, P(pf), P(Y), N, None, 0, None, hip.stream())
    assert rc != 0 and "not served" in L.cloudaae_last_error().decode()


def test_gemm_bf16x3_refuses_what_it_does_not_serve(hip):
    L = hip.lib()
    assert L.cloudaae_gemm_bf16x3_supported(0, 0, 100, 128, 32) == 0
    assert L.cloudaae_gemm_bf16x3_supported(0, 0, 128, 128, 24) == 0
    assert L.cloudaae_gemm_bf16x3_supported(1, 1, 128, 128, 32) == 0
    a = torch.zeros(128, 128, device="cuda")
    rc = L.cloudaae_gemm_bf16x3(0, 0, 100, 128, 32, a.data_ptr(), 32, a.data_ptr(), 128, a.data_ptr(), 128, None, 0, None,
                                hip.stream())
    assert rc != 0 and "not served" in L.cloudaae_last_error().decode()


def test_gemm_b16_refuses_what_it_does_not_serve(hip):
    L = hip.lib()
    assert L.cloudaae_gemm_b16_supported(0, 0, 100, 128, 64) == 0         # partial row tile
    assert L.cloudaae_gemm_b16_supported(0, 0, 128, 128, 96) == 0         # K not a multiple of 64
    assert L.cloudaae_gemm_b16_supported(1, 1, 128, 128, 64) == 0
    a = torch.zeros(128, 96, dtype=torch.bfloat16, device="cuda")
    c = torch.zeros(128, 128, device="cuda")
    rc = L.cloudaae_gemm_b16(0, 0, 128, 128, 96, a.data_ptr(), 96, a.data_ptr(), 128, c.data_ptr(), 128, 0, None, 0, None,
                             hip.stream())
    assert rc != 0 and "not served" in L.cloudaae_last_error().decode()


def test_to_bf16(hip):
    x = torch.randn(8 * 12345, generator=torch.Generator().manual_seed(5)).cuda() * 100
    x[:8] = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, float("inf"), -3.4e38, 1e-40], device="cuda")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device="cuda")
    hip.check(hip.lib().cloudaae_to_bf16(x.numel(), x.data_ptr(), out.data_ptr(), hip.stream()), "to_bf16")
    assert torch.equal(out.view(torch.int16), x.bfloat16().view(torch.int16))     # round to nearest even, as torch
    assert hip.lib().cloudaae_to_bf16(12, x.data_ptr(), out.data_ptr(), hip.stream()) != 0


@pytest.mark.parametrize("B,N,C", [(4, 256, 1024), (3, 1024, 256), (16, 64, 512)])
def test_bn_meanpool_16(hip, B, N, C):
    """bn16.hip: batch norm + ReLU + mean pool on a bfloat16 y, forward and backward, against the fp32-storage entry
    points (cloudaae_bn_forward_colstats / cloudaae_bn_backward) run on the widened copy of the same y: same moments
    (the column sums come from the fp32 y in both), same per-element arithmetic, dy rounded once to bfloat16."""
    L = hip.lib()
    M = B * N
    g = torch.Generator().manual_seed(B + N + C)
    y32 = (torch.randn(M, C, generator=g) * 2 + torch.randn(C, generator=g)).cuda()
    y16 = y32.bfloat16()
    yw = y16.float()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    dpooled = torch.randn(B, C, generator=g).cuda()
    decay = torch.full((1,), 0.9, device="cuda")
    cs = torch.stack([y32.double().sum(0), (y32.double() ** 2).sum(0)]).reshape(-1).contiguous()     # one part
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    ws = torch.empty(int(L.cloudaae_bn_workspace_bytes(C)) // 8 + 1, dtype=torch.float64, device="cuda")

    def run(sixteen):
        em, ev = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        sm, sv = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        pooled = torch.empty(B, C, device="cuda")
        ps = torch.empty(B * 3 * C, dtype=torch.float64, device="cuda")
        dg, db, dbias = torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        if sixteen:
            dy = torch.empty(M, C, dtype=torch.bfloat16, device="cuda")
            hip.check(L.cloudaae_bn_meanpool_forward16(M, C, P(y16), C, P(gamma), P(beta), P(decay), P(em), P(ev), P(sm),
                                                       P(sv), N, P(pooled), P(ps), P(ws), P(cs), 1, hip.stream()), "f16")
            hip.check(L.cloudaae_bn_meanpool_backward16(M, C, P(y16), C, P(gamma), P(beta), P(sm), P(sv), N, P(dpooled),
                                                        P(dy), C, P(dg), P(db), P(dbias), 0, P(ps), P(ws), hip.stream()),
                      "b16")
        else:
            dy = torch.empty(M, C, device="cuda")
            hip.check(L.cloudaae_bn_forward_colstats(M, C, P(yw), C, P(gamma), P(beta), 1, P(decay), P(em), P(ev), P(sm),
                                                     P(sv), 1, None, C, N, 1, P(pooled), None, P(ps), P(ws), P(cs), 1,
                                                     hip.stream()), "f32")
            hip.check(L.cloudaae_bn_backward(M, C, P(yw), C, P(gamma), P(beta), P(sm), P(sv), 1, 1, None, C, N, 1,
                                             P(dpooled), P(pooled), None, P(dy), C, P(dg), P(db), P(dbias), 0, P(ps), P(ws),
                                             hip.stream()), "b32")
        return dict(em=em, ev=ev, sm=sm, sv=sv, pooled=pooled, ps=ps, dg=dg, db=db, dbias=dbias, dy=dy)

    a, b = run(True), run(False)
    for k in ("em", "ev", "sm", "sv"):
        assert torch.equal(a[k], b[k]), k                    # moments: the same sums through the same finalise kernel
    assert _rel(a["pooled"], b["pooled"]) < 1e-6
    assert _rel(a["ps"], b["ps"]) < 1e-6       # (fp32 partial sums over 32 rows here, over 8 there)
    assert _rel(a["dg"], b["dg"]) < 1e-6 and _rel(a["db"], b["db"]) < 1e-6
    assert float((a["dbias"] - b["dbias"]).abs().max()) <= 1e-5 * float(b["dg"].abs().max() + 1)
    # dy: the fp32 value rounded to bfloat16 (a last-bit difference of the fp32 value can move a rounding boundary)
    want = b["dy"].bfloat16()
    diff = (a["dy"].float() - want.float()).abs()
    assert float((diff > 0).float().mean()) < 1e-3
    assert float(diff.max()) <= float(b["dy"].abs().max()) * 2 ** -7


def test_gemm_tn_group(hip):
    """cloudaae_gemm_f32_tn_group: several weight-gradient products C_j += A_j^T B_j in one launch -- partial tiles
    (M = 24), a folded output ([2*cin, cout] kernel addressed as [cin, 2*cout]), outputs cleared by the call or by the
    caller -- against float64 products."""
    import ctypes
    L = hip.lib()
    rng = np.random.default_rng(4)
    shapes = [(24, 128, 5000, 64, 1), (64, 128, 4096, 64, 0), (64, 256, 32768, 128, 1), (130, 70, 777, 0, 0)]   # M, N, K, fold_c, zeroed
    jobs = (hip.GemmTnJob * len(shapes))()
    keep, want = [], []
    for j, (M, N, K, fold, zeroed) in zip(jobs, shapes):
        lda, ldb = M + 8, N
        A = torch.from_numpy(rng.standard_normal((K, lda)).astype(np.float32)).cuda()
        B = torch.from_numpy(rng.standard_normal((K, ldb)).astype(np.float32)).cuda()
        if fold:
            C = torch.zeros((N // fold) * M, fold, device="cuda") if zeroed else torch.full(((N // fold) * M, fold), 7.0, device="cuda")
            ldc = fold
        else:
            C = torch.zeros(M, N, device="cuda") if zeroed else torch.full((M, N), 7.0, device="cuda")
            ldc = N
        j.M, j.N, j.K, j.A, j.lda, j.B, j.ldb, j.C, j.ldc, j.fold_c, j.zeroed = M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb, C.data_ptr(), ldc, fold, zeroed
        keep.append((A, B, C))
        want.append(A[:, :M].double().t().cpu() @ B.double().cpu())
    hip.check(L.cloudaae_gemm_f32_tn_group(len(shapes), jobs, hip.stream()), "group")
    torch.cuda.synchronize()
    for (M, N, K, fold, _), (_, _, C), w in zip(shapes, keep, want):
        got = C.cpu().double()
        if fold:      # logical (r, c) lives at row (c // fold) * M + r, column c % fold
            got = got.reshape(N // fold, M, fold).permute(1, 0, 2).reshape(M, N)
        assert float((got - w).abs().max()) / (math.sqrt(K) + 1) < 2e-5, (M, N, K)
    # more than eight products per launch is refused
    assert L.cloudaae_gemm_f32_tn_group(9, jobs, hip.stream()) != 0
