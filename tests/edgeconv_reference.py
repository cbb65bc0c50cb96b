"""NumPy restatement of the edge-convolution contract of include/cloudaae_hip.h (the comment above
cloudaae_edgeconv_forward), written from the edge-tensor definition: a yardstick for csrc/edgeconv.hip.

  e_ij = [x_i, x_nbr(i,j) - x_i],  y_ij = e_ij W + b;  batch norm over all B*N*k edges (biased variance, eps 1e-3, EMA
  s - (s - stat)(1 - decay)), ReLU, mean or max over k.  The batch-norm / ReLU / pool stage is bn_reference.forward /
  backward on the [P*k, C] edge rows with pool_rows = k.

The kernels are judged in three stages, each from that stage's own inputs, so that an error belongs to the kernel that made it:
  A  (x, W, b) -> pq = [U | Q],  U = X W_c - X W_n + b,  Q = X W_n                                (stage_a)
  B  (fp32 pq, nn_idx, gamma, beta, shadows, decay, dout) -> moments, shadows, out, tie_count, edge_stats, dgamma, dbeta,
     dbiases, dpq = [S | T - S],  y_ij = fl32(U_i + Q_nbr),  S_i = sum_j dy_ij,  T_m = sum_{nbr(i,j) = m} dy_ij  (stage_b)
  C  (the dpq the kernel returned, x, W) -> dx = dpq [W_c | W_n]^T (+ prior),  [dW_c | dW_n] = X^T dpq     (stage_c)
With gemm_bf16 the operands of A and C are rounded to bfloat16 (nearest even) first; from there the reference is exact.

dtype = float64 is the reference.  dtype = float32 performs the kernels' own formulas in fp32 (column sums in fp64 and the
moments rounded once; S from the edge statistics; T added in fp32 in list order; sequential fp32 dot products): the
constants of tests/test_22_edge_conv_paths_gpu.py are measured with it (tests/test_edgeconv_reference_host.py), and it is
never compared with a kernel.

Lattice inputs (x multiples of 2^-3 in [-2, 2], W and b multiples of 2^-4 in [-1, 1]) make every product a multiple of
2^-7 and every sum smaller than 2^9: P, Q, U and y are exact in fp32 in any order of summation, with bf16 operands too.
Stage A is then bit for bit, stage B's input is known before anything is sent, and equal y give natural ties.

The file also holds what the two test files share: the launcher's rules restated (launcher_paths), the case table, the
constructed neighbour lists, the normalised errors and the mutants that prove the bounds tight."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import bn_reference as BN

U, F32, F64 = BN.U, np.float32, np.float64

MUTANTS = ("first_64_sources_only", "tail_source_dropped", "k_plus_one", "unshared_ties", "m2_zero", "centre_not_subtracted",
           "odd_last_point_counted_twice", "drop_last_edge")
_BN_MUTANT = {"k_plus_one": "pool_rows_plus_one", "unshared_ties": "unshared_ties", "m2_zero": "m2_zero",
              "drop_last_edge": "drop_last_row"}
MAX_REDRAWS = 16


def rne_bf16(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    b = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(F32).reshape(np.shape(a))


def bf16_bits(a):
    return (rne_bf16(a).view(np.uint32) >> 16).astype(np.uint16)


def neighbours(idx, B, N, k):
    """global row of every edge's neighbour, [P, k]"""
    return (np.arange(B * N) // N * N)[:, None] + np.asarray(idx).reshape(B * N, k)


def _seqdot(a, b):
    """a [M,K] b [K,N] in fp32, one term after the other, every product and every sum rounded"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((a.shape[0], b.shape[1]), F32)
    for kk in range(a.shape[1]):
        acc = acc + a[:, kk:kk + 1] * b[kk]
    return acc


def _seqdot_t(a, b, chunk=128):
    """a^T b for a [M,K] b [M,N] in fp32, the M rows one after the other"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((1, a.shape[1], b.shape[1]), F32)
    for r in range(0, a.shape[0], chunk):
        prod = a[r:r + chunk, :, None] * b[r:r + chunk, None, :]
        acc = np.add.accumulate(np.concatenate([acc, prod], 0), axis=0, dtype=F32)[-1:]
    return acc[0]


# ---- the definition ---------------------------------------------------------------------------------------------------
def edge_preactivation(x, idx, W, b, B, N, k):
    """y [P*k, C] in float64 from the edge tensor e_ij = [x_i, x_nbr - x_i]"""
    x = np.asarray(x, F64)
    nb = neighbours(idx, B, N, k)
    e = np.concatenate([np.repeat(x[:, None, :], k, 1), x[nb] - x[:, None, :]], 2).reshape(B * N * k, -1)
    return e @ np.asarray(W, F64) + np.asarray(b, F64)


# ---- stage A ------------------------------------------------------------------------------------------------------------
def stage_a(x, W, b, bf16=0, dtype=F64, mutant=None):
    """pq [P, 2C] = [U | Q] and `t`, the sums of magnitudes its round-off bound is formed from"""
    cin = x.shape[1]
    xs, Ws = (rne_bf16(x), rne_bf16(W)) if bf16 else (np.asarray(x, F32), np.asarray(W, F32))
    if dtype is F64:
        X = xs.astype(F64)
        Pm, Q = X @ Ws[:cin].astype(F64), X @ Ws[cin:].astype(F64)
        Uh = Pm + b.astype(F64) if mutant == "centre_not_subtracted" else (Pm - Q) + b.astype(F64)
    else:
        Pm, Q = _seqdot(xs, Ws[:cin]), _seqdot(xs, Ws[cin:])
        Uh = (Pm - Q) + np.asarray(b, F32)
    ax = np.abs(xs.astype(F64))
    tQ = ax @ np.abs(Ws[cin:].astype(F64))
    tU = ax @ np.abs(Ws[:cin].astype(F64)) + tQ + np.abs(b.astype(F64))
    return SimpleNamespace(pq=np.concatenate([Uh, Q], 1), t=np.concatenate([tU, tQ], 1))


# ---- stage B ------------------------------------------------------------------------------------------------------------
def edge_rows(pq, idx, B, N, k):
    """y_ij = fl32(U_i + Q_nbr) as [P*k, C] float32"""
    pq = np.asarray(pq, F32)
    C = pq.shape[1] // 2
    nb = neighbours(idx, B, N, k)
    return (pq[:, None, :C] + pq[:, C:][nb]).reshape(B * N * k, C)


def _lists(nb, P):
    """edges sorted by the point they name (stable: by source inside a list), the lists' offsets [P+1], every sorted
    edge's position in its list and its list's length"""
    tgt = nb.ravel()
    order = np.argsort(tgt, kind="stable")
    deg = np.bincount(tgt, minlength=P)
    off = np.concatenate([[0], np.cumsum(deg)])
    rank = np.arange(tgt.size) - off[tgt[order]]
    return order, off, rank, deg


def _list_sums(rows, order, off, keep=None):
    """sum of `rows` over every list, float64 [P, C]"""
    P = off.size - 1
    r = np.asarray(rows, F64)[order]
    if keep is not None:
        r = np.where(keep[:, None], r, 0.0)
    out = np.zeros((P, rows.shape[1]), F64)
    full = np.nonzero(off[1:] > off[:-1])[0]
    if full.size:
        out[full] = np.add.reduceat(r, off[full], axis=0)
    return out


def stage_b(pq, idx, B, N, k, gamma, beta, training, ema_mean, ema_var, decay, pool, dout, dtype=F64, mutant=None):
    """everything between the two products.  Returns a namespace of the outputs (save_mean, save_var, out, ties,
    edge_stats [P,3,C], dgamma, dbeta, dbias, dpq) and, at float64, `den`: the terms of every bound."""
    f = dtype
    P, C = B * N, pq.shape[1] // 2
    nb = neighbours(idx, B, N, k)
    y = edge_rows(pq, idx, B, N, k)
    dout = np.asarray(dout, F32)
    twice = mutant == "odd_last_point_counted_twice"
    if twice:       # the statistics see the last point's edges once more
        y, dout = np.concatenate([y, y[-k:]], 0), np.concatenate([dout, dout[-1:]], 0)
    bw = BN.backward(y, gamma, beta, training, ema_mean, ema_var, 1, None, k, pool, dout, f, _BN_MUTANT.get(mutant))
    fw = bw.fw
    M = P * k
    zg, xg = fw.z[:M].reshape(P, k, C), fw.xh[:M].reshape(P, k, C)
    r = SimpleNamespace(save_mean=fw.mean, save_var=fw.var, ties=None if fw.ties is None else fw.ties[:P], edge_stats=None,
                        dgamma=bw.dgamma, dbeta=bw.dbeta, P=P, C=C, k=k)
    stats = bool(training) and pool == 1
    if f is F64:
        r.out = fw.pooled[:P]
        if stats:
            r.edge_stats = fw.pool_stats[:P]
    else:           # the kernel: a lane adds its k values one after the other in fp32
        acc, cnt, sx, sall = (np.zeros((P, C), F32) for _ in range(4))
        for j in range(k):
            acc = acc + zg[:, j]
            if stats:
                sall = sall + xg[:, j]
                cnt = cnt + (zg[:, j] > 0)
                sx = sx + np.where(zg[:, j] > 0, xg[:, j], F32(0))
        r.out = acc / F32(k) if pool == 1 else fw.pooled[:P]
        if stats:
            r.edge_stats = np.stack([cnt, sx, sall], 1)
    dyg = bw.dy[:M].reshape(P, k, C)
    order, off, rank, deg = _lists(nb, P)
    keep = None
    if mutant == "first_64_sources_only":
        keep = rank < 64
    elif mutant == "tail_source_dropped":
        keep = rank != (deg[nb.ravel()[order]] - 1)
    if f is F64:
        S = dyg.sum(1)
        T = _list_sums(bw.dy[:M], order, off, keep)
        r.dbias = bw.dbias
    else:
        if stats:       # S from the point's edge statistics
            gk = dout[:P] / F32(k)
            S = bw.gr * ((gk * r.edge_stats[:, 0] - F32(k) * bw.m1) - r.edge_stats[:, 2] * bw.m2)
        else:
            S = np.zeros((P, C), F32)
            for j in range(k):
                S = S + dyg[:, j]
        T = np.zeros((P, C), F32)
        dys, tg = bw.dy[:M][order], nb.ravel()[order]
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.searchsorted(rank[by_rank], np.arange(int(deg.max()) + 1))
        for q in range(int(deg.max())):
            sel = by_rank[cuts[q]:cuts[q + 1]]
            T[tg[sel]] = T[tg[sel]] + dys[sel]          # (one entry per list at a given position)
        n = float(M)
        gr64 = bw.gr.astype(F64)
        s3 = fw.xh[:M].astype(F64).sum(0)
        r.dbias = (gr64 * ((bw.dz[:M].astype(F64).sum(0) - n * bw.m1.astype(F64)) - bw.m2.astype(F64) * s3)).astype(F32)
    r.dpq = np.concatenate([S, T - S], 1)
    r.deg = deg
    if f is F64 and mutant is None:
        tz = fw.tz.reshape(P, k, C)
        agr = np.abs(bw.gr)
        adz, axm = np.abs(bw.dz), np.abs(bw.xh * bw.m2)
        Bij = agr * (adz + np.abs(bw.m1) + axm * (1.0 + np.abs(bw.mean) * bw.rstd))
        BS = Bij.reshape(P, k, C).sum(1)
        d = {"dS": U * BS, "dT": U * (_list_sums(Bij, order, off) + BS), "dgamma": U * np.abs(bw.dz * bw.xh).sum(0),
             "dbeta": U * adz.sum(0), "dbias": U * agr * (adz + np.abs(bw.m1) + axm).sum(0),
             "stats_sum": U * np.abs(xg).sum(1)}
        if pool == 1:
            d["out"] = U * tz.mean(1)
            r.out_slack = (k / 4.0) * U * np.abs(zg).mean(1)
        else:
            at_max = np.where(zg == r.out[:, None, :], tz, 0.0).max(1)
            d["out"] = U * np.where(r.out > 0, at_max, 0.0)         # after the ReLU a clipped maximum is an exact zero
            r.out_slack = 0.0
        r.den = d
        r.passing = float((zg > 0).mean())
    return r


def ambiguous_count(pq, idx, B, N, k, gamma, beta, training, ema_mean, ema_var, pool):
    """edges whose ReLU mask, or maxima whose runner-up, fp32 cannot decide (bn_reference.ambiguous: same constant, same tz)"""
    y = edge_rows(pq, idx, B, N, k)
    amb, _ = BN.ambiguous(y, gamma, beta, training, ema_mean, ema_var, 1, k, pool)
    return int(amb.sum())


def stage_b_errors(got, ref, start_shadows=None):
    """normalised errors of the outputs in `got` (a dict; None = not produced) against the float64 stage B"""
    e = {}
    g = lambda n: None if got.get(n) is None else np.asarray(got[n], F64)
    C = ref.C
    e["save_mean"] = BN.ulps(got["save_mean"], ref.save_mean.astype(F32))
    e["save_var"] = BN.ulps(got["save_var"], ref.save_var.astype(F32))
    e["out"] = BN._ratio(g("out") - ref.out, ref.den["out"], ref.out_slack)
    if ref.ties is not None and got.get("ties") is not None:
        e["ties"] = float((g("ties") != ref.ties).sum())
    if ref.edge_stats is not None and got.get("edge_stats") is not None:
        es = g("edge_stats")
        e["stats_count"] = float((es[:, 0] != ref.edge_stats[:, 0]).sum())
        e["stats_sum"] = max(BN._ratio(es[:, 1] - ref.edge_stats[:, 1], ref.den["stats_sum"]),
                             BN._ratio(es[:, 2] - ref.edge_stats[:, 2], ref.den["stats_sum"]))
    for n in ("dgamma", "dbeta", "dbias"):
        if got.get(n) is not None:
            e[n] = BN._ratio(g(n) - getattr(ref, n), ref.den[n])
    if got.get("dpq") is not None:
        d = g("dpq")
        e["dS"] = BN._ratio(d[:, :C] - ref.dpq[:, :C], ref.den["dS"])
        e["dT"] = BN._ratio(d[:, C:] - ref.dpq[:, C:], ref.den["dT"])
    return e


# ---- stage C ------------------------------------------------------------------------------------------------------------
def stage_c(dpq, x, W, bf16=0, dx_start=None, dtype=F64):
    """dx [P, cin] and dW [2 cin, C] from the dpq given, with the sums of magnitudes of their bounds (tdx, tdw)"""
    cin, C = x.shape[1], W.shape[1]
    d, xs, Ws = (rne_bf16(dpq), rne_bf16(x), rne_bf16(W)) if bf16 else (np.asarray(dpq, F32), np.asarray(x, F32), np.asarray(W, F32))
    Wf = np.concatenate([Ws[:cin], Ws[cin:]], 1)          # [cin, 2C] = [W_c | W_n]
    if dtype is F64:
        d64, x64, w64 = d.astype(F64), xs.astype(F64), Wf.astype(F64)
        dx, dwf = d64 @ w64.T, x64.T @ d64
        if dx_start is not None:
            dx = dx + dx_start.astype(F64)
    else:
        dx, dwf = _seqdot(d, Wf.T), _seqdot_t(xs, d)
        if dx_start is not None:
            dx = dx + np.asarray(dx_start, F32)
    tdx = np.abs(d.astype(F64)) @ np.abs(Wf.astype(F64)).T
    if dx_start is not None:
        tdx = tdx + np.abs(dx_start.astype(F64))
    tdwf = np.abs(xs.astype(F64)).T @ np.abs(d.astype(F64))
    fold = lambda a: np.concatenate([a[:, :C], a[:, C:]], 0)
    return SimpleNamespace(dx=dx, dw=fold(dwf), tdx=tdx, tdw=fold(tdwf))


# ---- constants ----------------------------------------------------------------------------------------------------------
CONSTANT_OF = {"out": "c_fwd", "stats_sum": "c_stats", "dgamma": "c_dgamma", "dbeta": "c_dbeta", "dbias": "c_dbias",
               "dS": "c_S", "dT": "c_T", "pq": "c_pq", "dx": "c_prod", "dw": "c_prod"}
FIXED = {"save_mean": 1.0, "save_var": 1.0, "ema_mean": 2.0, "ema_var": 2.0, "stats_count": 0.0, "ties": 0.0, "pq_exact": 0.0,
         "out16": 0.0}
# Measured by tests/test_edgeconv_reference_host.py::test_constants_are_four_times_the_restatement (largest normalised
# error of the float32 restatement against the float64 reference over CASES), times four, rounded up to a power of two.
# The measured values are in profiles/notes_edgeconv_paths.md.
ALLOWED = {"c_fwd": 16.0, "c_stats": 8192.0, "c_dgamma": 16.0, "c_dbeta": 8.0, "c_dbias": 4.0, "c_S": 1024.0, "c_T": 1024.0,
           "c_pq": 16.0, "c_prod": 32.0}


pow2_ceil = BN.pow2_ceil


def allowed_of(name):
    return FIXED[name] if name in FIXED else ALLOWED[CONSTANT_OF[name]]


# ---- the launcher's rules, restated ------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def _wave_counts(B, N, grid, nw):
    """points every wave of a launch is handed (ec_for_each_point)"""
    if B >= 8 and grid % 8 == 0:
        nslot = grid // 8
        return [len(range(xcd, B, 8)) * len(range(slot * nw + w, N, nslot * nw))
                for xcd in range(8) for slot in range(nslot) for w in range(nw)]
    return [len(range(g, B * N, grid * nw)) for g in range(grid * nw)]


def launcher_paths(c):
    """which kernels ec_forward_impl / ec_backward_impl (csrc/edgeconv.hip) take for a case: the predicates of the
    launcher evaluated in Python.  The case table states what each case is there for, and the host test asserts that this
    function agrees -- a change of the launcher's rules has to be repeated here, and then shows which cases moved."""
    P, cpl = c.B * c.N, c.cout // 64
    kcap = 10 if c.k <= 10 else (20 if c.k <= 20 else 32)
    fast = c.k == kcap
    ldx = c.cin + c.ldx_pad
    if c.bf16:
        product = "bf16"
    elif c.cin == 64 and P % 32 == 0 and ldx % 4 == 0:          # (x itself is 16-byte aligned in every case)
        product = "stream%d" % (2 * c.cout)
    else:
        product = "general"
    stats = bool(c.training) and c.pool == 1 and bool(c.estats)
    sgrid = max(8, min(256, _ceil_div(_ceil_div(P, 32), 8) * 8))
    agrid = max(8, min(4096, _ceil_div(_ceil_div(P, 8), 8) * 8))
    lddo = c.cout + c.lddo_pad
    quads = stats and lddo % 4 == 0 and c.dout_off % 4 == 0
    fix = 1 if c.k in (10, 20) else 2
    p = {"product": product,
         "ec_stats": ("ec_stats", cpl, kcap, fast) if c.training else None,
         "ec_apply": ("ec_apply", cpl, kcap, c.pool, fast, stats),
         "bwd_stats": ("ec_bwd_stats_pool", cpl) if stats else ("ec_bwd_stats", cpl, kcap, c.pool),
         "bwd_apply": ("ec_bwd_apply_mean4", c.cout, fix) if quads else
                      ("ec_bwd_apply", cpl, kcap, c.pool, "edge_stats" if stats else "gather"),
         "stat_grid": sgrid, "apply_grid": agrid, "stat_grid_capped": _ceil_div(_ceil_div(P, 32), 8) * 8 > 256,
         "apply_grid_capped": _ceil_div(_ceil_div(P, 8), 8) * 8 > 4096,
         "xcd": c.B >= 8 and sgrid % 8 == 0 and agrid % 8 == 0, "xcd_wraps": c.B > 8 and c.B % 8 != 0,
         "odd_tail": any(n % 2 == 1 for g, nw in ((sgrid, 16), (agrid, 4)) for n in _wave_counts(c.B, c.N, g, nw)),
         "fewer_points_than_waves": P < 4, "lds_bytes": 4 * c.N, "lds_over_48k": 4 * c.N > 48 * 1024}
    return p


def required_instantiations():
    s = set()
    for cpl in (1, 2):
        s.add(("ec_bwd_stats_pool", cpl))
        for fix in (1, 2):
            s.add(("ec_bwd_apply_mean4", 64 * cpl, fix))
        for kcap in (10, 20, 32):
            for fast in (True, False):
                s.add(("ec_stats", cpl, kcap, fast))
                for pool in (1, 2):
                    s.add(("ec_apply", cpl, kcap, pool, fast))
            for pool in (1, 2):
                s.add(("ec_bwd_stats", cpl, kcap, pool))
                s.add(("ec_bwd_apply", cpl, kcap, pool))
    return s


def instantiations_of(c):
    p = launcher_paths(c)
    out = set()
    for key in ("ec_stats", "ec_apply", "bwd_stats", "bwd_apply"):
        v = p[key]
        if v is None:
            continue
        if v[0] == "ec_apply":
            v = v[:5]
        elif v[0] == "ec_bwd_apply":
            v = v[:4]
        out.add(v)
    return out


# ---- the case table -----------------------------------------------------------------------------------------------------
def case(name, B=2, N=160, k=10, cin=24, cout=64, pool=1, training=1, family="lattice", bf16=0, ldx_pad=1, estats=1,
         lddo_pad=4, dout_off=0, dx="own", dw="own", null=None, rev=0, side=0, b16out=0, det=0, hub="all", variant=0, why=None):
    """pool 1 mean / 2 max; family lattice | gauss; ldx_pad, lddo_pad: row stride minus width; estats: the calls are
    given edge_stats (used by mean pool in training mode); dout_off: floats the dout pointer is moved by; dx own | null |
    acc; dw own | null | zeroed; null: which of dgamma / dbeta / dbiases is NULL; rev: lists prebuilt by
    cloudaae_edgeconv_revlists for this many layers (0: the backward call builds them); side: side stream; b16out: the
    bf16 twin; det: CLOUDAAE_DETERMINISTIC; hub: "all" = every point names the hub, an int = that many do, None = random
    lists only; why: what launcher_paths must say of the case (the branch it is there for)."""
    c = SimpleNamespace(name=name, B=B, N=N, k=k, cin=cin, cout=cout, pool=pool, training=training, family=family, bf16=bf16,
                        ldx_pad=ldx_pad, estats=estats, lddo_pad=lddo_pad, dout_off=dout_off, dx=dx, dw=dw, null=null, rev=rev,
                        side=side, b16out=b16out, det=det, hub=hub, variant=variant, why=why or {})
    c.data = "B%d_N%d_k%d_i%d_o%d_%s_%s_%s%s%s" % (B, N, k, cin, cout, "mean" if pool == 1 else "max",
                                                 "train" if training else "infer", family, "" if hub == "all" else "_hub%s" % hub,
                                                 "_v%d" % variant if variant else "")
    c.base_seed = zlib.crc32(c.data.encode()) % 1000000
    c.seed = c.base_seed + REDRAWS.get(c.data, 0)
    return c


# data sets whose first draw has an edge fp32 cannot decide: how many times they were drawn again (seed = base + this);
# found by tests/test_edgeconv_reference_host.py::test_every_case_is_conditioned_with_its_stored_seed's helper find_seed
REDRAWS = {"B2_N160_k5_i3_o64_mean_train_lattice": 1, "B2_N160_k27_i24_o128_mean_infer_lattice": 1}


def _cases():
    t = []
    PN = {1: "mean", 2: "max"}
    # instantiations: (CPL, KCAP, FAST, POOL) of the four gathering kernels, both statistics-from-edge_stats kernels and the
    # four quad kernels; the product path changes with k so that the streamed, general and bf16 products all see both widths
    for cout in (64, 128):
        cpl = cout // 64
        for k, kcap in ((10, 10), (20, 20), (32, 32), (5, 10), (13, 20), (27, 32)):
            cin, ldx_pad, bf16 = {10: (64, 0, 0), 20: (64, 1, 0), 32: (24, 1, 0), 5: (3, 1, 0), 13: (5, 1, 0), 27: (24, 1, 1)}[k]
            fast, fix = k == kcap, 1 if k in (10, 20) else 2
            product = "bf16" if bf16 else ("stream%d" % (2 * cout) if k == 10 else "general")
            t.append(case("inst_o%d_k%d_mean" % (cout, k), k=k, cin=cin, cout=cout, pool=1, ldx_pad=ldx_pad, bf16=bf16,
                          why={"product": product, "ec_stats": ("ec_stats", cpl, kcap, fast),
                               "ec_apply": ("ec_apply", cpl, kcap, 1, fast, True), "bwd_stats": ("ec_bwd_stats_pool", cpl),
                               "bwd_apply": ("ec_bwd_apply_mean4", cout, fix)}))
            t.append(case("inst_o%d_k%d_max" % (cout, k), k=k, cin=cin, cout=cout, pool=2, ldx_pad=ldx_pad, bf16=bf16,
                          why={"product": product, "ec_stats": ("ec_stats", cpl, kcap, fast),
                               "ec_apply": ("ec_apply", cpl, kcap, 2, fast, False), "bwd_stats": ("ec_bwd_stats", cpl, kcap, 2),
                               "bwd_apply": ("ec_bwd_apply", cpl, kcap, 2, "gather")}))
    # k = 1: no second slot to plant lists in; non-FAST, two corrections
    t.append(case("inst_o64_k1_mean", k=1, why={"ec_apply": ("ec_apply", 1, 10, 1, False, True), "bwd_apply": ("ec_bwd_apply_mean4", 64, 2)}))
    t.append(case("inst_o128_k1_max", k=1, cout=128, pool=2, why={"ec_apply": ("ec_apply", 2, 10, 2, False, False)}))
    # modes.  Inference: m1 = m2 = 0, the general statistics kernel, no edge_stats
    for cout, k, kcap, pool in ((64, 10, 10, 1), (128, 27, 32, 1), (64, 13, 20, 2), (128, 20, 20, 2)):
        cpl = cout // 64
        t.append(case("infer_o%d_k%d_%s" % (cout, k, PN[pool]), k=k, cout=cout, pool=pool, training=0,
                      why={"ec_stats": None, "ec_apply": ("ec_apply", cpl, kcap, pool, k == kcap, False),
                           "bwd_stats": ("ec_bwd_stats", cpl, kcap, pool), "bwd_apply": ("ec_bwd_apply", cpl, kcap, pool, "gather")}))
    # training, mean pool, edge_stats NULL in both calls: every edge gathered again
    for cout, k, kcap in ((64, 20, 20), (128, 5, 10), (64, 27, 32), (128, 13, 20)):
        cpl = cout // 64
        t.append(case("nostats_o%d_k%d" % (cout, k), k=k, cout=cout, estats=0,
                      why={"ec_apply": ("ec_apply", cpl, kcap, 1, k == kcap, False), "bwd_stats": ("ec_bwd_stats", cpl, kcap, 1),
                           "bwd_apply": ("ec_bwd_apply", cpl, kcap, 1, "gather")}))
    # training, mean pool, edge_stats, but rows of dout the quad kernel cannot load: lddo % 4 != 0; a pointer off by a float
    for cout, k, kcap in ((128, 10, 10), (64, 32, 32)):
        t.append(case("lddo_odd_o%d_k%d" % (cout, k), k=k, cout=cout, lddo_pad=1,
                      why={"bwd_stats": ("ec_bwd_stats_pool", cout // 64), "bwd_apply": ("ec_bwd_apply", cout // 64, kcap, 1, "edge_stats")}))
    for cout, k, kcap in ((128, 20, 20), (64, 13, 20)):
        t.append(case("dout_unaligned_o%d_k%d" % (cout, k), k=k, cout=cout, lddo_pad=4, dout_off=1,
                      why={"bwd_stats": ("ec_bwd_stats_pool", cout // 64), "bwd_apply": ("ec_bwd_apply", cout // 64, kcap, 1, "edge_stats")}))
    # product paths: P = 2 * 161 is no whole number of 32-row tiles; bf16 at 64 channels; one Gaussian case per path
    t.append(case("prod_P322", N=161, cin=64, ldx_pad=0, why={"product": "general"}))
    t.append(case("prod_bf16_i64", cin=64, ldx_pad=0, bf16=1, why={"product": "bf16"}))
    t.append(case("gauss_stream", cin=64, ldx_pad=0, family="gauss", hub=None, why={"product": "stream128"}))
    t.append(case("gauss_stream_o128", cin=64, cout=128, pool=2, ldx_pad=0, family="gauss", hub=None, why={"product": "stream256"}))
    t.append(case("gauss_general", cin=24, family="gauss", hub=None, why={"product": "general"}))
    t.append(case("gauss_general_i5", cin=5, cout=128, family="gauss", hub=None, why={"product": "general"}))
    t.append(case("gauss_bf16", cin=24, bf16=1, family="gauss", hub=None, why={"product": "bf16"}))
    t.append(case("gauss_bf16_i64", cin=64, ldx_pad=0, bf16=1, pool=2, family="gauss", hub=None, why={"product": "bf16"}))
    # point-to-wave assignment
    t.append(case("one_point", B=1, N=1, k=1, cin=3, hub=None, why={"fewer_points_than_waves": True}))
    t.append(case("three_points", B=1, N=3, k=5, cin=3, cout=128, pool=2, hub=None, why={"fewer_points_than_waves": True}))
    t.append(case("odd_tail_N33", B=1, N=33, hub=None, why={"odd_tail": True, "xcd": False}))
    t.append(case("xcd_B8_N19", B=8, N=19, k=5, pool=2, hub=None, why={"xcd": True, "xcd_wraps": False}))
    t.append(case("xcd_B9_N40", B=9, N=40, cout=128, hub=None, why={"xcd": True, "xcd_wraps": True}))
    t.append(case("stat_grid_capped", B=2, N=4101, k=5, cin=5, cout=128, hub=200, why={"stat_grid_capped": True, "stat_grid": 256}))
    t.append(case("apply_grid_capped", B=8, N=4100, k=5, cin=3, hub=200, why={"apply_grid_capped": True, "apply_grid": 4096, "xcd": True}))
    t.append(case("lds_over_48k", B=1, N=12289, k=2, cin=3, hub=200, why={"lds_over_48k": True}))
    # arguments the autograd wrapper never varies (one data set)
    A = dict(why={"bwd_apply": ("ec_bwd_apply_mean4", 64, 1)})
    t.append(case("arg_base", **A))
    t.append(case("arg_dx_null", dx="null", **A))
    t.append(case("arg_dx_accumulate", dx="acc", **A))
    t.append(case("arg_dw_null", dw="null", **A))
    t.append(case("arg_dw_zeroed", dw="zeroed", **A))
    for which in ("dgamma", "dbeta", "dbiases"):
        t.append(case("arg_null_%s" % which, null=which, **A))
    t.append(case("arg_rev_ready", rev=1, **A))
    t.append(case("arg_b16out", b16out=1, **A))
    t.append(case("arg_b16out_max", b16out=1, pool=2, cout=128))
    t.append(case("arg_deterministic", det=1, **A))
    t.append(case("arg_deterministic_max", det=1, pool=2, why={"bwd_apply": ("ec_bwd_apply", 1, 10, 2, "gather")}))
    return t


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
# three index arrays of one shape, their lists built by one launch (cloudaae_edgeconv_revlists, count = 3)
REV3 = [case("rev3_%d" % v, variant=v) for v in (0, 1, 2)]
SIDE = case("arg_side_stream", side=1)


# ---- inputs -------------------------------------------------------------------------------------------------------------
PLANTED = (64, 65, 21)      # in-degrees planted exactly: one chunk of sources, one more than a chunk, no multiple of 16 or 8
HUB, P64, P65, P21, NOBODY, SELF, SAME = 0, 1, 2, 3, 4, 5, 6       # cloud-local points the features sit at


def neighbour_lists(rng, c):
    """constructed lists [B, N, k]: random indices, then (hub is not None, N >= 140) a hub that every point names in slot 0
    (or `hub` points do), points named exactly 64, 65 and 21 times, a point nobody names, a point that names itself, and
    a point that names the hub in all its k slots.  k = 1 leaves no second slot: the hub gets what the planted lists leave."""
    B, N, k = c.B, c.N, c.k
    if c.hub is None or N < 140:
        return rng.integers(0, N, (B, N, k)).astype(np.int32)
    idx = rng.integers(7, N, (B, N, k))
    for b in range(B):
        first = 1 if k > 1 else 0
        slots = [(i, j) for i in range(N) if i not in (SELF, SAME) for j in range(first, k)]
        slots = [slots[s] for s in rng.permutation(len(slots))]
        at = 0
        for tgt, n in zip((P64, P65, P21), PLANTED):
            if at + n > len(slots):
                break
            for i, j in slots[at:at + n]:
                idx[b, i, j] = tgt
            at += n
        if k > 1:
            who = np.arange(N) if c.hub == "all" else rng.permutation(N)[:int(c.hub)]
            idx[b, who, 0] = HUB
        else:
            for i, j in slots[at:at + (len(slots) if c.hub == "all" else int(c.hub))]:
                idx[b, i, j] = HUB
        idx[b, SELF, k - 1] = SELF
        idx[b, SAME, :] = HUB
    return idx.astype(np.int32)


def draw(c, seed):
    """the inputs of a case's data set for one seed; `ambiguous` = edges fp32 cannot decide (lattice family; must be 0)"""
    rng = np.random.default_rng(seed)
    B, N, k, cin, C = c.B, c.N, c.k, c.cin, c.cout
    P = B * N
    rnd = lambda *s: rng.standard_normal(s)
    if c.family == "lattice":
        x = (rng.integers(-16, 17, (P, cin)) / 8.0).astype(F32)
        W = (rng.integers(-16, 17, (2 * cin, C)) / 16.0).astype(F32)
        b = (rng.integers(-16, 17, C) / 16.0).astype(F32)
    else:
        x, W, b = rnd(P, cin).astype(F32), (rnd(2 * cin, C) / np.sqrt(2.0 * cin)).astype(F32), rnd(C).astype(F32)
    idx = neighbour_lists(rng, c)
    gamma = (1.0 + 0.2 * rnd(C)).astype(F32)
    gamma[1::7] *= -1.0
    beta = 0.3 * rnd(C)
    beta = (np.where(beta < 0, -1.0, 1.0) * np.maximum(np.abs(beta), 0.05)).astype(F32)
    a = stage_a(x, W, b)
    pq = a.pq.astype(F32)
    y = edge_rows(pq, idx, B, N, k).astype(F64)
    if c.training:
        ema_mean, ema_var = (0.3 * rnd(C)).astype(F32), (0.5 + np.abs(rnd(C))).astype(F32)
    else:
        sd = np.sqrt(y.var(0) + 1.0)
        ema_mean, ema_var = (y.mean(0) + 0.3 * sd * rnd(C)).astype(F32), (sd ** 2 * (0.5 + np.abs(rnd(C)))).astype(F32)
    dout = rnd(P, C).astype(F32)
    r = SimpleNamespace(x=x, W=W, b=b, idx=idx, gamma=gamma, beta=beta, ema_mean=ema_mean, ema_var=ema_var, decay=F32(0.9),
                        dout=dout, pq=pq, pq64=a.pq, tpq=a.t, seed=seed, ambiguous=0)
    if c.family == "lattice":
        assert np.array_equal(pq.astype(F64), a.pq)        # the lattice: exact in fp32
        r.ambiguous = ambiguous_count(pq, idx, B, N, k, gamma, beta, c.training, ema_mean, ema_var, c.pool)
    return r


def find_seed(c):
    """the first seed from the base seed on whose draw is conditioned, or None after MAX_REDRAWS redraws"""
    for d in range(MAX_REDRAWS + 1):
        if draw(c, c.base_seed + d).ambiguous == 0:
            return c.base_seed + d
    return None


ALL_CASES = CASES + REV3 + [SIDE]
ALL_BY_NAME = {c.name: c for c in ALL_CASES}
_DATA = {}
for _c in ALL_CASES:
    _DATA.setdefault(_c.data, _c)       # cases that differ in arguments only share their data set


@functools.lru_cache(maxsize=4)
def _inputs(data, seed):
    return draw(_DATA[data], seed)


def make_inputs(c):
    return _inputs(c.data, c.seed)


@functools.lru_cache(maxsize=4)
def _reference(data, seed, dtype, mutant):
    c = _DATA[data]
    x = make_inputs(c)
    return stage_b(x.pq, x.idx, c.B, c.N, c.k, x.gamma, x.beta, c.training, x.ema_mean, x.ema_var, x.decay, c.pool, x.dout,
                   F64 if dtype == "f64" else F32, mutant)


def reference(c, dtype=F64, mutant=None):
    """stage B of a case on its stored seed (cached by data set: cases that differ in arguments only share it)"""
    return _reference(c.data, c.seed, "f64" if dtype is F64 else "f32", mutant)


def product_errors(got, ref, terms, name):
    return {name: BN._ratio(np.asarray(got, F64) - ref, U * terms)}
