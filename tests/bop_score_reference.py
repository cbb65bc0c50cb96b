"""NumPy restatement of DESIGN.md, "BOP pose errors (VSD, MSSD, MSPD)".  Written from the definition: float64 on exactly
widened inputs in the order the definition writes it (NumPy does not fuse a product into a sum; its / and sqrt are the
correctly rounded ones), so the counts are expected to equal the kernel's and MSSD / MSPD to equal it bit for bit.  The
images of VSD are rendered by render_reference.render."""
import numpy as np

import render_reference as R

DELTA = 0.015
TAUS = tuple(0.05 * k for k in range(1, 11))
THETAS = tuple(0.05 * j for j in range(1, 11))


def distance_image(depth, intr):
    """D(d) of a uint16 image [H,W] under intrinsics (fx, fy, cx, cy, factor) float32."""
    fx, fy, cx, cy, factor = (float(np.float32(k)) for k in np.asarray(intr).reshape(-1)[:5])
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    xn = (u.astype(np.float64) - cx) / fx
    yn = (v.astype(np.float64) - cy) / fy
    m = np.sqrt((xn * xn + yn * yn) + 1.0)
    return (depth.astype(np.float64) / factor) * m


def vsd_counts(depth_test, intrinsics, frame_of, depth_gt, depth_est, delta, tau):
    """depth_test [F,H,W], depth_gt [B,H,W], depth_est [B,P,H,W] uint16; intrinsics [F,5]; tau [B,K] float64.
    -> dict(inter, union [B,P], over [B,P,K], visib_gt [B]) int32.  A frame_of entry outside [0, F): zeros."""
    B, P = depth_est.shape[:2]
    K = np.asarray(tau).shape[1]
    inter, union = np.zeros((B, P), np.int32), np.zeros((B, P), np.int32)
    over, visib = np.zeros((B, P, K), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        f = int(frame_of[b])
        if f < 0 or f >= len(depth_test):
            continue
        dt, dg = depth_test[f], depth_gt[b]
        Dt, Dg = distance_image(dt, intrinsics[f]), distance_image(dg, intrinsics[f])
        valid_t = dt != 0
        vis_g = (dg != 0) & (~valid_t | (Dg - Dt <= delta))
        visib[b] = vis_g.sum()
        for p in range(P):
            de = depth_est[b, p]
            De = distance_image(de, intrinsics[f])
            vis_e = (de != 0) & (~valid_t | (De - Dt <= delta) | vis_g)
            both = vis_g & vis_e
            inter[b, p], union[b, p] = both.sum(), (vis_g | vis_e).sum()
            diff = np.abs(Dg - De)
            for k in range(K):
                over[b, p, k] = (both & (diff >= tau[b][k])).sum()
    return dict(inter=inter, union=union, over=over, visib_gt=visib)


def vsd_errors(inter, union, over):
    """e_k = (over[k] + union - inter) / union, 1.0 where union = 0; float64 [B,P,K]."""
    u = np.asarray(union, np.float64)[..., None]
    num = (np.asarray(over, np.int64) + (np.asarray(union, np.int64) - np.asarray(inter, np.int64))[..., None]).astype(np.float64)
    with np.errstate(all='ignore'):
        return np.where(u == 0, 1.0, num / np.where(u == 0, 1.0, u))


def vsd(meshes, mesh_index, est, gt, depth_test, intrinsics, frame_of, diameters, delta=DELTA, taus=TAUS):
    """The whole of VSD: meshes [(vertices, triangles, ...)], est [B,P,4,4], gt [B,4,4].  -> the counts, errors [B,P,K],
    the rendered depth_gt [B,H,W], depth_est [B,P,H,W] and dropped [B,1+P]."""
    est, gt = np.asarray(est, np.float64), np.asarray(gt, np.float64)
    B, P = est.shape[:2]
    F, H, W = depth_test.shape
    dg, de = np.zeros((B, H, W), np.uint16), np.zeros((B, P, H, W), np.uint16)
    dropped = np.zeros((B, 1 + P), np.int32)
    for b in range(B):
        frames = [[(int(mesh_index[b]), 1, gt[b])]] + [[(int(mesh_index[b]), 1, est[b, p])] for p in range(P)]
        r = R.render(meshes, frames, np.repeat(np.asarray(intrinsics, np.float32)[int(frame_of[b])][None], 1 + P, 0), H, W)
        dg[b], de[b], dropped[b] = r['depth'][0], r['depth'][1:], r['dropped']
    tau = np.asarray(taus, np.float64)[None, :] * np.broadcast_to(np.asarray(diameters, np.float64), (B,))[:, None]
    out = vsd_counts(depth_test, intrinsics, frame_of, dg, de, delta, tau)
    out.update(errors=vsd_errors(out['inter'], out['union'], out['over']), depth_gt=dg, depth_est=de, dropped=dropped)
    return out


def apply(A, x):
    """icp_apply: ((A00 x + A01 y) + A02 z) + A03 row by row; A 4x4 (top three rows), x [M,3] float64."""
    A = np.asarray(A, np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        return np.stack([((A[4 * r] * x[:, 0] + A[4 * r + 1] * x[:, 1]) + A[4 * r + 2] * x[:, 2]) + A[4 * r + 3]
                         for r in range(3)], axis=1)


def mssd_mspd(model, est, gt, intr=None, symmetries=None):
    """One sample, one pose: model [M,>=3] float32, est, gt 4x4, symmetries [n,4,4] (None: the identity).  -> (mssd,
    mspd or None) float64."""
    x = np.asarray(model, np.float32)[:, :3].astype(np.float64)
    syms = np.eye(4)[None] if symmetries is None else np.asarray(symmetries, np.float64).reshape(-1, 4, 4)
    e = apply(est, x)
    mssd, mspd = [], []
    if intr is not None:
        fx, fy, cx, cy = (float(np.float32(k)) for k in np.asarray(intr).reshape(-1)[:4])
    with np.errstate(all='ignore'):
        for S in syms:
            g = apply(gt, apply(S, x))
            d = e - g
            mssd.append(np.sqrt(np.max((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])))
            if intr is not None:
                ue, ve = (fx * e[:, 0]) / e[:, 2] + cx, (fy * e[:, 1]) / e[:, 2] + cy
                ug, vg = (fx * g[:, 0]) / g[:, 2] + cx, (fy * g[:, 1]) / g[:, 2] + cy
                du, dv = ue - ug, ve - vg
                d2 = np.where((e[:, 2] > 0) & (g[:, 2] > 0), du * du + dv * dv, np.inf)
                mspd.append(np.sqrt(np.max(d2)))
    return min(mssd), (min(mspd) if intr is not None else None)


def recall(errors, thetas):
    """[n]: per sample the share of (k, j) with errors[i, k] < thetas[i, j]."""
    e = np.asarray(errors, np.float64)
    e = e.reshape(len(e), -1)
    t = np.asarray(thetas, np.float64)
    t = np.broadcast_to(t.reshape(1, -1) if t.ndim == 1 else t, (len(e), t.shape[-1]))
    return np.array([np.mean([[e[i, k] < t[i, j] for j in range(t.shape[1])] for k in range(e.shape[1])])
                     for i in range(len(e))], np.float64)
