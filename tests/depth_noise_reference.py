"""NumPy restatement of DESIGN.md, "Sensor noise": the slope at a pixel (cloudaae_depth_normals) and the five stages of
cloudaae_depth_sensor_noise, with the host Philox of tests/pose_sampling_reference.py.  Written from the definition.
`dtype` is the type in which normal2 is evaluated: float32 (the definition) or float64 (the same draws wider: how far
fp32 rounding can move a decision, which sizes the tests' margin).  Everything after the draws is float64, un-fused, in
the definition's order.  The module also holds the inputs of tests/test_27_depth_noise_gpu.py (CASES), rendered here by
tests/render_reference.py, so that tests/test_depth_noise_host.py can fix the comparison rule on the CPU."""
import math

import numpy as np

import mesh_models_reference as MR
import pose_sampling_reference as PS
import render_reference as RR

STREAM_NORMALS, STREAM_DROP = 21, 22
HALF_PI = 1.5707963267948966
PARAMS = ('sigma_l', 'a0', 'a1', 'z0', 'a2', 'theta_max', 'theta_drop', 'p_drop', 'baseline', 'disparity_step')
NONE = dict(sigma_l=0.0, a0=0.0, a1=0.0, z0=0.0, a2=0.0, theta_max=0.0, theta_drop=math.pi, p_drop=0.0, baseline=0.0,
            disparity_step=0.0)
KINECT1 = dict(sigma_l=0.8, a0=0.0012, a1=0.0019, z0=0.4, a2=0.0001, theta_max=1.45, theta_drop=1.40, p_drop=0.005,
               baseline=0.075, disparity_step=0.125)
# each stage alone: 'none' with that stage's parameters of 'kinect1'
STAGES = {
    'none': NONE,
    'kinect1': KINECT1,
    'lateral': dict(NONE, sigma_l=0.8),
    'axial': dict(NONE, a0=0.0012, a1=0.0019, z0=0.4, a2=0.0001, theta_max=1.45),
    'dropout': dict(NONE, theta_drop=1.40, p_drop=0.005),
    'disparity': dict(NONE, baseline=0.075, disparity_step=0.125),
}


# ---- the slope -------------------------------------------------------------------------------------------------------
def backproject(dm, intr):
    """dm [H,W] float64 (d / factor_depth) -> P [H,W,3]: (((u - cx) dm) / fx, ((v - cy) dm) / fy, dm)."""
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in np.asarray(intr)[:4])
    H, W = dm.shape
    v, u = np.mgrid[0:H, 0:W]
    return np.stack([((u.astype(np.float64) - cx) * dm) / fx, ((v.astype(np.float64) - cy) * dm) / fy, dm], axis=-1)


def _dot(a, b, reverse):
    if reverse:
        return (a[..., 2] * b[..., 2] + a[..., 1] * b[..., 1]) + a[..., 0] * b[..., 0]
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _shift(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du], `fill` outside the image."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    vs, us = slice(max(dv, 0), H + min(dv, 0)), slice(max(du, 0), W + min(du, 0))
    vd, ud = slice(max(-dv, 0), H + min(-dv, 0)), slice(max(-du, 0), W + min(-du, 0))
    out[vd, ud] = a[vs, us]
    return out


def slope_dm(dm, has, label, intr, reverse=False):
    """The slope at every pixel of one frame from metric depths dm [H,W] float64, has [H,W] bool (depth != 0) and label
    [H,W].  -> (normal [H,W,3] float64, theta [H,W] float64, flat [H,W] bool: pixels with depth that are flat).
    `reverse` sums the three dot products in the opposite order (the tests' tolerance is measured with it)."""
    P = backproject(dm, intr)
    g, any_axis = [], []
    for dv, du in ((0, 1), (1, 0)):
        vhi = _shift(has, dv, du, False) & (_shift(label, dv, du, 0) == label)
        vlo = _shift(has, -dv, -du, False) & (_shift(label, -dv, -du, 0) == label)
        hi = np.where(vhi[..., None], _shift(P, dv, du, 0.0), P)
        lo = np.where(vlo[..., None], _shift(P, -dv, -du, 0.0), P)
        g.append(hi - lo)
        any_axis.append(vhi | vlo)
    gx, gy = g
    c = np.stack([gx[..., 1] * gy[..., 2] - gx[..., 2] * gy[..., 1], gx[..., 2] * gy[..., 0] - gx[..., 0] * gy[..., 2],
                  gx[..., 0] * gy[..., 1] - gx[..., 1] * gy[..., 0]], axis=-1)
    nn, nr, rr = _dot(c, c, reverse), _dot(c, P, reverse), _dot(P, P, reverse)
    with np.errstate(all='ignore'):
        length = np.sqrt(nn)
        cosine = np.abs(nr) / (length * np.sqrt(rr))
        ok = has & any_axis[0] & any_axis[1] & (nn > 0.0) & np.isfinite(nn) & (cosine >= 0.0)
        theta = np.where(ok, np.arccos(np.minimum(np.where(ok, cosine, 0.0), 1.0)), 0.0)
        sign = np.where(nr > 0.0, -1.0, 1.0)
        normal = np.where(ok[..., None], sign[..., None] * (c / length[..., None]), 0.0)
    return normal, theta, has & ~ok


def slope(depth, label, intr, reverse=False):
    """One frame: depth [H,W] uint16, label [H,W] uint8, intr [5] float32."""
    factor = np.float64(np.float32(np.asarray(intr)[4]))
    return slope_dm(depth.astype(np.float64) / factor, depth != 0, label, intr, reverse)


def depth_normals(depth, label, intrinsics, reverse=False):
    """cloudaae_depth_normals: -> dict(normals [F,H,W,3] float32, theta [F,H,W] float32, flat [F,H,W] bool,
    flat_counts [F] int32)."""
    out = [slope(d, l, k, reverse) for d, l, k in zip(depth, label, np.asarray(intrinsics, np.float32))]
    flat = np.stack([o[2] for o in out])
    return dict(normals=np.stack([o[0] for o in out]).astype(np.float32), theta=np.stack([o[1] for o in out]).astype(np.float32),
                flat=flat, flat_counts=flat.reshape(len(out), -1).sum(axis=1).astype(np.int32))


# ---- the sensor ------------------------------------------------------------------------------------------------------
def apply(depth, label, intrinsics, params, seed=0, first_frame=0, dtype=np.float32):
    """cloudaae_depth_sensor_noise.  depth [F,H,W] uint16, label [F,H,W] uint8, intrinsics [F,5] float32; params: a dict
    with the keys PARAMS.  -> dict(depth, label, counts [F,4] int32, z_noisy [F,H,W] float64) plus the quantities whose
    decision points the tests' comparison rule watches: lat_u, lat_v (n sigma_l), src_u, src_v, has (the source has
    depth), theta (unclamped, at the source), disp ((fx baseline / z') / disparity_step; nan without steps), k, quant
    (z'' factor_depth + 0.5)."""
    depth, label = np.asarray(depth), np.asarray(label)
    intr = np.asarray(intrinsics, np.float32)
    F, H, W = depth.shape
    p = {k: np.float64(params[k]) for k in PARAMS}
    drop_below = np.uint64(math.floor(float(params['p_drop']) * 4294967296.0))
    keys = ('depth', 'label', 'z_noisy', 'lat_u', 'lat_v', 'src_u', 'src_v', 'has', 'theta', 'disp', 'k', 'quant')
    out = {k: [] for k in keys}
    counts = np.zeros((F, 4), np.int32)
    v, u = np.mgrid[0:H, 0:W]
    pix = (v * W + u).astype(np.uint64).ravel()
    for f in range(F):
        fx, factor = np.float64(intr[f, 0]), np.float64(intr[f, 4])
        ctr = (np.uint64(first_frame + f) << np.uint64(24)) + pix
        r = PS.philox4x32(seed, ctr, STREAM_NORMALS)
        q = PS.philox4x32(seed, ctr, STREAM_DROP)
        n_u, n_v = (a.astype(np.float64).reshape(H, W) for a in PS.normal2(r[:, 0], r[:, 1], dtype))
        n_z = PS.normal2(r[:, 2], r[:, 3], dtype)[0].astype(np.float64).reshape(H, W)
        r0 = q[:, 0].astype(np.uint64).reshape(H, W)
        # 1. lateral jitter
        lat_u, lat_v = n_u * p['sigma_l'], n_v * p['sigma_l']
        su = np.clip(u + np.rint(lat_u), 0, W - 1).astype(np.int64)
        sv = np.clip(v + np.rint(lat_v), 0, H - 1).astype(np.int64)
        d = depth[f][sv, su]
        has = d != 0
        _, theta_all, _ = slope(depth[f], label[f], intr[f])
        theta_raw = theta_all[sv, su]
        with np.errstate(all='ignore'):
            # 2. axial noise
            z = d.astype(np.float64) / factor
            theta = np.minimum(theta_raw, p['theta_max'])
            dz, rest = z - p['z0'], HALF_PI - theta
            sigma_z = (p['a0'] + p['a1'] * (dz * dz)) + ((p['a2'] / np.sqrt(z)) * (theta * theta)) / (rest * rest)
            zn = z + n_z * sigma_z
            # 3. dropout
            angle = has & (theta_raw > p['theta_drop'])
            chance = has & ~angle & (r0 < drop_below)
            # 4. disparity steps
            if p['disparity_step'] > 0.0:
                fb = fx * p['baseline']
                disp = (fb / zn) / p['disparity_step']
                k = np.rint(disp)
                step_ok = k >= 1.0
                zq = fb / (k * p['disparity_step'])
            else:
                disp, k, step_ok, zq = np.full((H, W), np.nan), np.full((H, W), np.nan), np.ones((H, W), bool), zn
            # 5. quantisation
            quant = zq * factor + 0.5
            du = np.floor(quant)
            kept = has & ~angle & ~chance & step_ok & (du >= 1.0) & (du <= 65535.0)
        lost = has & ~angle & ~chance & ~kept
        counts[f] = [(depth[f] != 0).sum(), angle.sum(), chance.sum(), lost.sum()]
        vals = dict(depth=np.where(kept, np.where(kept, du, 0.0), 0.0).astype(np.uint16), label=label[f][sv, su],
                    z_noisy=np.where(has & np.isfinite(zn), zn, 0.0), lat_u=lat_u, lat_v=lat_v, src_u=su, src_v=sv, has=has,
                    theta=theta_raw, disp=disp, k=k, quant=quant)
        for key in keys:
            out[key].append(vals[key])
    out = {k: np.stack(x) for k, x in out.items()}
    out['counts'] = counts
    return out


def _to_half(x):
    """|x - the nearest half-integer|."""
    return np.abs((x - np.floor(x)) - 0.5)


def unsettled(r64, params, margin):
    """The pixels of apply(..., dtype=float64)'s result at which a decision lies within `margin` of its point: the
    lateral offsets against a half-integer (every pixel); theta against theta_drop, the disparity against a half-integer
    and z'' factor + 0.5 against an integer (pixels whose source has depth; a nan is far from everything)."""
    with np.errstate(all='ignore'):
        lat = (_to_half(r64['lat_u']) < margin) | (_to_half(r64['lat_v']) < margin)
        ang = np.abs(r64['theta'] - np.float64(params['theta_drop'])) < margin
        dsp = _to_half(r64['disp']) < margin
        qnt = np.abs(r64['quant'] - np.rint(r64['quant'])) < margin
    return lat | (r64['has'] & (ang | dsp | qnt))


def decision_change(r32, r64):
    """The largest change between the float32 and the float64 normal2 in the four watched quantities, over the pixels
    at which both pick the same source (and, for z'' factor + 0.5, the same disparity step k): elsewhere the quantity
    belongs to another pixel or step and its change is not a rounding."""
    same = (r32['src_u'] == r64['src_u']) & (r32['src_v'] == r64['src_v'])
    both = same & r32['has']
    same_k = both & ((r32['k'] == r64['k']) | (np.isnan(r32['k']) & np.isnan(r64['k'])))
    worst = 0.0
    for key, mask in (('lat_u', same), ('lat_v', same), ('theta', both), ('disp', both), ('quant', same_k)):
        d = np.abs(r32[key] - r64[key])[mask]
        d = d[np.isfinite(d)]
        if d.size:
            worst = max(worst, float(d.max()))
    return worst


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------
def plane_mesh(half=1.0):
    """A square of two triangles in the plane z = 0, side 2 * half."""
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def scenes():
    """name -> (meshes, frames, intrinsics [F,5], H, W): a sphere in front of a tilted plane at 37 x 70 (one frame, a
    partial last wave, every border clamp) and three frames of 48 x 64 with their own cameras, tilts and a sphere in one."""
    ico = MR.icosphere(2)
    meshes = [ico, plane_mesh()]
    P = RR.pose_matrix
    a = ([[(1, 1, P([0.5, 0.3, 0.0], [0.0, 0.0, 1.1])), (0, 2, _scaled(P([0.2, 0.1, 0.3], [0.05, 0.02, 0.8]), 0.22))]],
         np.array([[62.08, 60.9, 34.6, 18.3, 1000.0]], np.float32), 37, 70)
    b = ([[(1, 3, P([0.0, 0.9, 0.1], [0.0, 0.0, 0.9]))],
          [(1, 1, P([-0.7, 0.2, 0.0], [0.0, 0.05, 0.7])), (0, 5, _scaled(P([1.0, 0.4, 0.2], [-0.1, 0.0, 0.55]), 0.12))],
          [(1, 2, P([0.1, -1.2, 0.3], [0.1, 0.0, 1.3]))]],
         np.array([[58.88, 59.1, 31.5, 23.7, 1000.0], [70.4, 66.25, 30.1, 25.7, 2000.0], [53.12, 52.6, 33.0, 22.0, 1000.0]],
                  np.float32), 48, 64)
    return {'sphere_37x70': (meshes,) + a, 'planes_48x64': (meshes,) + b}


def _scaled(T, s):
    T = np.array(T, np.float64)
    T[:3, :3] *= s
    return T


# (scene, stage, seed, first_frame) of every GPU comparison against the restatement
CASES = [(sc, st, 100 + 7 * i + j, (0, 1 << 33)[j]) for j, sc in enumerate(('sphere_37x70', 'planes_48x64'))
         for i, st in enumerate(('kinect1', 'lateral', 'axial', 'dropout', 'disparity'))]
MARGIN_FLOOR = 1e-6
UNSETTLED_CAP = 0.02
_cache = {}


def rendered(name):
    """The scene's frames by tests/render_reference.py (equal to cloudaae_render_frames bit for bit), computed once."""
    if name not in _cache:
        meshes, frames, intr, H, W = scenes()[name]
        r = RR.render(meshes, frames, intr, H, W)
        _cache[name] = (r['depth'], r['label'], intr)
    return _cache[name]


def case_results(case):
    """(float32 result, float64 result) of one case, computed once and left unchanged."""
    if case not in _cache:
        sc, st, seed, first = case
        depth, label, intr = rendered(sc)
        _cache[case] = tuple(apply(depth, label, intr, STAGES[st], seed, first, dt) for dt in (np.float32, np.float64))
    return _cache[case]


def measured_margin():
    """10 x the largest decision_change over CASES, floored at MARGIN_FLOOR."""
    if 'margin' not in _cache:
        _cache['margin'] = max(10.0 * max(decision_change(*case_results(c)) for c in CASES), MARGIN_FLOOR)
    return _cache['margin']


def slope_tolerance():
    """(normals, theta): 10 x the change that reversing the order of the restatement's sums makes over the scenes,
    floored at 4 ulp of fp32 at the quantity's largest magnitude (1 for a unit normal, pi / 2 for theta)."""
    if 'slope_tol' not in _cache:
        dn = dt = 0.0
        for name in scenes():
            depth, label, intr = rendered(name)
            for f in range(len(depth)):
                a, b = slope(depth[f], label[f], intr[f]), slope(depth[f], label[f], intr[f], reverse=True)
                dn, dt = max(dn, float(np.abs(a[0] - b[0]).max())), max(dt, float(np.abs(a[1] - b[1]).max()))
        _cache['slope_tol'] = (max(10.0 * dn, 4.0 * float(np.spacing(np.float32(1.0)))),
                               max(10.0 * dt, 4.0 * float(np.spacing(np.float32(HALF_PI)))))
    return _cache['slope_tol']
