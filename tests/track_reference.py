"""NumPy float64 restatement of DESIGN.md, "Tracking": the slope of an image at a pixel, the pairs, the 28 sums (and the
sum of |terms| of each, which bounds what two orders of summation may differ by), the LDL^T solve, the step, the windows of
posed bounding boxes, the loop and the lost-track score.  Written from the definition: whole windows at once on arrays that
carry a border of one pixel, the sums as running sums in pixel order.  The hypotheses are rendered by render_reference.render
with the window's shifted principal point, the counts are detect_reference.fit_counts_window's."""
import numpy as np

import detect_reference as DR
import pose_verify_reference as V
import render_reference as R

Z_NEAR = 0.05
SUMS = 28                        # sum r r, A's upper triangle by rows (21), b (6)


# ---- the slope --------------------------------------------------------------------------------------------------------------
def bordered(image, u0, v0, wh, ww):
    """[wh + 2, ww + 2] int64: entry (y + 1, x + 1) is image pixel (u0 + x, v0 + y) for x in [-1, ww], y in [-1, wh], and 0
    where that is no pixel of the image."""
    H, W = image.shape
    v = v0 + np.arange(-1, wh + 1, dtype=np.int64)
    u = u0 + np.arange(-1, ww + 1, dtype=np.int64)
    inside = ((v >= 0) & (v < H))[:, None] & ((u >= 0) & (u < W))[None, :]
    vals = np.asarray(image)[np.clip(v, 0, H - 1)[:, None], np.clip(u, 0, W - 1)[None, :]].astype(np.int64)
    return np.where(inside, vals, 0)


def backproject(z, row):
    """z [h,w] int64 whose entry (i, j) is WINDOW pixel (x, y) = (j - 1, i - 1) -> P [h,w,3]: (((x - cxw) dm) / fx, ((y -
    cyw) dm) / fy, dm), dm = z / factor_depth."""
    fx, fy, cx, cy, factor = (np.float64(np.float32(k)) for k in np.asarray(row).reshape(-1)[:5])
    h, w = z.shape
    y, x = np.mgrid[-1:h - 1, -1:w - 1]
    dm = z.astype(np.float64) / factor
    return np.stack([((x.astype(np.float64) - cx) * dm) / fx, ((y.astype(np.float64) - cy) * dm) / fy, dm], axis=-1)


def unit_normals(zb, row, jump):
    """The unsigned unit normal at every window pixel of a bordered image zb [wh+2,ww+2] -> (normal [wh,ww,3] float64,
    zeros where there is none; ok [wh,ww] bool: the pixel has depth and is not flat)."""
    P = backproject(zb, row)
    c, Pc = zb[1:-1, 1:-1], P[1:-1, 1:-1]
    g, has = [], []
    for lo, hi in (((slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))),
                   ((slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1)))):
        vlo = (zb[lo] != 0) & (np.abs(zb[lo] - c) <= int(jump))
        vhi = (zb[hi] != 0) & (np.abs(zb[hi] - c) <= int(jump))
        g.append(np.where(vhi[..., None], P[hi], Pc) - np.where(vlo[..., None], P[lo], Pc))
        has.append(vlo | vhi)
    gx, gy = g
    n = np.stack([gx[..., 1] * gy[..., 2] - gx[..., 2] * gy[..., 1], gx[..., 2] * gy[..., 0] - gx[..., 0] * gy[..., 2],
                  gx[..., 0] * gy[..., 1] - gx[..., 1] * gy[..., 0]], axis=-1)
    with np.errstate(all='ignore'):
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        ok = (c != 0) & has[0] & has[1] & (nn > 0.0) & np.isfinite(nn)
        unit = np.where(ok[..., None], n / np.sqrt(np.where(ok, nn, 1.0))[..., None], 0.0)
    return unit, ok


# ---- pairs and sums ---------------------------------------------------------------------------------------------------------
def pairs(frame, origin, hyp, row, gate, jump, cos_min):
    """One sample.  frame [H,W] uint16, origin (u0, v0), hyp [wh,ww] uint16, row [5] float32 -> dict(pair [wh,ww] bool, p, q,
    n, m [wh,ww,3], dot [wh,ww])."""
    wh, ww = hyp.shape
    u0, v0 = int(origin[0]), int(origin[1])
    db = np.zeros((wh + 2, ww + 2), np.int64)
    db[1:-1, 1:-1] = hyp
    tb = bordered(frame, u0, v0, wh, ww)
    d, t = db[1:-1, 1:-1], tb[1:-1, 1:-1]
    pair = (d != 0) & (t != 0) & (np.abs(d - t) <= int(gate))
    n, n_ok = unit_normals(db, row, jump)
    pair &= n_ok
    m, dot = np.zeros_like(n), np.zeros(d.shape)
    if cos_min > 0.0:
        m, m_ok = unit_normals(tb, row, jump)
        dot = np.abs((n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2])
        pair &= m_ok & (dot >= cos_min)
    return dict(pair=pair, p=backproject(db, row)[1:-1, 1:-1], q=backproject(tb, row)[1:-1, 1:-1], n=n, m=m, dot=dot)


def sums_of(pr):
    """-> (n_pairs, sums [28], abs_sums [28]): the sums over the pairs in pixel order and the sums of |terms|."""
    sel = pr['pair'].reshape(-1)
    p, q, n = (pr[k].reshape(-1, 3)[sel] for k in ('p', 'q', 'n'))
    if len(p) == 0:
        return 0, np.zeros(SUMS), np.zeros(SUMS)
    e = p - q
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    a = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
    J = np.concatenate([a, n], axis=1)
    terms = [r * r] + [J[:, g] * J[:, c] for g in range(6) for c in range(g, 6)] + [J[:, g] * r for g in range(6)]
    terms = np.stack(terms, axis=1)
    return len(p), np.cumsum(terms, axis=0)[-1], np.abs(terms).sum(axis=0)


# ---- the solve and the step -------------------------------------------------------------------------------------------------
def solve(sums):
    """A x = -b by LDL^T without pivoting -> (status, x [6]): 0, or 2 for a pivot that is not a finite number > 0, 3 for a
    solution that is not finite (x zeros then)."""
    A = np.zeros((6, 6))
    e = 1
    for g in range(6):
        for c in range(g, 6):
            A[g, c] = A[c, g] = sums[e]
            e += 1
    b = sums[22:28]
    L, d = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all='ignore'):
        for j in range(6):
            dj = A[j, j]
            for k in range(j):
                dj = dj - (L[j, k] * L[j, k]) * d[k]
            if not (dj > 0.0) or not np.isfinite(dj):
                return 2, np.zeros(6)
            d[j] = dj
            for i in range(j + 1, 6):
                v = A[i, j]
                for k in range(j):
                    v = v - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = v / dj
        x = np.zeros(6)
        for i in range(6):
            v = -b[i]
            for k in range(i):
                v = v - L[i, k] * x[k]
            x[i] = v
        x = x / d
        for i in range(5, -1, -1):
            v = x[i]
            for k in range(i + 1, 6):
                v = v - L[k, i] * x[k]
            x[i] = v
    return (0, x) if np.all(np.isfinite(x)) else (3, np.zeros(6))


def update_matrix(x):
    """U = [Rz(gamma) Ry(beta) Rx(alpha) | t] for x = (alpha, beta, gamma, t)."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4)
    U[0, :3] = [cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa]
    U[1, :3] = [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa]
    U[2, :3] = [-sb, cb * sa, cb * ca]
    U[:3, 3] = x[3:]
    return U


def compose(U, T):
    """U T with the products of cloudaae_pose_compose; the last row is 0 0 0 1."""
    N = np.eye(4)
    for i in range(3):
        for c in range(3):
            N[i, c] = (U[i, 0] * T[0, c] + U[i, 1] * T[1, c]) + U[i, 2] * T[2, c]
        N[i, 3] = ((U[i, 0] * T[0, 3] + U[i, 1] * T[1, 3]) + U[i, 2] * T[2, 3]) + U[i, 3]
    return N


def step(depth_test, frame_of, origin, depth_hyp, intr_win, gate, jump, cos_min, pose_in):
    """cloudaae_depth_align_step -> dict(n_pairs [B] int32, sums, abs_sums [B,28], x [B,6], status [B] int32, pose_out
    [B,4,4])."""
    dt, dh = np.asarray(depth_test), np.asarray(depth_hyp)
    assert dt.dtype == np.uint16 and dh.dtype == np.uint16
    F, B = len(dt), len(dh)
    pose_in = np.asarray(pose_in, np.float64).reshape(B, 4, 4)
    out = dict(n_pairs=np.zeros(B, np.int32), sums=np.zeros((B, SUMS)), abs_sums=np.zeros((B, SUMS)), x=np.zeros((B, 6)),
               status=np.zeros(B, np.int32), pose_out=pose_in.copy())
    for b in range(B):
        fr = int(frame_of[b])
        if fr < 0 or fr >= F:
            out['status'][b] = 4
            continue
        pr = pairs(dt[fr], origin[b], dh[b], intr_win[b], gate[b], jump[b], float(cos_min))
        out['n_pairs'][b], out['sums'][b], out['abs_sums'][b] = sums_of(pr)
        if out['n_pairs'][b] < 6:
            out['status'][b] = 1
            continue
        out['status'][b], out['x'][b] = solve(out['sums'][b])
        if out['status'][b] == 0:
            out['pose_out'][b] = compose(update_matrix(out['x'][b]), pose_in[b])
    return out


# ---- windows of posed bounding boxes ----------------------------------------------------------------------------------------
def mesh_aabb(meshes):
    """[S,2,3] float64: the smallest and the largest vertex coordinates of every mesh."""
    return np.array([[np.asarray(m[0], np.float32).astype(np.float64).min(axis=0),
                      np.asarray(m[0], np.float32).astype(np.float64).max(axis=0)] for m in meshes])


def pose_windows(poses, aabb, intrinsics, H, W, margin=0.5, z_near=Z_NEAR):
    """poses [J,4,4], aabb [J,2,3] (each track's mesh), intrinsics [J,5] (each track's frame) -> (origin [J,2] int32, wh,
    ww, ok [J] bool).  The eight corners (x, y, z), each the low or the high coordinate, go through X = ((A0 x + A1 y) + A2
    z) + A3 (Y, Z alike) and u = (fx X) / Z + cx, v = (fy Y) / Z + cy; a track with a corner that has Z < z_near or a value
    that is not finite has no window; its box is (floor min u, floor min v, ceil max u, ceil max v) clipped to the frame, and
    an empty box is no window either.  Then the windows of "Detections" over the tracks that have one."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    J = len(poses)
    intr = np.broadcast_to(np.asarray(intrinsics, np.float32), (J, 5)).astype(np.float64)
    box, ok = np.zeros((J, 4), np.int64), np.zeros(J, bool)
    for j in range(J):
        A, lo_hi = poses[j], np.asarray(aabb[j], np.float64)
        us, vs, good = [], [], True
        for cx in (0, 1):
            for cy in (0, 1):
                for cz in (0, 1):
                    x, y, z = lo_hi[cx, 0], lo_hi[cy, 1], lo_hi[cz, 2]
                    X = ((A[0, 0] * x + A[0, 1] * y) + A[0, 2] * z) + A[0, 3]
                    Y = ((A[1, 0] * x + A[1, 1] * y) + A[1, 2] * z) + A[1, 3]
                    Z = ((A[2, 0] * x + A[2, 1] * y) + A[2, 2] * z) + A[2, 3]
                    if not (Z >= z_near) or not np.isfinite(Z):
                        good = False
                        continue
                    us.append((intr[j, 0] * X) / Z + intr[j, 2])
                    vs.append((intr[j, 1] * Y) / Z + intr[j, 3])
        if not good or not np.all(np.isfinite(us + vs)):
            continue
        b = [max(int(np.clip(np.floor(min(us)), -1, W)), 0), max(int(np.clip(np.floor(min(vs)), -1, H)), 0),
             min(int(np.clip(np.ceil(max(us)), -1, W)), W - 1), min(int(np.clip(np.ceil(max(vs)), -1, H)), H - 1)]
        if b[0] <= b[2] and b[1] <= b[3]:
            box[j], ok[j] = b, True
    live = np.nonzero(ok)[0]
    packed = np.zeros((1, max(len(live), 1), 4), np.int64)
    packed[0, :len(live)] = box[live]
    o, wh, ww = DR.windows(packed, [len(live)], H, W, margin)
    origin = np.zeros((J, 2), np.int32)
    origin[live] = o[0, :len(live)]
    return origin, wh, ww, ok


def window_rows(intr, origin):
    """The windows' rows (fx, fy, cx - u0, cy - v0, factor_depth), the differences in float32."""
    rows = np.array(np.asarray(intr, np.float32), np.float32).reshape(-1, 5).copy()
    rows[:, 2] = rows[:, 2] - np.asarray(origin)[:, 0].astype(np.float32)
    rows[:, 3] = rows[:, 3] - np.asarray(origin)[:, 1].astype(np.float32)
    return rows


def render_windows(meshes, mesh_of, poses, rows, wh, ww):
    """Every track's object alone in its window -> depth_hyp [J,wh,ww] uint16."""
    frames = [[(int(mesh_of[j]), 1, np.asarray(poses[j], np.float64))] for j in range(len(mesh_of))]
    return R.render(meshes, frames, rows, wh, ww)['depth']


# ---- the loop and the score -------------------------------------------------------------------------------------------------
def align(depth, intrinsics, meshes, mesh_of, frame_of, poses, iterations=4, gate=0.03, jump=0.005, cos_min=0.8, margin=0.5,
          window=None):
    """align_poses -> dict(poses [iterations+1,J,4,4]: before every step and after the last; n_pairs, status
    [iterations,J]; origin, wh, ww, ok)."""
    depth = np.asarray(depth)
    H, W = depth.shape[1:]
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    J = len(poses)
    frame_of = np.asarray(frame_of, np.int64).reshape(J)
    intr = np.asarray(intrinsics, np.float32).reshape(-1, 5)[np.clip(frame_of, 0, len(depth) - 1)]
    if window is None:
        origin, wh, ww, ok = pose_windows(poses, mesh_aabb(meshes)[np.asarray(mesh_of)], intr, H, W, margin)
    else:
        origin, wh, ww = window
        ok = np.ones(J, bool)
    rows = window_rows(intr, origin)
    factor = intr[:, 4].astype(np.float64)
    gu, ju = V.tau_units(np.broadcast_to(gate, (J,)), factor), V.tau_units(np.broadcast_to(jump, (J,)), factor)
    fo = np.where(ok, frame_of, -1)
    traj, n_pairs, status = [poses.copy()], [], []
    for _ in range(int(iterations)):
        hyp = render_windows(meshes, mesh_of, traj[-1], rows, wh, ww)
        r = step(depth, fo, origin, hyp, rows, gu, ju, cos_min, traj[-1])
        traj.append(r['pose_out'])
        n_pairs.append(r['n_pairs'])
        status.append(r['status'])
    return dict(poses=np.array(traj), n_pairs=np.array(n_pairs).reshape(-1, J), status=np.array(status).reshape(-1, J),
                origin=origin, wh=wh, ww=ww, ok=ok, rows=rows, frame_of=fo)


def score(depth, intrinsics, meshes, mesh_of, frame_of, poses, origin, wh, ww, tau=0.01):
    """The silhouette rule's (num, den) [J] of every track's pose rendered into its window: num = consistent, den =
    consistent + in_front + behind; 0 / 1 where den is 0 or the track has no frame."""
    J = len(mesh_of)
    frame_of = np.asarray(frame_of, np.int64)
    intr = np.asarray(intrinsics, np.float32).reshape(-1, 5)[np.clip(frame_of, 0, len(depth) - 1)]
    hyp = render_windows(meshes, mesh_of, poses, window_rows(intr, origin), wh, ww)
    tu = V.tau_units(np.broadcast_to(tau, (J,)), intr[:, 4].astype(np.float64))
    counts, _, _ = DR.fit_counts_window(depth, None, frame_of, None, origin, wh, ww, hyp[:, None], tu)
    num, den = np.zeros(J, np.int64), np.ones(J, np.int64)
    for j in range(J):
        num[j], den[j] = V.fraction(counts[j, 0], 0, True, 1)
    return num, den, counts[:, 0]


def invert(T):
    """(R^T, -R^T t) of a rigid T, the translation as -((R0i t0 + R1i t1) + R2i t2)."""
    N = np.eye(4)
    for i in range(3):
        N[i, :3] = T[:3, i]
        N[i, 3] = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
    return N


def predict(last, before, motion):
    """The start of a frame: the last pose, or with 'velocity' (T_{f-1} T_{f-2}^-1) T_{f-1} once two poses exist."""
    if motion == 'velocity' and before is not None:
        return compose(compose(last, invert(before)), last)
    return last.copy()


def is_lost(num, den, min_score):
    return int(num) * int(min_score[1]) < int(min_score[0]) * int(den)


def track(depth, intrinsics, meshes, mesh_of, init_poses, motion='constant', min_score=(1, 2), tau=0.01, on_lost=None, **kw):
    """track_objects -> dict(poses [F,J,4,4], num, den [F,J] int64, n_pairs, status [F,J] of the last step, lost [F,J])."""
    depth = np.asarray(depth)
    F, J = len(depth), len(mesh_of)
    intr = np.broadcast_to(np.asarray(intrinsics, np.float32).reshape(-1, 5), (F, 5))
    out = dict(poses=np.zeros((F, J, 4, 4)), num=np.zeros((F, J), np.int64), den=np.ones((F, J), np.int64),
               n_pairs=np.zeros((F, J), np.int32), status=np.zeros((F, J), np.int32), lost=np.zeros((F, J), bool))
    last = np.asarray(init_poses, np.float64).reshape(J, 4, 4).copy()
    before = [None] * J

    def attempt(f, idx, start):
        sub = [mesh_of[j] for j in idx]
        a = align(depth, intr, meshes, sub, [f] * len(idx), start, **kw)
        num, den, _ = score(depth, intr, meshes, sub, a['frame_of'], a['poses'][-1], a['origin'], a['wh'], a['ww'], tau)
        lost = np.array([not a['ok'][i] or is_lost(num[i], den[i], min_score) for i in range(len(idx))])
        return a, num, den, lost

    for f in range(F):
        idx = list(range(J))
        start = np.array([predict(last[j], before[j], motion) for j in idx])
        a, num, den, lost = attempt(f, idx, start)
        final = a['poses'][-1].copy()
        n_pairs, status = a['n_pairs'][-1].copy(), a['status'][-1].copy()
        if lost.any() and on_lost is not None:
            again = [j for j in idx if lost[j]]
            given = on_lost(f, again)
            if given is not None:
                a2, num2, den2, lost2 = attempt(f, again, np.asarray(given, np.float64).reshape(len(again), 4, 4))
                for i, j in enumerate(again):
                    final[j], num[j], den[j], lost[j] = a2['poses'][-1][i], num2[i], den2[i], lost2[i]
                    n_pairs[j], status[j] = a2['n_pairs'][-1][i], a2['status'][-1][i]
        for j in idx:
            if not lost[j]:
                before[j], last[j] = last[j].copy(), final[j]
            else:
                before[j] = None                       # a lost track starts again from its last good pose, at rest
        out['poses'][f], out['num'][f], out['den'][f], out['lost'][f] = last, num, den, lost
        out['n_pairs'][f], out['status'][f] = n_pairs, status
    return out


# ---- the scene the host and the GPU tests share -----------------------------------------------------------------------------
SCENE_H, SCENE_W = 384, 512
SCENE_INTR = np.array([[600.0, 600.0, 255.5, 191.5, 10000.0]], np.float32)
CUBE, TABLE = 2, 4                                   # meshes of detect_reference.scene_meshes()
TABLE_POSE = R.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])
SLOW = (0.011, 2.0, 180.0, 0.23, False)            # metres and degrees per frame, direction on the table (degrees), x at
FAST = (0.022, -5.0, 135.0, 0.23, True)             # frame 0, and whether the first interval is half a step (a start from rest)
FRAMES = 6
_cache = {}


def pose_error(T, truth):
    return float(np.abs(np.asarray(T) - np.asarray(truth)).max())


def cube_pose(f, motion=SLOW):
    """The cube of "Detections" on its table after f frames of `motion`: it slides over the table and turns about the table's
    normal, s = f steps of (metres, degrees) -- or f - 1/2 (0 at f = 0) when the motion starts from rest."""
    step, degrees, direction, x0, from_rest = motion
    s = max(f - 0.5, 0.0) if from_rest else float(f)
    return DR._on_table(TABLE_POSE, x0 + step * s * np.cos(np.radians(direction)), -0.02 + step * s * np.sin(np.radians(direction)),
                        0.035, [0.0, 0.0, 0.7 + np.radians(degrees) * s])


def frames(motion=SLOW, n=FRAMES, without=()):
    """depth [n,H,W] uint16 of the table and the moving cube (not drawn in the frames listed in `without`), and the cube's
    true poses [n,4,4]."""
    key = ('frames', motion, n, tuple(without))
    if key not in _cache:
        meshes = DR.scene_meshes()
        truth = np.array([cube_pose(f, motion) for f in range(n)])
        fr = [[(TABLE, 1, TABLE_POSE)] + ([] if f in without else [(CUBE, 2, truth[f])]) for f in range(n)]
        _cache[key] = (R.render(meshes, fr, np.tile(SCENE_INTR, (n, 1)), SCENE_H, SCENE_W)['depth'], truth)
    return _cache[key]


def off_pose(T, degrees=2.0, metres=0.005):
    """T turned by `degrees` about the camera's (1, 1, 1) axis through the object's origin and moved by `metres` along
    (1, -1, 1) / sqrt 3."""
    axis = np.ones(3) / np.sqrt(3.0)
    N = T.copy()
    N[:3, :3] = R.pose_matrix(axis * np.radians(degrees), [0, 0, 0])[:3, :3] @ T[:3, :3]
    N[:3, 3] = T[:3, 3] + metres * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    return N


def sequence(motion, start):
    """track() of the cube over the six frames of `motion` from its true first pose (cached) -> (result, truth)."""
    key = ('sequence', motion, start)
    if key not in _cache:
        depth, truth = frames(motion)
        _cache[key] = (track(depth, SCENE_INTR, DR.scene_meshes(), [CUBE], truth[:1], motion=start), truth)
    return _cache[key]


def render_scene(cubes, table=True):
    """depth [n,H,W] uint16: the table (unless table is False) and, per frame, the cube under each of the listed poses
    (cached by the poses' bytes)."""
    key = ('render', table, tuple(tuple(np.asarray(c, np.float64).tobytes() for c in fr) for fr in cubes))
    if key not in _cache:
        fr = [([(TABLE, 1, TABLE_POSE)] if table else []) + [(CUBE, 2, np.asarray(c, np.float64)) for c in cs] for cs in cubes]
        _cache[key] = R.render(DR.scene_meshes(), fr, np.tile(SCENE_INTR, (len(fr), 1)), SCENE_H, SCENE_W)['depth']
    return _cache[key]


def lost_sequence():
    """Five frames: the slow motion for three frames, no cube in frame 3, the cube back at its place of frame 2 in frame 4
    -> (depth, the cube's poses [5,4,4], the one of frame 3 being where it was last seen)."""
    c = [cube_pose(f) for f in range(3)]
    return render_scene([[c[0]], [c[1]], [c[2]], [], [c[2]]]), np.array(c + [c[2], c[2]])


def moved_sequence():
    """Three frames: two of the slow motion, then the cube 13 cm and 24 degrees further on, beyond what a step can follow."""
    c = [cube_pose(0), cube_pose(1), cube_pose(12)]
    return render_scene([[x] for x in c]), np.array(c)


def at_pixel(T, u, v):
    """T moved parallel to the image plane so that its origin projects to pixel (u, v)."""
    fx, fy, cx, cy = (float(k) for k in SCENE_INTR[0, :4])
    N = np.array(T, np.float64)
    N[0, 3], N[1, 3] = (u - cx) * N[2, 3] / fx, (v - cy) * N[2, 3] / fy
    return N


# ---- the inputs of single steps the host and the GPU tests share ------------------------------------------------------------
def cut(image, u0, v0, wh, ww):
    """[wh,ww] uint16: window pixel (x, y) = image pixel (u0 + x, v0 + y), 0 outside the image."""
    return bordered(image, u0, v0, wh, ww)[1:-1, 1:-1].astype(np.uint16)


def plane_patch(k=50, side=8, d0=8000):
    """The hand anchor: a fronto-parallel square of side x side pixels at d0 units in a window of 12 x 16 at (3, 2) of a frame
    of 20 x 24, against the same square k units nearer.  -> the arguments of step() as a dict (B = 1), plus the square's
    window columns xs and rows ys."""
    hyp, frame = np.zeros((1, 12, 16), np.uint16), np.zeros((1, 20, 24), np.uint16)
    xs, ys = np.arange(4, 4 + side), np.arange(2, 2 + side)
    hyp[0, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = d0
    frame[0, 2 + ys[0]:2 + ys[-1] + 1, 3 + xs[0]:3 + xs[-1] + 1] = d0 - k
    rows = np.array([[500.0, 480.0, 9.25, 4.25, 10000.0]], np.float32)
    return dict(depth_test=frame, frame_of=np.array([0], np.int32), origin=np.array([[3, 2]], np.int32), depth_hyp=hyp,
                intr_win=rows, gate=np.array([k], np.int32), jump=np.array([10], np.int32), cos_min=0.8,
                pose_in=off_pose(np.eye(4), 7.0, 0.3)[None], xs=xs, ys=ys)


def step_cases(render):
    """[(name, arguments of step())]: windows cut from renderings of the off-pose cube -- `render(frames of [cube pose])` ->
    depth [n,H,W] uint16 of the cube alone, the renderer under test or render_reference -- against two frames: frame 0 shows
    the cube on its table where "Detections" has it, frame 1 one cube at the upper left and one at the lower right corner of the
    image and nothing else (down there the table would hide a cube at that depth)."""
    truth = cube_pose(0)
    corner = [at_pixel(truth, 14.0, 12.0), at_pixel(truth, SCENE_W - 16.0, SCENE_H - 14.0)]
    depth = np.concatenate([render_scene([[truth]]), render_scene([corner], table=False)])
    starts = [off_pose(truth), off_pose(corner[0]), off_pose(corner[1], -2.0, 0.004)]
    images = render([[s] for s in starts])
    vs, us = np.nonzero(images[0])
    cu, cv = int(us.min() + us.max()) // 2, int(vs.min() + vs.max()) // 2      # the middle of the cube's box in frame 0
    factor = float(SCENE_INTR[0, 4])
    gate, jump = int(V.tau_units(0.03, factor)), int(V.tau_units(0.005, factor))

    def sample(which, frame, u0, v0, wh, ww, hyp=None):
        o = np.array([u0, v0], np.int32)
        return dict(depth_hyp=cut(images[which], u0, v0, wh, ww) if hyp is None else hyp, frame_of=frame, origin=o,
                    intr_win=window_rows(SCENE_INTR, o[None])[0], pose_in=starts[which])

    def call(samples, cos_min=0.8):
        return dict(depth_test=depth, frame_of=np.array([s['frame_of'] for s in samples], np.int32),
                    origin=np.array([s['origin'] for s in samples], np.int32),
                    depth_hyp=np.array([s['depth_hyp'] for s in samples], np.uint16),
                    intr_win=np.array([s['intr_win'] for s in samples], np.float32),
                    gate=np.full(len(samples), gate, np.int32), jump=np.full(len(samples), jump, np.int32), cos_min=cos_min,
                    pose_in=np.array([s['pose_in'] for s in samples]))

    def centred(wh, ww):
        return sample(0, 0, cu - ww // 2, cv - wh // 2, wh, ww)

    out = [('%dx%d' % s, call([centred(*s)])) for s in ((23, 89), (32, 64), (3, 683), (33, 67), (64, 1), (160, 152))]
    out.append(('negative origin', call([sample(1, 1, -5, -7, 56, 64)])))
    out.append(('over the right and bottom edges', call([sample(2, 1, SCENE_W - 44, SCENE_H - 40, 56, 64)])))
    out.append(('cos_min 0', call([centred(33, 67)], cos_min=0.0)))
    batch = [centred(33, 67), sample(0, 0, cu - 50, cv - 20, 33, 67), sample(1, 1, -9, -3, 33, 67),
             sample(2, 1, SCENE_W - 50, SCENE_H - 28, 33, 67), dict(centred(33, 67), frame_of=-1), dict(centred(33, 67), frame_of=2),
             sample(0, 0, cu - 33, cv - 16, 33, 67, hyp=np.zeros((33, 67), np.uint16))]
    out.append(('seven over two frames', call(batch)))
    p = plane_patch()
    out.append(('plane patch', {k: p[k] for k in p if k not in ('xs', 'ys')}))
    return out


def reference_renderer(cubes):
    """step_cases' `render` on render_reference: the cube alone in whole frames."""
    fr = [[(CUBE, 1, np.asarray(c, np.float64)) for c in cs] for cs in cubes]
    return R.render(DR.scene_meshes(), fr, np.tile(SCENE_INTR, (len(fr), 1)), SCENE_H, SCENE_W)['depth']
