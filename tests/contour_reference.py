"""NumPy float64 restatement of DESIGN.md, "Contours": the occluding-edge masks of a depth image, the nearest observed edge
of every window pixel, the contour pairs, their two rows each and the 28 sums (with the sums of |terms|), the combined solve,
and the loop and the tracker of track_reference with the contour term added.  Written from the definition; everything that
"Tracking" defines (the back-projection, the LDL^T solve, x -> U, the product U T, the windows, the score) is
track_reference's and is not restated here.

Why two passes give the nearest edge.  The key of a candidate (i, j) is (i i + j j, j, i), compared lexicographically, among
the candidates inside the disc i i + j j <= R R.  Within one row j the first two entries of the key grow with |i|, so the
best candidate of the row is the edge pixel of smallest |i|, the one at -|i| when both sides have one; and if that one lies
outside the disc every other candidate of the row does too.  Two candidates of different rows never have to be told apart
by i, because j comes before it.  So "per row the nearest edge by (|i|, i), then over the rows the smallest (i i + j j, j)
of those inside the disc" is the same choice -- which is how the kernel finds it.  nearest() below does not: it walks all
offsets of the disc in key order and keeps the first that is an edge."""
import numpy as np

import detect_reference as DR
import render_reference as R
import track_reference as TR

V = TR.V
SUMS = TR.SUMS
RADIUS, STEP, WEIGHT = 16, 0.02, 1.0 / 16.0              # the defaults of utils/track.py: choices ("Contours")
DEFAULTS = dict(radius=RADIUS, step=STEP, weight=WEIGHT)
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # bits 0..3: (x-1, y), (x+1, y), (x, y-1), (x, y+1)


# ---- edges ------------------------------------------------------------------------------------------------------------------
def edge_masks(image, step):
    """image [H,W] uint16 -> [H,W] uint8: bit k of a pixel with z != 0 is set when neighbour k lies inside the image and has
    z_nb = 0 or z_nb - z > step, in integers; a pixel with z = 0 has mask 0."""
    z = np.asarray(image).astype(np.int64)
    H, W = z.shape
    zp = np.full((H + 2, W + 2), -1, np.int64)           # -1: no pixel of the image
    zp[1:-1, 1:-1] = z
    m = np.zeros((H, W), np.uint8)
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        nb = zp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        m |= (((nb >= 0) & ((nb == 0) | (nb - z > int(step)))).astype(np.uint8) << k).astype(np.uint8)
    m[z == 0] = 0
    return m


def disc_offsets(radius):
    """The offsets (i, j) with i i + j j <= R R in the order of the key (i i + j j, j, i)."""
    r = int(radius)
    o = [(i * i + j * j, j, i) for j in range(-r, r + 1) for i in range(-r, r + 1) if i * i + j * j <= r * r]
    return [(i, j) for _, j, i in sorted(o)]


def nearest(mask, origin, wh, ww, radius):
    """mask [H,W] uint8: the frame's edge masks -> [wh,ww] int32: -1, or (mask_obs << 16) | ((j + R) << 8) | (i + R) of the
    nearest observed edge (u0 + x + i, v0 + y + j) of window pixel (x, y)."""
    r = int(radius)
    u0, v0 = int(origin[0]), int(origin[1])
    m = TR.cut(mask, u0 - r, v0 - r, wh + 2 * r, ww + 2 * r).astype(np.int32)      # 0 where the frame has no pixel
    out = np.full((wh, ww), -1, np.int32)
    for i, j in disc_offsets(r):
        c = m[r + j:r + j + wh, r + i:r + i + ww]
        take = (out < 0) & (c != 0)
        out[take] = ((c << 16) | ((j + r) << 8) | (i + r))[take]
    return out


def edge_nearest(depth_test, frame_of, origin, wh, ww, step, radius):
    """cloudaae_depth_edge_nearest -> nearest [B,wh,ww] int32; a sample whose frame_of lies outside [0, F) is all -1."""
    dt = np.asarray(depth_test)
    assert dt.dtype == np.uint16
    B = len(frame_of)
    out = np.full((B, wh, ww), -1, np.int32)
    masks = {}
    for b in range(B):
        fr, st = int(frame_of[b]), int(step[b])
        if 0 <= fr < len(dt):
            if (fr, st) not in masks:
                masks[fr, st] = edge_masks(dt[fr], st)
            out[b] = nearest(masks[fr, st], origin[b], wh, ww, radius)
    return out


# ---- pairs, rows and sums ---------------------------------------------------------------------------------------------------
def pairs(frame, origin, hyp, gate, step, radius, near):
    """One sample -> dict(pair [wh,ww] bool, i, j [wh,ww] int64: the offset of the nearest observed edge, mask_hyp)."""
    r = int(radius)
    H, W = frame.shape
    wh, ww = hyp.shape
    d = np.asarray(hyp).astype(np.int64)
    mh = edge_masks(hyp, step).astype(np.int64)          # "inside the image" is the window here
    near = np.asarray(near, np.int64)
    has = near >= 0
    i, j, mo = (near & 255) - r, ((near >> 8) & 255) - r, near >> 16
    y, x = np.mgrid[0:wh, 0:ww]
    u, v = int(origin[0]) + x + i, int(origin[1]) + y + j
    inside = has & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    t = np.where(inside, np.asarray(frame).astype(np.int64)[np.clip(v, 0, H - 1), np.clip(u, 0, W - 1)], 0)
    pair = (d != 0) & (mh != 0) & inside & (np.abs(d - t) <= int(gate)) & (mh == mo)
    return dict(pair=pair, i=np.where(has, i, 0), j=np.where(has, j, 0), mask_hyp=mh)


def rows_of(pr, hyp, row):
    """The rows of the pairs in pixel order, the u row before the v row -> (r [n], J [n,6])."""
    fx, fy = np.float64(np.float32(row[0])), np.float64(np.float32(row[1]))
    db = np.zeros((hyp.shape[0] + 2, hyp.shape[1] + 2), np.int64)
    db[1:-1, 1:-1] = hyp
    sel = pr['pair'].reshape(-1)
    p = TR.backproject(db, row)[1:-1, 1:-1].reshape(-1, 3)[sel]
    i, j = pr['i'].reshape(-1)[sel].astype(np.float64), pr['j'].reshape(-1)[sel].astype(np.float64)
    n = len(p)
    res, g = np.zeros((n, 2)), np.zeros((n, 2, 3))
    if n:
        dm = p[:, 2]
        res[:, 0], res[:, 1] = ((-i) * dm) / fx, ((-j) * dm) / fy
        g[:, 0, 0], g[:, 0, 2] = 1.0, -(p[:, 0] / p[:, 2])
        g[:, 1, 1], g[:, 1, 2] = 1.0, -(p[:, 1] / p[:, 2])
    res, g, p = res.reshape(-1), g.reshape(-1, 3), np.repeat(p, 2, axis=0)
    a = np.stack([p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1], p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2],
                  p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]], axis=1)
    return res, np.concatenate([a, g], axis=1)


def sums_of(r, J):
    """-> (sums [28], abs_sums [28]): the sums over the rows in order and the sums of |terms|."""
    if len(r) == 0:
        return np.zeros(SUMS), np.zeros(SUMS)
    terms = [r * r] + [J[:, g] * J[:, c] for g in range(6) for c in range(g, 6)] + [J[:, g] * r for g in range(6)]
    terms = np.stack(terms, axis=1)
    return np.cumsum(terms, axis=0)[-1], np.abs(terms).sum(axis=0)


def contour_sums(depth_test, frame_of, origin, depth_hyp, intr_win, gate, step, radius, near):
    """cloudaae_depth_contour_sums -> dict(n_rows [B] int32, sums, abs_sums [B,28])."""
    dt, dh = np.asarray(depth_test), np.asarray(depth_hyp)
    assert dt.dtype == np.uint16 and dh.dtype == np.uint16
    B = len(dh)
    out = dict(n_rows=np.zeros(B, np.int32), sums=np.zeros((B, SUMS)), abs_sums=np.zeros((B, SUMS)))
    for b in range(B):
        fr = int(frame_of[b])
        if fr < 0 or fr >= len(dt):
            continue
        pr = pairs(dt[fr], origin[b], dh[b], gate[b], step[b], radius, near[b])
        r, J = rows_of(pr, dh[b], intr_win[b])
        out['n_rows'][b] = len(r)
        out['sums'][b], out['abs_sums'][b] = sums_of(r, J)
    return out


# ---- the combined step ------------------------------------------------------------------------------------------------------
def solve_sums(plane_sums, n_pairs, plane_status, contour, n_rows, weight, pose_in):
    """cloudaae_depth_align_solve -> dict(sums [B,28]: plane + w contour, x [B,6], status [B] int32, pose_out [B,4,4])."""
    B = len(n_pairs)
    pose_in = np.asarray(pose_in, np.float64).reshape(B, 4, 4)
    w = np.float64(weight)
    out = dict(sums=np.asarray(plane_sums, np.float64) + w * np.asarray(contour, np.float64), x=np.zeros((B, 6)),
               status=np.zeros(B, np.int32), pose_out=pose_in.copy())
    for b in range(B):
        if int(plane_status[b]) == 4:
            out['status'][b] = 4
        elif int(n_pairs[b]) + int(n_rows[b]) < 6:
            out['status'][b] = 1
        else:
            out['status'][b], out['x'][b] = TR.solve(out['sums'][b])
            if out['status'][b] == 0:
                out['pose_out'][b] = TR.compose(TR.update_matrix(out['x'][b]), pose_in[b])
    return out


def step(depth_test, frame_of, origin, depth_hyp, intr_win, gate, jump, cos_min, pose_in, step, radius, weight, near=None):
    """One step with the contour term: the plane step, the contour sums and the combined solve -> dict(plane, contour,
    nearest, x, status, pose_out, n_pairs, n_rows)."""
    wh, ww = np.asarray(depth_hyp).shape[1:]
    if near is None:
        near = edge_nearest(depth_test, frame_of, origin, wh, ww, step, radius)
    plane = TR.step(depth_test, frame_of, origin, depth_hyp, intr_win, gate, jump, cos_min, pose_in)
    con = contour_sums(depth_test, frame_of, origin, depth_hyp, intr_win, gate, step, radius, near)
    s = solve_sums(plane['sums'], plane['n_pairs'], plane['status'], con['sums'], con['n_rows'], weight, pose_in)
    return dict(s, plane=plane, contour=con, nearest=near, n_pairs=plane['n_pairs'], n_rows=con['n_rows'])


# ---- the loop and the tracker -----------------------------------------------------------------------------------------------
def align(depth, intrinsics, meshes, mesh_of, frame_of, poses, iterations=4, gate=0.03, jump=0.005, cos_min=0.8, margin=0.5,
          window=None, contour=DEFAULTS):
    """track_reference.align with the contour term: one nearest map per call, the combined step per iteration."""
    c = dict(DEFAULTS, **(contour if isinstance(contour, dict) else {}))
    ref = TR.align(depth, intrinsics, meshes, mesh_of, frame_of, poses, iterations=0, gate=gate, jump=jump, cos_min=cos_min,
                   margin=margin, window=window)
    depth = np.asarray(depth)
    J = len(ref['rows'])
    factor = ref['rows'][:, 4].astype(np.float64)
    gu, ju, su = (V.tau_units(np.broadcast_to(v, (J,)), factor) for v in (gate, jump, c['step']))
    near = edge_nearest(depth, ref['frame_of'], ref['origin'], ref['wh'], ref['ww'], su, c['radius'])
    traj, n_pairs, n_rows, status = [ref['poses'][0]], [], [], []
    for _ in range(int(iterations)):
        hyp = TR.render_windows(meshes, mesh_of, traj[-1], ref['rows'], ref['wh'], ref['ww'])
        r = step(depth, ref['frame_of'], ref['origin'], hyp, ref['rows'], gu, ju, cos_min, traj[-1], su, c['radius'], c['weight'],
                 near)
        traj.append(r['pose_out'])
        n_pairs.append(r['n_pairs'])
        n_rows.append(r['n_rows'])
        status.append(r['status'])
    return dict(ref, poses=np.array(traj), n_pairs=np.array(n_pairs).reshape(-1, J), n_rows=np.array(n_rows).reshape(-1, J),
                status=np.array(status).reshape(-1, J), nearest=near)


def track(depth, intrinsics, meshes, mesh_of, init_poses, motion='constant', min_score=(1, 2), tau=0.01, **kw):
    """track_reference.track (without on_lost) on align() above; also status_steps [F,iterations,J]."""
    depth = np.asarray(depth)
    F, J = len(depth), len(mesh_of)
    intr = np.broadcast_to(np.asarray(intrinsics, np.float32).reshape(-1, 5), (F, 5))
    out = dict(poses=np.zeros((F, J, 4, 4)), num=np.zeros((F, J), np.int64), den=np.ones((F, J), np.int64),
               n_pairs=np.zeros((F, J), np.int32), status=np.zeros((F, J), np.int32), lost=np.zeros((F, J), bool), status_steps=[])
    last = np.asarray(init_poses, np.float64).reshape(J, 4, 4).copy()
    before = [None] * J
    for f in range(F):
        start = np.array([TR.predict(last[j], before[j], motion) for j in range(J)])
        a = align(depth, intr, meshes, mesh_of, [f] * J, start, **kw)
        num, den, _ = TR.score(depth, intr, meshes, mesh_of, a['frame_of'], a['poses'][-1], a['origin'], a['wh'], a['ww'], tau)
        for j in range(J):
            out['lost'][f, j] = not a['ok'][j] or TR.is_lost(num[j], den[j], min_score)
            if out['lost'][f, j]:
                before[j] = None
            else:
                before[j], last[j] = last[j].copy(), a['poses'][-1][j]
        out['poses'][f], out['num'][f], out['den'][f] = last, num, den
        out['n_pairs'][f], out['status'][f] = a['n_pairs'][-1], a['status'][-1]
        out['status_steps'].append(a['status'])
    out['status_steps'] = np.array(out['status_steps'])
    return out


# ---- the scene: one object at a time on the table of track_reference --------------------------------------------------------
PRISM, PLATE, CUBE = 0, 1, TR.CUBE
PLACE = {PRISM: (-0.24, 0.02, 0.02, [0.0, 0.0, 0.4]), PLATE: (0.0, 0.05, 0.06, [np.pi / 2, 0.0, 0.0])}
_cache = {}


def object_pose(obj, f, motion):
    """The cube as track_reference moves it; the L prism lying flat and the standing plate slide along the table's x and turn
    about its normal (the motions of profiles/notes_track.md)."""
    if obj == CUBE:
        return TR.cube_pose(f, motion)
    metres, degrees, _, _, from_rest = motion
    x, y, h, rot = PLACE[obj]
    s = max(f - 0.5, 0.0) if from_rest else float(f)
    turn = R.pose_matrix([0.0, 0.0, np.radians(degrees) * s], [0.0, 0.0, 0.0])
    return TR.TABLE_POSE @ R.pose_matrix([0.0, 0.0, 0.0], [x + metres * s, y, h]) @ turn @ R.pose_matrix(rot, [0.0, 0.0, 0.0])


def frames(obj, motion, n=TR.FRAMES):
    """depth [n,H,W] uint16 of the table and the moving object, and the object's true poses [n,4,4]."""
    key = ('frames', obj, motion, n)
    if key not in _cache:
        truth = np.array([object_pose(obj, f, motion) for f in range(n)])
        fr = [[(TR.TABLE, 1, TR.TABLE_POSE), (obj, 2, truth[f])] for f in range(n)]
        _cache[key] = (R.render(DR.scene_meshes(), fr, np.tile(TR.SCENE_INTR, (n, 1)), TR.SCENE_H, TR.SCENE_W)['depth'], truth)
    return _cache[key]


def sequence(obj, motion, start, contour=True):
    """The object tracked over the six frames from its true first pose, with the contour term at its defaults or, with contour
    = False, by track_reference alone (cached) -> (result, truth, max |T - T_true| per frame)."""
    key = ('sequence', obj, motion, start, bool(contour))
    if key not in _cache:
        depth, truth = frames(obj, motion)
        run = track if contour else TR.track
        r = run(depth, TR.SCENE_INTR, DR.scene_meshes(), [obj], truth[:1], motion=start)
        _cache[key] = (r, truth, [TR.pose_error(r['poses'][f, 0], truth[f]) for f in range(len(truth))])
    return _cache[key]


# ---- small inputs the host and the GPU tests share --------------------------------------------------------------------------
def brute_nearest(mask, origin, wh, ww, radius):
    """nearest() by sorting ALL edge pixels of the frame by the key, for every window pixel."""
    r = int(radius)
    vs, us = np.nonzero(mask)
    out = np.full((wh, ww), -1, np.int32)
    for y in range(wh):
        for x in range(ww):
            best = None
            for u, v in zip(us.tolist(), vs.tolist()):
                i, j = u - (int(origin[0]) + x), v - (int(origin[1]) + y)
                if i * i + j * j <= r * r and (best is None or (i * i + j * j, j, i) < best[0]):
                    best = ((i * i + j * j, j, i), (int(mask[v, u]) << 16) | ((j + r) << 8) | (i + r))
            if best is not None:
                out[y, x] = best[1]
    return out


def dots(H, W, points, z=8000):
    """A frame [H,W] uint16 of zeros with single pixels of depth z at the listed (u, v): each is an edge pixel."""
    f = np.zeros((H, W), np.uint16)
    for u, v in points:
        f[v, u] = z
    return f


def rectangle_pair(k=3, d0=8000, top=3, bottom=20, left=8, right=13):
    """The hand anchor: a fronto-parallel rectangle (window rows top..bottom, columns left..right) at d0 units over zero
    background in a window of 24 x 32 at (2, 1) of a frame of 28 x 40, against the same rectangle k pixels further right in
    the frame -> the arguments of contour_sums() without `near` (B = 1)."""
    hyp, frame = np.zeros((1, 24, 32), np.uint16), np.zeros((1, 28, 40), np.uint16)
    hyp[0, top:bottom + 1, left:right + 1] = d0
    frame[0, 1 + top:1 + bottom + 1, 2 + left + k:2 + right + k + 1] = d0
    rows = np.array([[500.0, 480.0, 15.25, 11.75, 10000.0]], np.float32)
    return dict(depth_test=frame, frame_of=np.array([0], np.int32), origin=np.array([[2, 1]], np.int32), depth_hyp=hyp,
                intr_win=rows, gate=np.array([10], np.int32), step=np.array([200], np.int32))
