"""NumPy float64 restatement of DESIGN.md, "Scanning on the field": one Gauss-Newton step that aligns depth frames on the
signed distance field of a TSDF volume (cloudaae_tsdf_align_step), and the scanning loop built on it (scan_object with
align='sdf').  Written from the definition: the window's pixels at once, every value formed in float64 from exactly widened
inputs in the order the definition writes it (NumPy does not fuse a product into a sum); the sums are running sums in pixel
order and the solve is track_reference's LDL^T, so a step is expected to equal the kernel's up to the order of the sums.

The loop imports scan_reference's integrate, raycast, windows and counts unchanged.  The second half holds the fields, the
cases and the scenes that the host and the GPU tests share."""
import functools

import numpy as np

import detect_reference as DR
import fuse_reference as FR
import pose_verify_reference as V
import scan_reference as S
import track_reference as TR

QUANT = 4096.0
SUMS = 28


# ---- the rows --------------------------------------------------------------------------------------------------------------
def rows(state, vol_origin, voxel, min_count, front, frame, label, want, origin, wh, ww, row, pose):
    """The rows of one sample.  state [nz,ny,nx,4] int32; frame [H,W] uint16; label [H,W] uint8 with want (one int), or both
    None: the filter is off; origin (u0, v0); row [5] float32: the window's camera; pose [4,4]: model -> camera.
    -> dict(ok [wh,ww] bool, J [wh,ww,6], r [wh,ww], and what they were formed of: p, q, g [wh,ww,3], cell [wh,ww,3] int64,
    val [wh,ww], grad [wh,ww,3])."""
    state = np.asarray(state)
    nz, ny, nx, _ = state.shape
    dims = (nx, ny, nz)
    H, W = frame.shape
    u0, v0 = int(origin[0]), int(origin[1])
    fx, fy, cxw, cyw, factor = (np.float64(np.float32(k)) for k in np.asarray(row).reshape(-1)[:5])
    A = np.asarray(pose, np.float64).reshape(4, 4)
    s, front = np.float64(voxel), np.float64(front)
    y, x = np.mgrid[0:wh, 0:ww]
    u, v = u0 + x.astype(np.int64), v0 + y.astype(np.int64)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    uc, vc = np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)
    d = np.where(inside, np.asarray(frame)[vc, uc].astype(np.int64), 0)
    ok = d != 0
    if label is not None and want is not None and int(want) != 0:
        ok &= np.asarray(label)[vc, uc].astype(np.int64) == int(want)
    with np.errstate(all='ignore'):
        dm = d.astype(np.float64) / factor
        p = np.stack([((x.astype(np.float64) - cxw) * dm) / fx, ((y.astype(np.float64) - cyw) * dm) / fy, dm], axis=-1)
        e = [p[..., i] - A[i, 3] for i in range(3)]
        q = np.stack([(A[0, a] * e[0] + A[1, a] * e[1]) + A[2, a] * e[2] for a in range(3)], axis=-1)
        g = np.stack([(q[..., a] - np.float64(vol_origin[a])) / s - 0.5 for a in range(3)], axis=-1)
        for a in range(3):
            ok &= (g[..., a] >= 0.0) & (g[..., a] <= np.float64(dims[a] - 1))          # a NaN fails
        cell, frac = [], []
        for a in range(3):
            fl = np.floor(g[..., a])
            i = np.where(fl >= 0.0, np.where(fl <= np.float64(dims[a] - 2), fl, np.float64(dims[a] - 2)), 0.0)
            i = np.where(ok, i, 0.0)
            cell.append(i.astype(np.int64))
            frac.append(g[..., a] - i)
        values, known = FR.corner_values(state, min_count)
        values, known = values.reshape(-1), known.reshape(-1)
        c = []
        for corner in range(8):
            idx = ((cell[2] + (corner >> 2)) * ny + (cell[1] + ((corner >> 1) & 1))) * nx + (cell[0] + (corner & 1))
            c.append(values[idx])
            ok &= known[idx]
        f0, f1, f2 = frac
        c00, c10 = c[0] + (c[1] - c[0]) * f0, c[2] + (c[3] - c[2]) * f0
        c01, c11 = c[4] + (c[5] - c[4]) * f0, c[6] + (c[7] - c[6]) * f0
        c0, c1 = c00 + (c10 - c00) * f1, c01 + (c11 - c01) * f1
        val = c0 + (c1 - c0) * f2
        d00, d10, d01, d11 = c[1] - c[0], c[3] - c[2], c[5] - c[4], c[7] - c[6]
        gx0, gx1 = d00 + (d10 - d00) * f1, d01 + (d11 - d01) * f1
        e0, e1 = c10 - c00, c11 - c01
        grad = np.stack([gx0 + (gx1 - gx0) * f2, e0 + (e1 - e0) * f2, c1 - c0], axis=-1)
        gg = (grad[..., 0] * grad[..., 0] + grad[..., 1] * grad[..., 1]) + grad[..., 2] * grad[..., 2]
        ok &= ~(val >= QUANT) & (gg > 0.0) & np.isfinite(gg)
        r = (val / QUANT) * front
        scale = (front / QUANT) / s
        go = [grad[..., a] * scale for a in range(3)]
        n = [(A[i, 0] * go[0] + A[i, 1] * go[1]) + A[i, 2] * go[2] for i in range(3)]
        J = np.stack([-(p[..., 1] * n[2] - p[..., 2] * n[1]), -(p[..., 2] * n[0] - p[..., 0] * n[2]),
                      -(p[..., 0] * n[1] - p[..., 1] * n[0]), -n[0], -n[1], -n[2]], axis=-1)
    return dict(ok=ok, J=J, r=r, p=p, q=q, g=g, cell=np.stack(cell, axis=-1), val=val, grad=grad)


def sums_of(rw):
    """-> (n_pairs, sums [28]): the sums over the rows in pixel order."""
    sel = rw['ok'].reshape(-1)
    J, r = rw['J'].reshape(-1, 6)[sel], rw['r'].reshape(-1)[sel]
    if len(r) == 0:
        return 0, np.zeros(SUMS)
    with np.errstate(all='ignore'):
        terms = [r * r] + [J[:, g] * J[:, c] for g in range(6) for c in range(g, 6)] + [J[:, g] * r for g in range(6)]
        return len(r), np.cumsum(np.stack(terms, axis=1), axis=0)[-1]


def step(state, vol_origin, voxel, min_count, front, depth, label, want, frame_of, origin, wh, ww, intr_win, pose_in):
    """cloudaae_tsdf_align_step.  depth [F,H,W] uint16; label [F,H,W] uint8 with want [F], or both None; b samples.
    -> dict(n_pairs [b] int32, sums [b,28], x [b,6], status [b] int32, pose_out [b,4,4])."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16
    F, b = len(depth), len(frame_of)
    pose_in = np.asarray(pose_in, np.float64).reshape(b, 4, 4)
    rows_ = np.asarray(intr_win, np.float32).reshape(b, 5)
    out = dict(n_pairs=np.zeros(b, np.int32), sums=np.zeros((b, SUMS)), x=np.zeros((b, 6)), status=np.zeros(b, np.int32),
               pose_out=pose_in.copy())
    filt = label is not None and want is not None
    for i in range(b):
        fr = int(frame_of[i])
        if fr < 0 or fr >= F:
            out['status'][i] = 4
            continue
        rw = rows(state, vol_origin, voxel, min_count, front, depth[fr], np.asarray(label)[fr] if filt else None,
                  int(np.asarray(want)[fr]) if filt else None, np.asarray(origin)[i], wh, ww, rows_[i], pose_in[i])
        out['n_pairs'][i], out['sums'][i] = sums_of(rw)
        if out['n_pairs'][i] < 6:
            out['status'][i] = 1
            continue
        out['status'][i], out['x'][i] = TR.solve(out['sums'][i])
        if out['status'][i] == 0:
            out['pose_out'][i] = TR.compose(TR.update_matrix(out['x'][i]), pose_in[i])
    return out


# ---- the loop --------------------------------------------------------------------------------------------------------------
def scan(depth, intrinsics, voxel, label=None, want=None, first_pose=None, aabb=None, grow=0.5, motion='constant', iterations=4,
         margin=0.5, min_score=(1, 2), tau=0.01, min_count=1, front=None, behind=None, step_=None, keep_states=False, **unused):
    """scan_object(align='sdf'): scan_reference.scan with a frame's `iterations` steps taken on the field -- no raycast
    inside them; the one raycast at the final pose, the counts and the silhouette rule are unchanged.  gate, jump and cos_min
    have no part in it (they are accepted and ignored, so one settings dict serves both loops).  -> the same dict."""
    depth = np.asarray(depth)
    F, H, W = depth.shape
    intr = np.ascontiguousarray(np.broadcast_to(np.asarray(intrinsics, np.float32).reshape(-1, 5), (F, 5)))
    wants = np.zeros(F, np.int32) if want is None else np.broadcast_to(np.asarray(want, np.int32), (F,))
    lab = None if label is None else np.asarray(label)
    first = S.default_first_pose(depth[0], None if lab is None else lab[0], intr[0], wants[0]) if first_pose is None \
        else np.asarray(first_pose, np.float64).reshape(4, 4)
    if aabb is None:
        aabb = S.grown(S.used_points_aabb(depth[0], None if lab is None else lab[0], intr[0], first, wants[0]), grow)
    aabb = np.asarray(aabb, np.float64)
    origin3, dims = FR.volume_for(aabb, voxel)
    dims = tuple(max(n, 2) for n in dims)
    front = FR.FRONT_VOXELS * voxel if front is None else float(front)
    behind = FR.BEHIND_VOXELS * voxel if behind is None else float(behind)
    cast_step = S.STEP_VOXELS * voxel if step_ is None else float(step_)
    state = FR.new_state(dims)

    def fuse(f, pose):
        FR.integrate(state, origin3, voxel, depth[f:f + 1], intr[f:f + 1], pose[None], front, behind,
                     label=None if lab is None else lab[f:f + 1], want=None if lab is None else wants[f:f + 1])

    out = dict(poses=np.zeros((F, 4, 4)), num=np.zeros(F, np.int64), den=np.ones(F, np.int64), n_pairs=np.zeros(F, np.int32),
               status=np.zeros(F, np.int32), lost=np.zeros(F, bool), steps=[[]], origin=origin3, dims=dims, aabb=aabb, states=[])
    fuse(0, first)
    out['poses'][0] = first
    if keep_states:
        out['states'].append(state.copy())
    last, before = first.copy(), None
    for f in range(1, F):
        pose = TR.predict(last, before, motion)
        origin, wh, ww, ok, rows_ = S.frame_window(pose, aabb, intr[f], H, W, margin)
        tu = V.tau_units(np.array([tau], np.float64), np.float64(intr[f, 4]))
        fo = np.array([f if ok else -1], np.int32)
        steps, n_pairs, status = [], 0, 0
        for _ in range(int(iterations)):
            r = step(state, origin3, voxel, min_count, front, depth, lab, None if lab is None else wants, fo, origin, wh, ww, rows_,
                     pose[None])
            n_pairs, status = int(r['n_pairs'][0]), int(r['status'][0])
            steps.append((pose, n_pairs, status, r['pose_out'][0]))
            pose = r['pose_out'][0]
        hyp = S.raycast(state, origin3, voxel, pose[None], rows_, wh, ww, cast_step, min_count)
        counts, _, _ = DR.fit_counts_window(depth, lab, fo, wants[f:f + 1], origin, wh, ww, hyp[:, None], tu)
        num, den = V.fraction(counts[0, 0], 0, True, 1)
        lost = not ok or TR.is_lost(num, den, min_score)
        if lost:
            before = None
        else:
            before, last = last.copy(), pose
            fuse(f, pose)
        out['poses'][f], out['num'][f], out['den'][f], out['lost'][f] = last, num, den, lost
        out['n_pairs'][f], out['status'][f] = n_pairs, status
        out['steps'].append(steps)
        if keep_states:
            out['states'].append(state.copy())
    out['state'] = state
    return out


@functools.lru_cache(maxsize=None)
def orbit(n=S.ORBIT_FRAMES, voxel=S.ORBIT_VOXEL):
    """scan_reference's orbit of the 7 cm cube scanned on the field from the true first pose (computed once per process; do
    not modify) -> dict(depth, truth, result)."""
    truth = S.orbit_poses(n)
    depth = S.orbit_depth(truth)
    result = scan(depth, FR.SCENE_INTR, voxel, first_pose=truth[0], aabb=S.cube_aabb(), keep_states=True, **S.ORBIT_SETTINGS)
    return dict(depth=depth, truth=truth, result=result)


def hold_errors(truth):
    """What holding the previous frame's true pose would give: pose_errors of truth[f - 1] against truth[f], f >= 1."""
    return S.pose_errors(truth[:-1], truth[1:])


# ---- fields written by hand ------------------------------------------------------------------------------------------------
def field_state(phi, front, count=1):
    """acc = count * rint(4096 min(phi, front) / front), cnt = count, for phi [nz,ny,nx] in metres."""
    phi = np.asarray(phi, np.float64)
    st = np.zeros(phi.shape + (4,), np.int32)
    st[..., 0] = np.rint(QUANT * np.minimum(phi, front) / front).astype(np.int32) * int(count)
    st[..., 1] = int(count)
    return st


def centre_grid(dims, vol_origin, voxel):
    nx, ny, nz = dims
    z, y, x = (FR.centres(vol_origin, voxel, n, a) for n, a in ((nz, 2), (ny, 1), (nx, 0)))
    return x[None, None, :], y[None, :, None], z[:, None, None]


def plane_field(dims, vol_origin, voxel, normal, offset):
    """phi = normal . c - offset at the voxel centres c (unit normal: a distance in metres)."""
    x, y, z = centre_grid(dims, vol_origin, voxel)
    n = np.asarray(normal, np.float64)
    return (n[0] * x + n[1] * y) + n[2] * z - offset


def sphere_field(dims, vol_origin, voxel, centre, radius):
    x, y, z = centre_grid(dims, vol_origin, voxel)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def depth_of_points(points, row, H, W, nearest=True):
    """The uint16 frame that holds camera points [n,3] at their nearest pixels: the nearest point of a pixel wins, or with
    nearest=False the last in the order given -- points all through a volume, which no surface would show."""
    fx, fy, cx, cy, factor = (float(np.float32(k)) for k in row)
    frame = np.zeros((H, W), np.uint16)
    u = np.rint(points[:, 0] * fx / points[:, 2] + cx).astype(np.int64)
    v = np.rint(points[:, 1] * fy / points[:, 2] + cy).astype(np.int64)
    du = np.rint(points[:, 2] * factor).astype(np.int64)
    keep = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (du >= 1) & (du <= 65535)
    u, v, du = u[keep], v[keep], du[keep]
    order = np.argsort(-du, kind='stable') if nearest else np.arange(len(du))
    flat = frame.reshape(-1)
    flat[v[order] * W + u[order]] = du[order]                                 # of a repeated index the last value stays
    return frame


def sphere_scene(n=24, voxel=0.004, radius=0.03, distance=0.5, H=64, W=64, focal=500.0):
    """A sphere field around the middle of n^3 voxels (front 4 voxels) and the depth frame a camera at `distance` along
    (0.3, -0.5, 1) sees of that sphere: the ray-sphere intersection per pixel.  -> dict(state, origin, voxel, dims, front,
    depth [1,H,W], intr [5], pose: the true one)."""
    origin, dims = np.array([0.1, -0.2, 0.3]), (n, n, n)
    front = 4.0 * voxel
    centre = origin + 0.5 * n * voxel
    state = field_state(sphere_field(dims, origin, voxel, centre, radius), front)
    d = np.array([0.3, -0.5, 1.0])
    pose = FR.look_at(d / np.sqrt((d * d).sum()), centre, distance)
    intr = np.array([focal, focal, (W - 1) / 2.0, (H - 1) / 2.0, 10000.0], np.float32)
    cc = pose[:3, :3] @ centre + pose[:3, 3]                                  # the sphere's centre in the camera's frame
    y, x = np.mgrid[0:H, 0:W]
    ray = np.stack([(x - float(intr[2])) / float(intr[0]), (y - float(intr[3])) / float(intr[1]), np.ones((H, W))], axis=-1)
    a, b, c = (ray * ray).sum(-1), (ray * cc).sum(-1), float(cc @ cc) - radius * radius
    disc = b * b - a * c
    z = np.where(disc > 0.0, (b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)
    depth = np.rint(z * float(intr[4])).astype(np.uint16)[None]
    return dict(state=state, origin=origin, voxel=voxel, dims=dims, front=front, depth=depth, intr=intr, pose=pose, centre=centre)


def off_pose(T, degrees, metres, centre):
    """T with the object turned by `degrees` about the axis (1, 2, 3) through `centre` (model frame) and then moved by
    `metres` along (1, -1, 1) of the camera's frame: `centre` lands exactly `metres` from where T puts it."""
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.radians(degrees)
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    M[:3, 3] = np.asarray(centre) - M[:3, :3] @ np.asarray(centre)
    out = np.asarray(T, np.float64) @ M
    out[:3, 3] += metres * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    return out


# ---- what the kernel is held to --------------------------------------------------------------------------------------------
def view_frame(state, vol_origin, voxel, pose, intr, H, W, min_count=1):
    """The depth frame [H,W] uint16 that the volume's own raycast gives under `pose`: pixels that lie on the field's zero."""
    return S.raycast(state, vol_origin, voxel, np.asarray(pose)[None], np.asarray(intr, np.float32)[None], H, W, None, min_count)[0]


def small_volume_cases():
    """[(name, state, origin, voxel, min_count)]: scan_reference's small volumes, 3 x 5 x 23 in place of 23 x 5 x 3."""
    return [("2 x 2 x 2", FR.wavy_state((2, 2, 2), 2), [0.015, 0.015, 0.015], 0.02, 1),
            ("3 x 5 x 23", FR.wavy_state((3, 5, 23), 4, zeros=20, unknown=12), [0.03, 0.025, -0.011], 0.004, 1),
            ("3 x 5 x 23, two votes", FR.wavy_state((3, 5, 23), 5, zeros=10, unknown=10, count=2), [0.03, 0.025, -0.011], 0.004, 2),
            ("65 x 2 x 2", FR.wavy_state((65, 2, 2), 1, zeros=8, unknown=5), [-0.03, 0.033, 0.068], 0.002, 1)]


def cloud_frame(dims, vol_origin, voxel, pose, intr, H, W, seed=0, spread=0.25):
    """A frame whose pixels back-project into and around the field: random points of the box of the voxel centres grown by
    `spread` voxels, carried to the camera by `pose`; a pixel keeps any one of its points, so the rows lie all through the
    field and not on its front faces alone."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(vol_origin, np.float64) + (0.5 - spread) * voxel
    hi = np.asarray(vol_origin, np.float64) + (np.asarray(dims, np.float64) - 0.5 + spread) * voxel
    pts = rng.uniform(lo, hi, (4 * H * W, 3))
    cam = pts @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3]
    return depth_of_points(cam[cam[:, 2] > 0.06], intr, H, W, nearest=False)


def sums_in_kernel_order(rw):
    """The sums of a window's rows added as the kernel adds them: a lane its eight consecutive pixels in order from 0, the 64
    lanes of a wave by a butterfly (lane ^ 32, 16, ..., 1), the four waves in order, the runs of 2048 pixels in order from 0.
    What this differs by from sums_of is what the kernel may differ by."""
    sel = rw['ok'].reshape(-1)
    J, r = rw['J'].reshape(-1, 6), rw['r'].reshape(-1)
    terms = np.stack([r * r] + [J[:, g] * J[:, c] for g in range(6) for c in range(g, 6)] + [J[:, g] * r for g in range(6)], axis=1)
    terms = np.where(sel[:, None], terms, 0.0)
    runs = -(-len(sel) // 2048)
    padded = np.zeros((runs * 2048, SUMS))
    padded[:len(sel)] = terms
    lanes = padded.reshape(runs, 4, 64, 8, SUMS)
    acc = np.zeros((runs, 4, 64, SUMS))
    for i in range(8):
        acc = acc + lanes[:, :, :, i]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ off]
    waves = acc[:, :, 0]
    part = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    total = np.zeros(SUMS)
    for t in range(runs):
        total = total + part[t]
    return total


def case(name, state, vol_origin, voxel, depth, frame_of, origin, wh, ww, rows_, poses, min_count=1, front=None, label=None, want=None):
    b = len(frame_of)
    return name, dict(state=np.ascontiguousarray(state), vol_origin=np.asarray(vol_origin, np.float64), voxel=float(voxel),
                      min_count=int(min_count), front=4.0 * float(voxel) if front is None else float(front),
                      depth=np.ascontiguousarray(depth, np.uint16), label=label, want=want, frame_of=np.asarray(frame_of, np.int32),
                      origin=np.asarray(origin, np.int32).reshape(b, 2), wh=int(wh), ww=int(ww),
                      intr_win=np.asarray(rows_, np.float32).reshape(b, 5), pose_in=np.asarray(poses, np.float64).reshape(b, 4, 4))


def run_case(c):
    return step(c['state'], c['vol_origin'], c['voxel'], c['min_count'], c['front'], c['depth'], c['label'], c['want'], c['frame_of'],
                c['origin'], c['wh'], c['ww'], c['intr_win'], c['pose_in'])


def window_rows(intr, origin):
    return TR.window_rows(np.asarray(intr, np.float32).reshape(-1, 5), np.asarray(origin).reshape(-1, 2))


def volume_view(dims, vol_origin, voxel, direction, H, W, distance=0.4, fill=1.2):
    """A pose that looks at the volume's middle and the intrinsics under which its largest side fills `fill` of the frame."""
    extent = max(dims) * voxel
    intr = np.array([fill * min(H, W) * distance / extent] * 2 + [(W - 1) / 2.0, (H - 1) / 2.0, 10000.0], np.float32)
    return S.view_of(dims, vol_origin, voxel, direction, distance), intr


BIG_H, BIG_W = 48, 720


@functools.lru_cache(maxsize=None)
def big_scene():
    """scan_reference's 13 x 9 x 7 wavy field with zeros and unknowns, and two frames of 48 x 720 pixels that look at it
    from two sides: the volume spans the frame's width, so windows of every shape find rows.  (Computed once; do not modify.)"""
    state, vol_origin, voxel = S.big_wavy()
    dims = (13, 9, 7)
    intr = np.array([3200.0, 3200.0, (BIG_W - 1) / 2.0, (BIG_H - 1) / 2.0, 10000.0], np.float32)
    poses = np.array([S.view_of(dims, vol_origin, voxel, d, 0.4) for d in ([0.3, -0.5, 1.0], [-0.2, 1.0, 0.4])])
    depth = np.stack([cloud_frame(dims, vol_origin, voxel, poses[f], intr, BIG_H, BIG_W, seed=10 + f) for f in range(2)])
    return dict(state=state, vol_origin=vol_origin, voxel=voxel, dims=dims, intr=intr, poses=poses, depth=depth)


def volume_cases():
    """[(name, args)]: the smallest volumes, one sample each over a whole 48 x 64 frame; two votes with min_count 1 and 2."""
    out = []
    for i, (name, state, vol_origin, voxel, min_count) in enumerate(small_volume_cases()):
        nz, ny, nx, _ = state.shape
        pose, intr = volume_view((nx, ny, nz), vol_origin, voxel, [0.6, -1.0, 0.5], 48, 64)
        depth = cloud_frame((nx, ny, nz), vol_origin, voxel, pose, intr, 48, 64, seed=20 + i)[None]
        for mc in sorted({1, min_count}):
            out.append(case("%s, min_count %d" % (name, mc), state, vol_origin, voxel, depth, [0], [[0, 0]], 48, 64, intr, pose, mc))
    return out


def window_cases():
    """[(name, args)] on big_scene(): 1 x 1; five rows; 2047, 2048 and 2049 pixels; 63, 64 and 65 columns; a window half off
    the frame on two sides."""
    b = big_scene()
    out = []

    def win(name, wh, ww, u0, v0, f=0):
        out.append(case(name, b['state'], b['vol_origin'], b['voxel'], b['depth'], [f], [[u0, v0]], wh, ww,
                        window_rows(b['intr'], [[u0, v0]]), b['poses'][f]))
    full = rows(b['state'], b['vol_origin'], b['voxel'], 1, 4.0 * b['voxel'], b['depth'][0], None, None, (0, 0), BIG_H, BIG_W, b['intr'],
                b['poses'][0])['ok']
    five = full[:-4] & full[1:-3] & full[2:-2] & full[3:-1] & full[4:]                   # five rows one below the other
    v0, u0 = (int(k[0]) for k in np.nonzero(five))
    win("1 x 1", 1, 1, u0, v0)
    win("5 x 1, five rows", 5, 1, u0, v0)
    for wh, ww in ((23, 89), (32, 64), (3, 683), (31, 63), (31, 64), (31, 65)):
        win("%d x %d = %d pixels" % (wh, ww, wh * ww), wh, ww, (BIG_W - ww) // 2, (BIG_H - wh) // 2)
    win("half off the frame", 40, 200, 300, -20, f=1)
    return out


def batch_case():
    """b = 7 on big_scene(): two good samples of either frame, a pose behind the camera, a NaN pose, frame_of -1 and F, and
    a third good one in a window of its own place."""
    b = big_scene()
    good = [off_pose(b['poses'][f], 0.5, 0.25 * b['voxel'], b['vol_origin'] + 0.02) for f in (0, 1)]
    behind = b['poses'][0].copy()
    behind[1:3] = -behind[1:3]                                           # turned half round about the camera's x: Z < 0
    nan = b['poses'][1].copy()
    nan[0, 3] = np.nan
    poses = np.array([good[0], good[1], behind, nan, good[0], good[1], b['poses'][1]])
    frame_of = [0, 1, 0, 1, -1, 2, 1]
    origin = np.array([[250, 4], [240, 2], [250, 4], [240, 2], [250, 4], [240, 2], [300, -6]], np.int32)
    return case("b = 7", b['state'], b['vol_origin'], b['voxel'], b['depth'], frame_of, origin, 41, 203,
                window_rows(np.tile(b['intr'], (7, 1)), origin), poses)


def alone(c, i):
    """Sample i of a case as a case of its own."""
    return dict(c, frame_of=c['frame_of'][i:i + 1], origin=c['origin'][i:i + 1], intr_win=c['intr_win'][i:i + 1], pose_in=c['pose_in'][i:i + 1])


def filter_cases():
    """[(name, args)] on big_scene(): the label filter off, on with want 0, a wanted label and one no pixel has."""
    b = big_scene()
    label = np.where(np.arange(BIG_W)[None, None, :] % 3 == 0, 2, 5).astype(np.uint8) * np.ones((2, BIG_H, 1), np.uint8)
    origin = np.array([[200, 0], [200, 0]], np.int32)
    rows_ = window_rows(np.tile(b['intr'], (2, 1)), origin)
    out = [case("filter off", b['state'], b['vol_origin'], b['voxel'], b['depth'], [0, 1], origin, 48, 300, rows_, b['poses'])]
    for want in ([0, 0], [2, 5], [5, 0], [7, 2]):
        out.append(case("want %s" % want, b['state'], b['vol_origin'], b['voxel'], b['depth'], [0, 1], origin, 48, 300, rows_, b['poses'],
                        label=label, want=np.array(want, np.int32)))
    return out


def min_count_cases():
    """[(name, args)] on big_scene()'s frames: single votes in the near band and another field in the deep band, so that
    min_count 2 reads the deep band where min_count 1 reads the near one."""
    b = big_scene()
    two = FR.wavy_state(b['dims'], 6, zeros=10, unknown=10)
    two[..., 2], two[..., 3] = FR.wavy_state(b['dims'], 7)[..., 0], 1          # (the negated field would give the same step)
    origin = np.array([[200, 0]], np.int32)
    return [case("single votes, min_count %d" % mc, two, b['vol_origin'], b['voxel'], b['depth'], [0], origin, 48, 300,
                 window_rows(b['intr'], origin), b['poses'][0], mc) for mc in (1, 2)]


def all_cases():
    return volume_cases() + window_cases() + [batch_case()] + filter_cases() + min_count_cases() + [sphere_case()]


def case_rows(c, i):
    """rows() of sample i of a case (frame_of inside [0, F))."""
    fr, filt = int(c['frame_of'][i]), c['label'] is not None
    return rows(c['state'], c['vol_origin'], c['voxel'], c['min_count'], c['front'], c['depth'][fr], c['label'][fr] if filt else None,
                int(c['want'][fr]) if filt else None, c['origin'][i], c['wh'], c['ww'], c['intr_win'][i], c['pose_in'][i])


def sphere_case():
    """The hand-filled sphere from 1 voxel and 1 degree off, and at the true pose."""
    sc = sphere_scene()
    H, W = sc['depth'].shape[1:]
    poses = np.array([off_pose(sc['pose'], 1.0, sc['voxel'], sc['centre']), sc['pose']])
    return case("sphere", sc['state'], sc['origin'], sc['voxel'], sc['depth'], [0, 0], np.zeros((2, 2), np.int32), H, W,
                np.tile(sc['intr'], (2, 1)), poses)
