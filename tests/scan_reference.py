"""NumPy float64 restatement of DESIGN.md, "Scanning": the raycast of a TSDF volume into a uint16 depth window, and the loop
that tracks every new depth frame against the volume fused so far and then fuses it.  Written from the definition: the rays
of a window at once, a loop over the samples; every value is formed in float64 from exactly widened inputs in the order the
definition writes it (NumPy does not fuse a product into a sum), so every pixel is expected to equal the kernel's.

The loop imports fuse_reference, track_reference, detect_reference and render_reference unchanged.  The second half holds the
scenes that the host and the GPU tests share."""
import functools

import numpy as np

import detect_reference as DR
import fuse_reference as FR
import pose_verify_reference as V
import render_reference as R
import track_reference as TR

Z_NEAR = 0.05
MAX_SAMPLES = 4096
STEP_VOXELS = 0.5


# ---- the raycast -----------------------------------------------------------------------------------------------------------
def ray_setup(origin, voxel, dims, pose, row, wh, ww, z_near=Z_NEAR):
    """The rays of one window -> (g0 [3], gd [3,wh,ww], z0, z1 [wh,ww], live [wh,ww] bool)."""
    fx, fy, cxw, cyw, factor = (np.float64(np.float32(k)) for k in np.asarray(row).reshape(-1)[:5])
    A = np.asarray(pose, np.float64).reshape(4, 4)
    s = np.float64(voxel)
    x = np.arange(ww, dtype=np.float64)[None, :] + np.zeros((wh, 1))
    y = np.arange(wh, dtype=np.float64)[:, None] + np.zeros((1, ww))
    with np.errstate(all='ignore'):
        dx, dy = (x - cxw) / fx, (y - cyw) / fy
        g0, gd = np.zeros(3), np.zeros((3, wh, ww))
        z0 = np.full((wh, ww), np.float64(z_near))
        z1 = np.full((wh, ww), np.float64(65535.0) / factor)
        live = np.ones((wh, ww), bool)
        for a in range(3):
            o = -((A[0, a] * A[0, 3] + A[1, a] * A[1, 3]) + A[2, a] * A[2, 3])
            d = (A[0, a] * dx + A[1, a] * dy) + A[2, a]
            g0[a] = (o - np.float64(origin[a])) / s - 0.5
            gd[a] = d / s
            top = np.float64(dims[a] - 1)
            flat = gd[a] == 0.0
            live &= ~flat | ((g0[a] >= 0.0) & (g0[a] <= top))
            ta, tb = (0.0 - g0[a]) / gd[a], (top - g0[a]) / gd[a]
            live &= flat | ~(np.isnan(ta) | np.isnan(tb))                # a NaN fails
            lo, hi = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            z0 = np.where(~flat & (lo > z0), lo, z0)
            z1 = np.where(~flat & (hi < z1), hi, z1)
        live &= z0 <= z1
    return g0, gd, z0, z1, live


def raycast(state, origin, voxel, poses, intr_win, wh, ww, step=None, min_count=1, z_near=Z_NEAR, details=False):
    """cloudaae_tsdf_raycast.  state [nz,ny,nx,4] int32, poses [B,4,4] (model -> camera), intr_win [B,5] float32 -> depth
    [B,wh,ww] uint16; with details also the number of samples every ray took, [B,wh,ww] int32."""
    state = np.asarray(state)
    nz, ny, nx, _ = state.shape
    dims = (nx, ny, nz)
    assert int(min_count) >= 1
    step = np.float64(STEP_VOXELS * voxel if step is None else step)
    assert np.isfinite(step) and step > 0 and np.isfinite(z_near) and z_near > 0
    val, known = FR.corner_values(state, min_count)
    val, known = val.reshape(-1), known.reshape(-1)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    rows = np.asarray(intr_win, np.float32).reshape(len(poses), 5)
    out = np.zeros((len(poses), wh, ww), np.uint16)
    taken = np.zeros((len(poses), wh, ww), np.int32)
    for b in range(len(poses)):
        factor = np.float64(rows[b, 4])
        g0, gd, z0, z1, live = ray_setup(origin, voxel, dims, poses[b], rows[b], wh, ww, z_near)
        at = np.nonzero(live.reshape(-1))[0]                              # the rays still marching
        gd, z0, z1 = gd.reshape(3, -1)[:, at], z0.reshape(-1)[at], z1.reshape(-1)[at]
        known_p = np.zeros(len(at), bool)
        v_p, z_p = np.zeros(len(at)), np.zeros(len(at))
        pixel = np.zeros(wh * ww, np.uint16)
        count = np.zeros(wh * ww, np.int32)
        for k in range(MAX_SAMPLES):
            with np.errstate(all='ignore'):
                zk = z0 + np.float64(k) * step
            go = zk <= z1
            if not go.all():
                at, gd, z0, z1, known_p, v_p, z_p, zk = (q[..., go] for q in (at, gd, z0, z1, known_p, v_p, z_p, zk))
            if not len(at):
                break
            count[at] += 1
            cell, frac = [], []
            with np.errstate(all='ignore'):
                for a in range(3):
                    g = g0[a] + zk * gd[a]
                    fl = np.floor(g)
                    i = np.where(fl >= 0.0, np.minimum(fl, np.float64(dims[a] - 2)), 0.0)     # the clamp, before the conversion
                    cell.append(i.astype(np.int64))
                    frac.append(g - i)
            c = []
            ok = np.ones(len(at), bool)
            for corner in range(8):
                idx = ((cell[2] + (corner >> 2)) * ny + (cell[1] + ((corner >> 1) & 1))) * nx + (cell[0] + (corner & 1))
                c.append(val[idx])
                ok &= known[idx]
            with np.errstate(all='ignore'):
                c00, c10 = c[0] + (c[1] - c[0]) * frac[0], c[2] + (c[3] - c[2]) * frac[0]
                c01, c11 = c[4] + (c[5] - c[4]) * frac[0], c[6] + (c[7] - c[6]) * frac[0]
                c0, c1 = c00 + (c10 - c00) * frac[1], c01 + (c11 - c01) * frac[1]
                v = c0 + (c1 - c0) * frac[2]
                inside = ok & (v < 0.0)
                hit = inside & known_p
                t = v_p[hit] / (v_p[hit] - v[hit])
                zs = z_p[hit] + (zk[hit] - z_p[hit]) * t
                du = np.floor(zs * factor + 0.5)
                good = (du >= 1.0) & (du <= 65535.0)
            pixel[at[hit]] = np.where(good, du, 0.0).astype(np.uint16)
            outside = ok & ~inside
            known_p = outside
            v_p, z_p = np.where(outside, v, 0.0), np.where(outside, zk, 0.0)
            if inside.any():                                              # v < 0 ends a ray, hit or not
                at, gd, z0, z1, known_p, v_p, z_p = (q[..., ~inside] for q in (at, gd, z0, z1, known_p, v_p, z_p))
        out[b], taken[b] = pixel.reshape(wh, ww), count.reshape(wh, ww)
    return (out, taken) if details else out


def backproject(depth, row, pose):
    """The set pixels of one window in the model frame: p_cam = ((x - cxw) dm / fx, (y - cyw) dm / fy, dm), dm = d / factor;
    p = R^T (p_cam - t).  -> [n,3] float64, in pixel order."""
    fx, fy, cxw, cyw, factor = (float(np.float32(k)) for k in np.asarray(row).reshape(-1)[:5])
    ys, xs = np.nonzero(depth)
    dm = depth[ys, xs].astype(np.float64) / factor
    cam = np.stack([(xs - cxw) * dm / fx, (ys - cyw) * dm / fy, dm], axis=1)
    A = np.asarray(pose, np.float64)
    return (cam - A[:3, 3]) @ A[:3, :3]


# ---- the loop --------------------------------------------------------------------------------------------------------------
def used_points_aabb(depth, label, intr, pose, want):
    """fuse.used_points_aabb of one frame, on the host."""
    d = np.asarray(depth)
    used = d != 0
    if label is not None and int(want) != 0:
        used &= np.asarray(label) == int(want)
    assert used.any(), "no pixel of the frame is used"
    pts = backproject(np.where(used, d, 0).astype(np.uint16), intr, pose)
    return np.stack([pts.min(axis=0), pts.max(axis=0)])


def default_first_pose(depth, label, intr, want):
    """No rotation; the translation is the centre of the used pixels' box in the camera's frame."""
    box = used_points_aabb(depth, label, intr, np.eye(4), want)
    T = np.eye(4)
    T[:3, 3] = (box[0] + box[1]) / 2.0
    return T


def grown(box, grow):
    side = float((box[1] - box[0]).max())
    return np.stack([box[0] - grow * side, box[1] + grow * side])


def frame_window(pose, aabb, intr_row, H, W, margin):
    """The window of one pose -> (origin [1,2] int32, wh, ww, ok, rows [1,5] float32)."""
    origin, wh, ww, ok = TR.pose_windows(np.asarray(pose)[None], np.asarray(aabb)[None], np.asarray(intr_row)[None], H, W, margin)
    return origin, wh, ww, bool(ok[0]), TR.window_rows(np.asarray(intr_row)[None], origin)


def scan(depth, intrinsics, voxel, label=None, want=None, first_pose=None, aabb=None, grow=0.5, motion='constant', iterations=4,
         gate=0.03, jump=0.005, cos_min=0.8, margin=0.5, min_score=(1, 2), tau=0.01, min_count=1, front=None, behind=None,
         step=None, keep_states=False):
    """scan_object -> dict(poses [F,4,4], num, den [F] int64, n_pairs, status [F] int32 of the last step, lost [F] bool,
    steps: per frame the (pose_in, n_pairs, status, pose_out) of every step, state, origin, dims; with keep_states also
    states: the state after every frame)."""
    depth = np.asarray(depth)
    F, H, W = depth.shape
    intr = np.ascontiguousarray(np.broadcast_to(np.asarray(intrinsics, np.float32).reshape(-1, 5), (F, 5)))
    wants = np.zeros(F, np.int32) if want is None else np.broadcast_to(np.asarray(want, np.int32), (F,))
    lab = None if label is None else np.asarray(label)
    first = default_first_pose(depth[0], None if lab is None else lab[0], intr[0], wants[0]) if first_pose is None \
        else np.asarray(first_pose, np.float64).reshape(4, 4)
    if aabb is None:
        aabb = grown(used_points_aabb(depth[0], None if lab is None else lab[0], intr[0], first, wants[0]), grow)
    aabb = np.asarray(aabb, np.float64)
    origin3, dims = FR.volume_for(aabb, voxel)
    dims = tuple(max(n, 2) for n in dims)
    front = FR.FRONT_VOXELS * voxel if front is None else float(front)
    behind = FR.BEHIND_VOXELS * voxel if behind is None else float(behind)
    step = STEP_VOXELS * voxel if step is None else float(step)
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
        origin, wh, ww, ok, rows = frame_window(pose, aabb, intr[f], H, W, margin)
        factor = np.float64(intr[f, 4])
        gu, ju, tu = (V.tau_units(np.array([q], np.float64), factor) for q in (gate, jump, tau))
        fo = np.array([f if ok else -1], np.int32)
        steps, n_pairs, status = [], 0, 0
        for _ in range(int(iterations)):
            hyp = raycast(state, origin3, voxel, pose[None], rows, wh, ww, step, min_count)
            r = TR.step(depth, fo, origin, hyp, rows, gu, ju, cos_min, pose[None])
            n_pairs, status = int(r['n_pairs'][0]), int(r['status'][0])
            steps.append((pose, n_pairs, status, r['pose_out'][0]))
            pose = r['pose_out'][0]
        hyp = raycast(state, origin3, voxel, pose[None], rows, wh, ww, step, min_count)
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


def mesh_of(result, voxel, min_count=1):
    return FR.extract_mesh(result['state'], result['origin'], voxel, min_count)


# ---- the scenes ------------------------------------------------------------------------------------------------------------
ORBIT_FRAMES = 10
ORBIT_VOXEL = 0.004
ORBIT_SETTINGS = dict(iterations=4, gate=0.03, jump=0.005, cos_min=0.8, margin=0.5)


def orbit_poses(n=ORBIT_FRAMES):
    """The camera goes round the 7 cm cube, 3 degrees a frame from 20 degrees on, looking down at 0.6 rad, so that three faces
    stay in view; the object also moves 4 mm a frame along the camera's x."""
    v = FR.cube_mesh()[0].astype(np.float64)
    centre = (v.min(axis=0) + v.max(axis=0)) / 2.0
    poses = []
    for f in range(n):
        th = np.radians(20.0 + 3.0 * f)
        T = FR.look_at(np.array([np.cos(th) * np.cos(0.6), np.sin(th) * np.cos(0.6), -np.sin(0.6)]), centre)
        T[0, 3] += 0.004 * f
        poses.append(T)
    return np.array(poses)


def cube_aabb():
    v = FR.cube_mesh()[0].astype(np.float64)
    return np.stack([v.min(axis=0), v.max(axis=0)])


def orbit_depth(poses, without=(), renderer=None):
    """depth [n,240,320] uint16 of the cube alone under `poses`; the frames listed in `without` are empty."""
    frames = [[] if f in without else [(0, 1, T)] for f, T in enumerate(poses)]
    intr = np.tile(FR.SCENE_INTR, (len(poses), 1))
    if renderer is not None:
        return renderer([FR.cube_mesh()], frames, intr, FR.SCENE_H, FR.SCENE_W)
    return R.render([FR.cube_mesh()], frames, intr, FR.SCENE_H, FR.SCENE_W)['depth']


@functools.lru_cache(maxsize=None)
def orbit(n=ORBIT_FRAMES, voxel=ORBIT_VOXEL, step_voxels=STEP_VOXELS, without=()):
    """The orbit scanned by this restatement from the true first pose (computed once per process; do not modify) ->
    dict(depth, truth, result)."""
    truth = orbit_poses(n)
    depth = orbit_depth(truth, without)
    result = scan(depth, FR.SCENE_INTR, voxel, first_pose=truth[0], aabb=cube_aabb(), step=step_voxels * voxel, keep_states=True,
                  **ORBIT_SETTINGS)
    return dict(depth=depth, truth=truth, result=result)


def pose_errors(poses, truth):
    return np.abs(np.asarray(poses) - np.asarray(truth)).reshape(len(truth), -1).max(axis=1)


def mesh_distance(result, voxel):
    """(largest vertex-to-surface distance of the scanned mesh in voxels, its components)."""
    v, t = mesh_of(result, voxel)
    rects = FR.union_surface(FR.mesh_boxes('cube'))
    return float(FR.surface_distance(v, rects).max() / voxel), FR.mesh_stats(v, t)['components']


# ---- hand cases of the raycast ---------------------------------------------------------------------------------------------
def linear_state(dims, axis, zero_at, slope=0.25, count=1):
    """v = slope (zero_at - g_axis) on (nx, ny, nz) voxels: outside (positive) in front of g = zero_at along `axis`, seen
    from low g.  slope a power of two and zero_at a multiple of 1 / (4096 slope): every value is exact."""
    nx, ny, nz = dims
    g = [np.arange(n, dtype=np.float64) for n in (nx, ny, nz)]
    field = slope * (zero_at - (g[0][None, None, :] if axis == 0 else g[1][None, :, None] if axis == 1 else g[2][:, None, None]))
    return FR.state_from_field(np.broadcast_to(field, (nz, ny, nx)), count)


def hand_cases():
    """[(name, dict of raycast's arguments)].  The volume has voxel 1/64 and its first centre at the camera's axis, the pose
    is the identity unless said, fx = fy = 64 and the factor is a power of two: along the central ray everything is exact.
    The closed forms are asserted in tests/test_scan_host.py."""
    s = 1.0 / 64.0
    cases = []

    def case(name, state, origin=None, pose=None, row=None, wh=1, ww=1, step=0.5 * s, min_count=1, z_near=Z_NEAR, voxel=s):
        # by default voxel centre (0, 0, 0) sits at (0, 0, 1): the central ray x = y = 0 runs through centres, g_z = 64 (z - 1)
        origin = [-0.5 * s, -0.5 * s, 1.0 - 0.5 * s] if origin is None else origin
        row = [64.0, 64.0, 0.0, 0.0, 8192.0] if row is None else row
        cases.append((name, dict(state=state, origin=np.asarray(origin, np.float64), voxel=voxel, poses=np.asarray(
            np.eye(4) if pose is None else pose, np.float64).reshape(-1, 4, 4), intr_win=np.asarray(row, np.float32).reshape(-1, 5),
            wh=wh, ww=ww, step=step, min_count=min_count, z_near=z_near)))

    dims = (4, 4, 16)
    # the zero crossing at g_z = 5.25: z* = 1 + 5.25 / 64, between the samples at g_z = 5 and 5.5
    case("linear field", linear_state(dims, 2, 5.25))
    # ... exactly on the sample at g_z = 6: v == 0 is outside, the hit comes one sample later with t = 0
    case("zero on a sample", linear_state(dims, 2, 6.0))
    # the central ray has gd_x = gd_y = 0 and g0 = 0: inside the slab; moved by one voxel below the volume: outside
    case("parallel outside", linear_state(dims, 2, 5.25), origin=[0.5 * s, -0.5 * s, 1.0 - 0.5 * s])
    # through the last row of centres, g_x = g_y = n - 1 = 3: the clamp, f = 1
    case("through the last centres", linear_state(dims, 2, 5.25), origin=[-3.5 * s, -3.5 * s, 1.0 - 0.5 * s])
    st = linear_state(dims, 2, 5.25)
    st[5, 1, 1] = 0                                                      # a corner of the cell (0, 0, 5) is unknown ...
    case("unknown beside the ray", st)                                   # ... and the central ray's cells are (0, 0, k): no hit
    st = linear_state(dims, 2, 5.25)
    st[:6] = 0                                                           # unknown up to g_z = 5, negative from 6 on: a back face
    case("unknown then negative", st)
    st = linear_state(dims, 2, 5.25)                                     # one vote in the near band, and a deep band at 7.25
    st[..., 2], st[..., 3] = linear_state(dims, 2, 7.25)[..., 0], 1
    case("min_count 2 takes the deep band", st, min_count=2)
    case("min_count 1 beside it", st, min_count=1)
    # du by the factor: z* = 1 + 5.25 / 64 = 1.08203125 times 1/4 and 1/2 rounds to 0 and to 1
    case("du 0", linear_state(dims, 2, 5.25), row=[64.0, 64.0, 0.0, 0.0, 0.25])
    case("du 1", linear_state(dims, 2, 5.25), row=[64.0, 64.0, 0.0, 0.0, 0.5])
    # 65535 needs a hit whose closing sample still lies in front of z1 = 65535 / factor: voxels of 1 m from z = 32760 m on
    # and factor 2, so z1 = 32767.5; the surface at g_z = 7.25 is closed by the sample at 7.5 = z1: z* factor + 0.5 = 65535
    far = dict(origin=[-0.5, -0.5, 32759.5], voxel=1.0, step=0.5, row=[64.0, 64.0, 0.0, 0.0, 2.0])
    case("du 65535", linear_state(dims, 2, 7.25), **far)
    # 65536 would need z* >= 32767.75, behind z1: the sample that would close it is never taken, so the far end of the
    # interval, not the test du <= 65535, keeps 65536 out; the pixel is 0 either way
    case("du 65536", linear_state(dims, 2, 7.75), **far)
    # z_near behind the surface: sampling starts inside, from nothing known
    case("surface in front of z_near", linear_state(dims, 2, 5.25), z_near=1.0 + 6.0 * s)
    back = np.eye(4)
    back[2, 3] = -2.0
    case("volume behind the camera", linear_state(dims, 2, 5.25), pose=back)
    nan = np.eye(4)
    nan[1, 1] = np.nan
    case("NaN pose", linear_state(dims, 2, 5.25), pose=nan)
    # 15 voxels in steps of 1/512 voxel are 7681 samples: the ray ends after 4096, at g_z = 8 - 1/512, before the surface at
    # 12.25; in steps of 1/256 voxel it arrives
    case("more than 4096 samples", linear_state(dims, 2, 12.25), step=s / 512.0)
    case("fewer than 4096 samples", linear_state(dims, 2, 12.25), step=s / 256.0)
    return cases


def run_case(args, **kw):
    return raycast(**dict(args, **kw))


# ---- what the kernel is held to: volumes, windows, batches -----------------------------------------------------------------
def view_of(dims, origin, voxel, direction, distance, shift=(0.0, 0.0)):
    """model -> camera: looking along `direction` at the volume's middle from `distance`, moved by `shift` in the image plane."""
    mid = np.asarray(origin, np.float64) + 0.5 * np.asarray(dims, np.float64) * voxel
    d = np.asarray(direction, np.float64)
    T = FR.look_at(d / np.sqrt((d * d).sum()), mid, distance)
    T[0, 3] += shift[0]
    T[1, 3] += shift[1]
    return T


def window_row(wh, ww, focal, factor=10000.0):
    return np.array([focal, focal, (ww - 1) / 2.0, (wh - 1) / 2.0, factor], np.float32)


def volume_cases():
    """[(name, state, origin, voxel, min_count)]."""
    return [("2 x 2 x 2", FR.wavy_state((2, 2, 2), 2), [0.015, 0.015, 0.015], 0.02, 1),
            ("23 x 5 x 3", FR.wavy_state((23, 5, 3), 4, zeros=20, unknown=12), [-0.011, 0.025, 0.03], 0.004, 1),
            ("23 x 5 x 3, two votes", FR.wavy_state((23, 5, 3), 5, zeros=10, unknown=10, count=2), [-0.011, 0.025, 0.03], 0.004, 2),
            ("65 x 2 x 2", FR.wavy_state((65, 2, 2), 1, zeros=8, unknown=5), [-0.03, 0.033, 0.068], 0.002, 1)]


def big_wavy():
    """A 13 x 9 x 7 field with zeros and unknowns, 5 mm voxels: what the window and batch cases look at."""
    return FR.wavy_state((13, 9, 7), 4, zeros=40, unknown=25), np.array([0.1, -0.2, 0.3]), 0.005


def window_cases():
    """[(name, wh, ww, pose, row)] on big_wavy()."""
    st, origin, voxel = big_wavy()
    dims = (13, 9, 7)
    look = view_of(dims, origin, voxel, [0.3, -0.5, 1.0], 0.4)
    out = []
    for wh, ww in ((1, 1), (9, 1), (23, 89), (32, 64), (3, 683), (33, 67), (31, 63), (31, 64), (31, 65)):
        out.append(("%d x %d" % (wh, ww), wh, ww, look, window_row(wh, ww, 8.0 * max(wh, ww))))
    out.append(("all rays miss", 17, 24, view_of(dims, origin, voxel, [0.3, -0.5, 1.0], 0.4, shift=(0.5, 0.0)), window_row(17, 24, 200.0)))
    out.append(("half off the volume", 33, 40, view_of(dims, origin, voxel, [0.3, -0.5, 1.0], 0.4, shift=(0.03, 0.01)), window_row(33, 40, 300.0)))
    return out


def batch_case():
    """B = 7 on big_wavy(): mixed poses, one behind the camera, one NaN, one looking along an axis exactly."""
    st, origin, voxel = big_wavy()
    dims = (13, 9, 7)
    poses = [view_of(dims, origin, voxel, d, 0.4) for d in ([0.3, -0.5, 1.0], [1.0, 0.2, -0.4], [-1.0, -1.0, 1.0], [0.0, 1.0, 0.1])]
    behind = view_of(dims, origin, voxel, [0.3, -0.5, 1.0], 0.4)
    behind[1:3] = -behind[1:3]                                           # turned half round about the camera's x: Z < 0
    nan = poses[0].copy()
    nan[0, 3] = np.nan
    mid = origin + 0.5 * np.asarray(dims) * voxel
    axis = np.eye(4)                                                     # along +z through voxel centres: gd_x = gd_y = 0 at x = cxw
    axis[:3, 3] = [-(origin[0] + 6.5 * voxel), -(origin[1] + 4.5 * voxel), 0.3 - mid[2]]
    poses = np.array(poses + [behind, nan, axis])
    rows = np.tile(window_row(33, 67, 450.0), (7, 1))
    rows[6, 2:4] = [33.0, 16.0]
    return poses, rows, 33, 67
