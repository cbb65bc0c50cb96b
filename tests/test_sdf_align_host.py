"""CPU: what anchors tests/sdf_align_reference.py, the NumPy restatement of DESIGN.md "Scanning on the field", before the
kernel is held to it (tests/test_51_sdf_align_gpu.py): the Jacobian against finite differences of the residual, the
convergence of repeated steps, the row rule case by case in closed form, the tracking condition on the 30 degree orbit,
and the ABI."""
import os
import re

import numpy as np

import fuse_reference as FR
import scan_reference as S
import sdf_align_reference as A
import track_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- finite differences ----------------------------------------------------------------------------------------------------
def field_bounds(state, voxel, front):
    """Bounds on the derivatives of the trilinear field in metres, per cell [nz-1,ny-1,nx-1]: (D1 >= |grad|, D2 >= |v^T H v|
    for unit v, D3 >= the third derivative along a unit v).  Within a cell the field is a0 + ... + a_xyz fx fy fz: its Hessian
    has the mixed terms alone (|v^T H v| = 2 |a_xy vx vy + ...| <= |a_xy| + |a_xz| + |a_yz|, each at most the largest second
    difference over the cell's faces) and its third derivative along v is 6 a_xyz vx vy vz, at most 6 / 3^1.5 |a_xyz|."""
    v = FR.corner_values(state)[0] * (front / A.QUANT)                          # [z,y,x], metres
    dx, dy, dz = np.abs(np.diff(v, axis=2)), np.abs(np.diff(v, axis=1)), np.abs(np.diff(v, axis=0))
    mx = np.maximum(np.maximum(dx[:-1, :-1], dx[:-1, 1:]), np.maximum(dx[1:, :-1], dx[1:, 1:]))
    my = np.maximum(np.maximum(dy[:-1, :, :-1], dy[:-1, :, 1:]), np.maximum(dy[1:, :, :-1], dy[1:, :, 1:]))
    mz = np.maximum(np.maximum(dz[:, :-1, :-1], dz[:, :-1, 1:]), np.maximum(dz[:, 1:, :-1], dz[:, 1:, 1:]))
    d1 = np.sqrt(mx ** 2 + my ** 2 + mz ** 2) / voxel
    sxy, sxz, syz = (np.abs(np.diff(np.diff(v, axis=a), axis=b)) for a, b in ((2, 1), (2, 0), (1, 0)))
    d2 = (np.maximum(sxy[:-1], sxy[1:]) + np.maximum(sxz[:, :-1], sxz[:, 1:]) + np.maximum(syz[:, :, :-1], syz[:, :, 1:])) / voxel ** 2
    d3 = 6.0 / 3.0 ** 1.5 * np.abs(np.diff(np.diff(np.diff(v, axis=2), axis=1), axis=0)) / voxel ** 3
    return d1, d2, d3


def check_jacobian(state, origin, voxel, front, frame, intr, pose, h=1e-4):
    """J against (r(+h) - r(-h)) / 2h in each of the six parameters of U, over the pixels that have a row in the same cell
    at all three poses (the field's gradient jumps between cells: a difference quotient across a cell face measures the
    jump).  The tolerance, per pixel from its own cell: the quotient's second-order term h^2 / 6 |r'''| plus the rounding of
    r over 2h.  r = phi(q(x)), q = (U(x) T)^-1 p: r''' = phi'''[q', q', q'] + 3 phi''[q', q''] + phi'[q'''], and |q'|, |q''|,
    |q'''| <= rho = max(1, |p|) for a rotation about the camera's origin (|q'| = 1, the others 0 for a translation).  q is
    formed of a dozen operations on magnitudes <= rho (and the grid coordinate of it, <= 32 voxels): 64 eps rho D1 bounds
    the rounding of r."""
    H, W = frame.shape
    at = lambda T: A.rows(state, origin, voxel, 1, front, frame, None, None, (0, 0), H, W, intr, T)
    base = at(pose)
    cz, cy, cx = base['cell'][..., 2], base['cell'][..., 1], base['cell'][..., 0]
    d1, d2, d3 = (d[cz, cy, cx] for d in field_bounds(state, voxel, front))
    rho = np.maximum(1.0, np.sqrt((base['p'] ** 2).sum(axis=-1)))
    tol = h * h / 6.0 * (d3 * rho ** 3 + 3.0 * d2 * rho ** 2 + d1 * rho) + 64.0 * EPS * rho * d1 / h
    worst, used = 0.0, 0
    for k in range(6):
        x = np.zeros(6)
        x[k] = h
        plus, minus = at(TR.compose(TR.update_matrix(x), pose)), at(TR.compose(TR.update_matrix(-x), pose))
        sel = base['ok'] & plus['ok'] & minus['ok'] & np.all((plus['cell'] == base['cell']) & (minus['cell'] == base['cell']), axis=-1)
        fd = (plus['r'][sel] - minus['r'][sel]) / (2.0 * h)
        off = np.abs(fd - base['J'][sel][:, k])
        worst = max(worst, float((off / tol[sel]).max()))
        used = max(used, int(sel.sum()))
        assert sel.sum() > 200, (k, int(sel.sum()))
        assert np.abs(base['J'][sel][:, k]).max() > 1000.0 * np.median(tol[sel]), k   # the check can tell a wrong sign or order
    print("rows %d, tolerance %.3g (median) to %.3g, largest |J - finite difference| / tolerance %.3g"
          % (used, np.median(tol[base['ok']]), tol[base['ok']].max(), worst))
    assert worst <= 1.0


def hand_volume(n=24, voxel=0.004):
    origin, dims = np.array([0.1, -0.2, 0.3]), (n, n, n)
    d = np.array([0.3, -0.5, 1.0])
    pose = FR.look_at(d / np.sqrt((d * d).sum()), origin + 0.5 * n * voxel, 0.5)
    intr = np.array([500.0, 500.0, 31.5, 31.5, 10000.0], np.float32)
    return origin, dims, voxel, 4.0 * voxel, pose, intr


def test_jacobian_equals_finite_differences_on_a_plane_field():
    origin, dims, voxel, front, pose, intr = hand_volume()
    n = np.array([2.0, -1.0, 2.0]) / 3.0
    state = A.field_state(A.plane_field(dims, origin, voxel, n, float(n @ (origin + 12 * voxel))), front)
    frame = A.cloud_frame(dims, origin, voxel, pose, intr, 64, 64, seed=1)
    check_jacobian(state, origin, voxel, front, frame, intr, pose)


def test_jacobian_equals_finite_differences_on_a_sphere_field():
    origin, dims, voxel, front, pose, intr = hand_volume()
    state = A.field_state(A.sphere_field(dims, origin, voxel, origin + 12 * voxel, 0.03), front)
    frame = A.cloud_frame(dims, origin, voxel, pose, intr, 64, 64, seed=2)
    check_jacobian(state, origin, voxel, front, frame, intr, pose)


# ---- convergence -----------------------------------------------------------------------------------------------------------
def test_steps_converge_on_the_sphere():
    """From 1 voxel and 1 degree off the true pose (the sphere turned about its centre, then moved): a sphere fixes its
    centre and nothing else, so the distance is that of the centre's place in the camera's frame from the true one.  One
    step lands closer, repeated steps converge to within the depth quantum and the field's quantisation, a few hundredths
    of a voxel.  One step does not arrive: the three rotations about the centre are free, the undamped solve fills them with
    a large angle (0.07 rad here), and its second-order term moves the centre (1 -> 0.56 -> 0.02 voxels)."""
    sc = A.sphere_scene()
    fo, org = np.array([0], np.int32), np.zeros((1, 2), np.int32)
    H, W = sc['depth'].shape[1:]
    place = lambda T: T[:3, :3] @ sc['centre'] + T[:3, 3]

    def dist(T):
        return float(np.sqrt(((place(T) - place(sc['pose'])) ** 2).sum()))
    T = A.off_pose(sc['pose'], 1.0, sc['voxel'], sc['centre'])
    d = [dist(T)]
    for _ in range(6):
        r = A.step(sc['state'], sc['origin'], sc['voxel'], 1, sc['front'], sc['depth'], None, None, fo, org, H, W, sc['intr'][None], T[None])
        assert r['status'][0] == 0 and r['n_pairs'][0] > 500
        T = r['pose_out'][0]
        d.append(dist(T))
    print("distance of the centre per step, voxels: %s" % np.array2string(np.array(d) / sc['voxel'], precision=4))
    assert abs(d[0] - sc['voxel']) < 1e-12
    assert d[1] < d[0]
    assert all(q < 0.1 * sc['voxel'] for q in d[2:])
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12


# ---- the row rule, case by case --------------------------------------------------------------------------------------------
# Voxels of 1/64 m, the centre of voxel (0, 0, 0) at (0, 0, 1) of the camera, the identity pose, fx = fy = 64 and a factor of
# 8192: window pixel (0, 0) with principal point 0 back-projects to (0, 0, d / 8192), so g = (0, 0, (d - 8192) / 128) exactly.
S64 = 1.0 / 64.0
FRONT = 4.0 * S64
ROW = np.array([64.0, 64.0, 0.0, 0.0, 8192.0], np.float32)
DIMS = (4, 4, 8)


def one_pixel(state, d, origin=None, label=None, want=None, pose=None, row=ROW):
    origin = [-0.5 * S64, -0.5 * S64, 1.0 - 0.5 * S64] if origin is None else origin
    frame = np.full((1, 1), d, np.uint16)
    lab = None if label is None else np.full((1, 1), label, np.uint8)
    rw = A.rows(state, origin, S64, 1, FRONT, frame, lab, want, (0, 0), 1, 1, row, np.eye(4) if pose is None else pose)
    return bool(rw['ok'][0, 0]), rw['J'][0, 0], float(rw['r'][0, 0]), rw


def test_row_in_closed_form():
    """v = 1024 (5 - g_z) (a quarter of the front per voxel): at g_z = 2.5, r = 0.625 front, the gradient (0, 0, -0.25 front /
    s) = (0, 0, -1), so J = -(p x n, n) = (0, 0, 0, 0, 0, 1) for p on the axis; beside the axis, at pixel x = 1, p_x = dm / 64
    and p x n = (0, p_x, 0): J = (0, -p_x, 0, 0, 0, 1)."""
    state = S.linear_state(DIMS, 2, 5.0)
    ok, J, r, _ = one_pixel(state, 8192 + 320)
    assert ok and r == 0.625 * FRONT and np.array_equal(J, [0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    frame = np.array([[0, 8192 + 320]], np.uint16)
    rw = A.rows(state, [-0.5 * S64, -0.5 * S64, 1.0 - 0.5 * S64], S64, 1, FRONT, frame, None, None, (0, 0), 1, 2, ROW, np.eye(4))
    dm = (8192 + 320) / 8192.0
    assert rw['ok'].tolist() == [[False, True]] and np.array_equal(rw['g'][0, 1], [dm, 0.0, 2.5])
    assert np.array_equal(rw['J'][0, 1], [0.0, -(dm / 64.0), 0.0, 0.0, 0.0, 1.0]) and rw['r'][0, 1] == 0.625 * FRONT


def test_row_rule_case_by_case():
    state = S.linear_state(DIMS, 2, 5.0)
    assert not one_pixel(state, 0)[0]                                             # a zero depth
    assert one_pixel(state, 8192 + 320, label=3, want=3)[0]                       # the wanted label
    assert not one_pixel(state, 8192 + 320, label=3, want=4)[0]                   # an unwanted one
    assert one_pixel(state, 8192 + 320, label=3, want=0)[0]                       # want 0: every pixel with a depth
    # g exactly 0 and exactly n - 1 on z (and exactly 0 on x and y); just outside by 1 / 128 voxel
    ok, _, _, rw = one_pixel(state, 8192 + 256)
    assert ok and np.array_equal(rw['g'][0, 0], [0.0, 0.0, 2.0])
    assert one_pixel(state, 8192 + 128 + 1)[0] and np.array_equal(one_pixel(state, 8192 + 7 * 128)[3]['g'][0, 0], [0.0, 0.0, 7.0])
    assert one_pixel(state, 8192 + 7 * 128)[0] and np.array_equal(one_pixel(state, 8192 + 7 * 128)[3]['cell'][0, 0], [0, 0, 6])
    assert not one_pixel(state, 8192 + 7 * 128 + 1)[0]
    low = S.linear_state(DIMS, 2, 2.0)                                            # v(0) = 2048: g_z = 0 has a row
    assert one_pixel(low, 8192)[0] and one_pixel(low, 8192)[2] == 0.5 * FRONT
    assert not one_pixel(low, 8191)[0]
    # g exactly n - 1 = 3 on x and y (the volume moved by three voxels), and one 1 / 128 voxel beyond on x
    ok, _, _, rw = one_pixel(state, 8192 + 320, origin=[-3.5 * S64, -3.5 * S64, 1.0 - 0.5 * S64])
    assert ok and np.array_equal(rw['g'][0, 0], [3.0, 3.0, 2.5]) and np.array_equal(rw['cell'][0, 0], [2, 2, 2])
    assert not one_pixel(state, 8192 + 320, origin=[-3.5 * S64 - S64 / 128.0, -3.5 * S64, 1.0 - 0.5 * S64])[0]
    assert not one_pixel(state, 8192 + 320, origin=[-0.5 * S64 + S64 / 128.0, -0.5 * S64, 1.0 - 0.5 * S64])[0]
    # one unknown corner of the cell (0, 0, 2), and the same voxel unknown beside another cell
    hole = state.copy()
    hole[3, 1, 1] = 0
    assert not one_pixel(hole, 8192 + 320)[0] and one_pixel(hole, 8192 + 4 * 128 + 64)[0]
    # val exactly 4096 at g_z = 1, one quantum below it at g_z = 1 + 1 / 128, above it at g_z < 1
    assert not one_pixel(state, 8192 + 128)[0] and one_pixel(state, 8192 + 128)[3]['val'][0, 0] == 4096.0
    assert one_pixel(state, 8192 + 129)[0] and not one_pixel(state, 8192 + 127)[0]
    # a zero gradient: a constant field below the truncation
    assert not one_pixel(FR.state_from_field(np.full((8, 4, 4), 0.5)), 8192 + 320)[0]
    # a NaN pose: no row, whichever entry
    for i, j in ((0, 0), (1, 2), (2, 3)):
        T = np.eye(4)
        T[i, j] = np.nan
        assert not one_pixel(state, 8192 + 320, pose=T)[0]


def test_step_statuses():
    """Five rows: status 1 and the pose untouched; frame_of outside [0, F): status 4; a NaN pose: no row, status 1, pose_in
    bit for bit; a plane field alone leaves three of six parameters free: status 2."""
    state = S.linear_state(DIMS, 2, 5.0)
    origin = [-0.5 * S64, -0.5 * S64, 1.0 - 0.5 * S64]
    depth = np.full((1, 5, 1), 8192 + 320, np.uint16)
    T = np.eye(4)
    nan = T.copy()
    nan[0, 3] = np.nan
    row = np.array([128.0, 128.0, 0.0, 0.0, 8192.0], np.float32)                  # g_y = y dm / 2: all five pixels inside
    r = A.step(state, origin, S64, 1, FRONT, depth, None, None, np.array([0, -1, 1, 0], np.int32), np.zeros((4, 2), np.int32), 5, 1,
               np.tile(row, (4, 1)), np.array([T, T, T, nan]))
    assert r['n_pairs'].tolist() == [5, 0, 0, 0] and r['status'].tolist() == [1, 4, 4, 1]
    assert r['pose_out'].tobytes() == np.array([T, T, T, nan]).tobytes() and not r['x'].any()
    wide = np.full((1, 4, 4), 8192 + 320, np.uint16)
    r = A.step(state, origin, S64, 1, FRONT, wide, None, None, np.array([0], np.int32), np.zeros((1, 2), np.int32), 4, 4, row[None], T[None])
    assert r['n_pairs'][0] == 16 and r['status'][0] == 2 and r['pose_out'].tobytes() == T[None].tobytes()


# ---- the cases the kernel is held to --------------------------------------------------------------------------------------
def test_the_gpu_cases_do_not_depend_on_the_order_of_the_sums():
    """The kernel adds a window's rows lane by lane, by a butterfly and run by run, the restatement in pixel order.  On every
    case of tests/test_51_sdf_align_gpu.py the two orders give the same x within 1e-10 and the same status: the bound of
    1e-9 there is held by the arithmetic, not by luck; and the cases cover what their names say."""
    seen, xs = {}, {}
    for name, c in A.all_cases():
        want = A.run_case(c)
        for i in range(len(c['frame_of'])):
            if want['status'][i] == 4:
                continue
            rw = A.case_rows(c, i)
            status, x = TR.solve(A.sums_in_kernel_order(rw)) if want['n_pairs'][i] >= 6 else (1, np.zeros(6))
            assert status == want['status'][i] and np.abs(x - want['x'][i]).max() <= 1e-10, (name, i)
        seen[name], xs[name] = (want['n_pairs'].tolist(), want['status'].tolist()), want['x']
    assert seen["1 x 1"] == ([1], [1]) and seen["5 x 1, five rows"] == ([5], [1])
    assert seen["b = 7"][1] == [0, 0, 1, 1, 4, 4, 0] and seen["b = 7"][0][2:6] == [0, 0, 0, 0]
    assert seen["want [7, 2]"][0][0] == 0 and seen["want [0, 0]"] == seen["filter off"] and seen["want [2, 5]"] != seen["filter off"]
    assert np.abs(xs["single votes, min_count 1"] - xs["single votes, min_count 2"]).max() > 1e-3
    assert all(st == [0] and n[0] >= 20 for k, (n, st) in seen.items() if " x " in k and k not in ("1 x 1", "5 x 1, five rows"))
    pixels = [c['wh'] * c['ww'] for _, c in A.window_cases()]
    assert {2047, 2048, 2049} <= set(pixels) and {63, 64, 65} <= {c['ww'] for _, c in A.window_cases()}


# ---- the loop --------------------------------------------------------------------------------------------------------------
def test_tracking_condition_on_the_30_degree_orbit():
    """Following, told from not following: in every frame the error is below a quarter of what holding the previous frame's
    true pose would give, and no frame is lost (front 4 voxels, 4 iterations: the defaults)."""
    o = A.orbit()
    err, hold = S.pose_errors(o['result']['poses'], o['truth'])[1:], A.hold_errors(o['truth'])
    print("pose error per frame, align='sdf': %s" % np.array2string(err, precision=5))
    print("holding the previous true pose:    %s" % np.array2string(hold, precision=5))
    assert not o['result']['lost'].any() and not o['result']['status'].any()
    assert np.all(err < hold / 4.0)
    assert all(len(steps) == 4 for steps in o['result']['steps'][1:])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_lists_the_step_under_602():
    header = open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read()
    assert int(re.search(r"#define\s+CLOUDAAE_ABI_VERSION\s+(\d+)", header).group(1)) == 602
    additions = header[header.index("602: cloudaae_icp_point_to_point"):header.index("#define CLOUDAAE_ABI_VERSION")]
    assert "cloudaae_tsdf_align_step with its workspace query" in additions
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint cloudaae_tsdf_align_step\s*\(", plain) and re.search(r"\blong long cloudaae_tsdf_align_step_workspace\s*\(", plain)
    from cloudaae_amd import _lib
    assert _lib.ABI_VERSION == 602
    assert len(_lib._SIGNATURES["cloudaae_tsdf_align_step"]) == 30
    text = open(os.path.join(ROOT, "cloudaae_amd", "csrc", "Makefile")).read()
    assert "tsdf_align.o" not in text                                             # not in PK_OBJS: built without packed fp32


def test_workspace_query_and_a_workspace_one_byte_short():
    """The step's workspace has the layout of cloudaae_depth_align_step's: the sizes tests/test_workspace_sizes_host.py
    records for that query, literally, and 0 outside the limits; a workspace one byte short is refused in validation, before
    anything is launched (the pointers are fake and never dereferenced, as there)."""
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    cdll = _lib.lib()._cdll
    for args, want in (((3, 33, 35), 688), ((1, 1, 1), 232), ((1, 4096, 4096), 1867776), ((16, 4096, 4096), 29884416),
                       ((1 << 28, 1, 1), 61203283968), ((3, 23, 89), 688), ((1, 3, 683), 456),
                       ((0, 1, 1), 0), ((1, 0, 1), 0), ((1, 1, 0), 0), ((1, 4097, 4096), 0), ((17, 4096, 4096), 0)):
        assert cdll.cloudaae_tsdf_align_step_workspace(*args) == want, args
        if want and args[1] * args[2] != 2047 and args[1] * args[2] != 2049:
            assert cdll.cloudaae_depth_align_step_workspace_bytes(*args) == want, args
    X = 0x1000
    rc = _lib.lib().cloudaae_tsdf_align_step(2, 2, 2, 0.0, 0.0, 0.0, 1.0, X, 1, 4.0, 1, 40, 40, X, None, None, 3, X, X, 33, 35, X, X, X, X, X, X,
                                             X, 688 - 1, None)
    assert rc != 0
    assert cdll.cloudaae_last_error().decode() == ("cloudaae_tsdf_align_step: the workspace is smaller than "
                                                   "cloudaae_tsdf_align_step_workspace or not 8-byte aligned")
