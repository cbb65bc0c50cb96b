"""GPU: cloudaae_depth_edge_nearest, cloudaae_depth_contour_sums and cloudaae_depth_align_solve (csrc/depth_contour.hip)
against the NumPy restatement of DESIGN.md "Contours" (tests/contour_reference.py) from identical inputs, then utils/track.py
with contour=True -- the loop and the sequences -- on the scene whose conditions tests/test_contour_host.py asserts for the
restatement alone.

The nearest map and n_rows are integers and must be equal.  A sum may differ from the restatement's by what two orders of
summation may differ by: 2 wh ww 2^-53 times its sum of |terms| (the bound of tests/test_42_track_gpu.py).  The solve is
held to the restatement's on the SAME sums (the GPU's): status equal, pose_out within 1e-9; a pose that the definition leaves
unchanged is compared bit for bit."""
import numpy as np
import pytest
import torch

import contour_reference as CR
import detect_reference as DR
import track_reference as TR

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
TILE = 32                                                  # EN_TILE of csrc/depth_contour.hip
STEP_UNITS = 200                                           # 2 cm at factor_depth 10000


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def track(hip):
    from cloudaae_amd.utils import track
    return track


@pytest.fixture(scope="module")
def packed(dev):
    from cloudaae_amd.utils import mesh_models
    return mesh_models.pack_meshes(DR.scene_meshes(), device=dev)


def _bits(t):
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int16))


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


# ---- the nearest map --------------------------------------------------------------------------------------------------------
H, W = 72, 96


def nearest_frames():
    """[5,H,W] uint16.  0: sparse single pixels, and a block at 8000 units standing on a block at 8150 (an edge for a step
    below 150 units, none above) with pixels in the frame's four corners; 1: the tie patterns of test_contour_host.py; 2: all
    zero; 3: dense noise; 4: two single pixels placed for the tile border cases."""
    rng = np.random.RandomState(11)
    f = np.zeros((5, H, W), np.uint16)
    f[0] = np.where(rng.rand(H, W) < 0.004, 8000, 0)
    f[0, 20:60, 30:80] = 8150
    f[0, 30:50, 40:70] = 8000
    f[0, 0, 0] = f[0, 0, W - 1] = f[0, H - 1, 0] = f[0, H - 1, W - 1] = 7000
    for u, v in ((4, 7), (10, 7), (27, 4), (27, 10), (44, 7), (50, 7), (47, 4), (47, 10), (65, 5), (69, 5), (65, 9), (69, 9)):
        f[1, v, u] = 8000                                  # left / right about (7, 7), up / down about (27, 7), four ways, diagonal
    f[4, 40, 47] = 8000                                    # 16 pixels right of window pixel (31, 40) of a window at (0, 0)
    f[4, 63, 90] = 8000                                    # 32 pixels below (90, 31)
    f[3] = (7000 + 300 * rng.randint(0, 4, (H, W))) * (rng.rand(H, W) < 0.7)
    return f


def nearest_cases():
    """[(name, frame_of [B], origin [B,2], wh, ww, step [B], radius)]"""
    one = lambda fr, o, wh, ww, R, step=100: ([fr], [o], wh, ww, [step], R)
    out = [('1x1', ) + one(0, (40, 30), 1, 1, 5), ('ww = 1', ) + one(0, (39, 3), 64, 1, 16), ('33x67', ) + one(0, (10, 20), 33, 67, 16)]
    for wh, ww in ((TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (2 * TILE + 1, TILE), (TILE, 2 * TILE + 1),
                   (2 * TILE + 1, 2 * TILE + 1)):
        out.append(('%dx%d' % (wh, ww), ) + one(0, (3, 2), wh, ww, 16))
    out += [('R = %d' % R, ) + one(3 if R < 16 else 0, (5, 1), 40, 70, R) for R in (1, 5, 16, 32)]
    out.append(('exactly R across a tile border, R = 16', ) + one(4, (0, 0), 50, 80, 16))
    out.append(('exactly R across a tile border, R = 32', ) + one(4, (0, 0), 66, 96, 32))
    out.append(('ties', ) + one(1, (0, 0), 15, 80, 5))
    out.append(('negative origin', ) + one(0, (-9, -13), 50, 60, 16))
    out.append(('right and bottom frame edges', ) + one(0, (W - 30, H - 25), 50, 60, 16))
    out.append(('far outside the frame', ) + one(0, (W + 40, -100), 20, 20, 32))
    out.append(('all-zero frame', ) + one(2, (5, 5), 40, 40, 16))
    out.append(('step above the block', ) + one(0, (20, 10), 50, 70, 16, 150))
    out.append(('seven over two frames', [0, 3, -1, 0, 5, 3, 0], [(3, 2), (10, 5), (3, 2), (-20, 40), (3, 2), (60, 50), (30, 20)], 45, 50,
                [100, 100, 100, 100, 100, 400, 150], 16))
    return out


def gpu_nearest(track, dev, frames, case, only=None):
    _, fo, origin, wh, ww, step, R = case
    sel = slice(None) if only is None else slice(only, only + 1)
    n = track.edge_nearest(_bits(frames).to(dev), _i32(fo[sel], dev), _i32(origin[sel], dev).reshape(-1, 2), wh, ww,
                           _i32(step[sel], dev), R)
    torch.cuda.synchronize()
    return n.cpu().numpy()


def test_nearest_equals_the_restatement_bit_for_bit(track, dev):
    frames = nearest_frames()
    for case in nearest_cases():
        name, fo, origin, wh, ww, step, R = case
        want = CR.edge_nearest(frames, fo, origin, wh, ww, step, R)
        got = gpu_nearest(track, dev, frames, case)
        print("%s: %d of %d pixels have an edge within %d" % (name, int((want >= 0).sum()), want.size, R))
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), name
        if name.startswith('exactly R') and R == 16:
            assert (got[0, 40, 31] & 255) - R == 16 and got[0, 40, 30] == -1
        if name.startswith('exactly R') and R == 32:
            assert ((got[0, 31, 90] >> 8) & 255) - R == 32 and got[0, 30, 90] == -1
        if name == 'ties':
            dec = lambda c: ((int(c) & 255) - R, ((int(c) >> 8) & 255) - R)
            assert [dec(got[0, 7, x]) for x in (7, 27, 47, 67)] == [(-3, 0), (0, -3), (0, -3), (-2, -2)]
        if name in ('all-zero frame', 'far outside the frame', 'step above the block'):
            assert (name == 'step above the block') == bool((got >= 0).any())
    seven = nearest_cases()[-1]
    a, b = gpu_nearest(track, dev, frames, seven), gpu_nearest(track, dev, frames, seven)
    assert a.tobytes() == b.tobytes() and np.all(a[2] == -1) and np.all(a[4] == -1)
    for i in range(7):
        assert gpu_nearest(track, dev, frames, seven, only=i)[0].tobytes() == a[i].tobytes(), i


# ---- contour sums and the solve ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(packed):
    """track_reference.step_cases with the hypothesis windows cut from the GPU renderer's own output (as test 42 has them:
    2047, 2048 and 2049 window pixels, ww = 1, 33 x 67, a negative origin, the frame's right and bottom edges, B = 7 over two
    frames with frame_of = -1 and = F and an all-zero hypothesis, the plane patch), each with the step and the radius."""
    from cloudaae_amd.utils import render

    def gpu_renderer(cubes):
        inst = [[(TR.CUBE, 1, np.asarray(c, np.float64)) for c in cs] for cs in cubes]
        out = render.render_frames(packed, inst, np.tile(TR.SCENE_INTR, (len(inst), 1)), TR.SCENE_H, TR.SCENE_W)
        return out['depth'].cpu().numpy().view(np.uint16)
    out = []
    for name, c in TR.step_cases(gpu_renderer):
        B = len(c['frame_of'])
        R = 5 if name == '32x64' else 32 if name == '23x89' else 16
        out.append((name, dict(c, step=np.full(B, 40 if name == 'plane patch' else STEP_UNITS, np.int32), radius=R)))
    return out


def launch(track, dev, c, weight=CR.WEIGHT, only=None):
    """edge_nearest, align_step, contour_sums and solve_sums on the case's arrays (sample `only` alone when given) -> dict of
    numpy arrays: nearest, plane_*, n_rows, sums, x, status, pose_out."""
    sel = slice(None) if only is None else slice(only, only + 1)
    wh, ww = c['depth_hyp'].shape[1:]
    dt, dh = _bits(c['depth_test']).to(dev), _bits(c['depth_hyp'][sel]).to(dev)
    fo, org = _i32(c['frame_of'][sel], dev), _i32(c['origin'][sel], dev)
    rows = torch.from_numpy(np.ascontiguousarray(c['intr_win'][sel], np.float32)).to(dev)
    gate, jump, step = _i32(c['gate'][sel], dev), _i32(c['jump'][sel], dev), _i32(c['step'][sel], dev)
    pose = torch.from_numpy(np.ascontiguousarray(c['pose_in'][sel], np.float64)).to(dev)
    near = track.edge_nearest(dt, fo, org, wh, ww, step, c['radius'])
    plane = track.align_step(dt, fo, org, dh, rows, gate, jump, c['cos_min'], pose)
    con = track.contour_sums(dt, fo, org, dh, rows, gate, step, c['radius'], near)
    s = track.solve_sums(plane, con, weight, pose)
    torch.cuda.synchronize()
    out = {'plane_' + k: v.cpu().numpy() for k, v in plane.items()}
    out.update(nearest=near.cpu().numpy(), n_rows=con['n_rows'].cpu().numpy(), sums=con['sums'].cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in s.items()})
    return out


def test_contour_sums_and_solve_equal_the_restatement(track, dev, cases):
    seen, rows_seen = set(), 0
    for name, c in cases:
        got = launch(track, dev, c)
        B, wh, ww = c['depth_hyp'].shape
        near = CR.edge_nearest(c['depth_test'], c['frame_of'], c['origin'], wh, ww, c['step'], c['radius'])
        assert np.array_equal(got['nearest'], near), name
        want = CR.contour_sums(c['depth_test'], c['frame_of'], c['origin'], c['depth_hyp'], c['intr_win'], c['gate'], c['step'],
                               c['radius'], near)
        bound = 2.0 * wh * ww * 2.0 ** -53 * want['abs_sums']
        diff = np.abs(got['sums'] - want['sums'])
        worst = float((diff / np.where(bound > 0, bound, 1.0)).max())
        solved = CR.solve_sums(got['plane_sums'], got['plane_n_pairs'], got['plane_status'], got['sums'], got['n_rows'], CR.WEIGHT,
                               c['pose_in'])
        print("%s: n_rows %s n_pairs %s status %s (plane alone %s); worst sum at %.3g of its bound; pose within %.3g"
              % (name, got['n_rows'], got['plane_n_pairs'], got['status'], got['plane_status'], worst,
                 float(np.abs(got['pose_out'] - solved['pose_out']).max())))
        assert np.array_equal(got['n_rows'], want['n_rows']), name
        assert np.all(diff <= bound), name
        assert np.array_equal(got['status'], solved['status']), name
        assert np.abs(got['pose_out'] - solved['pose_out']).max() <= POSE_TOL, name
        assert np.abs(got['x'] - solved['x']).max() <= POSE_TOL, name
        zero_w = launch(track, dev, c, weight=0.0)
        rows_seen += int(got['n_rows'].sum())
        for b in range(B):
            seen.add(int(got['status'][b]))
            if got['status'][b] != 0:
                assert got['pose_out'][b].tobytes() == np.asarray(c['pose_in'][b], np.float64).tobytes(), (name, b)
                assert np.all(got['x'][b] == 0.0)
            else:
                assert got['plane_n_pairs'][b] + got['n_rows'][b] >= 6 and np.all(got['pose_out'][b, 3] == [0.0, 0.0, 0.0, 1.0])
            if got['plane_status'][b] == 4:
                assert got['status'][b] == 4 and got['n_rows'][b] == 0 and np.all(got['sums'][b] == 0.0)
                assert np.all(got['nearest'][b] == -1)
            if got['plane_status'][b] != 1:                # weight 0: align_step's own pose (a step with fewer than six
                assert zero_w['pose_out'][b].tobytes() == got['plane_pose_out'][b].tobytes(), (name, b)    # pairs solves nothing)
    assert {0, 1, 4} <= seen and rows_seen > 500


def test_the_all_zero_hypothesis_has_no_rows_and_status_1(track, dev, cases):
    c = dict(cases)['seven over two frames']
    got = launch(track, dev, c)
    assert not c['depth_hyp'][6].any() and got['n_rows'][6] == 0 and got['plane_n_pairs'][6] == 0 and got['status'][6] == 1
    assert np.all(got['sums'][6] == 0.0)


def test_two_runs_and_the_batch_give_the_same_bits(track, dev, cases):
    c = dict(cases)['seven over two frames']
    a, b = launch(track, dev, c), launch(track, dev, c)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for i in range(len(c['frame_of'])):
        alone = launch(track, dev, c, only=i)
        for k in a:
            assert alone[k][0].tobytes() == a[k][i].tobytes(), (k, i)


def test_solve_statuses_on_hand_made_sums(track, dev):
    """Every status of the shared solve from hand-made sums (1, A's upper triangle by rows, b), status 3 -- a solution that is
    not finite -- among them, which no image of the other tests reaches.  Eight rows with n_pairs = 6, n_rows = 0 and plane
    status 0, then three rows on the good sums that the counts and the plane status decide; the eight alone must give the
    same bits as inside the eleven."""
    good, b0 = np.diag(np.arange(1.0, 7.0)) + 0.1, np.arange(1.0, 7.0) * 1e-3
    edit = lambda a, at, v: np.where(np.isin(np.arange(a.size).reshape(a.shape), at), v, a)
    table = [(good, b0, 0), (np.zeros((6, 6)), b0, 2), (np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]), b0, 2),
             (edit(good, [0], np.inf), b0, 2), (edit(good, [1, 6], np.nan), b0, 2), (np.ones((6, 6)), b0, 2),
             (good, edit(b0, [2], np.nan), 3), (good, edit(b0, [5], np.inf), 3)]
    table += [(good, b0, 1), (good, b0, 0), (good, b0, 4)]
    sums = np.array([np.concatenate([[1.0], A[np.triu_indices(6)], b]) for A, b, _ in table])
    n_pairs = np.array([6] * 8 + [5, 3, 6], np.int32)
    n_rows = np.array([0] * 8 + [0, 3, 0], np.int32)
    plane_status = np.array([0] * 8 + [0, 0, 4], np.int32)
    expected = np.array([st for _, _, st in table], np.int32)
    pose_in = np.tile(TR.update_matrix([0.3, -0.2, 0.5, 0.1, -0.05, 0.9]), (len(table), 1, 1))

    def gpu(contour, weight, B):
        plane = dict(sums=torch.from_numpy(sums[:B]).to(dev), n_pairs=_i32(n_pairs[:B], dev), status=_i32(plane_status[:B], dev))
        con = dict(sums=torch.from_numpy(np.ascontiguousarray(contour[:B])).to(dev), n_rows=_i32(n_rows[:B], dev))
        out = track.solve_sums(plane, con, weight, torch.from_numpy(pose_in[:B].copy()).to(dev))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    for contour, weight in ((np.zeros_like(sums), 0.0), (sums, 0.5)):
        with np.errstate(all='ignore'):
            want = CR.solve_sums(sums, n_pairs, plane_status, contour, n_rows, weight, pose_in)
        got, eight = gpu(contour, weight, len(table)), gpu(contour, weight, 8)
        print("weight %g: status %s (restatement %s)" % (weight, got['status'], want['status']))
        assert np.array_equal(want['status'], expected) and np.array_equal(got['status'], want['status'])
        for b in range(len(table)):
            if expected[b] == 0:
                print("row %d: x within %.3g, pose within %.3g" % (b, np.abs(got['x'][b] - want['x'][b]).max(),
                                                                   np.abs(got['pose_out'][b] - want['pose_out'][b]).max()))
                assert np.abs(got['x'][b] - want['x'][b]).max() <= POSE_TOL
                assert np.abs(got['pose_out'][b] - want['pose_out'][b]).max() <= POSE_TOL
            else:
                assert got['pose_out'][b].tobytes() == pose_in[b].tobytes() and np.all(got['x'][b] == 0.0), b
        for k in got:
            assert eight[k].tobytes() == got[k][:8].tobytes(), k


def test_errors_launch_nothing(hip, dev):
    L = hip.lib()
    d = torch.zeros(64, dtype=torch.int64, device=dev)
    p = d.data_ptr()
    assert L.cloudaae_depth_contour_sums_workspace_bytes(1, 8, 8) == 232 and L.cloudaae_depth_contour_sums_workspace_bytes(0, 8, 8) == 0
    assert L.cloudaae_depth_contour_sums_workspace_bytes(3, 33, 67) == 3 * 2 * 28 * 8 + 24

    def nearest(f=1, h=4, w=4, b=1, wh=2, ww=2, radius=4, out=p):
        return L.cloudaae_depth_edge_nearest(f, h, w, p, b, p, p, wh, ww, p, radius, out, hip.stream())

    def sums(f=1, h=4, w=4, b=1, wh=2, ww=2, radius=4, ws=p, ws_bytes=232, near=p):
        return L.cloudaae_depth_contour_sums(f, h, w, p, b, p, p, wh, ww, p, p, p, p, radius, near, p, p, ws, ws_bytes, hip.stream())

    def solve(b=1, weight=0.5, pose=p):
        return L.cloudaae_depth_align_solve(b, p, p, p, p, p, weight, pose, p, p, p, hip.stream())
    for fn, name, kws in ((nearest, b"cloudaae_depth_edge_nearest", (dict(f=0), dict(b=0), dict(ww=0), dict(h=1 << 13, w=(1 << 11) + 1),
                                                                     dict(radius=0), dict(radius=33), dict(out=None))),
                          (sums, b"cloudaae_depth_contour_sums", (dict(f=0), dict(wh=0), dict(radius=0), dict(radius=33), dict(near=None),
                                                                  dict(ws=None), dict(ws_bytes=231), dict(ws=p + 4))),
                          (solve, b"cloudaae_depth_align_solve", (dict(b=0), dict(weight=float('nan')), dict(pose=None)))):
        for kw in kws:
            assert fn(**kw) != 0, (name, kw)
            assert name in L.cloudaae_last_error(), (name, kw)
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0


# ---- the loop and the sequences ---------------------------------------------------------------------------------------------
def test_loop_follows_the_restatement_step_by_step(track, dev, packed):
    depth, truth = CR.frames(CR.PRISM, TR.SLOW)
    start = TR.off_pose(truth[0])
    meshes = DR.scene_meshes()
    a = track.align_poses(depth[:1], TR.SCENE_INTR, packed, [CR.PRISM], [0], start[None], return_trajectory=True, contour=True)
    traj = a['trajectory'].cpu().numpy()
    n_pairs, status = a['n_pairs_steps'].cpu().numpy(), a['status_steps'].cpu().numpy()
    ref = TR.align(depth[:1], TR.SCENE_INTR, meshes, [CR.PRISM], [0], start[None], iterations=0)
    assert np.array_equal(a['origin'], ref['origin']) and (a['wh'], a['ww']) == (ref['wh'], ref['ww']) and a['ok'].all()
    assert traj.shape == (5, 1, 4, 4) and traj[0].tobytes() == start[None].tobytes()
    factor = float(TR.SCENE_INTR[0, 4])
    gate, jump, step = (TR.V.tau_units([v], [factor]) for v in (0.03, 0.005, CR.STEP))
    near = CR.edge_nearest(depth[:1], [0], ref['origin'], ref['wh'], ref['ww'], step, CR.RADIUS)
    for i in range(4):
        hyp = TR.render_windows(meshes, [CR.PRISM], traj[i], ref['rows'], ref['wh'], ref['ww'])
        want = CR.step(depth[:1], [0], ref['origin'], hyp, ref['rows'], gate, jump, 0.8, traj[i], step, CR.RADIUS, CR.WEIGHT, near)
        print("step %d: n_pairs %d n_rows %d, pose within %.3g of the restatement's step, %.3g of the truth"
              % (i, n_pairs[i, 0], want['n_rows'][0], np.abs(traj[i + 1] - want['pose_out']).max(), TR.pose_error(traj[i + 1, 0], truth[0])))
        assert n_pairs[i, 0] == want['n_pairs'][0] and status[i, 0] == want['status'][0] == 0 and want['n_rows'][0] > 0
        assert np.abs(traj[i + 1] - want['pose_out']).max() <= POSE_TOL
    assert a['poses'].cpu().numpy().tobytes() == traj[4].tobytes()


@pytest.mark.parametrize("obj", [CR.PRISM, CR.PLATE], ids=["prism", "plate"])
def test_sequences(track, packed, obj):
    want, truth, ref = CR.sequence(obj, TR.SLOW, 'constant')
    depth, _ = CR.frames(obj, TR.SLOW)
    t = track.track_objects(depth, TR.SCENE_INTR, packed, ([obj], truth[:1]), contour=True)
    for f in range(TR.FRAMES):
        got = TR.pose_error(t.poses[f, 0], truth[f])
        print("frame %d: error %.3g (restatement %.3g), score %d / %d, pairs %d" % (f, got, ref[f], t.num[f, 0], t.den[f, 0], t.n_pairs[f, 0]))
        assert got <= ref[f] + 1e-6
    assert not t.lost.any() and np.all(t.status == 0)


def test_tracking_with_the_term_replayed_by_hand(track, dev, packed):
    """track_objects(contour=True) over two frames, then the same frames by hand with the bindings alone -- pose_windows, one
    edge_nearest per frame, per step render, align_step, contour_sums, solve_sums, then the final render and the counts:
    poses, num, den, n_pairs and status are equal bit for bit."""
    from cloudaae_amd.utils import detect, render
    depth, truth = CR.frames(CR.PRISM, TR.SLOW)
    t = track.track_objects(depth[:2], TR.SCENE_INTR, packed, ([CR.PRISM], truth[:1]), contour=True)
    dt = _bits(depth[:2]).to(dev)
    intr = np.asarray(TR.SCENE_INTR, np.float32).reshape(-1, 5)[:1]
    factor = [float(intr[0, 4])]
    gate, jump, step, tau = (_i32(TR.V.tau_units([v], factor), dev) for v in (0.03, 0.005, CR.STEP, 0.01))
    mesh, ones, offs = np.array([CR.PRISM]), np.ones(1, np.int64), np.arange(2)
    last = truth[0]
    for f in range(2):
        origin, wh, ww, ok = track.pose_windows(last[None], track.mesh_aabb(packed)[mesh], intr, TR.SCENE_H, TR.SCENE_W)
        assert ok[0]
        rows_host = intr.copy()
        rows_host[:, 2] = intr[0, 2] - origin[:, 0].astype(np.float32)
        rows_host[:, 3] = intr[0, 3] - origin[:, 1].astype(np.float32)
        rows, org, frame = torch.from_numpy(rows_host).to(dev), _i32(origin, dev), _i32([f], dev)
        pose = torch.from_numpy(last[None].copy()).to(dev)
        near = track.edge_nearest(dt, frame, org, wh, ww, step, CR.RADIUS)
        for _ in range(4):
            d = render.render_instances(packed, rows, offs, mesh, ones, pose.view(1, 16), wh, ww)[0]
            plane = track.align_step(dt, frame, org, d, rows, gate, jump, 0.8, pose)
            con = track.contour_sums(dt, frame, org, d, rows, gate, step, CR.RADIUS, near)
            solved = track.solve_sums(plane, con, CR.WEIGHT, pose)
            pose = solved['pose_out']
        d = render.render_instances(packed, rows, offs, mesh, ones, pose.view(1, 16), wh, ww)[0]
        c = detect.fit_counts_window(dt, None, frame, None, org, d.view(1, 1, wh, ww), tau)['counts'].cpu().numpy().reshape(6).astype(np.int64)
        num, den = int(c[1]), int(c[1] + c[2] + c[3])
        num, den = (num, den) if den > 0 else (0, 1)
        assert not num * 2 < 1 * den and not t.lost[f, 0]
        last = pose.cpu().numpy()[0]
        print("frame %d: score %d / %d, pairs %d, rows %d" % (f, num, den, int(plane['n_pairs'][0]), int(con['n_rows'][0])))
        assert t.poses[f, 0].tobytes() == last.tobytes(), f
        assert (int(t.num[f, 0]), int(t.den[f, 0])) == (num, den), f
        assert (int(t.n_pairs[f, 0]), int(t.status[f, 0])) == (int(plane['n_pairs'][0]), int(solved['status'][0])), f
    assert t.poses.dtype == np.float64 and t.n_pairs.dtype == np.int32 and t.status.dtype == np.int32


def test_contour_none_is_the_tracker_as_before(track, dev, packed, monkeypatch):
    """With contour=None none of the new entries is called, and the loop is render + align_step, bit for bit."""
    from cloudaae_amd.utils import render
    depth, truth = CR.frames(CR.PRISM, TR.SLOW)
    with_term = track.track_objects(depth[:3], TR.SCENE_INTR, packed, ([CR.PRISM], truth[:1]), contour=True)

    def never(*a, **k):
        raise AssertionError("a contour entry was called with contour=None")
    for fn in ("edge_nearest", "contour_sums", "solve_sums"):
        monkeypatch.setattr(track, fn, never)
    a = track.align_poses(depth[:2], np.tile(TR.SCENE_INTR, (2, 1)), packed, [CR.PRISM], [1], truth[:1], return_trajectory=True,
                          contour=None)
    dv = a['device']
    factor = float(TR.SCENE_INTR[0, 4])
    gate, jump = (_i32(TR.V.tau_units([v], [factor]), dev) for v in (0.03, 0.005))
    pose = torch.from_numpy(truth[:1].copy()).to(dev)
    for i in range(4):
        d = render.render_instances(packed, dv['rows'], np.arange(2), np.array([CR.PRISM]), np.ones(1, np.int64), pose.view(1, 16),
                                    a['wh'], a['ww'])[0]
        pose = track.align_step(dv['depth'], dv['frame_of'], dv['origin'], d, dv['rows'], gate, jump, 0.8, pose)['pose_out']
        assert a['trajectory'][i + 1].cpu().numpy().tobytes() == pose.cpu().numpy().tobytes(), i
    off = track.track_objects(depth[:3], TR.SCENE_INTR, packed, ([CR.PRISM], truth[:1]), contour=None)
    default = track.track_objects(depth[:3], TR.SCENE_INTR, packed, ([CR.PRISM], truth[:1]))
    assert off.poses.tobytes() == default.poses.tobytes() and np.array_equal(off.status, default.status)
    assert np.array_equal(off.n_pairs, default.n_pairs) and np.array_equal(off.num, default.num)
    assert off.poses.tobytes() != with_term.poses.tobytes()
