"""NumPy restatement of DESIGN.md, "Depth components": the dominant plane of a depth frame by hypothesis voting, the
foreground that stands on it, its connected components and their ordered table.  Written from the definition.  The
back-projection is float32 (NumPy rounds every operation, as the un-fused kernel does), everything after it float64 in
the written order, the components come from a plain union-find -- so every output is an integer, or a double of one
hypothesis, and is expected to equal the kernels' bit for bit.  The input builders of the tests are at the end."""
import numpy as np

import depth_noise_reference as DN
import mesh_models_reference as MR
import pose_sampling_reference as PS
import render_reference as RR

STREAM_PLANE = 25
DEFAULTS = dict(n_hyp=256, stride=4, tol=0.01, max_height=0.5, min_plane_percent=10, jump=0.02, min_pixels=200,
                max_components=32)


def backproject(depth, intr):
    """[H,W] uint16 -> [H,W,3] float64: "Frame segments" in float32, then widened."""
    fx, fy, cx, cy, factor = (np.float32(k) for k in np.asarray(intr, np.float32))
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    with np.errstate(all='ignore'):
        dm = depth.astype(np.float32) / factor
        x = ((u.astype(np.float32) - cx) * dm) / fx
        y = ((v.astype(np.float32) - cy) * dm) / fy
    assert x.dtype == np.float32 and y.dtype == np.float32 and dm.dtype == np.float32
    return np.stack([x, y, dm], axis=-1).astype(np.float64)


def hypotheses(depth, pts, seed, frame_index, n_hyp):
    """The n_hyp hypotheses of one frame: (n [n_hyp,3], d, q [n_hyp], void [n_hyp] bool, pixels [n_hyp,3]); a void
    hypothesis has n = d = q = 0."""
    H, W = depth.shape
    ctr = (np.uint64(frame_index) << np.uint64(20)) | np.arange(n_hyp, dtype=np.uint64)
    r = PS.philox4x32(seed, ctr, STREAM_PLANE)
    pix = ((r[:, :3].astype(np.uint64) * np.uint64(H * W)) >> np.uint64(32)).astype(np.int64)
    flat, P = depth.reshape(-1), pts.reshape(-1, 3)
    n, d, q = np.zeros((n_hyp, 3)), np.zeros(n_hyp), np.zeros(n_hyp)
    void = np.ones(n_hyp, bool)
    for h in range(n_hyp):
        if np.any(flat[pix[h]] == 0):
            continue
        P0, P1, P2 = (P[p] for p in pix[h])
        e1, e2 = P1 - P0, P2 - P0
        nx = e1[1] * e2[2] - e1[2] * e2[1]
        ny = e1[2] * e2[0] - e1[0] * e2[2]
        nz = e1[0] * e2[1] - e1[1] * e2[0]
        qq = (nx * nx + ny * ny) + nz * nz
        if not qq > 0:
            continue
        dd = -((nx * P0[0] + ny * P0[1]) + nz * P0[2])
        if dd < 0:
            nx, ny, nz, dd = -nx, -ny, -nz, -dd
        n[h], d[h], q[h], void[h] = (nx, ny, nz), dd, qq, False
    return n, d, q, void, pix


def signed(pts, n, d):
    return ((n[0] * pts[..., 0] + n[1] * pts[..., 1]) + n[2] * pts[..., 2]) + d


def plane(depth, intr, seed=0, first_frame=0, n_hyp=256, stride=4, tol=0.01, min_plane_percent=10):
    """One frame's plane stage (the frame's global index is first_frame): dict(count [n_hyp], tested, plane [4], plane_hyp)."""
    pts = backproject(depth, intr)
    n, d, q, void, _ = hypotheses(depth, pts, seed, first_frame, n_hyp)
    sub, sub_pts = depth[::stride, ::stride], pts[::stride, ::stride]
    valid = sub != 0
    tested = int(valid.sum())
    count = np.zeros(n_hyp, np.int32)
    for h in range(n_hyp):
        if void[h]:
            continue
        s = signed(sub_pts, n[h], d[h])
        count[h] = int((valid & (s * s <= (tol * tol) * q[h])).sum())
    best = int(np.argmax(count))                    # the first of the largest: ties to the lowest h
    has = int(count[best]) >= 3 and int(count[best]) * 100 >= int(min_plane_percent) * tested
    return dict(count=count, tested=tested, plane=np.concatenate([n[best], [d[best]]]) if has else np.zeros(4),
                plane_hyp=best if has else -1)


def foreground(depth, intr, pl, plane_hyp, tol=0.01, max_height=0.5):
    valid = depth != 0
    if plane_hyp < 0:
        return valid.astype(np.uint8)
    pts = backproject(depth, intr)
    n, d = pl[:3], pl[3]
    q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    s = signed(pts, n, d)
    with np.errstate(all='ignore'):
        on = valid & (s > 0) & (s * s > (tol * tol) * q) & (s * s <= (max_height * max_height) * q)
    return on.astype(np.uint8)


def components(depth, fg, jump_units):
    """root [H,W] int32: the smallest pixel index of the pixel's component, -1 for background.  A plain union-find."""
    H, W = depth.shape
    on = (np.asarray(fg) != 0).reshape(-1)
    d = depth.astype(np.int64).reshape(-1)
    parent = np.arange(H * W)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for p in np.nonzero(on)[0]:
        u, v = p % W, p // W
        if u + 1 < W and on[p + 1] and abs(d[p] - d[p + 1]) <= jump_units:
            unite(p, p + 1)
        if v + 1 < H and on[p + W] and abs(d[p] - d[p + W]) <= jump_units:
            unite(p, p + W)
    root = np.full(H * W, -1, np.int32)
    for p in np.nonzero(on)[0]:
        root[p] = find(p)
    return root.reshape(H, W)


def table(root, min_pixels=200, max_components=32):
    """dict(label [H,W] uint8, n_components, n_candidates, comp_root, comp_size [max_components], comp_box [.,4])."""
    H, W = root.shape
    flat = root.reshape(-1)
    roots, sizes = np.unique(flat[flat >= 0], return_counts=True)
    cand = [(int(r), int(s)) for r, s in zip(roots, sizes) if s >= min_pixels]
    cand.sort(key=lambda rs: (-rs[1], rs[0]))
    keep = cand[:max_components]
    label = np.zeros((H, W), np.uint8)
    comp_root = np.full(max_components, -1, np.int32)
    comp_size = np.full(max_components, -1, np.int32)
    comp_box = np.full((max_components, 4), -1, np.int32)
    for k, (r, s) in enumerate(keep):
        m = root == r
        label[m] = k + 1
        v, u = np.nonzero(m)
        comp_root[k], comp_size[k], comp_box[k] = r, s, (u.min(), v.min(), u.max(), v.max())
    return dict(label=label, n_components=len(keep), n_candidates=len(cand), comp_root=comp_root, comp_size=comp_size,
                comp_box=comp_box, n_all=len(roots))


def jump_units(jump, factor_depth):
    return int(np.floor(float(jump) * float(np.float32(factor_depth)) + 0.5))


def segment(depth, intrinsics, seed=0, first_frame=0, n_hyp=256, stride=4, tol=0.01, max_height=0.5, min_plane_percent=10,
            jump=0.02, min_pixels=200, max_components=32, jump_units_=None):
    """The whole definition for depth [F,H,W]: a list of per-frame dicts (plane stage, fg, root, table)."""
    out = []
    for f in range(len(depth)):
        r = plane(depth[f], intrinsics[f], seed, first_frame + f, n_hyp, stride, tol, min_plane_percent)
        r['fg'] = foreground(depth[f], intrinsics[f], r['plane'], r['plane_hyp'], tol, max_height)
        ju = jump_units(jump, intrinsics[f][4]) if jump_units_ is None else int(jump_units_[f])
        r['jump_units'] = ju
        r['root'] = components(depth[f], r['fg'], ju)
        r.update(table(r['root'], min_pixels, max_components))
        out.append(r)
    return out


def match(found_label, other_label, depth, value):
    """(k, iou) of one frame: the component with the largest IoU against other_label == value on valid pixels, compared in
    integers (n_k union_j > n_j union_k, ties to the lowest k); (0, 0.0) when nothing overlaps."""
    target = (other_label == value) & (depth != 0)
    best, best_n, best_u = 0, 0, 1
    for k in range(1, int(found_label.max()) + 1):
        m = found_label == k
        n, u = int((m & target).sum()), int((m | target).sum())
        if n > 0 and n * best_u > best_n * u:
            best, best_n, best_u = k, n, u
    return best, (float(best_n) / float(best_u) if best else 0.0)


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------
SCENE_INTR = np.array([[75.0, 74.0, 39.3, 29.6, 1000.0]], np.float32)
SCENE_H, SCENE_W = 60, 80
SCENE_PARAMS = dict(seed=1, n_hyp=64, stride=2, tol=0.01, max_height=0.5, min_plane_percent=10)
SCENE_JUMP_UNITS = 20
SCENE_SPHERES = [(-0.25, 0.0, 0.10), (0.2, 0.1, 0.07), (0.22, -0.12, 0.05)]
_cache = {}


def scene_frames():
    """The table scene: a plane (label 1) and three spheres resting on it (labels 2-4)."""
    T = RR.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])
    normal = T[:3, :3] @ np.array([0.0, 0.0, 1.0])
    if normal @ T[:3, 3] > 0:                      # towards the camera, which sits at the origin
        normal = -normal
    frame = [(1, 1, T)]
    for i, (x, y, rad) in enumerate(SCENE_SPHERES):
        centre = (T @ np.array([x, y, 0.0, 1.0]))[:3] + rad * normal
        S = np.eye(4)
        S[:3, :3] *= rad
        S[:3, 3] = centre
        frame.append((0, 2 + i, S))
    return [MR.icosphere(2), DN.plane_mesh()], [frame]


def scene():
    """(depth [1,60,80] uint16, label [1,60,80] uint8, intrinsics [1,5]) of the table scene, rendered once."""
    if 'scene' not in _cache:
        meshes, frames = scene_frames()
        r = RR.render(meshes, frames, SCENE_INTR, SCENE_H, SCENE_W)
        _cache['scene'] = (r['depth'], r['label'], SCENE_INTR)
    return _cache['scene']


def scene_result(min_pixels=16, max_components=32):
    key = ('result', min_pixels, max_components)
    if key not in _cache:
        depth, _, intr = scene()
        _cache[key] = segment(depth, intr, jump_units_=[SCENE_JUMP_UNITS], min_pixels=min_pixels,
                              max_components=max_components, **SCENE_PARAMS)[0]
    return _cache[key]


def serpentine(H, W):
    """A one-pixel-wide path that covers every other row and joins the rows at alternating ends: one component whose
    pixels, in path order, start at pixel 0.  -> (mask [H,W] bool, length)."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for i, v in enumerate(range(1, H, 2)):
        m[v, W - 1 if i % 2 == 0 else 0] = True
    if H % 2 == 0:
        m[H - 1] = False                           # the last row would hang below the last full row: leave it out
    return m, int(m.sum())


def u_shape(H, W):
    """Two arms down the left and right columns that meet only in the last row."""
    m = np.zeros((H, W), bool)
    m[:, 0] = m[:, W - 1] = m[H - 1, :] = True
    return m


def combs(H, W):
    """Two interleaved combs that never touch: spine on the top row with teeth down the columns 0, 4, 8, ..; spine on the
    bottom row with teeth up the columns 2, 6, ...  -> (mask, mask of the first comb)."""
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    if H < 5 or W < 3:
        a[0, 0] = True
        return a, a
    a[0, :] = True
    a[0:H - 2, 0::4] = True
    b[H - 1, :] = True
    b[2:H, 2::4] = True
    assert not (a & b).any()
    return a | b, a


def checkerboard(H, W):
    v, u = np.mgrid[0:H, 0:W]
    return (u + v) % 2 == 0
