"""NumPy restatement of DESIGN.md, "Detections".  Written from the definition: the windowed counts gather every window
pixel from its frame pixel (or nothing, outside the frame) and count on int64; the assignment uses Python's unbounded
integers and plain loops; the windows are integer arithmetic.  The hypotheses' images are rendered by
render_reference.render with the window's shifted principal point."""
from fractions import Fraction

import numpy as np

import depth_components_reference as D
import depth_noise_reference as DN
import mesh_models_reference as MR
import pose_verify_reference as V
import render_reference as R


# ---- cloudaae_depth_fit_counts_window ------------------------------------------------------------------------------------
def window_pixels(image, u0, v0, wh, ww, outside):
    """[wh,ww] int64: window pixel (x, y) = image pixel (u0 + x, v0 + y), `outside` where that is no pixel of the image."""
    H, W = image.shape
    out = np.full((wh, ww), outside, np.int64)
    for y in range(wh):
        v = v0 + y
        if v < 0 or v >= H:
            continue
        for x in range(ww):
            u = u0 + x
            if 0 <= u < W:
                out[y, x] = int(image[v, u])
    return out


def fit_counts_window(depth_test, label, frame_of, want, origin, wh, ww, depth_hyp, tau):
    """-> counts [B,P,6] int32, seg_total [B] int32, abs_sum [B,P] int64.  depth_hyp [B,P,wh,ww] uint16, origin [B,2]."""
    dt, dh = np.asarray(depth_test), np.asarray(depth_hyp)
    assert dt.dtype == np.uint16 and dh.dtype == np.uint16 and dh.shape[2:] == (wh, ww)
    F = len(dt)
    B, P = dh.shape[:2]
    counts = np.zeros((B, P, 6), np.int32)
    seg_total = np.zeros(B, np.int32)
    abs_sum = np.zeros((B, P), np.int64)
    for b in range(B):
        fr = int(frame_of[b])
        if fr < 0 or fr >= F:
            continue
        u0, v0 = int(origin[b][0]), int(origin[b][1])
        t = window_pixels(dt[fr], u0, v0, wh, ww, 0)
        seg = np.zeros((wh, ww), bool)
        if label is not None:
            seg = (window_pixels(np.asarray(label)[fr], u0, v0, wh, ww, -1) == int(want[b])) & (t != 0)
        seg_total[b] = seg.sum()
        tu = int(tau[b])
        for j in range(P):
            d = dh[b, j].astype(np.int64)
            rendered, both = d != 0, (d != 0) & (t != 0)
            consistent = both & (np.abs(d - t) <= tu)
            counts[b, j] = [rendered.sum(), consistent.sum(), (both & (t - d > tu)).sum(), (both & (d - t > tu)).sum(),
                            (rendered & (t == 0)).sum(), (seg & consistent).sum()]
            abs_sum[b, j] = np.abs(d - t)[consistent].sum()
    return counts, seg_total, abs_sum


# ---- cloudaae_detect_assign ------------------------------------------------------------------------------------------------
def pair_fractions(counts, seg_total, valid, n_components, mode):
    """Step 1 -> (hyp, num, den) [F,K,C] as Python-int object arrays would be: int64 arrays."""
    counts = np.asarray(counts)
    F, K, C, P = counts.shape[:4]
    hyp, num, den = (np.zeros((F, K, C), np.int64) for _ in range(3))
    for f in range(F):
        nc = min(max(int(n_components[f]), 0), K)
        for k in range(K):
            for c in range(C):
                fr = [V.fraction(counts[f, k, c, j], seg_total[f, k, c], bool(valid[f, k, c, j]) and k < nc, mode)
                      for j in range(P)]
                w = 0
                for j in range(1, P):
                    if fr[j][0] * fr[w][1] > fr[w][0] * fr[j][1]:
                        w = j
                hyp[f, k, c], num[f, k, c], den[f, k, c] = w, fr[w][0], fr[w][1]
    return hyp, num, den


def greedy(num, den, nc, min_num, min_den, max_per_class):
    """Step 2 of one frame on num, den [K,C] -> the assignments [(k, c)] in the order of their rounds."""
    K, C = num.shape
    taken, used, out = set(), [0] * C, []
    for _ in range(nc):
        best = None
        for k in range(nc):
            for c in range(C):
                n, d = int(num[k, c]), int(den[k, c])
                if k in taken or used[c] >= max_per_class or n <= 0 or n * min_den < min_num * d:
                    continue
                if best is None or n * best[1] > best[0] * d:       # (k, c) ascending: a tie stays with the earlier pair
                    best = (n, d, k, c)
        if best is None:
            break
        taken.add(best[2])
        used[best[3]] += 1
        out.append((best[2], best[3]))
    return out


def assign(counts, seg_total, valid, pose, n_components, mode=0, min_num=1, min_den=2, max_per_class=1):
    """-> dict of pair_hyp, pair_num, pair_den [F,K,C] int32, pair_score [F,K,C] float64, det_class, det_hyp, det_num,
    det_den, det_rank, alt_class, alt_num, alt_den [F,K] int32, det_score [F,K], det_pose [F,K,4,4] float64, n_det [F]."""
    counts, pose = np.asarray(counts), np.asarray(pose, np.float64)
    F, K, C, P = counts.shape[:4]
    pose = pose.reshape(F, K, C, P, 4, 4)
    hyp, num, den = pair_fractions(counts, seg_total, valid, n_components, mode)
    r = dict(pair_hyp=hyp.astype(np.int32), pair_num=num.astype(np.int32), pair_den=den.astype(np.int32),
             pair_score=np.array([float(n) / float(d) for n, d in zip(num.ravel(), den.ravel())], np.float64).reshape(F, K, C))
    for key, fill in (("det_class", -1), ("det_hyp", -1), ("det_num", 0), ("det_den", 1), ("det_rank", -1), ("alt_class", -1),
                      ("alt_num", 0), ("alt_den", 1)):
        r[key] = np.full((F, K), fill, np.int32)
    r["det_score"] = np.zeros((F, K), np.float64)
    r["det_pose"] = np.zeros((F, K, 4, 4), np.float64)
    r["n_det"] = np.zeros(F, np.int32)
    for f in range(F):
        nc = min(max(int(n_components[f]), 0), K)
        picked = greedy(num[f], den[f], nc, int(min_num), int(min_den), int(max_per_class))
        r["n_det"][f] = len(picked)
        for rank, (k, c) in enumerate(picked):
            r["det_class"][f, k], r["det_hyp"][f, k], r["det_rank"][f, k] = c, hyp[f, k, c], rank
            r["det_num"][f, k], r["det_den"][f, k] = num[f, k, c], den[f, k, c]
            r["det_score"][f, k] = float(num[f, k, c]) / float(den[f, k, c])
            r["det_pose"][f, k] = pose[f, k, c, hyp[f, k, c]]
        for k in range(K):
            best = None
            for c in range(C):
                if c == r["det_class"][f, k]:
                    continue
                n, d = int(num[f, k, c]), int(den[f, k, c])
                if best is None or n * best[1] > best[0] * d:
                    best = (n, d, c)
            if best is not None:
                r["alt_num"][f, k], r["alt_den"][f, k], r["alt_class"][f, k] = best
    return r


# ---- windows ---------------------------------------------------------------------------------------------------------------
def _ceil_times(margin, n):
    m = Fraction(str(margin)) if isinstance(margin, float) else Fraction(margin)
    q = m * n
    return -((-q.numerator) // q.denominator)


def windows(comp_box, n_components, H, W, margin=0.5):
    """-> (origin [F,K,2] int32, wh, ww).  comp_box [F,K,4] = (u_min, v_min, u_max, v_max); the first n_components [f] boxes
    of a frame count."""
    box = np.asarray(comp_box, np.int64)
    F, K = box.shape[:2]
    live = [(f, k) for f in range(F) for k in range(min(int(n_components[f]), K))]
    need_w, need_h = 1, 1
    for f, k in live:
        bw, bh = int(box[f, k, 2] - box[f, k, 0] + 1), int(box[f, k, 3] - box[f, k, 1] + 1)
        need_w, need_h = max(need_w, bw + 2 * _ceil_times(margin, bw)), max(need_h, bh + 2 * _ceil_times(margin, bh))
    ww = (min(need_w, W) + 7) // 8 * 8
    wh = min(need_h, H)
    origin = np.zeros((F, K, 2), np.int32)
    for f, k in live:
        bw, bh = int(box[f, k, 2] - box[f, k, 0] + 1), int(box[f, k, 3] - box[f, k, 1] + 1)
        origin[f, k] = (int(box[f, k, 0]) - (ww - bw) // 2, int(box[f, k, 1]) - (wh - bh) // 2)
    return origin, wh, ww


# ---- score_candidates ------------------------------------------------------------------------------------------------------
def render_windows(meshes, mesh_of_class, poses, intr, origin, n_components, wh, ww):
    """Every hypothesis of a live sample alone in its window: -> (depth_hyp [F,K,C,P,wh,ww] uint16, zeros for k >=
    n_components, dropped [F,K,C,P] int32).  The window's intrinsics are (fx, fy, cx - u0, cy - v0, factor), the
    differences in float32."""
    poses = np.asarray(poses, np.float64)
    F, K, C, P = poses.shape[:4]
    intr = np.asarray(intr, np.float32)
    out = np.zeros((F, K, C, P, wh, ww), np.uint16)
    dropped = np.zeros((F, K, C, P), np.int32)
    for f in range(F):
        for k in range(min(int(n_components[f]), K)):
            row = np.array([intr[f, 0], intr[f, 1], intr[f, 2] - np.float32(origin[f, k, 0]),
                            intr[f, 3] - np.float32(origin[f, k, 1]), intr[f, 4]], np.float32)
            frames = [[(int(mesh_of_class[c]), 1, poses[f, k, c, j])] for c in range(C) for j in range(P)]
            r = R.render(meshes, frames, np.tile(row, (C * P, 1)), wh, ww)
            out[f, k] = r['depth'].reshape(C, P, wh, ww)
            dropped[f, k] = r['dropped'].reshape(C, P)
    return out, dropped


def sample_arrays(F, K, C, n_components, origin, tau_per_frame):
    """The per-sample inputs of the windowed counts for sample (f K + k) C + c: frame_of (-1 for k >= n_components), want
    = k + 1, origin, tau."""
    frame_of = np.array([f if k < int(n_components[f]) else -1 for f in range(F) for k in range(K) for _ in range(C)], np.int32)
    want = np.array([k + 1 for _ in range(F) for k in range(K) for _ in range(C)], np.int32)
    org = np.repeat(np.asarray(origin, np.int32).reshape(F * K, 2), C, axis=0)
    tau = np.repeat(np.asarray(tau_per_frame, np.int32), K * C)
    return frame_of, want, org, tau


def score(found_label, comp_box, n_components, poses, valid, meshes, mesh_of_class, intr, depth, tau=0.01, mode=0,
          margin=0.5, min_score=(1, 2), max_per_class=1, depth_hyp=None, window=None):
    """score_candidates on the NumPy renderer (or on given depth_hyp [F,K,C,P,wh,ww]) -> the assignment's dict plus
    counts [F,K,C,P,6], seg_total [F,K,C], abs_sum, origin, wh, ww, depth_hyp, dropped."""
    poses = np.asarray(poses, np.float64)
    F, K, C, P = poses.shape[:4]
    H, W = depth.shape[1:]
    origin, wh, ww = windows(np.asarray(comp_box)[:, :K], n_components, H, W, margin) if window is None else window
    dropped = None
    if depth_hyp is None:
        depth_hyp, dropped = render_windows(meshes, mesh_of_class, poses, intr, origin, n_components, wh, ww)
    tu = V.tau_units(np.broadcast_to(np.asarray(tau, np.float64), (F,)), np.asarray(intr, np.float32)[:, 4].astype(np.float64))
    frame_of, want, org, tau_s = sample_arrays(F, K, C, n_components, origin, tu)
    counts, seg_total, abs_sum = fit_counts_window(depth, found_label, frame_of, want, org, wh, ww,
                                                   depth_hyp.reshape(F * K * C, P, wh, ww), tau_s)
    valid = np.ones((F, K, C, P), np.int32) if valid is None else np.asarray(valid)
    r = assign(counts.reshape(F, K, C, P, 6), seg_total.reshape(F, K, C), valid, poses, n_components, mode, min_score[0],
               min_score[1], max_per_class)
    r.update(counts=counts.reshape(F, K, C, P, 6), seg_total=seg_total.reshape(F, K, C), abs_sum=abs_sum.reshape(F, K, C, P),
             origin=origin, wh=wh, ww=ww, depth_hyp=depth_hyp, dropped=dropped)
    return r


# ---- the scene the host and the GPU tests share --------------------------------------------------------------------------
SCENE_H, SCENE_W = 96, 128
SCENE_INTR = np.array([[150.0, 150.0, 63.5, 47.5, 10000.0]], np.float32)
SCENE_SEGMENT = dict(seed=1, n_hyp=64, stride=2, tol=0.01, max_height=0.5, min_plane_percent=10, jump=0.02, min_pixels=40,
                     max_components=8)
SHIFT = np.array([0.03, 0.0, 0.0])                 # "the wrong place": 3 cm along the camera's x
_cache = {}


def scene_meshes():
    """Classes 0 .. 3: the L prism, the plate, a cube of 7 cm (centred) and a small sphere, which no frame shows; mesh 4 is
    the table."""
    cv, ct, _ = MR.cube()
    cube = (((cv - np.float32(0.5)) * np.float32(0.07)).astype(np.float32), ct)
    return [V.l_prism(), V.plate(), cube, MR.icosphere(1, 0.03), DN.plane_mesh()]


def _on_table(T, x, y, h, rot):
    """The pose of an object at (x, y) of the table, its origin h above it, turned by the rotation vector `rot` first."""
    return T @ R.pose_matrix([0.0, 0.0, 0.0], [x, y, h]) @ R.pose_matrix(rot, [0.0, 0.0, 0.0])


def scene():
    """A table and three objects standing apart on it, one frame of 96 x 128: dict(meshes, intr, depth [1,H,W] uint16, label
    [1,H,W] uint8 (1 the table, class c = value c + 2), gt {class: pose})."""
    if 'scene' not in _cache:
        meshes = scene_meshes()
        T = R.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])      # the table's normal (its +z) looks at the camera
        gt = {0: _on_table(T, -0.24, 0.02, 0.02, [0.0, 0.0, 0.4]),
              1: _on_table(T, 0.0, 0.05, 0.06, [np.pi / 2, 0.0, 0.0]),   # the plate stands on its short edge
              2: _on_table(T, 0.23, -0.02, 0.035, [0.0, 0.0, 0.7])}
        frame = [(4, 1, T)] + [(c, c + 2, gt[c]) for c in sorted(gt)]
        r = R.render(meshes, [frame], SCENE_INTR, SCENE_H, SCENE_W)
        _cache['scene'] = dict(meshes=meshes, intr=SCENE_INTR, depth=r['depth'], label=r['label'], gt=gt)
    return _cache['scene']


def scene_segments():
    """The restatement of "Depth components" on the scene -> dict(label [1,H,W] uint8, n_components [1], comp_box [1,K,4],
    comp_size [1,K], object_of [n_components]: the class whose pixels component k covers best)."""
    if 'segments' not in _cache:
        s = scene()
        seg = D.segment(s['depth'], s['intr'], **SCENE_SEGMENT)[0]
        n = int(seg['n_components'])
        object_of = []
        for k in range(n):
            ious = [D.match((seg['label'] == k + 1).astype(np.uint8), s['label'][0], s['depth'][0], c + 2)[1] for c in range(3)]
            object_of.append(int(np.argmax(ious)))
        _cache['segments'] = dict(label=seg['label'][None], n_components=np.array([n], np.int32), comp_box=seg['comp_box'][None],
                                  comp_size=seg['comp_size'][None], object_of=object_of)
    return _cache['segments']


def scene_hypotheses(K=None):
    """poses [1,K,4,3,4,4] for the scene's components: for component k, which shows object o, and class c the model of c at
    o's true pose, that pose after the first principal half turn of c's model, and that pose moved by SHIFT."""
    s, g = scene(), scene_segments()
    n = int(g['n_components'][0])
    K = n if K is None else K
    poses = np.tile(np.eye(4), (1, K, 4, 3, 1, 1))
    for k in range(min(n, K)):
        base = s['gt'][g['object_of'][k]]
        for c in range(4):
            flip = V.flip_hypotheses(V.surface_points(*s['meshes'][c][:2], per_edge=3))[1]
            moved = base.copy()
            moved[:3, 3] += SHIFT
            poses[0, k, c] = [base, base @ flip, moved]
    return poses


def scene_score(**kw):
    """score() of the scene with the given hypotheses (cached for the defaults)."""
    key = ('score', tuple(sorted(kw.items())))
    if key not in _cache:
        s, g = scene(), scene_segments()
        _cache[key] = score(g['label'], g['comp_box'], g['n_components'], scene_hypotheses(), None, s['meshes'], [0, 1, 2, 3],
                            s['intr'], s['depth'], **kw)
    return _cache[key]
