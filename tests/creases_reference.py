"""NumPy restatement of DESIGN.md, "Creases": the integer box sums of the foreground's depths, the smoothed points in
float64 (NumPy rounds every operation, as the un-fused kernel does) in the written order, and the concave-crease test of
the four directions.  Written from the definition, on whole images shifted against each other.  Every output is an
integer and is expected to equal the kernels' bit for bit.  The input builders of the tests are at the end."""
import math

import numpy as np

import depth_components_reference as D
import depth_noise_reference as DN
import detect_reference as DR
import mesh_models_reference as MR
import render_reference as RR

DIRECTIONS = [(1, 0), (0, 1), (1, 1), (1, -1)]     # (du, dv) of direction bit b
DEFAULTS = dict(step=3, smooth=1, angle=30.0)


def cos2_of(angle_degrees):
    """The double both sides are given: cos(angle)^2, formed once."""
    c = math.cos(math.radians(float(angle_degrees)))
    return c * c


def shifted(a, du, dv, fill):
    """out[v, u] = a[v + dv, u + du] where that is a pixel of the image, else `fill`."""
    H, W = a.shape
    out = np.full((H, W), fill, a.dtype)
    us, vs = slice(max(0, -du), min(W, W - du)), slice(max(0, -dv), min(H, H - dv))
    if us.start < us.stop and vs.start < vs.stop:
        out[vs, us] = a[vs.start + dv:vs.stop + dv, us.start + du:us.stop + du]
    return out


def smooth_map(depth, fg, jump_units, smooth):
    """Stage 1 of one frame -> [H,W] uint32 = (S << 8) | n."""
    d = depth.astype(np.int64)
    on = np.asarray(fg) != 0
    S, n = np.zeros(d.shape, np.int64), np.zeros(d.shape, np.int64)
    if int(jump_units) < 0:
        return np.zeros(d.shape, np.uint32)
    r = int(smooth)
    for dv in range(-r, r + 1):
        for du in range(-r, r + 1):
            dq, onq = shifted(d, du, dv, 0), shifted(on, du, dv, False)
            member = on & onq & (np.abs(dq - d) <= int(jump_units))
            S += np.where(member, dq, 0)
            n += member
    assert S.max() < (1 << 24) and n.max() < (1 << 8) and np.all(n[on] >= 1)
    return ((S << 8) | n).astype(np.uint32)


def smoothed_points(smap, intr):
    """-> x, y, z [H,W] float64; whatever a pixel with n = 0 gets is never used."""
    fx, fy, cx, cy, factor = (np.float64(np.float32(k)) for k in np.asarray(intr, np.float32))
    H, W = smap.shape
    v, u = np.mgrid[0:H, 0:W]
    S, n = (smap >> 8).astype(np.float64), (smap & 255).astype(np.float64)
    with np.errstate(all='ignore'):
        z = S / (n * factor)
        x = ((u.astype(np.float64) - cx) * z) / fx
        y = ((v.astype(np.float64) - cy) * z) / fy
    return x, y, z


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def creases(depth, fg, intr, jump_units, step=3, smooth=1, cos2=None):
    """One frame -> dict(smooth_map uint32, crease, tested, fg_cut uint8 [H,W], n_crease)."""
    cos2 = np.float64(cos2_of(DEFAULTS['angle']) if cos2 is None else cos2)
    s, ju = int(step), int(jump_units)
    d = depth.astype(np.int64)
    on = np.asarray(fg) != 0
    smap = smooth_map(depth, fg, ju, smooth)
    P = smoothed_points(smap, intr)
    crease, tested = np.zeros(d.shape, np.uint8), np.zeros(d.shape, np.uint8)
    for b, (du, dv) in enumerate(DIRECTIONS):
        side = []
        ok = on.copy()
        for sign in (-1, 1):
            ou, ov = sign * s * du, sign * s * dv
            ok &= shifted(on, ou, ov, False) & (np.abs(shifted(d, ou, ov, 0) - d) <= s * ju)
            side.append([shifted(c, ou, ov, np.float64(0)) for c in P])
        with np.errstate(all='ignore'):
            e1, e2 = [side[0][i] - P[i] for i in range(3)], [side[1][i] - P[i] for i in range(3)]
            g = _dot(e1, e2)
            m = [e1[i] + e2[i] for i in range(3)]
            cc = _dot(m, P)
            q1, q2 = _dot(e1, e1), _dot(e2, e2)
            flag = ok & (cc < 0) & ((g >= 0) | (g * g < cos2 * (q1 * q2)))
        tested |= (ok.astype(np.uint8) << b)
        crease |= (flag.astype(np.uint8) << b)
    return dict(smooth_map=smap, crease=crease, tested=tested, fg_cut=(on & (crease == 0)).astype(np.uint8),
                n_crease=int((crease != 0).sum()))


def creases_batch(depth, fg, intr, jump_units, step, smooth, cos2):
    """[F,...] inputs -> dict of stacked outputs, n_crease [F] int32."""
    rs = [creases(depth[f], fg[f], intr[f], jump_units[f], step, smooth, cos2) for f in range(len(depth))]
    out = {k: np.stack([r[k] for r in rs]) for k in ('smooth_map', 'crease', 'tested', 'fg_cut')}
    out['n_crease'] = np.array([r['n_crease'] for r in rs], np.int32)
    return out


def segment(depth, intrinsics, creases_=None, jump_units_=None, **params):
    """depth_components_reference.segment with the cut in front of the components when creases_ is a dict(step, smooth,
    angle): a list of per-frame dicts; fg stays the uncut image."""
    if creases_ is None:
        return D.segment(depth, intrinsics, jump_units_=jump_units_, **params)
    p = dict(D.DEFAULTS)
    p.update(seed=0, first_frame=0)
    p.update(params)
    c = dict(DEFAULTS)
    c.update(creases_)
    out = []
    for f in range(len(depth)):
        r = D.plane(depth[f], intrinsics[f], p['seed'], p['first_frame'] + f, p['n_hyp'], p['stride'], p['tol'],
                    p['min_plane_percent'])
        r['fg'] = D.foreground(depth[f], intrinsics[f], r['plane'], r['plane_hyp'], p['tol'], p['max_height'])
        ju = D.jump_units(p['jump'], intrinsics[f][4]) if jump_units_ is None else int(jump_units_[f])
        r['jump_units'] = ju
        cr = creases(depth[f], r['fg'], intrinsics[f], ju, c['step'], c['smooth'], cos2_of(c['angle']))
        r.update(crease=cr['crease'], tested=cr['tested'], fg_cut=cr['fg_cut'], n_crease=cr['n_crease'],
                 smooth_map=cr['smooth_map'])
        r['root'] = D.components(depth[f], r['fg_cut'], ju)
        r.update(D.table(r['root'], p['min_pixels'], p['max_components']))
        out.append(r)
    return out


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------
_cache = {}

# hand-made folds: depth images written from a formula, the whole image foreground
FOLD_H, FOLD_W = 24, 41
FOLD_INTR = np.array([150.0, 150.0, 20.0, 11.5, 10000.0], np.float32)    # the fold runs down column 20 = cx
FOLD_JUMP_UNITS = 400


def fold_depth(deviation_degrees, valley=True, z0=1.0):
    """Two planes that meet in the camera's x = 0 and deviate from one flat plane by the given angle: z = z0 -+ t |x| with
    t = tan(deviation / 2), a valley (its fold farthest from the camera) or a roof.  The ray of column u has x = k z with
    k = (u - cx) / fx, so z = z0 / (1 +- t |k|)."""
    t = math.tan(math.radians(deviation_degrees) / 2.0) * (1.0 if valley else -1.0)
    k = np.abs((np.arange(FOLD_W, dtype=np.float64) - float(FOLD_INTR[2])) / float(FOLD_INTR[0]))
    z = z0 / (1.0 + t * k)
    return np.tile(np.floor(z * float(FOLD_INTR[4]) + 0.5).astype(np.uint16), (FOLD_H, 1))


def oblique_plane_depth(a=0.8, b=-0.5, z0=1.0):
    """The plane z = z0 + a x + b y: z = z0 / (1 - a ku - b kv)."""
    v, u = np.mgrid[0:FOLD_H, 0:FOLD_W]
    ku = (u - float(FOLD_INTR[2])) / float(FOLD_INTR[0])
    kv = (v - float(FOLD_INTR[3])) / float(FOLD_INTR[1])
    return np.floor(z0 / (1.0 - a * ku - b * kv) * float(FOLD_INTR[4]) + 0.5).astype(np.uint16)


def depth_step(units):
    """Two planes that face the camera, the right one (from column 20 on) `units` farther."""
    d = np.full((FOLD_H, FOLD_W), 10000, np.uint16)
    d[:, 20:] += np.uint16(units)
    return d


# the table scene of depth_components_reference with other spheres, at the two cameras of the issue
TOUCHING_SPHERES = [(-0.1, 0.0, 0.10), (0.05, 0.0, 0.07), (0.22, -0.2, 0.05)]
BIG_INTR = np.array([[150.0, 148.0, 79.3, 59.6, 1000.0]], np.float32)
BIG_H, BIG_W = 120, 160
BIG_MIN_PIXELS = 40
CLEAN_CUT = dict(step=2, smooth=0, angle=30.0)
NOISY_CUT = dict(step=3, smooth=1, angle=30.0)


def table_pose():
    return RR.pose_matrix([2.2, 0.0, 0.0], [0.0, 0.05, 1.0])


def sphere_centres(spheres):
    """The camera-frame centres of spheres (x, y, radius) resting on the table of depth_components_reference.scene_frames."""
    T = table_pose()
    normal = T[:3, :3] @ np.array([0.0, 0.0, 1.0])
    if normal @ T[:3, 3] > 0:
        normal = -normal
    return [(T @ np.array([x, y, 0.0, 1.0]))[:3] + rad * normal for x, y, rad in spheres]


def sphere_scene(spheres, intr, H, W):
    """-> (depth [1,H,W] uint16, label [1,H,W] uint8: 1 the table, sphere i = value 2 + i), rendered once per argument."""
    key = ('scene', tuple(spheres), H, W)
    if key not in _cache:
        frame = [(1, 1, table_pose())]
        for i, (centre, (_, _, rad)) in enumerate(zip(sphere_centres(spheres), spheres)):
            S = np.eye(4)
            S[:3, :3] *= rad
            S[:3, 3] = centre
            frame.append((0, 2 + i, S))
        r = RR.render([MR.icosphere(2), DN.plane_mesh()], [frame], intr, H, W)
        _cache[key] = (r['depth'], r['label'])
    return _cache[key]


def noisy(depth, label, intr, seed=3):
    """The frame through the kinect1 sensor model -> (depth, label)."""
    r = DN.apply(depth, label, intr, DN.KINECT1, seed=seed)
    return r['depth'], r['label']


def big_scene(spheres=None, noise=True):
    """The 120 x 160 frame of the touching spheres (or the given ones), through the sensor model or not."""
    spheres = TOUCHING_SPHERES if spheres is None else spheres
    key = ('big', tuple(spheres), noise)
    if key not in _cache:
        depth, label = sphere_scene(spheres, BIG_INTR, BIG_H, BIG_W)
        _cache[key] = noisy(depth, label, BIG_INTR) if noise else (depth, label)
    return _cache[key]


def scene_segments(depth, intr, creases_, min_pixels, key):
    """segment() of one of the scenes with the components tests' parameters, cached under `key`."""
    key = ('segments', key, None if creases_ is None else tuple(sorted(creases_.items())), min_pixels)
    if key not in _cache:
        _cache[key] = segment(depth, intr, creases_, jump_units_=[D.SCENE_JUMP_UNITS], min_pixels=min_pixels, max_components=32,
                              **D.SCENE_PARAMS)[0]
    return _cache[key]


def shares(seg, label, n_objects=3):
    """[n_components, n_objects + 1] int: the pixels of component k on the table (column 0) and on each sphere."""
    return np.array([[int(((seg['label'] == k + 1) & (label == 1 + j)).sum()) for j in range(n_objects + 1)]
                     for k in range(int(seg['n_components']))]).reshape(-1, n_objects + 1)


# ---- detection across a touch ------------------------------------------------------------------------------------------------
DETECT_SEGMENT = dict(D.SCENE_PARAMS, jump=0.02, min_pixels=16, max_components=8)


def detect_meshes():
    """Classes 0 .. 2: the three spheres at their sizes, centred."""
    return [MR.icosphere(2, rad) for _, _, rad in TOUCHING_SPHERES]


def detect_scene(creases_):
    """The clean 60 x 80 frame of the touching spheres, segmented with or without the cut, and the hypotheses of
    detect_reference.scene_hypotheses's kind: for component k, which shows sphere o, and class c the model of c at o's true
    centre and that pose moved by detect_reference.SHIFT.  -> dict(depth, label, intr, seg, object_of, poses [1,K,3,2,4,4])."""
    key = ('detect', None if creases_ is None else tuple(sorted(creases_.items())))
    if key not in _cache:
        depth, label = sphere_scene(TOUCHING_SPHERES, D.SCENE_INTR, D.SCENE_H, D.SCENE_W)
        seg = segment(depth, D.SCENE_INTR, creases_, **DETECT_SEGMENT)[0]
        sh = shares(seg, label[0])
        object_of = [int(np.argmax(row[1:])) for row in sh]
        centres = sphere_centres(TOUCHING_SPHERES)
        K = len(object_of)
        poses = np.tile(np.eye(4), (1, K, 3, 2, 1, 1))
        for k, o in enumerate(object_of):
            poses[0, k, :, 0, :3, 3] = centres[o]
            poses[0, k, :, 1, :3, 3] = centres[o] + DR.SHIFT
        _cache[key] = dict(depth=depth, label=label, intr=D.SCENE_INTR, seg=seg, object_of=object_of, poses=poses, shares=sh)
    return _cache[key]


def detect_score(creases_):
    """detect_reference.score on the restatement's segments of detect_scene."""
    key = ('detect_score', None if creases_ is None else tuple(sorted(creases_.items())))
    if key not in _cache:
        s = detect_scene(creases_)
        seg = s['seg']
        _cache[key] = DR.score(seg['label'][None], seg['comp_box'][None], np.array([seg['n_components']], np.int32), s['poses'], None,
                               detect_meshes(), [0, 1, 2], s['intr'], s['depth'])
    return _cache[key]


# ---- the random cases of the GPU test ----------------------------------------------------------------------------------------
# (name, F, H, W, step, smooth, cos2 or None for the default angle).  Shapes: one pixel; a row and a column; frames no
# wider or higher than the step, where nothing is tested; one tile, one pixel more, one short of a tile by two tiles and a
# pixel; three frames of two by three tiles.  Parameters: both at their lowest, both at their highest, the defaults, and the
# two mixed ends; cos2 at 0, at 1 and at the default.
CASES = [
    ("1x1", 1, 1, 1, 1, 0, None),
    ("1x70", 1, 1, 70, 3, 1, None),
    ("70x1", 1, 70, 1, 3, 1, None),
    ("40x3_step3", 1, 40, 3, 3, 1, None),
    ("8x50_step8", 1, 8, 50, 8, 7, None),
    ("32x32", 1, 32, 32, 3, 1, None),
    ("33x33", 1, 33, 33, 8, 7, None),
    ("31x65", 1, 31, 65, 1, 0, None),
    ("33x33_8_0", 1, 33, 33, 8, 0, 0.0),
    ("31x65_1_7", 1, 31, 65, 1, 7, 1.0),
    ("40x72x3", 3, 40, 72, 3, 1, None),
    ("40x72x3_cos0", 3, 40, 72, 1, 0, 0.0),
    ("40x72x3_cos1", 3, 40, 72, 8, 7, 1.0),
    ("65535", 1, 33, 40, 8, 7, None),
]
CASE_NOISE = 3             # depth units, uniform in [-3, 3]
CASE_JUMP_UNITS = 30       # ten times the noise: about the steepest fold


def case_inputs(name):
    """-> dict(depth [F,H,W] uint16, fg [F,H,W] uint8, intr [F,5] float32, jump_units [F] int32, step, smooth, cos2).  Depth
    ramps folded along slanted lines plus a few units of integer noise, nine pixels in ten foreground; the foreground's
    values are 1, or 255 in places (any non-zero value counts)."""
    name, F, H, W, step, smooth, cos2 = [c for c in CASES if c[0] == name][0]
    rng = np.random.default_rng([ord(ch) for ch in name])
    v, u = np.mgrid[0:H, 0:W]
    depth = np.zeros((F, H, W), np.int64)
    intr = np.zeros((F, 5), np.float32)
    for f in range(F):
        a, b = rng.uniform(-4, 4, 2)
        fold = rng.uniform(6, 24) * (1 + f) * np.abs((u + v // 2) % 12 - 6)       # valleys and roofs six pixels apart
        depth[f] = np.floor(1000 + 150 * f + a * u + b * v + fold + 0.5) + rng.integers(-CASE_NOISE, CASE_NOISE + 1, (H, W))
        intr[f] = [75.0 + 20 * f, 74.0 + 15 * f, 0.45 * W + f, 0.55 * H - f, 1000.0 * (1 + f)]
    fg = np.where(rng.random((F, H, W)) < 0.9, 1, 0).astype(np.uint8)
    fg[(fg != 0) & (rng.random((F, H, W)) < 0.1)] = 255
    ju = np.full(F, CASE_JUMP_UNITS, np.int32)
    if name == "65535":
        depth = 65535 - rng.integers(0, 2 * CASE_NOISE + 1, (F, H, W))
        fg[:] = 1                                  # the packing's bound: boxes of 225 members of 65535
        depth[0, 10:30, 10:30] = 65535
    if F == 3:
        ju[0] = -1                                 # nothing is smoothed, nothing tested, fg_cut = fg
        fg[1] = 0                                  # an empty foreground
        fg[2] = 1                                  # all foreground
        depth[2, ::7, ::5] = 0                     # (a depth of 0 is a depth like any other here: fg decides)
        ju[2] = 2 * CASE_JUMP_UNITS
    assert depth.min() >= 0 and depth.max() <= 65535
    return dict(depth=depth.astype(np.uint16), fg=fg, intr=intr, jump_units=ju, step=step, smooth=smooth,
                cos2=cos2_of(DEFAULTS['angle']) if cos2 is None else float(cos2))


def case_result(name):
    """The restatement on a case, computed once and not changed afterwards."""
    if ('case', name) not in _cache:
        c = case_inputs(name)
        _cache[('case', name)] = creases_batch(c['depth'], c['fg'], c['intr'], c['jump_units'], c['step'], c['smooth'], c['cos2'])
    return _cache[('case', name)]
