"""NumPy restatement of DESIGN.md, "Pose sampling": a host Philox4x32-10 (integer arithmetic, exact), u01 and normal2 of
csrc/philox.h, and every draw of cloudaae_sample_poses / cloudaae_random_object_occluder as a function of
(seed, global sample index g, stream id).  Written from the definition; `dtype` is float32 (the definition) or float64
(the same formulas evaluated wider: how far fp32 rounding can move a result, which sizes the tests' tolerances)."""
import math

import numpy as np

STREAM_POSE, STREAM_TRANS, STREAM_OCC_CENTRE, STREAM_OCC_CLASS = 16, 17, 18, 19
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# camera parameter sets: vertical_fov (degrees, used AS RADIANS by the frustum: kept quirk), near, far, ratio, then the
# pinhole camera; the YCB-Video intrinsics are the data set's published ones for its first camera -- a choice
CAMERAS = {
    'linemod': dict(vertical_fov=45., nearDist=0.4, farDist=1.5, ratio=57.5 / 45., fx=572.4114, fy=573.57043, cx=325.2611,
                    cy=242.04899, width=640., height=480.),
    'ycbv': dict(vertical_fov=45., nearDist=0.5, farDist=1., ratio=58. / 45., fx=1066.778, fy=1067.487, cx=312.9869,
                 cy=241.3109, width=640., height=480.),
}


def philox_rounds(counter, key):
    """Philox4x32-10 proper: counter [..., 4], key [..., 2] (uint32 values) -> [..., 4] uint32."""
    c = [np.asarray(counter[..., k], np.uint64) & MASK for k in range(4)]
    k0 = np.asarray(key[..., 0], np.uint64) & MASK
    k1 = np.asarray(key[..., 1], np.uint64) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def philox4x32(seed, ctr, stream):
    """philox4x32(seed, ctr, stream) of csrc/philox.h: counter = (ctr low, ctr high, stream, 0x9E3779B9), key = seed's
    two halves.  ctr: array of uint64 -> [n, 4] uint32."""
    ctr = np.atleast_1d(np.asarray(ctr, np.uint64))
    seed = int(seed) % (1 << 64)
    counter = np.stack([ctr & MASK, ctr >> np.uint64(32), np.full(ctr.shape, stream, np.uint64),
                        np.full(ctr.shape, W0, np.uint64)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), ctr.shape + (2,))
    return philox_rounds(counter, key)


def u01(x, dtype=np.float32):
    """((float)(x >> 8) + 0.5) / 2^24 in `dtype` (fp32: the top value rounds to 1.0, so the range is (0, 1])."""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)


def normal2(a, b, dtype=np.float32):
    r = np.sqrt(dtype(-2.0) * np.log(u01(a, dtype)))
    t = dtype(6.283185307179586) * u01(b, dtype)
    return r * np.cos(t), r * np.sin(t)


def pick(r, n):
    """floor(r n / 2^32): the integer rule of every class draw."""
    return ((np.asarray(r, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def get_frustum(vertical_fov, nearDist, farDist, ratio):
    """(Hnear, Wnear, Hfar, Wfar) in double, tan of the DEGREES taken as radians."""
    t = math.tan(float(vertical_fov) / 2)
    Hnear = 2 * t * nearDist
    Hfar = 2 * t * farDist
    return Hnear, Hnear * ratio, Hfar, Hfar * ratio


def camera_constants(dataset='ycbv', camera=None):
    """The ten float32 constants of a launch (wnear, wfar, near, far, fx, fy, cx, cy, width, height) and hnear."""
    cam = dict(CAMERAS[dataset])
    cam.update(camera or {})
    Hnear, Wnear, _, Wfar = get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    c = dict(wnear=Wnear, wfar=Wfar, near=cam['nearDist'], far=cam['farDist'], fx=cam['fx'], fy=cam['fy'], cx=cam['cx'],
             cy=cam['cy'], width=cam['width'], height=cam['height'], hnear=Hnear)
    return {k: np.float32(v) for k, v in c.items()}


def exponential_map(axag):
    """losses/angular_distance_taylor.py:30-66 in float64, the op order of csrc/so3_dual.h; axag [n,3] -> [n,3,3]."""
    a = np.asarray(axag, np.float64)
    n = a.shape[0]
    z = np.zeros(n)
    ss = [[z, -a[:, 2], a[:, 1]], [a[:, 2], z, -a[:, 0]], [-a[:, 1], a[:, 0], z]]
    tsq = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    p4, p6, p8 = tsq * tsq, (tsq * tsq) * tsq, ((tsq * tsq) * tsq) * tsq
    t1s = (((1.0 - tsq / 6.0) + p4 / 120.0) - p6 / 5040.0) + p8 / 362880.0
    t2s = (((0.5 - tsq / 24.0) + p4 / 720.0) - p6 / 40320.0) + p8 / 3628800.0
    safe = np.where(tsq < 1e-2, 1.0, tsq)
    th = np.sqrt(safe)
    t1 = np.where(tsq < 1e-2, t1s, np.sin(th) / th)
    t2 = np.where(tsq < 1e-2, t2s, (1.0 - np.cos(th)) / safe)
    R = np.empty((n, 3, 3))
    for i in range(3):
        for j in range(3):
            sq = z
            for k in range(3):
                sq = sq + ss[i][k] * ss[k][j]
            R[:, i, j] = ((1.0 if i == j else 0.0) + t1 * ss[i][j]) + t2 * sq
    return R


def sample_poses(batch, seed, first_index, classes, dataset='ycbv', camera=None, dtype=np.float32):
    """The whole of cloudaae_sample_poses for samples g = first_index .. first_index + batch - 1.  classes: the list of
    class ids.  Returns a dict: raw [n,8] uint32, class_id int64, axisangle float64 [n,3] (the `dtype` axis * angle,
    widened), rot_mat64, translation [n,3] `dtype`, in_fov bool, drawn [n,5] `dtype` (x, y, z, u, v)."""
    f = dtype
    g = np.uint64(first_index) + np.arange(batch, dtype=np.uint64)
    r = philox4x32(seed, g, STREAM_POSE)
    q = philox4x32(seed, g, STREAM_TRANS)
    classes = np.asarray(classes, np.int64)
    class_id = classes[pick(r[:, 0], len(classes))]
    # rotation
    theta = f(6.283185307179586) * u01(r[:, 1], f)
    u = f(2.0) * u01(r[:, 2], f) - f(1.0)
    s = np.sqrt(f(1.0) - u * u)
    axis = np.stack([s * np.cos(theta), s * np.sin(theta), u], axis=1)
    angle = f(np.float32(3.14159265358979) if f is np.float32 else np.pi) * (f(2.0) * u01(r[:, 3], f) - f(1.0))
    a = (axis * angle[:, None]).astype(f)
    axisangle = a.astype(np.float64)
    # translation
    c = {k: f(v) for k, v in camera_constants(dataset, camera).items()}
    n0, n1 = normal2(q[:, 0], q[:, 1], f)
    n2, _ = normal2(q[:, 2], q[:, 3], f)
    sxy = (c['wnear'] + c['wfar']) / f(7.0)
    zmid = (c['far'] + c['near']) / f(2.0)
    sz = (c['far'] - c['near']) / f(7.0)
    x, y, z = n0 * sxy, n1 * sxy, zmid + n2 * sz
    with np.errstate(divide='ignore', invalid='ignore'):
        pu = (c['fx'] * x + c['cx'] * z) / z
        pv = (c['fy'] * y + c['cy'] * z) / z
    keep = (pu > 0) & (pu < c['width']) & (pv > 0) & (pv < c['height'])
    middle = np.array([0.0, 0.0, zmid], f)
    drawn3 = np.stack([x, y, z], axis=1).astype(f)
    translation = np.where(keep[:, None], drawn3, middle[None, :]).astype(f)
    return dict(raw=np.concatenate([r, q], axis=1), class_id=class_id, axisangle=axisangle,
                rot_mat64=exponential_map(axisangle), translation=translation, in_fov=keep,
                drawn=np.stack([x, y, z, pu, pv], axis=1).astype(f), frustum_middle=middle)


def object_occluder(models, batch, seed, first_index, classes, rot_mat64, translation, per=512, dataset='ycbv',
                    camera=None, dtype=np.float32):
    """cloudaae_random_object_occluder: models [C,npts,>=3] float32.  Returns occluder [n,per,3] `dtype`, occ_class,
    centre [n,3], raw [n,8]."""
    f = dtype
    g = np.uint64(first_index) + np.arange(batch, dtype=np.uint64)
    r = philox4x32(seed, g, STREAM_OCC_CENTRE)
    q = philox4x32(seed, g, STREAM_OCC_CLASS)
    classes = np.asarray(classes, np.int64)
    occ_class = classes[pick(q[:, 0], len(classes))]
    c = {k: f(v) for k, v in camera_constants(dataset, camera).items()}
    z = np.asarray(translation)[:, 2].astype(f)
    n0, n1 = normal2(r[:, 0], r[:, 1], f)
    n2, _ = normal2(r[:, 2], r[:, 3], f)
    centre = np.stack([n0 * (c['wnear'] / f(8.0)), n1 * (c['hnear'] / f(8.0)),
                       (c['near'] + z) / f(2.0) + n2 * ((z - c['near']) / f(6.0))], axis=1).astype(f)
    p = np.asarray(models)[occ_class, :per, 0:3].astype(f)                         # [n,per,3]
    R = np.asarray(rot_mat64, np.float64).astype(np.float32).astype(f)           # float32(R), as the kernel reads it
    occ = np.empty((batch, per, 3), f)
    for row in range(3):
        a = p[:, :, 0] * R[:, row, 0][:, None]
        b = p[:, :, 1] * R[:, row, 1][:, None]
        cc = p[:, :, 2] * R[:, row, 2][:, None]
        occ[:, :, row] = ((a + b) + cc) + centre[:, row][:, None]
    return dict(occluder=occ, occ_class=occ_class, centre=centre, raw=np.concatenate([r, q], axis=1))


def global_index(step, global_batch, rank, local_batch, i=0):
    """g = step * global_batch + rank * local_batch + i."""
    return step * global_batch + rank * local_batch + i


def edge_distance(drawn, dataset='ycbv', camera=None):
    """Per sample, the distance in pixels of the restated (u, v) from the nearest image edge (inf where not finite)."""
    c = camera_constants(dataset, camera)
    u, v = drawn[:, 3].astype(np.float64), drawn[:, 4].astype(np.float64)
    d = np.minimum(np.minimum(np.abs(u), np.abs(u - float(c['width']))),
                   np.minimum(np.abs(v), np.abs(v - float(c['height']))))
    return np.where(np.isfinite(d), d, np.inf)


def float_tolerances(seed, n, dataset, models, classes):
    """The tests' absolute tolerances, measured: 10 x the largest change that evaluating the restatement in float64
    instead of float32 makes to axisangle, translation (of samples both keep) and the occluder points, with a floor of
    4 ulp of fp32 at the quantity's largest magnitude."""
    a32 = sample_poses(n, seed, 0, classes, dataset)
    a64 = sample_poses(n, seed, 0, classes, dataset, dtype=np.float64)
    both = a32['in_fov'] & a64['in_fov']
    o32 = object_occluder(models, n, seed, 0, classes, a32['rot_mat64'], a32['translation'], dataset=dataset)
    o64 = object_occluder(models, n, seed, 0, classes, a32['rot_mat64'], a32['translation'], dataset=dataset,
                          dtype=np.float64)
    out = {}
    for key, x, y in (('axisangle', a32['axisangle'], a64['axisangle']),
                      ('translation', a32['translation'][both].astype(np.float64), a64['translation'][both]),
                      ('occluder', o32['occluder'].astype(np.float64), o64['occluder'])):
        change = float(np.abs(x - y).max())
        floor = 4.0 * float(np.spacing(np.float32(np.abs(x).max())))
        out[key] = max(10.0 * change, floor)
    return out
