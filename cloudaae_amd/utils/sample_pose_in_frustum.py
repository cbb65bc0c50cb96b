"""Mirror of the reference's utils/sample_pose_in_frustum.py, batched: training poses (class, rotation,
translation) drawn on the GPU by cloudaae_sample_poses (csrc/pose_sample.hip; DESIGN.md, "Pose sampling", is the
definition).  get_frustum (:42-70) stays host-side constants: four scalars and eight corner points.

A draw is a function of (seed, global sample index, stream id): sample i of a call is global sample first_index + i,
so the same (seed, index) gives the same pose whatever the batch size, the number of ranks or the launch."""
import ctypes
import math

import torch

from .. import _lib
from .._lib import ptr, require, stream

# parameter sets of translation_generation (:130-138, 'linemod') and of generate_occluder.py:47-51 ('ycbv').  The
# reference has no YCB-Video intrinsics in this file: fx, fy, cx, cy, width, height of 'ycbv' are the data set's
# published ones for its first camera -- a choice; pass camera=dict(fx=..., ...) for others.
CAMERAS = {
    'linemod': dict(vertical_fov=45., nearDist=0.4, farDist=1.5, ratio=57.5 / 45., fx=572.4114, fy=573.57043, cx=325.2611,
                    cy=242.04899, width=640., height=480.),
    'ycbv': dict(vertical_fov=45., nearDist=0.5, farDist=1., ratio=58. / 45., fx=1066.778, fy=1067.487, cx=312.9869,
                 cy=241.3109, width=640., height=480.),
}
NUM_MODELS = 21
_FRUSTA = {}


def get_frustum(vertical_fov, nearDist, farDist, ratio):
    """Returns (frustum_corners [3,8], Hnear, Wnear, Hfar, Wfar).
    NOTE (kept on purpose): the reference applies tf.math.tan to
    vertical_fov/2 = 22.5 *as radians* (it never converts degrees), so for ycbv
    Hnear = 2*tan(22.5 rad)*0.5 = 0.55785 and Wnear = 0.71901."""
    t = math.tan(float(vertical_fov) / 2)
    Hnear = 2 * t * nearDist
    Wnear = Hnear * ratio
    Hfar = 2 * t * farDist
    Wfar = Hfar * ratio
    cam_direction = torch.tensor([0., 0., 1.])
    up = torch.tensor([0., 1., 0.])
    right = torch.linalg.cross(up, cam_direction)
    fc = cam_direction * farDist
    nc = cam_direction * nearDist
    corners = torch.stack([fc + up * Hfar / 2 - right * Wfar / 2, fc + up * Hfar / 2 + right * Wfar / 2,
                           fc - up * Hfar / 2 - right * Wfar / 2, fc - up * Hfar / 2 + right * Wfar / 2,
                           nc + up * Hnear / 2 - right * Wnear / 2, nc + up * Hnear / 2 + right * Wnear / 2,
                           nc - up * Hnear / 2 - right * Wnear / 2, nc - up * Hnear / 2 + right * Wnear / 2], dim=1)
    return corners, Hnear, Wnear, Hfar, Wfar


def camera_parameters(dataset='ycbv', camera=None):
    """The parameter set of `dataset` with the entries of `camera` (a dict) replacing its own."""
    require(dataset in CAMERAS, "dataset must be 'linemod' or 'ycbv'")
    cam = dict(CAMERAS[dataset])
    for k, v in (camera or {}).items():
        require(k in cam, "unknown camera parameter %r" % (k,))
        cam[k] = float(v)
    return cam


def class_list(classes):
    """(n, host int array or None) of a class list for the C ABI (None: every model)."""
    if classes is None:
        return 0, None
    ids = [int(c) for c in classes]
    return len(ids), (ctypes.c_int * max(len(ids), 1))(*ids)


def _launch(B, seed, first_index, classes, num_models, wnear, wfar, near, far, fx, fy, cx, cy, width, height, dev, debug):
    """cloudaae_sample_poses with its outputs from _lib.empty (inside a recorded step the call replays)."""
    B = int(B)
    n, ids = class_list(classes)
    cls = _lib.empty((B,), dtype=torch.int64, device=dev)
    axag = _lib.empty((B, 3), dtype=torch.float64, device=dev)
    rot = _lib.empty((B, 3, 3), dtype=torch.float64, device=dev)
    rot32 = _lib.empty((B, 3, 3), dtype=torch.float32, device=dev)
    trans = _lib.empty((B, 3), dtype=torch.float32, device=dev)
    fov = _lib.empty((B,), dtype=torch.uint8, device=dev)
    drawn = _lib.empty((B, 5), dtype=torch.float32, device=dev) if debug else None
    raw = _lib.empty((B, 8), dtype=torch.int32, device=dev) if debug else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_sample_poses(B, int(first_index), int(seed) % (1 << 64), n, ids, int(num_models),
                                                    float(wnear), float(wfar), float(near), float(far), float(fx), float(fy),
                                                    float(cx), float(cy), float(width), float(height), ptr(cls), ptr(axag),
                                                    ptr(rot), ptr(rot32), ptr(trans), ptr(fov), ptr(drawn), ptr(raw),
                                                    stream()), "cloudaae_sample_poses")
    out = dict(class_id=cls, axisangle=axag, translation=trans, rot_mat64=rot, rot_gen_mat=rot32, rot_gen_axag=axag,
               trans_gen=trans, in_fov=fov)
    if debug:
        out['drawn'], out['raw'] = drawn, raw
    return out


def _device(device):
    return torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())


def sample_poses(batch, seed, first_index, classes=None, dataset='ycbv', camera=None, device=None,
                 num_models=NUM_MODELS, debug=False):
    """`batch` poses, global samples first_index .. first_index + batch - 1, in ONE launch and without a read-back.
    classes: the class ids to draw from (default: all `num_models` models).  Returns the dict that a
    tfrecord_io.PoseRecords.epoch item becomes on the device -- class_id [B] int64, axisangle [B,3] float64,
    translation [B,3] float32 -- plus rot_mat64 [B,3,3], rot_gen_mat (its float32), rot_gen_axag (= axisangle),
    trans_gen (= translation), in_fov [B] uint8 (0: the draw left the image and became the frustum middle) and
    frustum_corners.  debug=True adds drawn [B,5] (x, y, z, u, v before replacement) and raw [B,8] (the Philox words).
    The outputs come from _lib.empty: inside a recorded step the call replays."""
    cam = camera_parameters(dataset, camera)
    key = (cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    if key not in _FRUSTA:            # (the corner tensor costs a dozen host-side torch ops: once per camera, not per step)
        _FRUSTA[key] = get_frustum(*key)
    corners, _, Wnear, _, Wfar = _FRUSTA[key]
    out = _launch(batch, seed, first_index, classes, num_models, Wnear, Wfar, cam['nearDist'], cam['farDist'], cam['fx'],
                  cam['fy'], cam['cx'], cam['cy'], cam['width'], cam['height'], _device(device), debug)
    out['frustum_corners'] = corners
    return out


# ---- the reference's own function names.  Each is one launch of the same kernel and keeps the part its name stands for
# (the kernel has no cheaper half: a pose is ~300 instructions of one lane); a training loop calls sample_poses, which
# gives all of it at once.  The rotation does not depend on the camera, so the rotation helpers take none.
def sample_rot(npoints, seed=0, first_index=0, device=None):
    """(:8-27) -> (axag [npoints,3] float64, rot_mat [npoints,3,3] float64).  The reference draws one axis per call with
    npoints = 1; batched, that is one axis and one angle per sample."""
    p = sample_poses(npoints, seed, first_index, device=device)
    return p['axisangle'], p['rot_mat64']


def rotation_generation(x, seed=0, first_index=0, batch=None, device=None):
    """(:30-39) adds x['rot_gen_mat'] [B,3,3] float32 and x['rot_gen_axag'] [B,3] float64."""
    B = batch if batch is not None else x['class_id'].shape[0]
    dev = device if device is not None else (x['class_id'].device if 'class_id' in x else None)
    p = sample_poses(B, seed, first_index, device=dev)
    x['rot_gen_axag'] = p['rot_gen_axag']
    x['rot_gen_mat'] = p['rot_gen_mat']
    return x


def in_frustum_translation(npoints, Wnear, Wfar, farDist, nearDist, seed=0, first_index=0, device=None):
    """(:73-82) -> (the draws [npoints,4], homogeneous, BEFORE the image test; frustum_middle [1,4]), both on the device:
    x, y ~ N(0, (Wnear+Wfar)/7), z ~ N((far+near)/2, (far-near)/7) for ANY frustum (the image test of the launch is not
    used here, so it runs with a unit camera)."""
    dev = _device(device)
    p = _launch(npoints, seed, first_index, None, 1, Wnear, Wfar, nearDist, farDist, 1., 1., 0., 0., 1., 1., dev, True)
    ones = torch.ones((int(npoints), 1), dtype=torch.float32, device=dev)
    middle = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    middle[0, 2] = (torch.tensor(farDist, dtype=torch.float32) + torch.tensor(nearDist, dtype=torch.float32)) / 2
    middle[0, 3] = 1.
    return torch.cat([p['drawn'][:, 0:3], ones], dim=1), middle


def get_proj_matrix(cam_intrin, extrin_rot, extrin_trans):
    """(:85-90) cam_intrin [3,3] x [extrin_rot | extrin_trans] -> [3,4] (host-side constants)."""
    return torch.as_tensor(cam_intrin, dtype=torch.float32) @ torch.cat(
        [torch.as_tensor(extrin_rot, dtype=torch.float32), torch.as_tensor(extrin_trans, dtype=torch.float32)], dim=1)


def camera_matrix(dataset='ycbv', camera=None):
    cam = camera_parameters(dataset, camera)
    return torch.tensor([[cam['fx'], 0., cam['cx']], [0., cam['fy'], cam['cy']], [0., 0., 1.]], dtype=torch.float32)


def project_pts_to_image(proj_matrix, pts_3d):
    """(:93-101) pts_3d [4,n] homogeneous -> [2,n] pixels (row 0 = u, row 1 = v).  An inspection helper on small
    tensors: the training path takes the test inside cloudaae_sample_poses."""
    p = proj_matrix.to(pts_3d.device) @ pts_3d
    return torch.stack([p[0] / p[2], p[1] / p[2]], dim=0)


def check_pts_in_image_fov(pts_2d, xmax, ymax):
    """(:104-116) strict on all four edges."""
    return (pts_2d[0] > 0) & (pts_2d[0] < xmax) & (pts_2d[1] > 0) & (pts_2d[1] < ymax)


def get_final_translation(proj_matrix, pts_3d, xmax, ymax, frustum_middle):
    """(:119-124) pts_3d [n,4] -> (the point where it projects inside the image, else frustum_middle; pts_2d)."""
    pts_2d = project_pts_to_image(proj_matrix, pts_3d.t())
    keep = check_pts_in_image_fov(pts_2d, xmax, ymax)
    return torch.where(keep[:, None], pts_3d, frustum_middle.to(pts_3d.device)), pts_2d


def translation_generation(x, seed=0, first_index=0, dataset='linemod', camera=None, batch=None, device=None):
    """(:127-153) adds x['trans_gen'] [B,3] and x['frustum_corners'], drawn and tested on the GPU."""
    B = batch if batch is not None else x['class_id'].shape[0]
    dev = device if device is not None else (x['class_id'].device if 'class_id' in x else None)
    p = sample_poses(B, seed, first_index, dataset=dataset, camera=camera, device=dev)
    x['trans_gen'] = p['translation']
    x['in_fov'] = p['in_fov']
    x['frustum_corners'] = p['frustum_corners']
    return x
