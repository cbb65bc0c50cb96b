"""Random occluders -- mirror of the reference's utils/generate_occluder.py, batched and generated on the GPU:
the two spherical blobs of :38-81 (cloudaae_random_spherical_occluder) and the object occluder of :5-35
(cloudaae_random_object_occluder; DESIGN.md, "Pose sampling")."""
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .sample_pose_in_frustum import class_list, get_frustum

_CAMERAS = {  # generate_occluder.py:40-52
    'linemod': dict(vertical_fov=45., nearDist=0.4, farDist=1.5, ratio=57.5 / 45.),
    'ycbv': dict(vertical_fov=45., nearDist=0.5, farDist=1., ratio=58. / 45.),
}


def get_random_spherical_occluder(x, dataset, seed=0):
    """x: dict with 'translation' [B,3] (device).  Adds x['occluder'] [B,400,3] (two Gaussian
    blobs of 200 points, sigma 0.01, between the camera's near plane and the object) and
    x['frustum_corners']."""
    require(dataset in _CAMERAS, "dataset must be 'linemod' or 'ycbv'")
    cam = _CAMERAS[dataset]
    corners, Hnear, Wnear, _, _ = get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    t = x['translation'].to(torch.float32).contiguous()
    B = t.shape[0]
    occ = torch.empty((B, 400, 3), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().cloudaae_random_spherical_occluder(B, 200, ptr(t), float(Wnear), float(Hnear),
                                                             float(cam['nearDist']), 0.01, int(seed), ptr(occ),
                                                             stream()), "cloudaae_random_spherical_occluder")
    x['occluder'] = occ
    x['frustum_corners'] = corners
    return x


def get_random_object_occluder(x, NUM_CLASS, seed=0, dataset='ycbv', first_index=0, classes=None, per=512):
    """(:5-35) x: dict with 'obj_model' [C,npts,6], 'translation' [B,3] and the sampled rotation -- 'rot_gen_mat'
    (or 'rot_mat64', which a record-driven batch has).  Adds x['occluder'] [B,512,3]: the first 512 points of a class
    model rotated by the sample's own rotation, centred between the near plane and the object; x['occluder_class']
    [B] int64 and x['frustum_corners'].  The class is drawn per sample among `classes` (default: the first NUM_CLASS
    models); the reference draws one per process when it builds its graph -- a deliberate difference."""
    require(dataset in _CAMERAS, "dataset must be 'linemod' or 'ycbv'")
    cam = _CAMERAS[dataset]
    corners, Hnear, Wnear, _, _ = get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    models = x['obj_model'].to(torch.float32).contiguous()
    nmodels, npts, width = models.shape
    require(width == 6, "obj_model must be [C, npts, 6]")
    require(1 <= int(NUM_CLASS) <= nmodels, "NUM_CLASS outside the models")
    t = x['translation'].to(torch.float32).contiguous()
    rot = x['rot_mat64'] if x.get('rot_mat64') is not None else x['rot_gen_mat']
    rot = rot.to(torch.float64).contiguous()
    B = t.shape[0]
    n, ids = class_list(classes if classes is not None else range(int(NUM_CLASS)))
    occ = _lib.empty((B, int(per), 3), dtype=torch.float32, device=t.device)
    occ_cls = _lib.empty((B,), dtype=torch.int64, device=t.device)
    _lib.check(_lib.lib().cloudaae_random_object_occluder(B, int(first_index), int(seed) % (1 << 64), nmodels, npts,
                                                          ptr(models), n, ids, ptr(rot), ptr(t), int(per), float(Wnear),
                                                          float(Hnear), float(cam['nearDist']), ptr(occ), ptr(occ_cls),
                                                          None, stream()), "cloudaae_random_object_occluder")
    x['occluder'] = occ
    x['occluder_class'] = occ_cls
    x['frustum_corners'] = corners
    return x
