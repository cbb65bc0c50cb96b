"""Pose refinement by point-to-point ICP (evaluate_cloudAAE_ycbv.py:606-628: open3d registration_icp, ten calls,
correspondence radius 0.01 m times 0.9 after each call) -- one launch of cloudaae_icp_point_to_point for the batch --
or, on request, by point-to-plane ICP on the target's normals (cloudaae_icp_point_to_plane, the same schedule).
The definitions are in DESIGN.md ("Pose refinement")."""
import torch

from .. import _lib
from .._lib import ptr, require, stream


def _points(t, name):
    """(pointer, point stride, cloud stride, count) of a [B, P, >=3] float32 GPU tensor whose points have
    contiguous coordinates (row strides allowed: obj_batch [B,2048,6], a prefix of the points)."""
    require(isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[2] >= 3, "%s must be a [B, P, >=3] tensor" % name)
    require(t.dtype == torch.float32, "%s must be float32" % name)
    if not t.is_cuda:
        raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got a %s tensor" % t.device)
    require(t.stride(2) == 1, "%s: the coordinates of a point must be contiguous" % name)
    return t.data_ptr(), int(t.stride(1)), int(t.stride(0)), int(t.shape[1])


ESTIMATIONS = ("point_to_point", "point_to_plane")


def refine_pose_icp(model_xyz, scene_xyz, rot_axag, trans, radius=0.01, decay=0.9, rounds=10, max_iteration=30,
                    relative_fitness=1e-6, relative_rmse=1e-6, estimation="point_to_point", normals=None,
                    pose_maps_target_to_source=False):
    """Refine B initial poses [rot_axag | trans] that map the object models model_xyz [B,M,>=3] (object frame) onto
    the observed points scene_xyz [B,N,>=3] (camera frame).  float32 inputs on one GPU; rot_axag and trans [B,3].
    Returns a dict of transformation [B,4,4] f64, rot_axag [B,3] f64 (angle in [0, pi]), trans [B,3] f32,
    fitness [B] f64, inlier_rmse [B] f64 (both of the last round) and iterations [B,rounds] int32.  Only the
    library's kernel runs (outputs from _lib.empty), so the call records into a StepPlan and replays.
    estimation="point_to_plane" (cloudaae_icp_point_to_plane): the first cloud is the source, the second the target,
    and normals [B,N,3] float64 holds one normal per target point (utils/normals.py).  With
    pose_maps_target_to_source the given and the returned poses map the target onto the source: pass the scene as
    the source and the model with its normals as the target, and give and get model -> camera poses.  fitness and
    inlier_rmse are those of the source points."""
    require(estimation in ESTIMATIONS, "estimation must be one of %s" % (ESTIMATIONS,))
    plane = estimation == "point_to_plane"
    require(plane or (normals is None and not pose_maps_target_to_source),
            "normals and pose_maps_target_to_source belong to estimation='point_to_plane'")
    sp, sps, scs, M = _points(model_xyz, "model_xyz")
    dp, dps, dcs, N = _points(scene_xyz, "scene_xyz")
    B = int(model_xyz.shape[0])
    require(scene_xyz.shape[0] == B, "model_xyz and scene_xyz must have the same batch size")
    for name, t in (("rot_axag", rot_axag), ("trans", trans)):
        require(isinstance(t, torch.Tensor) and tuple(t.shape) == (B, 3) and t.dtype == torch.float32,
                "%s must be a float32 [B, 3] tensor" % name)
        require(t.device == model_xyz.device and scene_xyz.device == model_xyz.device,
                "all inputs must be on one device")
    dev = model_xyz.device
    if plane:
        require(isinstance(normals, torch.Tensor) and tuple(normals.shape) == (B, N, 3) and
                normals.dtype == torch.float64 and normals.device == dev,
                "point_to_plane needs normals: a float64 [B, N, 3] tensor, one normal per target point")
    T = _lib.empty((B, 4, 4), dtype=torch.float64, device=dev)
    rot = _lib.empty((B, 3), dtype=torch.float64, device=dev)
    tr = _lib.empty((B, 3), dtype=torch.float32, device=dev)
    fit = _lib.empty((B,), dtype=torch.float64, device=dev)
    rmse = _lib.empty((B,), dtype=torch.float64, device=dev)
    its = _lib.empty((B, int(rounds)), dtype=torch.int32, device=dev)
    if plane:
        _lib.check(_lib.lib().cloudaae_icp_point_to_plane(
            B, M, sp, sps, scs, N, dp, dps, dcs, ptr(normals), int(bool(pose_maps_target_to_source)), ptr(rot_axag),
            ptr(trans), float(radius), float(decay), int(rounds), int(max_iteration), float(relative_fitness),
            float(relative_rmse), ptr(T), ptr(rot), ptr(tr), ptr(fit), ptr(rmse),
            its.data_ptr() if its.numel() else None, stream()), "cloudaae_icp_point_to_plane")
        return dict(transformation=T, rot_axag=rot, trans=tr, fitness=fit, inlier_rmse=rmse, iterations=its)
    _lib.check(_lib.lib().cloudaae_icp_point_to_point(
        B, M, sp, sps, scs, N, dp, dps, dcs, ptr(rot_axag), ptr(trans), float(radius), float(decay), int(rounds),
        int(max_iteration), float(relative_fitness), float(relative_rmse), ptr(T), ptr(rot), ptr(tr), ptr(fit),
        ptr(rmse), its.data_ptr() if its.numel() else None, stream()), "cloudaae_icp_point_to_point")
    return dict(transformation=T, rot_axag=rot, trans=tr, fitness=fit, inlier_rmse=rmse, iterations=its)


def to_float32(x):
    """float32 copy of a float64 GPU tensor by the library's kernel (replayable, unlike .float())."""
    x = x.contiguous()
    out = _lib.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().cloudaae_f64_to_f32(x.numel(), ptr(x), ptr(out), stream()), "cloudaae_f64_to_f32")
    return out
