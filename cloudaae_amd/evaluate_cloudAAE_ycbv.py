"""Inference step -- mirror of the graph the reference's evaluate_cloudAAE_ycbv.py builds
(:405-477), MI355X-native.

What is mirrored: the eval-mode forward (batch-norm statistics from the moving averages, no noise),
the 4N -> N farthest point sampling of the reconstruction + gather + Chamfer against the first N
observed points (:449-451), the translation error of the prediction and of the plain centroid
(:455-460), the SO(3) error (:468-474), and on request the ICP refinement of the predicted pose against the first N
inlier points (:606-628, open3d's point-to-point registration_icp; here utils/icp.py, one HIP launch).  What is NOT:
reading the YCB-Video test frames and the result files (out of scope).

    graph = T.TrainGraph(...); graph.restore("model.ckpt")
    out = evaluate_batch(graph, element)       # element: xyz_inlier, visiblePoints_org, class_id,
                                               #          translation, axisangle (device tensors)
    out = evaluate_batch(graph, element, icp=True) # + obj_batch [B,M,>=3]: adds the *_icp outputs
"""
import torch

from . import _lib
from ._lib import ptr, require, stream
from .losses import angular_distance_taylor, chamfer_loss, trans_distance
from .tf_ops.sampling import tf_sampling
from .train_cloudAAE_ycbv import NUM_CLASS
from .utils import _functions as F
from .utils import icp as icp_util


def evaluate_batch(graph, element, replay=False, icp=None):
    """One pass of evaluate_cloudAAE_ycbv.py:421-477 on a batch.  Returns the tensors its loop
    fetches (:546-560): xyz_recon [B,4N,3], xyz_recon_FPS [B,N,3], rot_pred, trans_pred, the three
    losses with their per-sample values, mean_dist_loss, element_mean.
    replay=True: the pass is recorded once per input shape (_lib.StepPlan) and re-issued afterwards
    without Python layers in between -- the batch-1 latency is then the kernels', not the host's;
    the returned tensors are the same objects every call, overwritten in place.
    icp=True (the reference's schedule) or a dict of utils.icp.refine_pose_icp parameters: the predicted pose is also
    refined against the network's input points; needs element['obj_batch'] [B,M,>=3] float32 (the class's object
    model) and adds rot_icp, trans_icp, transformation_icp, fitness_icp, inlier_rmse_icp, iterations_icp and the
    errors of the refined pose, trans_loss_icp / axag_loss_icp with their per-sample values.  The other outputs
    are those of icp=None."""
    icp = _icp_params(icp)
    if replay:
        return _replayed(graph, element, icp)
    return _evaluate(graph, element, icp)


def _icp_params(icp):
    if icp is None or icp is False:
        return None
    if icp is True:
        return {}
    require(isinstance(icp, dict), "icp must be None, True or a dict of refine_pose_icp parameters")
    return dict(icp)


def _replayed(graph, element, icp=None):
    N = graph.NUM_POINT
    src = {'xyz_inlier': (element['xyz_inlier'], torch.float32),
           'visiblePoints_org': (element['visiblePoints_org'][:, 0:N, :], torch.float32),
           'class_id': (element['class_id'], torch.int64), 'translation': (element['translation'], torch.float32),
           'axisangle': (element['axisangle'], torch.float64)}
    if icp is not None:
        src['obj_batch'] = (element['obj_batch'], torch.float32)
    key = tuple((k, tuple(v.shape)) for k, (v, _) in src.items())
    if icp is not None:
        key += (('icp', tuple(sorted(icp.items()))),)
    plans = graph.__dict__.setdefault('_eval_plans', {})
    if key not in plans:
        static = {k: torch.empty(tuple(v.shape), dtype=dt, device=graph.device) for k, (v, dt) in src.items()}
        plans[key] = [None, None, static]
        while len(plans) > 4:
            plans.pop(next(iter(plans)))
    plan, out, static = plans[key]
    for k, (v, _) in src.items():
        static[k].copy_(v, non_blocking=True)
    if plan is None:
        plan = _lib.StepPlan(graph.device)
        with _lib.record(plan):
            out = _evaluate(graph, static, icp)
        if plan.foreign_ops:
            import warnings
            warnings.warn("evaluation pass not replayable (torch kernels inside: %s)" % sorted(set(plan.foreign_ops)))
            plans.pop(key)
            return out
        plans[key][0], plans[key][1] = plan, out
        return out
    plan.replay()
    return out


def _evaluate(graph, element, icp=None):
    N = graph.NUM_POINT
    xyz = element['xyz_inlier']
    require(xyz.dim() == 3 and xyz.shape[1] >= N and xyz.shape[2] == 3, "xyz_inlier must be [B, >=num_point, 3]")
    xyz = xyz.to(torch.float32).contiguous()
    B, P, _ = xyz.shape
    cls = element['class_id'].to(torch.int64).contiguous()
    with torch.no_grad():
        # :421-438 -- first N inlier points, centroid, centring, one-hot class; no noise in evaluation
        pc = _lib.empty((B, N, 3 + NUM_CLASS), dtype=torch.float32, device=xyz.device)
        element_mean = _lib.empty((B, 3), dtype=torch.float32, device=xyz.device)
        _lib.check(_lib.lib().cloudaae_input_assemble(B, P, N, NUM_CLASS, ptr(xyz), None, ptr(cls), ptr(pc),
                                                      ptr(element_mean), None, stream()), "cloudaae_input_assemble")
        xyz_recon_res, rot_pred, trans_pred_res, end_points = graph._call_model(pc, False)      # :441-444
        xyz_recon = F.AddRowVecFn.apply(xyz_recon_res, element_mean)                             # :446
        trans_pred = F.AddRowVecFn.apply(trans_pred_res.unsqueeze(1), element_mean).squeeze(1)   # :447
        # :450 -- for all decoder: FPS of the 4N reconstructed points down to N, then Chamfer (:452)
        xyz_recon_FPS = tf_sampling.gather_point(xyz_recon, tf_sampling.farthest_point_sample(N, xyz_recon))
        visiblePoints_final = element['visiblePoints_org'][:, 0:N, :].to(torch.float32).contiguous()   # :431-433
        xyz_loss, xyz_per = chamfer_loss.get_loss(xyz_recon_FPS, visiblePoints_final)
        translation = element['translation'].to(torch.float32)
        trans_loss, trans_per = trans_distance.get_translation_error(trans_pred, translation)            # :455
        mean_dist_loss, mean_dist_per = trans_distance.get_translation_error(element_mean, translation)  # :457
        axag_loss, axag_per = angular_distance_taylor.get_rotation_error(rot_pred, element['axisangle'])  # :470-474
    out = dict(xyz_recon=xyz_recon, xyz_recon_FPS=xyz_recon_FPS, rot_pred=rot_pred, trans_pred=trans_pred,
               xyz_loss=xyz_loss, xyz_loss_per_sample=xyz_per, trans_loss=trans_loss,
               trans_loss_perSample=trans_per, mean_dist_loss=mean_dist_loss,
               mean_dist_loss_perSample=mean_dist_per, axag_loss=axag_loss, axag_loss_perSample=axag_per,
               element_mean=element_mean, end_points=end_points)
    if icp is not None:
        out.update(_refine(element, xyz[:, 0:N, :], rot_pred, trans_pred, translation, icp))
    return out


def _refine(element, scene, rot_pred, trans_pred, translation, params):
    """:606-628 -- ICP of the class's object model (source, object frame) onto the network's input points (target,
    camera frame, not centred), from the predicted pose; then the errors of the refined pose."""
    obj = element.get('obj_batch')
    require(obj is not None, "icp needs element['obj_batch'] [B, M, >=3] (the object model of each sample's class)")
    require(obj.dim() == 3 and obj.shape[0] == scene.shape[0] and obj.shape[2] >= 3 and obj.dtype == torch.float32,
            "obj_batch must be a float32 [B, M, >=3] tensor")
    with torch.no_grad():
        r = icp_util.refine_pose_icp(obj, scene, rot_pred.contiguous(), trans_pred.contiguous(), **params)
        trans_loss, trans_per = trans_distance.get_translation_error(r['trans'], translation)
        # the rotation error kernel takes an fp32 prediction, as for the network's output
        axag_loss, axag_per = angular_distance_taylor.get_rotation_error(icp_util.to_float32(r['rot_axag']),
                                                                         element['axisangle'])
    return dict(rot_icp=r['rot_axag'], trans_icp=r['trans'], transformation_icp=r['transformation'],
                fitness_icp=r['fitness'], inlier_rmse_icp=r['inlier_rmse'], iterations_icp=r['iterations'],
                trans_loss_icp=trans_loss, trans_loss_perSample_icp=trans_per, axag_loss_icp=axag_loss,
                axag_loss_perSample_icp=axag_per)
