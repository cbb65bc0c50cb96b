"""Inference step -- mirror of the graph the reference's evaluate_cloudAAE_ycbv.py builds
(:405-477), MI355X-native.

What is mirrored: the eval-mode forward (batch-norm statistics from the moving averages, no noise),
the 4N -> N farthest point sampling of the reconstruction + gather + Chamfer against the first N
observed points (:449-451), the translation error of the prediction and of the plain centroid
(:455-460), the SO(3) error (:468-474), and on request the ICP refinement of the predicted pose against the first N
inlier points (:606-628, open3d's point-to-point registration_icp; here utils/icp.py, one HIP launch).  On request the
predicted and the refined pose are scored with ADD and ADD-S (utils/pose_score.py: not in the reference, which prints
mean translation and rotation errors only; DESIGN.md "Pose scores").  The input side, from the
YCB-Video test records (<seq>_pcnn.tfrecord) to the element, is element_from_frames (utils/segment.py on the GPU,
:125-335); main() is the reference's command line without the visualisation.  What is NOT: the RGB channels, the
result files.

    graph = T.TrainGraph(...); graph.restore("model.ckpt")
    out = evaluate_batch(graph, element)       # element: xyz_inlier, visiblePoints_org, class_id,
                                               #          translation, axisangle (device tensors)
    out = evaluate_batch(graph, element, icp=True) # + obj_batch [B,M,>=3]: adds the *_icp outputs
    out = evaluate_batch(graph, element, icp=True, score=True)   # adds add_pred, adds_pred, add_icp, adds_icp [B]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib, tfrecord_io
from ._lib import ptr, require, stream
from .losses import angular_distance_taylor, chamfer_loss, trans_distance
from .tf_ops.sampling import tf_sampling
from .train_cloudAAE_ycbv import NUM_CLASS
from .utils import _functions as F
from .utils import bop_score as bop_util
from .utils import icp as icp_util
from .utils import mesh_models
from .utils import normals as normals_util
from .utils import pose_equiv
from .utils import pose_score as score_util
from .utils import pose_verify as verify_util
from .utils import ppf as ppf_util
from .utils import segment as seg_util
from .utils.frame_inputs import record_intrinsics


def evaluate_batch(graph, element, replay=False, icp=None, score=None, bop=None, symmetries=None, verify=None, propose=None):
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
    are those of icp=None.
    icp={'estimation': 'point_to_plane', ...}: point-to-plane ICP of the network's N input points (source) onto the
    object model (target) along the model's normals: element['obj_normals'] [B,M,3] float64 when present, otherwise
    utils.normals.estimate_normals(obj_batch, radius=normal_radius) (a key of the dict, default 0.015 m).  The
    outputs keep their names and are model -> camera poses as before; fitness_icp and inlier_rmse_icp are then those
    of the scene points (the share of the N input points with a model point within the radius), not of the model's.
    score=True: the predicted pose [rot_pred | trans_pred] and, with icp, the refined one (transformation_icp) are
    scored against [axisangle | translation] on element['obj_batch'] by one cloudaae_pose_score launch: adds add_pred,
    adds_pred and, with icp, add_icp, adds_icp [B] float64 (ADD and ADD-S in metres).  The other outputs are those of
    score=None.
    bop=dict(meshes=PackedMeshes, mesh_index=[B] host integers or None (then class_id), diameters=[C] (metres, per class),
    symmetries=None or {class: [n,4,4] transforms that hold the identity}): the same poses are scored with BOP's errors
    (utils/bop_score.py, DESIGN.md "BOP pose errors") against the sample's own frame, element['frame_depth'] [B,H,W]
    and element['frame_intrinsics'] [B,5] (element_from_frames(keep_frames=True)): adds vsd_pred [B,K], mssd_pred,
    mspd_pred [B] float64 and, with icp, vsd_icp, mssd_icp, mspd_icp.  MSSD and MSPD are taken on element['obj_batch'].
    Not with replay=True.  The other outputs are those of bop=None.
    symmetries=a utils.pose_equiv.SymmetryTable (or bop['symmetries_table']): the rotation and translation errors are also
    taken against the label that is equivalent under the class's symmetries and nearest the pose's rotation (DESIGN.md,
    "Equivalent poses"; one cloudaae_nearest_equivalent_pose launch per pose set): adds axag_loss_sym, trans_loss_sym,
    axag_loss_perSample_sym, trans_loss_perSample_sym and, with icp, axag_loss_icp_sym, trans_loss_icp_sym,
    axag_loss_perSample_icp_sym, trans_loss_perSample_icp_sym.  Works with replay=True.  The other outputs are those of
    symmetries=None.
    verify=dict(meshes=PackedMeshes, mesh_index=[B] host integers or None (then class_id), hypotheses=a
    utils.pose_verify.HypothesisTable, tau=0.01 (metres), mode=0, base=None or [B,4,4] float64 poses to take the
    predicted pose's place): the predicted pose is the base of the class's hypotheses (cloudaae_pose_compose); with icp all B P of them are refined in one refine_pose_icp call with the same parameters
    (candidate 0 is then transformation_icp bit for bit); every candidate is rendered and compared with the sample's own
    frame (utils/pose_verify.py, DESIGN.md "Pose verification"), element['frame_depth'], ['frame_intrinsics'] and, for mode
    0, ['frame_label'] and ['frame_want'] (element_from_frames(keep_frames=True, keep_labels=True)), and the winner is
    kept: adds verify_best [B] int32, verify_score [B,P], verify_margin [B], verify_counts [B,P,6], verify_candidates
    [B,P,4,4], transformation_ver [B,4,4], rot_ver [B,3] float64, trans_ver [B,3] float32, trans_loss_ver / axag_loss_ver
    with their per-sample values and, with score, bop and symmetries, the _ver twins of their _pred outputs.  Not with
    replay=True.  The other outputs are those of verify=None.
    propose=dict(models=a utils.ppf.PPFModels, top=4, ref_step=5, peaks=2, normal_radius=0.02 (metres)): pose hypotheses by
    point-pair-feature voting (utils/ppf.py, DESIGN.md "Pose proposals") from the first N points of element['xyz_inlier']
    with normals estimated towards the camera: adds proposed_poses [B,top,4,4] float64, proposed_score and proposed_valid
    [B,top] int32.  With verify they are appended after the class's hypotheses as candidates P_h .. P_h + top - 1 (an
    invalid proposal repeats candidate 0, as compose does past a set's end), refined with icp by the same single call, judged
    with the others and their valid passed to cloudaae_select_pose; the first P_h candidates' poses, counts and scores are
    those of the call without propose bit for bit.  Not with replay=True.  The other outputs are those of propose=None."""
    icp = _icp_params(icp)
    score = bool(score)
    if bop is not None:
        require(isinstance(bop, dict) and bop.get('meshes') is not None and bop.get('diameters') is not None,
                "bop must be a dict with 'meshes' and 'diameters'")
        require(not replay, "bop scores are not available with replay=True: every chunk of rendered frames is allocated by "
                            "its own sizes and read back, which does not fit a recorded plan")
    if verify is not None:
        require(isinstance(verify, dict) and verify.get('meshes') is not None and
                isinstance(verify.get('hypotheses'), verify_util.HypothesisTable),
                "verify must be a dict with 'meshes' and 'hypotheses' (a pose_verify.HypothesisTable)")
        require(not replay, "pose verification is not available with replay=True: every chunk of rendered frames is allocated "
                            "by its own sizes and read back, which does not fit a recorded plan")
    if propose is not None:
        require(isinstance(propose, dict) and isinstance(propose.get('models'), ppf_util.PPFModels),
                "propose must be a dict with 'models' (a ppf.PPFModels)")
        require(not replay, "pose proposals are not available with replay=True: the mask, the candidates and the table pass "
                            "through allocations and kernels of their own sizes, which does not fit a recorded plan")
    if symmetries is None and bop is not None:
        symmetries = bop.get('symmetries_table')
    if symmetries is not None:
        require(isinstance(symmetries, pose_equiv.SymmetryTable), "symmetries must be a pose_equiv.SymmetryTable")
    if replay:
        return _replayed(graph, element, icp, score, symmetries)
    out = _evaluate(graph, element, icp, score, symmetries)
    prop = None
    if propose is not None:
        prop = _propose(graph, element, propose)
        out.update(proposed_poses=prop['pose'], proposed_score=prop['score'], proposed_valid=prop['valid'])
    if verify is not None:
        out.update(_verify(graph, element, out, verify, icp, score, symmetries, prop))
    if bop is not None:
        out.update(_bop(element, bop, *_pred_icp_poses(out)))
        if verify is not None:
            out.update(_bop(element, bop, ("ver",), out['transformation_ver'].unsqueeze(1)))
    return out


PROPOSE_NORMAL_RADIUS = 0.02     # neighbourhood of the scene normals of the proposals, metres


def _propose(graph, element, propose):
    """The pose proposals of the network's N input points."""
    N = graph.NUM_POINT
    with torch.no_grad():
        scene = element['xyz_inlier'].to(torch.float32).contiguous()[:, 0:N, :].contiguous()
        normals, mask = ppf_util.scene_normals(scene, float(propose.get('normal_radius', PROPOSE_NORMAL_RADIUS)))
        return ppf_util.propose_poses(propose['models'], scene, normals, mask, element['class_id'].to(torch.int64),
                                      top=int(propose.get('top', 4)), ref_step=int(propose.get('ref_step', 5)),
                                      peaks=int(propose.get('peaks', 2)))


def _verify(graph, element, out, verify, icp, score, symmetries, prop=None):
    """The hypotheses of the predicted pose and, when given, the proposals, refined like the prediction when there is an
    ICP, judged against the sample's frame; the winner's pose and its errors."""
    depth, intr = element.get('frame_depth'), element.get('frame_intrinsics')
    mode = int(verify.get('mode', verify_util.MODE_SEGMENT))
    label, want = (element.get('frame_label'), element.get('frame_want')) if mode == verify_util.MODE_SEGMENT else (None, None)
    require(depth is not None and intr is not None and (mode != verify_util.MODE_SEGMENT or (label is not None and want is not None)),
            "verify needs element['frame_depth'], ['frame_intrinsics'] and, for mode 0, ['frame_label'] and ['frame_want'] "
            "(element_from_frames(keep_frames=True, keep_labels=True))")
    cls = element['class_id'].to(torch.int64)
    B, N = int(cls.shape[0]), graph.NUM_POINT
    translation = element['translation'].to(torch.float32)
    with torch.no_grad():
        base = verify.get('base')
        predicted = base is None
        if predicted:
            base = score_util.pose_matrix(out['rot_pred'].contiguous(), out['trans_pred'].contiguous())
        c = verify_util.compose(base, cls, verify['hypotheses'])
        P = int(c['pose'].shape[1])
        cand, rot, trans, valid = c['pose'], c['rot_axag'], c['trans'], c['valid']
        if prop is not None:
            # candidates P .. P + top - 1; a proposal that is none repeats candidate 0
            ok = prop['valid'] != 0
            cand = torch.cat([cand, torch.where(ok[:, :, None, None], prop['pose'], cand[:, 0:1])], dim=1).contiguous()
            rot = torch.cat([rot, torch.where(ok[:, :, None], prop['rot_axag'], rot[:, 0:1])], dim=1).contiguous()
            trans = torch.cat([trans, torch.where(ok[:, :, None], prop['trans'], trans[:, 0:1])], dim=1).contiguous()
            valid = torch.cat([valid, prop['valid']], dim=1).contiguous()
            P = int(cand.shape[1])
        if icp is not None:
            # candidate 0 starts from the prediction itself, as _refine does; the kernel's samples are independent
            rot0, trans0 = icp_util.to_float32(rot), trans.clone()
            if predicted:
                rot0[:, 0] = out['rot_pred']
                trans0[:, 0] = out['trans_pred']
            scene = element['xyz_inlier'].to(torch.float32).contiguous()[:, 0:N, :]
            r = _icp_call(element, element['obj_batch'].repeat_interleave(P, dim=0),
                          scene.repeat_interleave(P, dim=0).contiguous(), rot0.view(B * P, 3), trans0.view(B * P, 3), icp, P)
            cand, rot, trans = r['transformation'].view(B, P, 4, 4), r['rot_axag'].view(B, P, 3), r['trans'].view(B, P, 3)
        mesh_index = verify.get('mesh_index')
        v = verify_util.verify_poses(verify['meshes'], cls.cpu().numpy() if mesh_index is None else mesh_index, cand, depth,
                                     label, want, intr, np.arange(B), tau=verify.get('tau', 0.01), mode=mode,
                                     valid=valid, **{k: verify[k] for k in ('samples_per_launch',) if k in verify})
        pick = v['best'].to(torch.int64).view(B, 1, 1).expand(B, 1, 3)
        rot_ver = rot.gather(1, pick).squeeze(1).contiguous()
        trans_ver = trans.gather(1, pick).squeeze(1).contiguous()
    res = dict(verify_best=v['best'], verify_score=v['score'], verify_margin=v['margin'], verify_counts=v['counts'],
               verify_candidates=cand, transformation_ver=v['pose_best'], rot_ver=rot_ver, trans_ver=trans_ver)
    res.update(_pose_errors(element, cls, icp_util.to_float32(rot_ver), trans_ver, translation, '_ver', symmetries))
    if score:
        res.update(_add_scores(element, translation, ("ver",), v['pose_best'].unsqueeze(1)))
    return res


def _icp_call(element, obj, scene, rot, trans, params, repeat=1):
    """The evaluation's one refine_pose_icp call, on models and scenes that hold every sample `repeat` times in a row.
    Point to point (:606-628): the class's object model (source, object frame) onto the network's input points (target,
    camera frame, not centred).  Point to plane: the input points onto the model along the model's normals; the poses
    given and returned stay model -> camera."""
    if params.get('estimation', 'point_to_point') == 'point_to_plane':
        params = dict(params)
        normal_radius = params.pop('normal_radius', NORMAL_RADIUS)
        params.pop('pose_maps_target_to_source', None)
        normals = element.get('obj_normals')
        if normals is None:
            normals = normals_util.estimate_normals(element['obj_batch'], radius=normal_radius)[0]
        if repeat != 1:                         # a torch kernel: not in the recorded pass, which refines every sample once
            normals = normals.repeat_interleave(repeat, dim=0).contiguous()
        return icp_util.refine_pose_icp(scene, obj, rot.contiguous(), trans.contiguous(), normals=normals,
                                        pose_maps_target_to_source=True, **params)
    return icp_util.refine_pose_icp(obj, scene, rot.contiguous(), trans.contiguous(), **params)


def _pred_icp_poses(out):
    """(names, est [B,K,4,4]) of the predicted pose and, when there is one, of the refined pose: one launch scores both."""
    with torch.no_grad():
        est = score_util.pose_matrix(out['rot_pred'].contiguous(), out['trans_pred'].contiguous())
        if out.get('transformation_icp') is None:
            return ("pred",), est.unsqueeze(1)
        return ("pred", "icp"), score_util.stack_poses(est, out['transformation_icp'])


def _bop(element, bop, names, est):
    """VSD, MSSD and MSPD of the poses est [B,K,4,4], one per name.  The verified pose comes in a call of its own, so that
    the others' numbers are formed as without verification."""
    obj, depth, intr = element.get('obj_batch'), element.get('frame_depth'), element.get('frame_intrinsics')
    require(obj is not None and depth is not None and intr is not None,
            "bop needs element['obj_batch'], ['frame_depth'] and ['frame_intrinsics'] (element_from_frames(keep_frames=True))")
    cls = element['class_id'].to(torch.int64)
    B = int(cls.shape[0])
    with torch.no_grad():
        gt = score_util.pose_matrix(element['axisangle'], element['translation'].to(torch.float32).contiguous())
        diam = bop['diameters']
        diam = diam if isinstance(diam, torch.Tensor) else torch.from_numpy(np.asarray(diam, np.float64))
        diam = diam.to(device=cls.device, dtype=torch.float64).index_select(0, cls)
        mesh_index = bop.get('mesh_index')
        sym = bop.get('symmetries')
        cls_host = cls.cpu().numpy() if (mesh_index is None or sym is not None) else None
        v = bop_util.vsd(bop['meshes'], cls_host if mesh_index is None else mesh_index, est, gt, depth, intr,
                         np.arange(B), diam, **{k: bop[k] for k in ('delta', 'taus', 'samples_per_launch') if k in bop})
        d = bop_util.mssd_mspd(obj, est, gt, intr.to(torch.float32),
                               None if sym is None else [sym.get(int(c)) for c in cls_host])
    res = {}
    for k, name in enumerate(names):
        res['vsd_' + name], res['mssd_' + name], res['mspd_' + name] = v['errors'][:, k], d['mssd'][:, k], d['mspd'][:, k]
    return res


NORMAL_RADIUS = 0.015     # neighbourhood of the class models' normals, metres (profiles/notes_icp_plane.md)


def _icp_params(icp):
    if icp is None or icp is False:
        return None
    if icp is True:
        return {}
    require(isinstance(icp, dict), "icp must be None, True or a dict of refine_pose_icp parameters")
    return dict(icp)


def _replayed(graph, element, icp=None, score=False, symmetries=None):
    N = graph.NUM_POINT
    src = {'xyz_inlier': (element['xyz_inlier'], torch.float32),
           'visiblePoints_org': (element['visiblePoints_org'][:, 0:N, :], torch.float32),
           'class_id': (element['class_id'], torch.int64), 'translation': (element['translation'], torch.float32),
           'axisangle': (element['axisangle'], torch.float64)}
    if icp is not None or score:
        require(element.get('obj_batch') is not None, "icp and score need element['obj_batch'] [B, M, >=3]")
        src['obj_batch'] = (element['obj_batch'], torch.float32)
    if icp is not None and icp.get('estimation') == 'point_to_plane' and element.get('obj_normals') is not None:
        src['obj_normals'] = (element['obj_normals'], torch.float64)
    key = tuple((k, tuple(v.shape)) for k, (v, _) in src.items())
    if icp is not None:
        key += (('icp', tuple(sorted(icp.items()))),)
    if score:
        key += (('score',),)
    if symmetries is not None:
        key += (('symmetries', id(symmetries)),)
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
            out = _evaluate(graph, static, icp, score, symmetries)
        if plan.foreign_ops:
            import warnings
            warnings.warn("evaluation pass not replayable (torch kernels inside: %s)" % sorted(set(plan.foreign_ops)))
            plans.pop(key)
            return out
        plans[key][0], plans[key][1] = plan, out
        return out
    plan.replay()
    return out


def _evaluate(graph, element, icp=None, score=False, symmetries=None):
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
        mean_dist_loss, mean_dist_per = trans_distance.get_translation_error(element_mean, translation)  # :457
    out = dict(xyz_recon=xyz_recon, xyz_recon_FPS=xyz_recon_FPS, rot_pred=rot_pred, trans_pred=trans_pred,
               xyz_loss=xyz_loss, xyz_loss_per_sample=xyz_per, mean_dist_loss=mean_dist_loss,
               mean_dist_loss_perSample=mean_dist_per, element_mean=element_mean, end_points=end_points)
    out.update(_pose_errors(element, cls, rot_pred, trans_pred, translation, '', symmetries))           # :455, :470-474
    if icp is not None:
        out.update(_refine(element, cls, xyz[:, 0:N, :], rot_pred, trans_pred, translation, icp, symmetries))
    if score:
        out.update(_add_scores(element, translation, *_pred_icp_poses(out)))
    return out


def _pose_errors(element, cls, rot32, trans, translation, tag, symmetries):
    """The translation and rotation errors of one pose set (rot32: its rotation in fp32, as the rotation error kernel takes
    it) under the keys of `tag` ('', '_icp', '_ver'); with a symmetry table also those against the equivalent label nearest
    the pose's rotation, under the same keys with '_sym' behind."""
    def errors(trans_label, rot_label, suffix):
        trans_loss, trans_per = trans_distance.get_translation_error(trans, trans_label)
        axag_loss, axag_per = angular_distance_taylor.get_rotation_error(rot32, rot_label)
        return {'trans_loss' + suffix: trans_loss, 'trans_loss_perSample' + suffix: trans_per,
                'axag_loss' + suffix: axag_loss, 'axag_loss_perSample' + suffix: axag_per}
    with torch.no_grad():
        res = errors(translation, element['axisangle'], tag)
        if symmetries is not None:
            near = pose_equiv.nearest_equivalent_pose(rot32, element['axisangle'], translation, cls, symmetries)
            res.update(errors(near['trans_equiv'], near['rot_equiv'], tag + '_sym'))
    return res


def _add_scores(element, translation, names, est):
    """ADD and ADD-S of the poses est [B,K,4,4], one per name, against the ground-truth pose: one launch."""
    obj = element.get('obj_batch')
    require(obj is not None, "score needs element['obj_batch'] [B, M, >=3] (the object model of each sample's class)")
    require(obj.dim() == 3 and obj.shape[0] == est.shape[0] and obj.shape[2] >= 3 and obj.dtype == torch.float32,
            "obj_batch must be a float32 [B, M, >=3] tensor")
    axisangle = element['axisangle']
    require(axisangle.dtype in (torch.float32, torch.float64), "axisangle must be float32 or float64")
    with torch.no_grad():
        r = score_util.score_poses(obj, est, score_util.pose_matrix(axisangle, translation.contiguous()))
    res = {}
    for k, name in enumerate(names):
        res['add_' + name], res['adds_' + name] = r['add'][:, k], r['adds'][:, k]
    return res


def _refine(element, cls, scene, rot_pred, trans_pred, translation, params, symmetries):
    """The predicted pose refined by ICP against the network's input points (_icp_call); then the errors of the refined
    pose."""
    obj = element.get('obj_batch')
    require(obj is not None, "icp needs element['obj_batch'] [B, M, >=3] (the object model of each sample's class)")
    require(obj.dim() == 3 and obj.shape[0] == scene.shape[0] and obj.shape[2] >= 3 and obj.dtype == torch.float32,
            "obj_batch must be a float32 [B, M, >=3] tensor")
    with torch.no_grad():
        r = _icp_call(element, obj, scene, rot_pred, trans_pred, params)
    res = dict(rot_icp=r['rot_axag'], trans_icp=r['trans'], transformation_icp=r['transformation'],
               fitness_icp=r['fitness'], inlier_rmse_icp=r['inlier_rmse'], iterations_icp=r['iterations'])
    res.update(_pose_errors(element, cls, icp_util.to_float32(r['rot_axag']), r['trans'], translation, '_icp', symmetries))
    return res


# ---- the input side: frames -> element (:125-335) -------------------------------------------------------------------

# the test sequences of each class (:43-63)
VALID_SEQ_ID = [[48, 51, 55, 56], [50, 54, 59], [49, 51, 54, 55, 58], [50, 51, 53, 55, 57, 59], [50, 52],
                [48, 49, 52, 59], [58], [58], [49, 53, 59], [50, 56], [52, 56, 58], [51, 54, 55, 57], [49, 53],
                [48, 55], [50, 54, 56, 59], [55], [51], [57, 59], [48, 54], [48, 57], [57]]


def element_from_frames(frames, target_cls, num_point, obj_models, seed=0, device=None, keep_frames=False,
                        keep_labels=False, labels="record", components=None, counts=None, choose="record", detector=None):
    """create_tfrecord_dataset (:287-335) on decoded frame records (tfrecord_io.decode_frame): the frames that hold
    target_cls, their target_cls segment, the mean-distance filter, radius outlier removal, FPS_random of the inliers
    and of the filtered points from seeded starts, the > 100 and >= num_point rules, quat2axangle, the object model,
    its hidden point removal (centre 0, 0.8 pi).  obj_models: [21, 2048, 6] float32 (numpy or device tensor).
    Returns the element evaluate_batch takes (device tensors: xyz_inlier [B,N,3], xyz, visiblePoints_org
    [B,2049,3], class_id [B], translation [B,3], axisangle [B,3] float64, obj_batch [B,2048,6]) plus seq_id,
    frame_id and num_valid_points_in_segment [B] (numpy); None when no segment survives.  keep_frames=True adds each
    sample's own frame, frame_depth [B,H,W] int16 (the uint16 bits) and frame_intrinsics [B,5] float32 (device tensors):
    what evaluate_batch(bop=...) compares the rendered object with.  keep_labels=True adds frame_label [B,H,W] uint8, the
    same frame's label image, and frame_want [B] int32, the label value by which extract_segments selects target_cls
    (target_cls + 1): what evaluate_batch(verify=...) takes the object's segment from.
    labels="components" (the default "record" uses the records' label images): the label images are found from the depth
    alone by utils.depth_components.segment_depth(depth, intrinsics, **components) -- components: its parameters, seed and
    first_frame among them, and creases=True or dict(step, smooth, angle) to cut touching objects apart at their concave
    creases first -- on every frame of the call, so that frame i of `frames` draws its plane hypotheses from
    first_frame + i whether or not its neighbours hold the class.  The record's label serves for association only: the component with the largest IoU against
    its target_cls + 1 pixels (match_components) takes their place, as value target_cls + 1 of an otherwise empty label
    image, and everything after is unchanged.  Frames without such a component are dropped.  The element gains
    segment_iou [B] float64 (numpy), and with keep_labels frame_label is the found image; counts, a dict, has the frames
    that hold the class added to its 'frames' and those with a component to its 'matched'.
    choose="detect" (with labels="components"; the default "record" is the above): the component is chosen without the
    record's label, by utils.detect.detect_objects(depth, intrinsics, segments=the found ones, seed and first_frame of
    components, **detector) on every frame of the call -- detector: its meshes, ppf_models and parameters -- as the
    component it assigned to target_cls (the earliest round when there are several).  The record's label is read only to
    report: segment_iou is the chosen component's IoU against the record's target_cls + 1 pixels, detect_agree [B] bool
    (numpy) says whether match_components would have picked the same component, and counts gains 'detected' (in place of
    'matched') and 'agree'.  Frames in which nothing was assigned to the class are dropped.  (The element is formed before
    evaluate_batch runs, so replay=True there neither sees nor records the detection.)"""
    from .train_cloudAAE_ycbv import get_object_model, get_rotation_matrix, transform_object_model
    from .utils import hidden_point_removal as hpr
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    require(labels in ("record", "components"), "labels must be 'record' or 'components'")
    require(components is None or labels == "components", "components= needs labels='components'")
    require(choose in ("record", "detect"), "choose must be 'record' or 'detect'")
    require(choose == "record" or (labels == "components" and detector is not None),
            "choose='detect' needs labels='components' and detector=dict(meshes=..., ppf_models=...)")
    require(detector is None or choose == "detect", "detector= needs choose='detect'")
    position = [i for i, f in enumerate(frames) if int(f["class_one_hot"][target_cls]) == 1]
    chunk = frames                                                                # (components mode segments all of it)
    frames = [frames[i] for i in position]                                        # :294
    if not frames:
        return None
    shapes = {f["depth"].shape for f in (chunk if labels == "components" else frames)}
    require(len(shapes) == 1, "frames of one call must share their size")
    depth = np.stack([f["depth"] for f in frames])
    label = np.stack([f["label"] for f in frames])
    intr = record_intrinsics(frames)
    segment_iou, agree = None, None
    if labels == "components":
        found = _component_labels(chunk, position, (frames, depth, intr, label), target_cls, device, components, counts,
                                  detector)
        if found is None:
            return None
        frames, depth, intr, label, segment_iou, agree = found
    r = seg_util.extract_segments(depth, label, intr, classes=[[target_cls]] * len(frames),
                                  quaternions=np.stack([f["quaternions"] for f in frames]),
                                  translations=np.stack([f["translations"] for f in frames]), num_point=num_point,
                                  device=device)
    smp = seg_util.sample_segments(r, num_point, seed=seed)
    keep = np.nonzero(r.kept)[0]
    if len(keep) == 0:
        return None
    sel = torch.from_numpy(keep).to(device)
    B = len(keep)
    el = dict(xyz_inlier=smp["xyz_inlier"].index_select(0, sel), xyz=smp["xyz"].index_select(0, sel),
              class_id=torch.full((B,), int(target_cls), dtype=torch.int64, device=device),
              translation=torch.from_numpy(r.translation[keep]).to(device),
              axisangle=torch.from_numpy(np.stack([seg_util.quat2axag(q) for q in r.quaternion[keep]])
                                         .astype(np.float64)).to(device))
    models = obj_models if isinstance(obj_models, torch.Tensor) else torch.from_numpy(np.asarray(obj_models, np.float32))
    models = models.to(device=device, dtype=torch.float32).contiguous()
    el["obj_batch"] = models.index_select(0, el["class_id"]).contiguous()
    x = dict(class_id=el["class_id"], translation=el["translation"], axisangle=el["axisangle"].clone())
    x = transform_object_model(get_rotation_matrix(get_object_model(x, models)))
    x = hpr.hidden_point_removal_org(hpr.sphericalFlip_org(x, None, 0.8 * math.pi), seed=int(seed))
    el["visiblePoints_org"] = x["visiblePoints_org"]
    of = np.asarray(r.frame, np.int64)[keep]                                      # the kept samples' frames
    el["seq_id"] = np.array([int(frames[i]["seq_id"]) for i in of], np.int64)
    el["frame_id"] = np.array([int(frames[i]["frame_id"]) for i in of], np.int64)
    el["num_valid_points_in_segment"] = r.num_valid_points_in_segment[keep]
    if keep_frames:
        el["frame_depth"] = torch.from_numpy(np.ascontiguousarray(depth[of].astype(np.uint16)).view(np.int16)).to(device)
        el["frame_intrinsics"] = torch.from_numpy(intr[of]).to(device)
    if keep_labels:
        el["frame_label"] = torch.from_numpy(np.ascontiguousarray(label[of].astype(np.uint8))).to(device)
        el["frame_want"] = torch.full((B,), int(target_cls) + 1, dtype=torch.int32, device=device)
    if segment_iou is not None:
        el["segment_iou"] = segment_iou[of]
    if agree is not None:
        el["detect_agree"] = agree[of]
    return el


def _component_labels(chunk, position, held, target_cls, device, components, counts, detector):
    """labels="components" of element_from_frames.  held: (frames, depth, intr, label) of the frames `position` of the call,
    those that hold the class.  -> those of them that have a component for the class, their label images holding that
    component alone as target_cls + 1, with the components' IoUs and, with a detector, whether the record's label agrees:
    (frames, depth, intr, label, segment_iou, agree); None when no frame has one.  counts is updated either way."""
    from .utils import depth_components as dc_util
    frames, depth, intr, label = held
    # every frame of the call is segmented, also those without the class: frame i of the call then has the global
    # index first_frame + i whatever its neighbours hold
    chunk_depth, chunk_intr = np.stack([f["depth"] for f in chunk]), record_intrinsics(chunk)
    found = dc_util.segment_depth(chunk_depth, chunk_intr, device=device, **(components or {}))
    found_label = found.label.index_select(0, torch.tensor(position, dtype=torch.int64, device=device))
    ks, ious = dc_util.match_components(found_label, torch.from_numpy(np.ascontiguousarray(label, np.uint8)).to(device),
                                        depth, int(target_cls) + 1)
    agree = None
    if detector is not None:
        ks_record = ks
        ks, ious = _detected_components(chunk_depth, chunk_intr, position, found, found_label, label, depth, target_cls,
                                        components, detector)
        agree = ks == ks_record
    hit = np.nonzero(ks > 0)[0]
    if counts is not None:
        counts["frames"] = counts.get("frames", 0) + len(frames)
        key = "matched" if detector is None else "detected"
        counts[key] = counts.get(key, 0) + len(hit)
        if agree is not None:
            counts["agree"] = counts.get("agree", 0) + int(agree[hit].sum())
    if len(hit) == 0:
        return None
    k_dev = torch.from_numpy(ks[hit]).to(device=device, dtype=torch.uint8)[:, None, None]
    sel_f = torch.from_numpy(hit).to(device)
    relabelled = torch.where(found_label.index_select(0, sel_f) == k_dev,
                             torch.full((), int(target_cls) + 1, dtype=torch.uint8, device=device),
                             torch.zeros((), dtype=torch.uint8, device=device))
    return ([frames[int(i)] for i in hit], depth[hit], intr[hit], relabelled.cpu().numpy(), ious[hit],
            None if agree is None else agree[hit])


def _detected_components(chunk_depth, chunk_intr, position, found, found_label, label, depth, target_cls, components, detector):
    """For the frames `position` of the call: the label value (k + 1; 0: none) of the component that detect_objects assigned
    to target_cls, and that component's IoU against the record's target_cls + 1 pixels with depth (the report)."""
    from .utils import detect as detect_util
    device = found_label.device
    comp = components or {}
    det = detect_util.detect_objects(chunk_depth, chunk_intr, segments=found, seed=comp.get("seed", 0),
                                     first_frame=comp.get("first_frame", 0), **detector)
    ks = np.zeros(len(position), np.int64)
    for i, f in enumerate(position):
        mine = np.nonzero(det.table["det_class"][f] == int(target_cls))[0]
        if len(mine):
            ks[i] = int(mine[np.argmin(det.table["det_rank"][f][mine])]) + 1
    chosen = (found_label == torch.from_numpy(ks).to(device=device, dtype=torch.uint8)[:, None, None]) & (found_label != 0)
    target = (torch.from_numpy(np.ascontiguousarray(label, np.uint8)).to(device) == int(target_cls) + 1) & \
        (torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device) != 0)
    both = torch.stack([(chosen & target).sum(dim=(1, 2)), (chosen | target).sum(dim=(1, 2))]).cpu().numpy().astype(np.float64)
    return ks, np.where(ks > 0, both[0] / np.maximum(both[1], 1.0), 0.0)


def verify_lines(rows):
    """One line per class from (class_id, verify_best, verify_margin) device tensors of the batches (one read-back): how
    many samples kept hypothesis 0 (the prediction) and how many chose each of the next three, and the mean margin."""
    if not rows:
        return []
    cls = torch.cat([r[0] for r in rows]).cpu().numpy()
    best = torch.cat([r[1] for r in rows]).cpu().numpy()
    margin = torch.cat([r[2] for r in rows]).cpu().numpy()
    out = []
    for c in np.unique(cls):
        sel = cls == c
        k = [int((best[sel] == j).sum()) for j in range(4)]
        out.append("verify class %d n %d kept0 %d chose1 %d chose2 %d chose3 %d mean_margin %f"
                   % (int(c), int(sel.sum()), k[0], k[1], k[2], k[3], float(margin[sel].mean())))
    return out


def propose_lines(rows, flips):
    """One line per class from (class_id, verify_best) device tensors of the batches (one read-back) when the candidates
    were candidate 0 (the prediction), `flips` - 1 further hypotheses of the class and then the proposals: how many winners
    came from each."""
    if not rows:
        return []
    cls = torch.cat([r[0] for r in rows]).cpu().numpy()
    best = torch.cat([r[1] for r in rows]).cpu().numpy()
    out = []
    for c in np.unique(cls):
        b = best[cls == c]
        out.append("propose class %d n %d from_prediction %d from_flip %d from_proposal %d"
                   % (int(c), len(b), int((b == 0).sum()), int(((b > 0) & (b < flips)).sum()), int((b >= flips).sum())))
    return out


def _take(el, lo, hi):
    return {k: v[lo:hi] for k, v in el.items()}


def main(argv=None):
    """evaluate_cloudAAE_ycbv.py's command line (:688-716, :356-657) without the visualisation and without RGB.
    Reads <data_dir>/<seq>_pcnn.tfrecord of the class's test sequences (:43-63) -- or, with --files A,B,..., those files,
    e.g. rendered ones (utils/render.py) -- file after file, in record order (the
    reference interleaves them at random with sample_from_datasets), and prints the per-batch and the final loss
    lines (:568, :652-657).  A last batch smaller than --batch_size is not evaluated (the reference's reshape to
    BATCH_SIZE, :338, cannot take it).  --icp adds the refined pose's losses; --icp_plane refines by point-to-plane ICP
    on the class models' normals instead (computed once, before the loop).  --score prints, after the final line,
    the ADD / ADD-S summary of the predicted (and refined) poses per class and over all (PoseScoreLog.lines).  --bop
    --meshes DIR [--mesh_scale X] prints, after those, BOP's average recalls (BopScoreLog.lines): class i is the i-th
    *.ply of DIR in sorted order (the convention of utils/render.py).  --symmetries none|auto|FILE: the transform sets
    MSSD and MSPD take the minimum over -- none (the default): the identity alone; auto: utils.symmetry.find_symmetries
    for the run's class, on the mesh when --meshes is given, else on the class model; FILE: what `python -m
    cloudaae_amd.utils.symmetry` wrote.  The found kinds are printed before the score lines, and with --score the
    classes whose set holds more than the identity take the place of pose_score.SYMMETRIC_CLASSES.  With a symmetry set
    the translation and rotation errors are also taken against the nearest equivalent label (evaluate_batch(symmetries=)):
    every batch line and the final line get their *_sym twins.  --verify --meshes DIR: the identity and the three principal
    half turns of the class model (utils.pose_verify.flip_hypotheses) are composed with the predicted pose, refined like
    it under --icp, and judged against the frame (evaluate_batch(verify=)); the winner is scored as a further pose `ver`
    in every summary, and after the summaries one line per class says how often which hypothesis was kept.  --propose ppf
    (with --verify --meshes): --propose_top pose proposals by point-pair-feature voting on --propose_points oriented
    points of the class's mesh (utils/ppf.py) join the candidates, and a last line per class says how many winners came
    from the prediction, from a flip and from a proposal.  --labels components (with the --components_* parameters): the
    label images are found from the depth alone (element_from_frames(labels="components")); a last line says how many
    frames held the class, how many of them had a matching component, and the mean IoU of the segments that were kept.
    --choose detect (with --labels components --meshes DIR; --detect_classes, --detect_top, --detect_min_score N/D,
    --detect_margin): the component is chosen by utils.detect.detect_objects among the meshes' classes instead of by the
    record's label (element_from_frames(choose="detect")); the last line then reads `detect class c frames n detected m
    agree a mean_iou x`: the frames that held the class, those in which a component was assigned to it, those of them in
    which the record's label would have picked the same component, and the mean IoU of the segments that were kept."""
    from . import train_cloudAAE_ycbv as T
    args = _arguments(argv)
    torch.cuda.set_device(args.gpu)
    obj_path = args.object_model or os.path.join(os.path.dirname(os.path.abspath(args.data_dir)),
                                                 "object_model_tfrecord", "obj_models.tfrecords")
    models, _ = tfrecord_io.read_and_decode_obj_model(obj_path)
    graph = T.TrainGraph({"num_point": args.num_point, "gpu": args.gpu}, {}, {"batch_size": args.batch_size})
    graph.restore(args.trained_model)
    files = _record_files(args)
    icp, model_normals = args.icp, None
    if args.icp_plane:
        icp = {'estimation': 'point_to_plane'}
        # the normals of the 21 class models, once; a batch selects its classes' rows
        model_normals = normals_util.estimate_normals(
            torch.from_numpy(np.ascontiguousarray(models, np.float32)).cuda(), radius=NORMAL_RADIUS)[0]
    sym_sets, sym_lines, sym_table = _symmetry_inputs(args, models, graph.device)
    names = ("pred",) + (("icp",) if args.icp else ()) + (("ver",) if args.verify else ())      # the scored poses
    log, bop, bop_log, verify, propose, detector = _scoring_inputs(args, models, names, sym_sets)
    comp_counts, comp_iou, verify_rows = {}, [], []
    comp = _components_inputs(args, comp_counts, detector)
    batch_idx = 0
    tot = {}                                     # sums of the batch lines' means, by key
    for b in _batches(args, files, models, comp, comp_iou):
        el_b = {k: v for k, v in b.items() if isinstance(v, torch.Tensor)}
        if model_normals is not None:
            el_b['obj_normals'] = model_normals.index_select(0, el_b['class_id'])
        out = evaluate_batch(graph, el_b, icp=icp, score=args.score, bop=bop, symmetries=sym_table, verify=verify,
                             propose=propose)
        if verify is not None:
            verify_rows.append((b["class_id"].to(torch.int64), out["verify_best"].to(torch.int64), out["verify_margin"]))
        if bop_log is not None:
            bop_log.append(b["class_id"], *[torch.stack([out[m + n] for n in bop_log.poses], dim=1)
                                            for m in ("vsd_", "mssd_", "mspd_")],
                           width=int(b["frame_depth"].shape[2]), seq=b["seq_id"], frame=b["frame_id"])
        if log is not None:
            log.append(b["class_id"], torch.stack([out["add_" + n] for n in log.poses], dim=1),
                       torch.stack([out["adds_" + n] for n in log.poses], dim=1), seq=b["seq_id"], frame=b["frame_id"])
        line, values = _batch_line(batch_idx, b, out, names, sym_table is not None)
        for k, v in values.items():
            tot[k] = tot.get(k, 0.0) + v
        print(line)
        batch_idx += 1
    print("batch size %d" % batch_idx)
    if batch_idx:
        print("trans_loss %f axag_loss %f" % (tot["trans_loss"] / batch_idx, tot["axag_loss"] / batch_idx))
        if sym_table is not None:
            print(" ".join("%s %f" % (k, v / batch_idx) for k, v in tot.items() if k.endswith("_sym")))
    lines = sym_lines + (log.lines() if log is not None else []) + (bop_log.lines() if bop_log is not None else [])
    lines += verify_lines(verify_rows)
    if propose is not None:
        lines += propose_lines([r[:2] for r in verify_rows], verify['hypotheses'].max_members)
    if args.labels == "components":
        lines.append(_components_line(args, comp_counts, comp_iou))
    for line in lines:
        print(line)
    sys.stdout.flush()
    return 0


def _arguments(argv):
    """The command line's arguments, parsed and checked; --icp_plane sets --icp."""
    from .utils import depth_components as dc_util
    from .utils import detect as detect_util
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", default="ycb_video_data_tfRecords")
    p.add_argument("--files", default=None,
                   help="comma-separated frame record files to read instead of the class's test sequences under --data_dir "
                        "(e.g. what `python -m cloudaae_amd.utils.render` wrote)")
    p.add_argument("--object_model", default=None,
                   help="obj_models.tfrecords [default: <data_dir>/../object_model_tfrecord/obj_models.tfrecords]")
    p.add_argument("--trained_model", required=True, help="checkpoint prefix (TrainGraph.restore)")
    p.add_argument("--target_cls", type=int, default=9)
    p.add_argument("--num_point", type=int, default=256)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--icp", action="store_true")
    p.add_argument("--icp_plane", action="store_true",
                   help="refine by point-to-plane ICP on the class models' normals (implies --icp)")
    p.add_argument("--score", action="store_true", help="ADD / ADD-S, AUC and accuracy summary of the scored poses")
    p.add_argument("--bop", action="store_true", help="BOP's VSD / MSSD / MSPD average recalls of the scored poses (needs --meshes)")
    p.add_argument("--meshes", default=None, help="directory of *.ply files; class i is the i-th in sorted order")
    p.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the meshes' coordinates (0.001: millimetres to metres)")
    p.add_argument("--symmetries", default="none",
                   help="none, auto (found from --meshes, else from the class models) or a file written by "
                        "`python -m cloudaae_amd.utils.symmetry`: the objects' symmetry transforms for --bop and --score")
    p.add_argument("--verify", action="store_true",
                   help="verify the flip hypotheses of the predicted pose against the observed depth and score the winner "
                        "as the pose `ver` (needs --meshes)")
    p.add_argument("--verify_tau", type=float, default=0.01, help="depth tolerance of --verify, metres")
    p.add_argument("--propose", default=None, choices=("ppf",),
                   help="add pose proposals by point-pair-feature voting to the candidates of --verify (needs --verify --meshes)")
    p.add_argument("--propose_top", type=int, default=4, help="proposals per sample")
    p.add_argument("--propose_points", type=int, default=256, help="oriented points of the class's mesh in the pair table")
    p.add_argument("--labels", default="record", choices=("record", "components"),
                   help="record: the records' label images; components: label images found from the depth alone "
                        "(utils/depth_components.py), the record's label associating the class with a component")
    p.add_argument("--components_n_hyp", type=int, default=dc_util.N_HYP, help="plane hypotheses per frame")
    p.add_argument("--components_stride", type=int, default=dc_util.STRIDE, help="every stride-th pixel votes for the plane")
    p.add_argument("--components_tol", type=float, default=dc_util.TOL, help="distance of a plane inlier, metres")
    p.add_argument("--components_max_height", type=float, default=dc_util.MAX_HEIGHT, help="foreground height above the plane, metres")
    p.add_argument("--components_min_plane_percent", type=int, default=dc_util.MIN_PLANE_PERCENT,
                   help="a plane needs this share of the tested pixels")
    p.add_argument("--components_jump", type=float, default=dc_util.JUMP, help="depth step that cuts a component, metres")
    p.add_argument("--components_min_pixels", type=int, default=dc_util.MIN_PIXELS)
    p.add_argument("--components_max", type=int, default=dc_util.MAX_COMPONENTS, help="components kept per frame")
    p.add_argument("--components_creases", action="store_true",
                   help="cut the foreground along its concave creases before labelling, so that touching objects separate")
    p.add_argument("--components_crease_step", type=int, default=dc_util.STEP, help="pixels to either end of a chord, 1 .. 8")
    p.add_argument("--components_crease_smooth", type=int, default=dc_util.SMOOTH, help="half side of the smoothing box, 0 .. 7")
    p.add_argument("--components_crease_angle", type=float, default=dc_util.ANGLE,
                   help="degrees a fold must deviate from flat to count as a crease")
    p.add_argument("--choose", default="record", choices=("record", "detect"),
                   help="with --labels components: record associates the class with a component by the record's label; "
                        "detect decides it without the label (utils/detect.py; needs --meshes DIR)")
    p.add_argument("--detect_classes", default=None, help="comma-separated class ids the detector knows [default: every mesh]")
    p.add_argument("--detect_top", type=int, default=detect_util.TOP, help="pose proposals per (component, class)")
    p.add_argument("--detect_min_score", default="%d/%d" % detect_util.MIN_SCORE, help="N/D: a pair below this fraction is not assigned")
    p.add_argument("--detect_margin", type=float, default=detect_util.MARGIN, help="of a component's box, added on either side")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--frames_per_launch", type=int, default=8)
    p.add_argument("--gpu", type=int, default=0)
    args = p.parse_args(argv)
    if args.bop and not args.meshes:
        p.error("--bop needs --meshes DIR")
    if args.verify and not args.meshes:
        p.error("--verify needs --meshes DIR")
    if args.propose and not (args.verify and args.meshes):
        p.error("--propose needs --verify and --meshes DIR")
    if args.choose == "detect" and not (args.labels == "components" and args.meshes):
        p.error("--choose detect needs --labels components and --meshes DIR")
    args.icp = args.icp or args.icp_plane
    return args


def _record_files(args):
    """The frame record files to read: those of --files, or the class's test sequences under --data_dir that exist."""
    if args.files:
        files = [f for f in args.files.split(",") if f]
        missing = [f for f in files if not os.path.exists(f)]
        require(files and not missing, "--files: no such file: %s" % ", ".join(missing))
        return files
    files = [os.path.join(args.data_dir, str(i).zfill(4) + "_pcnn.tfrecord") for i in VALID_SEQ_ID[args.target_cls]]
    files = [f for f in files if os.path.exists(f)]
    require(files, "no <seq>_pcnn.tfrecord of class %d under %s" % (args.target_cls, args.data_dir))
    return files


def _frame_chunks(files, frames_per_launch):
    """The decoded records of the files in order, frames_per_launch at a time; a chunk does not span two files."""
    for fn in files:
        buf = []
        for rec in tfrecord_io.tf_record_iterator(fn):
            buf.append(tfrecord_io.decode_frame(rec))
            if len(buf) == frames_per_launch:
                yield buf
                buf = []
        if buf:
            yield buf


def _batches(args, files, models, comp, comp_iou):
    """The elements of the record files, one per chunk of frames (its seed --seed + the chunk's number), cut into batches
    of --batch_size, host and device entries alike; a last smaller batch is not given.  comp: _components_inputs, whose
    first_frame is set per chunk; the kept segments' IoUs are added to comp_iou."""
    pending, n_frames_seen = None, 0
    for n_launch, chunk in enumerate(_frame_chunks(files, args.frames_per_launch)):
        if comp:
            comp["components"]["first_frame"] = n_frames_seen
        el = element_from_frames(chunk, args.target_cls, args.num_point, models, seed=args.seed + n_launch,
                                 keep_frames=args.bop or args.verify, keep_labels=args.verify, **comp)
        n_frames_seen += len(chunk)
        if el is None:
            continue
        if "segment_iou" in el:
            comp_iou.append(el["segment_iou"])
        pending = el if pending is None else {k: (torch.cat([pending[k], v]) if isinstance(v, torch.Tensor)
                                                  else np.concatenate([pending[k], v])) for k, v in el.items()}
        while len(pending["class_id"]) >= args.batch_size:
            yield _take(pending, 0, args.batch_size)
            pending = _take(pending, args.batch_size, len(pending["class_id"]))


def _components_line(args, counts, ious):
    """The closing line of --labels components, or of --choose detect: the frames that held the class, those with a
    component for it (and, detected, those where the record's label agrees), and the mean IoU of the kept segments."""
    iou = float(np.concatenate(ious).mean()) if ious else 0.0
    if args.choose == "detect":
        return "detect class %d frames %d detected %d agree %d mean_iou %f" % (
            args.target_cls, counts.get("frames", 0), counts.get("detected", 0), counts.get("agree", 0), iou)
    return "components class %d frames %d matched %d mean_iou %f" % (
        args.target_cls, counts.get("frames", 0), counts.get("matched", 0), iou)


def _symmetry_inputs(args, models, device):
    """--symmetries -> (sym_sets {class: [n,4,4]} or None, the lines that report them, the SymmetryTable or None)."""
    if args.symmetries == "none":
        return None, [], None
    from .utils import symmetry as sym_util
    if args.symmetries == "auto":
        c = args.target_cls                      # the one class this run evaluates
        if args.meshes:
            found = sym_util.symmetries_of_meshes([mesh_models.mesh_files(args.meshes)[c]], scale=args.mesh_scale, mesh_ids=[c])
        else:
            found = sym_util.symmetries_of_models(models[c:c + 1])
        return ({c: found[0]["transforms"]}, sym_util.kind_lines(found, classes=[c]),
                pose_equiv.SymmetryTable.from_results(found, len(models), [c], device))
    require(os.path.exists(args.symmetries), "--symmetries: no such file: %s" % args.symmetries)
    sym_sets = sym_util.load_symmetries(args.symmetries)
    return (sym_sets, ["symmetry class %d transforms %d" % (c, len(t)) for c, t in sorted(sym_sets.items())],
            pose_equiv.load_symmetry_table(args.symmetries, len(models), device))


def _scoring_inputs(args, models, names, sym_sets):
    """What --score, --bop, --verify, --propose and --choose detect need -> (log, bop, bop_log, verify, propose, detector),
    None where the option is off.  The mesh directory is packed once and the class models' diameters are taken once: the
    consumers get the same PackedMeshes, which none of them writes into (they pass its tensors to the kernels as inputs)."""
    c = args.target_cls
    log = bop = bop_log = verify = propose = detector = None
    if args.score or args.bop:
        diam = score_util.model_diameter(torch.from_numpy(np.ascontiguousarray(models, np.float32)).cuda())
    if args.bop or args.verify or args.choose == "detect":
        mesh_paths = mesh_models.mesh_files(args.meshes)
        packed = mesh_models.pack_meshes(mesh_paths, args.mesh_scale)
    if args.score:
        symmetric = {} if sym_sets is None else dict(symmetric=[k for k, t in sym_sets.items() if len(t) > 1])
        log = score_util.PoseScoreLog(names, diameters=diam, **symmetric)
    if args.bop:
        bop = dict(meshes=packed, diameters=diam)
        if sym_sets is not None:
            bop['symmetries'] = sym_sets
        bop_log = bop_util.BopScoreLog(names, diameters=diam)
    if args.verify:
        verify = dict(meshes=packed, hypotheses=verify_util.HypothesisTable.from_models(models[c:c + 1], [c], len(models)),
                      tau=args.verify_tau)
    if args.propose:
        propose = dict(models=ppf_util.PPFModels.from_meshes([mesh_paths[c]], num_point=args.propose_points,
                                                              scale=args.mesh_scale, classes=[c], num_class=len(models)),
                       top=args.propose_top)
    if args.choose == "detect":
        det_classes = (list(range(len(mesh_paths))) if args.detect_classes is None
                       else [int(k) for k in args.detect_classes.split(",") if k])
        num, den = (int(x) for x in args.detect_min_score.split("/"))
        detector = dict(meshes=packed,
                        ppf_models=ppf_util.PPFModels.from_meshes([mesh_paths[k] for k in det_classes],
                                                                  num_point=args.propose_points, scale=args.mesh_scale,
                                                                  classes=det_classes, num_class=len(mesh_paths)),
                        classes=det_classes, top=args.detect_top, min_score=(num, den), margin=args.detect_margin,
                        num_point=args.num_point)
    return log, bop, bop_log, verify, propose, detector


def _components_inputs(args, counts, detector):
    """The labels, components, counts, choose and detector arguments of element_from_frames under --labels components
    (first_frame is set per chunk); nothing otherwise."""
    if args.labels != "components":
        return {}
    comp = dict(labels="components", counts=counts,
                components=dict(seed=args.seed, first_frame=0, n_hyp=args.components_n_hyp, stride=args.components_stride,
                                tol=args.components_tol, max_height=args.components_max_height,
                                min_plane_percent=args.components_min_plane_percent, jump=args.components_jump,
                                min_pixels=args.components_min_pixels, max_components=args.components_max))
    if args.components_creases:
        comp["components"]["creases"] = dict(step=args.components_crease_step, smooth=args.components_crease_smooth,
                                             angle=args.components_crease_angle)
    if detector is not None:
        comp.update(choose="detect", detector=detector)
    return comp


def _batch_line(batch_idx, b, out, names, with_sym):
    """(the line of one batch, {key: value} of the means it prints): the errors of the poses `names` in turn, then,
    with_sym, their _sym twins in the same order; axag is printed as rot."""
    tags = ["" if n == "pred" else "_" + n for n in names]
    keys = [k + tag + sym for sym in (("", "_sym") if with_sym else ("",)) for tag in tags for k in ("trans_loss", "axag_loss")]
    values = {k: float(out[k]) for k in keys}
    line = "Validation batch %d seq_id %d frame_id %d" % (batch_idx, int(b["seq_id"][0]), int(b["frame_id"][0]))
    return line + "".join(" %s %f" % (k.replace("axag", "rot"), v) for k, v in values.items()), values


if __name__ == "__main__":
    sys.exit(main())
