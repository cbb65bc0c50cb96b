"""GPU: evaluate_batch replayed by hand.  Every pose set it scores -- the predicted pose, the refined one (both ICP
estimations), the verified one -- is formed and scored here through the public functions of utils/ and losses/ alone
(refine_pose_icp, estimate_normals, get_translation_error, get_rotation_error, nearest_equivalent_pose, score_poses, vsd,
mssd_mspd) and compared with what evaluate_batch returns bit for bit, for the option combinations one by one; then the
recorded pass and the command line's batch line.  Nothing here depends on how evaluate_cloudAAE_ycbv.py is organised."""
import os
import warnings

import numpy as np
import pytest
import torch

import mesh_models_reference as MR
import pose_verify_reference as V

pytestmark = pytest.mark.gpu

N = 128
PLANE = {"estimation": "point_to_plane"}
ICP_NAMES = dict(transformation="transformation_icp", rot_axag="rot_icp", trans="trans_icp", fitness="fitness_icp",
                 inlier_rmse="inlier_rmse_icp", iterations="iterations_icp")
ERRORS = ("trans_loss", "trans_loss_perSample", "axag_loss", "axag_loss_perSample")
TAG = dict(pred="", icp="_icp", ver="_ver")
BASE = {"xyz_recon", "xyz_recon_FPS", "rot_pred", "trans_pred", "xyz_loss", "xyz_loss_per_sample", "mean_dist_loss",
        "mean_dist_loss_perSample", "element_mean", "end_points"}
VERIFY = {"verify_best", "verify_score", "verify_margin", "verify_counts", "verify_candidates", "transformation_ver", "rot_ver",
          "trans_ver"}
# the identity and the three half turns about the axes through the origin: a group, so a finite symmetry set
HALF_TURNS = np.stack([np.diag(d) for d in ([1.0, 1, 1, 1], [1.0, -1, -1, 1], [-1.0, 1, -1, 1], [-1.0, -1, 1, 1])])


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def records(hip, dev, tmp_path_factory):
    """The two made-up meshes, four rendered frames of 160 x 120 and the class models as tests/test_32_pose_verify_gpu.py
    builds them; the element of class 0 with its frames and labels from two seeds, a randomly initialised graph, its
    checkpoint, and the tables the options take."""
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import normals as normals_util
    from cloudaae_amd.utils import pose_equiv, pose_score, render
    from cloudaae_amd.utils import pose_verify as PV
    tmp = tmp_path_factory.mktemp("paths")
    os.makedirs(str(tmp / "meshes"))
    lv, lt = V.l_prism()
    cv, ct, _ = MR.cube()
    _write_ply(str(tmp / "meshes" / "obj_000001.ply"), lv * np.float32(1500.0), lt)
    _write_ply(str(tmp / "meshes" / "obj_000002.ply"), (cv - np.float32(0.5)) * np.array([240.0, 240.0, 30.0], np.float32), ct)
    render.main(["--meshes", str(tmp / "meshes"), "--out", str(tmp / "data"), "--frames", "4", "--objects", "2", "--seq", "48",
                 "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    path = str(tmp / "data" / "0048_pcnn.tfrecord")
    obj = str(tmp / "obj_models.tfrecords")
    mm.main(["--meshes", str(tmp / "meshes"), "--out", obj, "--scale", "0.001", "--oversample", "2"])
    models, _ = tfrecord_io.read_and_decode_obj_model(obj)
    files = mm.mesh_files(str(tmp / "meshes"))
    packed = mm.pack_meshes(files, 0.001, dev)
    frames = tfrecord_io.read_frames(path, verify=True)
    els = []
    for seed in (4, 5):
        el = E.element_from_frames(frames, 0, N, models, seed=seed, device=dev, keep_frames=True, keep_labels=True)
        assert el is not None
        els.append({k: v for k, v in el.items() if isinstance(v, torch.Tensor)})
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": 1})
    # a randomly initialised network predicts poses far outside the frame, where no ICP finds a pair and no rendering a
    # pixel; with the two pose heads' last layers set to a constant the prediction is a fixed rotation at the segment's
    # centroid (plus an offset): near enough for the refinement and the verification to have something to do
    heads = {"dgcnn_output_rot": [0.3, -0.2, 0.5], "dgcnn_output_trans": [0.01, -0.01, 0.02]}
    state = graph.store.state_dict()
    head_state = {}
    for scope, bias in heads.items():
        head_state[scope + "/weights"] = torch.zeros_like(state[scope + "/weights"])
        head_state[scope + "/biases"] = torch.tensor(bias).reshape(state[scope + "/biases"].shape)
    graph.store.load_state_dict(head_state, strict=False)
    ckpt = graph.save(str(tmp / "model.ckpt"))
    models_dev = torch.from_numpy(np.ascontiguousarray(models, np.float32)).to(dev)
    # normals that are not the default's, so that given normals can be told from estimated ones
    given = normals_util.estimate_normals(models_dev, radius=0.03)[0].index_select(0, els[0]['class_id'])
    table = pose_equiv.SymmetryTable.from_results([dict(kind="finite", centre=[0.0, 0.0, 0.0], transforms=HALF_TURNS)],
                                                  num_class=len(models), classes=[0], device=dev)
    verify = dict(meshes=packed, mesh_index=None, hypotheses=PV.HypothesisTable.from_models(models[:1], classes=[0], num_class=2),
                  tau=0.01, mode=0)
    bop = dict(meshes=packed, diameters=pose_score.model_diameter(models_dev), symmetries={0: HALF_TURNS})
    return dict(tmp=tmp, path=path, obj=obj, files=files, models=models, frames=frames, el=els[0], el2=els[1], graph=graph,
                ckpt=ckpt[:-len(".npz")], given=given, table=table, verify=verify, bop=bop)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), what


# ---- 1: the refined pose, both estimations ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["point_to_point", "plane_estimated_normals", "plane_given_normals"])
def test_the_refined_pose_is_one_refine_pose_icp_call(hip, dev, records, case):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import icp as icp_util
    from cloudaae_amd.utils import normals as normals_util
    el, graph = dict(records['el']), records['graph']
    if case == "plane_given_normals":
        el['obj_normals'] = records['given']
    out = E.evaluate_batch(graph, el, icp=True if case == "point_to_point" else PLANE)
    scene = el['xyz_inlier'][:, :N]
    if case == "point_to_point":
        direct = icp_util.refine_pose_icp(el['obj_batch'], scene, out['rot_pred'], out['trans_pred'])
    else:
        normals = el.get('obj_normals')
        if normals is None:
            normals = normals_util.estimate_normals(el['obj_batch'], radius=0.015)[0]
            assert not torch.equal(normals, records['given'])
        direct = icp_util.refine_pose_icp(scene, el['obj_batch'], out['rot_pred'], out['trans_pred'], estimation="point_to_plane",
                                          normals=normals, pose_maps_target_to_source=True)
    for k, name in ICP_NAMES.items():
        _same(out[name], direct[k], name)
    assert float(out['fitness_icp'].max()) > 0.0 and not torch.equal(out['trans_icp'], out['trans_pred'])    # it had pairs and moved


# ---- 2: candidate 0 of the verification -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["point_to_point", "plane_estimated_normals", "plane_given_normals"])
def test_candidate_0_is_the_refined_prediction(hip, dev, records, case):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    el, graph = dict(records['el']), records['graph']
    if case == "plane_given_normals":
        el['obj_normals'] = records['given']
    icp = True if case == "point_to_point" else PLANE
    plain = E.evaluate_batch(graph, el, icp=icp)
    ver = E.evaluate_batch(graph, el, icp=icp, verify=records['verify'])
    assert int(ver['verify_candidates'].shape[1]) == 4
    _same(ver['verify_candidates'][:, 0], plain['transformation_icp'], case)
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            _same(ver[k], v, k)


# ---- 3: every pose set scored alike ---------------------------------------------------------------------------------------------
def _keys(icp=False, score=False, symmetries=False, verify=False, bop=False):
    names = ["pred"] + (["icp"] if icp else []) + (["ver"] if verify else [])
    keys = set(BASE) | (set(ICP_NAMES.values()) if icp else set()) | (VERIFY if verify else set())
    for n in names:
        keys |= {k + TAG[n] for k in ERRORS}
        if symmetries:
            keys |= {k + TAG[n] + "_sym" for k in ERRORS}
        if score:
            keys |= {"add_" + n, "adds_" + n}
        if bop:
            keys |= {"vsd_" + n, "mssd_" + n, "mspd_" + n}
    return keys


def _by_hand(el, out, names, table, bop):
    """The errors and scores of the pose sets `names` of `out`, from its rot_*, trans_* and transformation_* alone."""
    from cloudaae_amd.losses import angular_distance_taylor, trans_distance
    from cloudaae_amd.utils import bop_score, pose_equiv, pose_score
    from cloudaae_amd.utils import icp as icp_util
    want = {}
    cls = el['class_id'].to(torch.int64)
    translation, axisangle = el['translation'].to(torch.float32), el['axisangle']
    for n in names:
        rot = out['rot_pred'] if n == "pred" else icp_util.to_float32(out['rot_' + n])
        labels = [("", translation, axisangle)]
        if table is not None:
            near = pose_equiv.nearest_equivalent_pose(rot, axisangle, translation, cls, table)
            labels.append(("_sym", near['trans_equiv'], near['rot_equiv']))
        for sym, t, r in labels:
            want["trans_loss%s%s" % (TAG[n], sym)], want["trans_loss_perSample%s%s" % (TAG[n], sym)] = \
                trans_distance.get_translation_error(out['trans_' + n], t)
            want["axag_loss%s%s" % (TAG[n], sym)], want["axag_loss_perSample%s%s" % (TAG[n], sym)] = \
                angular_distance_taylor.get_rotation_error(rot, r)
    gt = pose_score.pose_matrix(axisangle, translation.contiguous())
    pred = pose_score.pose_matrix(out['rot_pred'].contiguous(), out['trans_pred'].contiguous())
    # the predicted and the refined pose go through one launch, the verified one through its own
    sets = [(("pred", "icp"), pose_score.stack_poses(pred, out['transformation_icp'])) if "icp" in names else
            (("pred",), pred.unsqueeze(1))]
    if "ver" in names:
        sets.append((("ver",), out['transformation_ver'].unsqueeze(1)))
    B = int(cls.shape[0])
    cls_host = cls.cpu().numpy()
    for group, est in sets:
        s = pose_score.score_poses(el['obj_batch'], est, gt)
        for k, n in enumerate(group):
            want["add_" + n], want["adds_" + n] = s['add'][:, k], s['adds'][:, k]
        if bop is not None:
            v = bop_score.vsd(bop['meshes'], cls_host, est, gt, el['frame_depth'], el['frame_intrinsics'], np.arange(B),
                              bop['diameters'].index_select(0, cls))
            d = bop_score.mssd_mspd(el['obj_batch'], est, gt, el['frame_intrinsics'],
                                    [bop['symmetries'].get(int(c)) for c in cls_host])
            for k, n in enumerate(group):
                want["vsd_" + n], want["mssd_" + n], want["mspd_" + n] = v['errors'][:, k], d['mssd'][:, k], d['mspd'][:, k]
    return want


def test_every_pose_set_is_scored_alike(hip, dev, records):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    el, graph, table, verify, bop = records['el'], records['graph'], records['table'], records['verify'], records['bop']
    out = E.evaluate_batch(graph, el, icp=True, score=True, symmetries=table, verify=verify, bop=bop)
    assert set(out) == _keys(icp=True, score=True, symmetries=True, verify=True, bop=True), sorted(set(out))
    want = _by_hand(el, out, ("pred", "icp", "ver"), table, bop)
    assert set(want) == set(out) - BASE - set(ICP_NAMES.values()) - VERIFY
    for k, v in want.items():
        _same(out[k], v, k)
    B = len(el['class_id'])
    assert tuple(out['vsd_ver'].shape)[0] == B and tuple(out['add_ver'].shape) == (B,) and tuple(out['mspd_icp'].shape) == (B,)
    # the symmetry set is more than the identity: some error moved
    assert any(not torch.equal(out['axag_loss_perSample%s_sym' % TAG[n]], out['axag_loss_perSample' + TAG[n]])
               for n in ("pred", "icp", "ver"))
    # the smaller combinations: their keys, and their bits are those of the full call
    for kw in (dict(), dict(icp=True), dict(score=True), dict(icp=True, score=True, symmetries=table)):
        got = E.evaluate_batch(graph, el, **kw)
        assert set(got) == _keys(**{k: True for k in kw}), (sorted(kw), sorted(set(got)))
        hand = _by_hand(el, got, ("pred", "icp") if "icp" in kw else ("pred",), kw.get("symmetries"), None)
        for k, v in got.items():
            if isinstance(v, torch.Tensor):
                _same(v, out[k], k)
                if k in hand:
                    _same(v, hand[k], k)


# ---- 4: the recorded pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icp", [True, PLANE], ids=["point_to_point", "point_to_plane"])
def test_the_recorded_pass_gives_the_same_bits(hip, dev, records, icp):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    graph, table = records['graph'], records['table']
    replayable = ("xyz_inlier", "visiblePoints_org", "class_id", "translation", "axisangle", "obj_batch")
    el, el2 = ({k: e[k] for k in replayable} for e in (records['el'], records['el2']))
    assert all(el[k].shape == el2[k].shape for k in el) and not torch.equal(el['xyz_inlier'], el2['xyz_inlier'])
    kw = dict(icp=icp, score=True, symmetries=table)
    want, want2 = E.evaluate_batch(graph, el, **kw), E.evaluate_batch(graph, el2, **kw)
    assert not torch.equal(want['trans_icp'], want2['trans_icp'])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                       # "evaluation pass not replayable"
        for e, w in ((el, want), (el2, want2), (el, want)):                  # records, replays, replays
            got = E.evaluate_batch(graph, e, replay=True, **kw)
            assert set(got) == set(w)
            for k, v in w.items():
                if isinstance(v, torch.Tensor):
                    _same(got[k], v, k)


# ---- 5: the command line --------------------------------------------------------------------------------------------------------------
def test_the_batch_line_prints_the_outputs_in_order(hip, dev, records, capsys):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import pose_equiv, pose_score, ppf
    from cloudaae_amd.utils import pose_verify as PV
    from cloudaae_amd.utils import symmetry as sym_util
    tmp, files, models, graph = records['tmp'], records['files'], records['models'], records['graph']
    capsys.readouterr()
    assert E.main(["--files", records['path'], "--object_model", records['obj'], "--trained_model", records['ckpt'],
                   "--target_cls", "0", "--num_point", str(N), "--batch_size", "1", "--verify", "--icp", "--score", "--bop",
                   "--symmetries", "auto", "--meshes", str(tmp / "meshes"), "--mesh_scale", "0.001", "--propose", "ppf",
                   "--propose_top", "2", "--propose_points", "128"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Validation batch ")]
    # what the command line builds from its arguments, through the public functions
    found = sym_util.symmetries_of_meshes([files[0]], scale=0.001, mesh_ids=[0])
    table = pose_equiv.SymmetryTable.from_results(found, len(models), [0], dev)
    packed = mm.pack_meshes(files, 0.001)
    bop = dict(meshes=packed, diameters=pose_score.model_diameter(torch.from_numpy(np.ascontiguousarray(models, np.float32)).cuda()),
               symmetries={0: found[0]["transforms"]})
    verify = dict(meshes=packed, hypotheses=PV.HypothesisTable.from_models(models[0:1], [0], len(models)), tau=0.01)
    propose = dict(models=ppf.PPFModels.from_meshes([files[0]], num_point=128, scale=0.001, classes=[0], num_class=len(models)),
                   top=2)
    el = E.element_from_frames(records['frames'], 0, N, models, seed=0, keep_frames=True, keep_labels=True)
    B = len(el['class_id'])
    assert len(lines) == B and B >= 1
    fields = ["trans_loss", "axag_loss", "trans_loss_icp", "axag_loss_icp", "trans_loss_ver", "axag_loss_ver", "trans_loss_sym",
              "axag_loss_sym", "trans_loss_icp_sym", "axag_loss_icp_sym", "trans_loss_ver_sym", "axag_loss_ver_sym"]
    for b, line in enumerate(lines):
        el_b = {k: v[b:b + 1] for k, v in el.items() if isinstance(v, torch.Tensor)}
        out = E.evaluate_batch(graph, el_b, icp=True, score=True, bop=bop, symmetries=table, verify=verify, propose=propose)
        want = ["Validation", "batch", "%d" % b, "seq_id", "%d" % int(el['seq_id'][b]), "frame_id", "%d" % int(el['frame_id'][b])]
        for k in fields:
            want += [k.replace("axag", "rot"), "%f" % float(out[k])]
        assert line.split() == want and line == " ".join(want), (b, line)
