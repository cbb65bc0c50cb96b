"""Training clouds from rendered, sensor-noised depth frames: the renderer (render.py) and the sensor model
(depth_noise.py) as a training input.  cloudaae_rendered_scene (csrc/pose_sample.hip) assembles two frames per sample on
the device -- the target alone, and the target behind an object occluder --, cloudaae_render_frames draws them,
depth_noise.apply gives them a depth sensor's noise, and cloudaae_frame_clouds (csrc/frame_clouds.hip) turns the labelled
pixels into the fixed-size clouds TrainGraph.forward takes.  Nothing is read back; a sample is a function of (seed, its
global index), whatever the batch split.  The definition is in DESIGN.md ("Rendered training clouds").  The reference
approximates visibility by hidden point removal on 2048-point models; nothing here is matched to it.

    rec = sample_pose_in_frustum.sample_poses(B, seed, g0, num_models=len(files))
    el = rendered_element(rec, mesh_models.pack_meshes(files), None, 1024, seed, g0, sensor='kinect1')
    out = graph.train_step(el)
"""
import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from . import render as render_mod
from .sample_pose_in_frustum import camera_parameters, class_list, get_frustum

MAX_INDEX = 1 << 39
MIN_VISIBLE = 64                 # a choice: fewer target pixels behind the occluder and the input is the unoccluded view


def _frames(depth, label, intrinsics):
    from .depth_noise import _frames as frames
    return frames(depth, label, intrinsics)


def _ints(x, n, dtype, dev, what):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x).astype(
        np.int64 if dtype == torch.int64 else np.int32))
    require(t.dim() == 1 and int(t.shape[0]) == n, "%s must be [C]" % what)
    return t.to(device=dev, dtype=dtype).contiguous()


def frame_clouds(depth, label, intrinsics, frame_of, want, index, rows, seed, fallback=None):
    """cloudaae_frame_clouds: C clouds of `rows` points from the pixels of depth [F,H,W] (int16 tensor holding the uint16
    bits, or a uint16 array) whose label [F,H,W] uint8 equals want[c] and whose depth is not 0, in frame frame_of[c];
    index[c] is the cloud's global index for the draws (below 2^39), fallback [C,3] the point an empty mask gives
    (default zeros).  -> dict of device tensors: cloud [C,rows,3] float32, num_pixels [C] int32 (the mask's size n),
    num_distinct [C] int64 and row_src [C,rows] int32 (rows below num_distinct are distinct pixels, row j above is a copy
    of row row_src[j]: the form the prefix Chamfer search takes).  With n >= rows the rows are one pixel per stratum, in
    pixel order.  No read-back."""
    depth, label, intr = _frames(depth, label, intrinsics)
    F, H, W = (int(x) for x in depth.shape)
    dev = depth.device
    C = int(frame_of.shape[0]) if isinstance(frame_of, torch.Tensor) else len(frame_of)
    rows = int(rows)
    frame_of = _ints(frame_of, C, torch.int32, dev, "frame_of")
    want = _ints(want, C, torch.int32, dev, "want")
    index = _ints(index, C, torch.int64, dev, "index")
    if fallback is not None:
        if not isinstance(fallback, torch.Tensor):
            fallback = torch.from_numpy(np.ascontiguousarray(fallback, np.float32))
        require(tuple(fallback.shape) == (C, 3), "fallback must be [C, 3]")
        fallback = fallback.to(device=dev, dtype=torch.float32).contiguous()
    L = _lib.lib()
    nbytes = int(L.cloudaae_frame_clouds_workspace_bytes(F, H, W, C, rows))
    require(nbytes > 0, "outside the limits: C >= 1, H W <= 2^24, F H W <= 2^28, 1 <= rows <= 2^20, C rows below 2^31")
    cloud = _lib.empty((C, rows, 3), dtype=torch.float32, device=dev)
    num_pixels = _lib.empty((C,), dtype=torch.int32, device=dev)
    num_distinct = _lib.empty((C,), dtype=torch.int64, device=dev)
    row_src = _lib.empty((C, rows), dtype=torch.int32, device=dev)
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_frame_clouds(F, H, W, ptr(depth), ptr(label), ptr(intr), C, ptr(frame_of), ptr(want), ptr(index),
                                           ptr(fallback), rows, int(seed) % (1 << 64), ptr(cloud), ptr(num_pixels),
                                           ptr(num_distinct), ptr(row_src), ptr(ws), nbytes, stream()),
                   "cloudaae_frame_clouds")
    return dict(cloud=cloud, num_pixels=num_pixels, num_distinct=num_distinct, row_src=row_src)


def rendered_scene(records, packed_meshes, mesh_index, seed, first_index, dataset='ycbv', camera=None, classes=None,
                   return_centre=False):
    """cloudaae_rendered_scene: the device instance arrays of 2B frames (frame 2i: sample i's target alone, label 1;
    frame 2i+1: the target and an object occluder, label 2) with bases strided by the largest mesh, as
    render.render_instances_strided takes them.  records: class_id [B], translation [B,3], rot_mat64 [B,3,3] on the
    device; mesh_index [num_classes] int32 (class -> mesh of packed_meshes; None: the identity); the occluder of sample i
    is get_random_object_occluder's for (seed, first_index + i), drawn among `classes` (default: every class).
    -> dict: inst_offsets, inst_mesh, inst_label, inst_pose, vert_base, tri_base, occluder_class [B] int64 and, with
    return_centre, occluder_centre [B,3] float32."""
    p = packed_meshes
    dev = p.device
    S = len(p.num_triangles)
    if mesh_index is None:
        mesh_index = torch.arange(S, dtype=torch.int32, device=dev)
    elif not isinstance(mesh_index, torch.Tensor):
        mesh_index = torch.from_numpy(np.ascontiguousarray(mesh_index).astype(np.int32))
    mesh_index = mesh_index.to(device=dev, dtype=torch.int32).contiguous()
    nmodels = int(mesh_index.shape[0])
    require(mesh_index.dim() == 1 and nmodels >= 1, "mesh_index must be [num_classes]")
    cam = camera_parameters(dataset, camera)
    _, Hnear, Wnear, _, _ = get_frustum(cam['vertical_fov'], cam['nearDist'], cam['farDist'], cam['ratio'])
    cls = records['class_id'].to(device=dev, dtype=torch.int64).contiguous()
    t = records['translation'].to(device=dev, dtype=torch.float32).contiguous()
    rot = records['rot_mat64'].to(device=dev, dtype=torch.float64).contiguous()
    B = int(cls.shape[0])
    require(tuple(t.shape) == (B, 3) and rot.numel() == 9 * B, "translation must be [B, 3] and rot_mat64 [B, 3, 3]")
    maxv, maxt = int(np.max(p.num_vertices)), int(np.max(p.num_triangles))
    n, ids = class_list(classes)
    ints = _lib.empty((2 * B + 1 + 6 * B + 2 * (3 * B + 1),), dtype=torch.int32, device=dev)
    o = np.cumsum([0, 2 * B + 1, 3 * B, 3 * B, 3 * B + 1, 3 * B + 1])
    inst_offsets, inst_mesh, inst_label, vert_base, tri_base = (ints[o[k]:o[k + 1]] for k in range(5))
    pose = _lib.empty((3 * B, 16), dtype=torch.float64, device=dev)
    occ_cls = _lib.empty((B,), dtype=torch.int64, device=dev)
    centre = _lib.empty((B, 3), dtype=torch.float32, device=dev) if return_centre else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_rendered_scene(B, int(first_index), int(seed) % (1 << 64), nmodels, n, ids, ptr(cls),
                                                      ptr(mesh_index), ptr(rot), ptr(t), float(Wnear), float(Hnear),
                                                      float(cam['nearDist']), maxv, maxt, inst_offsets.data_ptr(),
                                                      inst_mesh.data_ptr(), inst_label.data_ptr(), ptr(pose),
                                                      vert_base.data_ptr(), tri_base.data_ptr(), ptr(occ_cls), ptr(centre),
                                                      stream()), "cloudaae_rendered_scene")
    out = dict(inst_offsets=inst_offsets, inst_mesh=inst_mesh, inst_label=inst_label, inst_pose=pose, vert_base=vert_base,
               tri_base=tri_base, occluder_class=occ_cls)
    if return_centre:
        out['occluder_centre'] = centre
    return out


def frame_intrinsics(frames, height, width, dataset='ycbv', camera=None, device=None):
    """[frames,5] float32 on the device: the camera's fx, fy, cx, cy scaled to a height x width image (the same view at
    another resolution) and render.FACTOR_DEPTH."""
    cam = camera_parameters(dataset, camera)
    sx, sy = int(width) / cam['width'], int(height) / cam['height']
    row = np.array([cam['fx'] * sx, cam['fy'] * sy, cam['cx'] * sx, cam['cy'] * sy, render_mod.FACTOR_DEPTH], np.float32)
    return torch.from_numpy(np.tile(row, (int(frames), 1))).to(device)


def rendered_element(records, packed_meshes, mesh_index, num_point, seed, first_index, dataset='ycbv', camera=None,
                     height=None, width=None, sensor=None, min_visible=MIN_VISIBLE, sensor_seed=None, scene=None,
                     return_frames=False):
    """The element of one training batch from rendered frames: what get_small_data returns, as far as TrainGraph.forward
    reads it.  records: the dict of sample_pose_in_frustum.sample_poses (class_id, translation, axisangle, rot_mat64) for
    global samples first_index .. first_index + B - 1; packed_meshes: mesh_models.pack_meshes' result; mesh_index: class
    -> mesh (None: the identity); height, width: the image (default: the camera's; the intrinsics scale with them);
    scene: the result of rendered_scene to draw instead of assembling one (a caller that edits the instances, e.g.
    places an occluder).  sensor: None, a preset's name or a parameter dict of depth_noise.sensor_params; frame 2g is
    sample g alone and 2g+1 sample g occluded, their global frame indices under sensor_seed (default: seed).
      visiblePoints [B,N,3]        label 1 of the occluded frame, the sensor's depth when there is one -- or of the alone
                                   frame where the occluder leaves fewer than min_visible target pixels (occluded_out [B]
                                   bool says where; a device-side choice, no read-back)
      visiblePoints_org [B,4N,3]   label 1 of the clean, alone frame, with num_vis_point_org [B] int64 and
                                   visiblePoints_org_src [B,4N] int32; an empty view gives the translation
      num_vis_point [B] int32      the target pixels behind visiblePoints
      class_id, translation, axisangle, rot_mat64, rot_mat, occluder_class
    The clouds of global sample g draw under the indices 4g (input, alone), 4g+1 (input, occluded) and 4g+2 (target)."""
    from . import depth_noise
    p = packed_meshes
    dev = p.device
    N = int(num_point)
    g0 = int(first_index)
    cam = camera_parameters(dataset, camera)
    H = int(height) if height else int(cam['height'])
    W = int(width) if width else int(cam['width'])
    if scene is None:
        scene = rendered_scene(records, p, mesh_index, seed, g0, dataset=dataset, camera=camera)
    B = int(scene['occluder_class'].shape[0])
    require(g0 >= 0 and 4 * (g0 + B) <= MAX_INDEX, "global sample indices must lie below 2^37")
    intr = frame_intrinsics(2 * B, H, W, dataset, camera, dev)
    clean, clean_label, _, _ = render_mod.render_instances_strided(
        p, intr, scene['inst_offsets'], scene['inst_mesh'], scene['inst_label'], scene['inst_pose'], scene['vert_base'],
        scene['tri_base'], H, W)
    depth, label = clean, clean_label
    if sensor is not None and sensor != 'none':
        noisy = depth_noise.apply(clean, clean_label, intr, sensor, seed=seed if sensor_seed is None else sensor_seed,
                                  first_frame=2 * g0)
        depth, label = noisy['depth'], noisy['label']
    # host-made descriptions of the clouds (functions of B and g0 alone)
    i = np.arange(B, dtype=np.int64)
    frame_in = np.concatenate([2 * i + 1, 2 * i]).astype(np.int32)
    index_in = np.concatenate([4 * (g0 + i) + 1, 4 * (g0 + i)])
    desc = torch.from_numpy(np.concatenate([frame_in.astype(np.int64), index_in, 2 * i, 4 * (g0 + i) + 2])).to(dev)
    t = records['translation'].to(device=dev, dtype=torch.float32).contiguous()
    ones = torch.ones((2 * B,), dtype=torch.int32, device=dev)
    seen = frame_clouds(depth, label, intr, desc[:2 * B].to(torch.int32), ones, desc[2 * B:4 * B], N, seed,
                        fallback=torch.cat([t, t], dim=0))
    org = frame_clouds(clean, clean_label, intr, desc[4 * B:5 * B].to(torch.int32), ones[:B], desc[5 * B:], 4 * N, seed,
                       fallback=t)
    n_occ, n_alone = seen['num_pixels'][:B], seen['num_pixels'][B:]
    occluded_out = n_occ < int(min_visible)
    visible = torch.where(occluded_out[:, None, None], seen['cloud'][B:], seen['cloud'][:B])
    out = dict(records)
    out.update(visiblePoints=visible, visiblePoints_org=org['cloud'], num_vis_point_org=org['num_distinct'],
               visiblePoints_org_src=org['row_src'], num_vis_point=torch.where(occluded_out, n_alone, n_occ),
               occluded_out=occluded_out, occluder_class=scene['occluder_class'], translation=t,
               axisangle=records['axisangle'].to(device=dev, dtype=torch.float64),
               rot_mat=records['rot_gen_mat'] if records.get('rot_gen_mat') is not None
               else records['rot_mat64'].to(torch.float32),
               num_pixels_occluded=n_occ, num_pixels_alone=n_alone, num_pixels_org=org['num_pixels'])
    if return_frames:
        out.update(frames=dict(depth=depth, label=label, clean_depth=clean, clean_label=clean_label, intrinsics=intr),
                   scene=scene, input_clouds=seen)
    return out
