"""Depth and label frames of posed triangle meshes: the RGB-D side of a scene, rendered on the GPU by
cloudaae_render_frames (csrc/render.hip) -- a z-buffer rasteriser whose outputs are the `depth` uint16 and `label` uint8
images that segment.extract_segments takes, and, written as frame records, the <seq>_pcnn.tfrecord files that
evaluate_cloudAAE_ycbv reads.  The definition is in DESIGN.md ("Rendered frames").  The reference has no renderer (it
approximates visibility on 2048-point models by hidden point removal); nothing here is matched to it.

    out = render_frames(meshes, [[(0, 1, pose_a), (1, 2, pose_b)], ...], intrinsics, 480, 640)
    r = segment.extract_segments(out['depth'], out['label'], intrinsics, classes=[[0, 1], ...])      # no host copy
    tfrecord_io.write_records(path, frame_records(out['depth'], out['label'], intrinsics, poses, classes, 48, ids))

    python -m cloudaae_amd.utils.render --meshes DIR --out DIR --frames N --objects K --seq ID --seed S [--mesh_scale X]
                                        [--sensor kinect1 --sensor_seed S]
"""
import argparse
import os

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from . import mesh_models

Z_NEAR = 0.05
FACTOR_DEPTH = 10000.0           # YCB-Video's depth unit: 0.1 mm
NUM_CLASS = 21                   # classes of a frame record (tfrecord_io.decode_frame)
DEFAULT_SEED = 123456789


def _host(x, dtype):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype)


def _poses(flat, device):
    """The instances' poses -> [J,16] float64 on the device.  A pose is a 4x4 array / tensor or a (rot, trans) pair: an
    axis-angle and a translation, which go through pose_score.pose_matrix (cloudaae_pose_matrix) in one launch."""
    from . import pose_score
    J = len(flat)
    host = np.zeros((J, 4, 4), np.float64)
    pairs = []
    for j, (_, _, pose) in enumerate(flat):
        if isinstance(pose, (tuple, list)) and len(pose) == 2:
            pairs.append(j)
        else:
            m = _host(pose, np.float64)
            require(m.shape == (4, 4), "a pose must be a 4x4 matrix or a (rot, trans) pair")
            host[j] = m
    out = torch.from_numpy(host).to(device)
    if pairs:
        rot = torch.from_numpy(np.stack([_host(flat[j][2][0], np.float64).reshape(3) for j in pairs])).to(device)
        trans = torch.from_numpy(np.stack([_host(flat[j][2][1], np.float32).reshape(3) for j in pairs])).to(device)
        out[torch.tensor(pairs, device=device)] = pose_score.pose_matrix(rot, trans)
    return out.view(J, 16)


def render_instances(p, intr, offs, mesh, lab, poses, H, W, z_near=Z_NEAR, return_tri=False):
    """The launch behind render_frames, for callers whose poses are already on the device (bop_score.vsd): p a
    PackedMeshes, intr [F,5] float32 on its device, offs [F+1], mesh, lab [J] host integers (checked by the caller),
    poses [J,16] float64 on the device.  -> (depth [F,H,W] int16, label uint8, tri int32 or None, counts [2,J] int32:
    dropped and degenerate, all on the device; tri_base [J+1] numpy).  No read-back."""
    dev = p.device
    F, J, S = len(offs) - 1, len(mesh), len(p.num_triangles)
    vb = np.concatenate([[0], np.cumsum(np.asarray(p.num_vertices, np.int64)[mesh])])
    tb = np.concatenate([[0], np.cumsum(np.asarray(p.num_triangles, np.int64)[mesh])])
    L = _lib.lib()
    nbytes = int(L.cloudaae_render_workspace_bytes(F, H, W, J, int(vb[-1]), int(tb[-1])))
    require(nbytes > 0, "outside the renderer's limits: H W <= 2^24, F H W <= 2^28, fewer than 2^31 triangles drawn")
    ints = torch.from_numpy(np.concatenate([offs, mesh, lab, vb, tb]).astype(np.int32)).to(dev)
    inst_offsets, inst_mesh, inst_label = ints[:F + 1], ints[F + 1:F + 1 + J], ints[F + 1 + J:F + 1 + 2 * J]
    vert_base, tri_base = ints[F + 1 + 2 * J:F + 2 + 3 * J], ints[F + 2 + 3 * J:]
    depth = _lib.empty((F, H, W), dtype=torch.int16, device=dev)
    label = _lib.empty((F, H, W), dtype=torch.uint8, device=dev)
    tri = _lib.empty((F, H, W), dtype=torch.int32, device=dev) if return_tri else None
    counts = _lib.empty((2, J), dtype=torch.int32, device=dev)
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_render_frames(S, ptr(p.vert_offsets), ptr(p.tri_offsets), int(p.vertices.shape[0]),
                                            int(p.triangles.shape[0]), ptr(p.vertices), ptr(p.triangles), F, H, W, ptr(intr),
                                            inst_offsets.data_ptr(), J, inst_mesh.data_ptr(), inst_label.data_ptr(),
                                            ptr(poses), vert_base.data_ptr(), tri_base.data_ptr(), int(vb[-1]), int(tb[-1]),
                                            float(z_near), depth.data_ptr(), label.data_ptr(), ptr(tri),
                                            counts[0].data_ptr(), counts[1].data_ptr(), ptr(ws), nbytes, stream()),
                   "cloudaae_render_frames")
    return depth, label, tri, counts, tb


def render_instances_strided(p, intr, inst_offsets, inst_mesh, inst_label, poses, vert_base, tri_base, H, W, z_near=Z_NEAR,
                             return_tri=False):
    """render_instances for instance arrays that live on the device (cloudaae_rendered_scene writes them): inst_offsets
    [F+1], inst_mesh, inst_label [J], vert_base, tri_base [J+1] int32 and poses [J,16] float64 device tensors, the bases
    strided by the largest mesh of p -- vert_base[j] = j maxV, tri_base[j] = j maxT -- because the host does not know
    which mesh an instance draws.  Ranks past a mesh's own counts are no triangle / an unusable vertex to the renderer.
    -> (depth [F,H,W] int16, label uint8, tri int32 or None, counts [2,J] int32).  No read-back."""
    dev = p.device
    F, J, S = int(inst_offsets.shape[0]) - 1, int(inst_mesh.shape[0]), len(p.num_triangles)
    require(F >= 1 and J >= 1, "no frame or no instance to draw")
    require(tuple(intr.shape) == (F, 5) and tuple(poses.shape) == (J, 16), "intrinsics must be [F, 5] and poses [J, 16]")
    require(int(inst_label.shape[0]) == J and int(vert_base.shape[0]) == J + 1 and int(tri_base.shape[0]) == J + 1,
            "inst_label must be [J], vert_base and tri_base [J + 1]")
    require(all(t.dtype == torch.int32 for t in (inst_offsets, inst_mesh, inst_label, vert_base, tri_base)) and
            poses.dtype == torch.float64, "instance arrays must be int32 and poses float64")
    sum_v, sum_t = J * int(np.max(p.num_vertices)), J * int(np.max(p.num_triangles))
    L = _lib.lib()
    nbytes = int(L.cloudaae_render_workspace_bytes(F, H, W, J, sum_v, sum_t))
    require(nbytes > 0, "outside the renderer's limits: H W <= 2^24, F H W <= 2^28, fewer than 2^31 strided ranks")
    depth = _lib.empty((F, H, W), dtype=torch.int16, device=dev)
    label = _lib.empty((F, H, W), dtype=torch.uint8, device=dev)
    tri = _lib.empty((F, H, W), dtype=torch.int32, device=dev) if return_tri else None
    counts = _lib.empty((2, J), dtype=torch.int32, device=dev)
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_render_frames(S, ptr(p.vert_offsets), ptr(p.tri_offsets), int(p.vertices.shape[0]),
                                            int(p.triangles.shape[0]), ptr(p.vertices), ptr(p.triangles), F, H, W, ptr(intr),
                                            ptr(inst_offsets), J, ptr(inst_mesh), ptr(inst_label), ptr(poses),
                                            ptr(vert_base), ptr(tri_base), sum_v, sum_t, float(z_near), ptr(depth),
                                            ptr(label), ptr(tri), counts[0].data_ptr(), counts[1].data_ptr(), ptr(ws),
                                            nbytes, stream()),
                   "cloudaae_render_frames")
    return depth, label, tri, counts


def render_frames(meshes, instances, intrinsics, height, width, z_near=Z_NEAR, return_tri=False, scale=1.0, device=None,
                  sensor=None, sensor_seed=0, first_frame=0):
    """F frames of height x width.  meshes: a PackedMeshes or what mesh_models.pack_meshes takes (`scale` applies then).
    instances: per frame a list of (mesh index, label in 1..255, pose); a frame may be empty.  pose: model -> camera, a
    4x4 array or a (rot, trans) pair (axis-angle [3], translation [3]).  intrinsics [F,5] float32: fx, fy, cx, cy,
    factor_depth.  Returns a dict of device tensors depth [F,H,W] int16 (the uint16 bit pattern, the form
    extract_segments takes for a device depth; 0: nothing drawn), label [F,H,W] uint8 (0: background; the segment code
    reads class = label - 1) and, with return_tri, tri [F,H,W] int32 (the winning draw rank, -1 where empty), plus
    dropped, degenerate [J] int32 (numpy, one read-back: triangles left out because a vertex lay behind z_near or
    outside the guard band, or an index outside its mesh; triangles of zero screen area) and tri_base [J+1] (numpy: the
    draw rank of triangle t of instance j is tri_base[j] + t).  With `sensor` (a preset's name or the dict of
    depth_noise.sensor_params) the depth sensor model of depth_noise.apply follows the resolve: depth and label are the
    sensor's, clean_depth is the rendering, sensor_counts [F,4] int32 (device) its counts; frame f has the global index
    first_frame + f under sensor_seed."""
    p = mesh_models.pack_meshes(meshes, scale, device)
    dev = p.device
    F = len(instances)
    H, W = int(height), int(width)
    intr = intrinsics if isinstance(intrinsics, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(intrinsics, np.float32))
    intr = intr.to(device=dev, dtype=torch.float32).contiguous()
    require(F >= 1 and tuple(intr.shape) == (F, 5), "intrinsics must be [F, 5], one row per frame")
    flat = [tuple(inst) for fr in instances for inst in fr]
    J, S = len(flat), len(p.num_triangles)
    require(J >= 1, "no instance to draw")
    require(all(len(i) == 3 for i in flat), "an instance is (mesh index, label, pose)")
    mesh = np.array([int(i[0]) for i in flat], np.int64)
    lab = np.array([int(i[1]) for i in flat], np.int64)
    require(mesh.min() >= 0 and mesh.max() < S, "a mesh index outside the meshes")
    require(lab.min() >= 1 and lab.max() <= 255, "labels must lie in 1..255 (0 is the background)")
    require(float(z_near) > 0.0, "z_near must be positive")
    offs = np.cumsum([0] + [len(fr) for fr in instances])
    depth, label, tri, counts, tb = render_instances(p, intr, offs, mesh, lab, _poses(flat, dev), H, W, z_near, return_tri)
    host = counts.cpu().numpy()
    out = dict(depth=depth, label=label, dropped=host[0], degenerate=host[1], tri_base=tb)
    if return_tri:
        out['tri'] = tri
    if sensor is not None:
        from . import depth_noise
        noisy = depth_noise.apply(depth, label, intr, sensor, seed=sensor_seed, first_frame=first_frame)
        out.update(depth=noisy['depth'], label=noisy['label'], clean_depth=depth, sensor_counts=noisy['counts'])
    return out


def mat2quat(R):
    """A rotation matrix -> the unit quaternion (w, x, y, z) with w >= 0, float64: the branch with the largest
    denominator (Shepperd's method), so no case divides by a small number."""
    R = np.asarray(R, np.float64)
    require(R.shape == (3, 3), "a rotation matrix is 3 x 3")
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([1.0 + t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2 * R[0, 0] - t[0], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2 * R[1, 1] - t[0], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2 * R[2, 2] - t[0]])
    q = q / np.sqrt((q * q).sum())
    return -q if q[0] < 0 else q


def frame_records(depth, label, intrinsics, poses, classes, seq_id, frame_ids):
    """The frames as the records tfrecord_io.decode_frame reads (the schema of <seq>_pcnn.tfrecord): one payload per
    frame, for tfrecord_io.write_records.  depth [F,H,W] (uint16 array, or the int16 tensor of render_frames), label
    [F,H,W] uint8, intrinsics [F,5]; poses: per frame the 4x4 model -> camera poses of its objects; classes: per frame
    their 0-based classes (label - 1), each below 21 and named once per frame.  `image` is zeros [H,W,3]; quaternions
    [21,4] (w, x, y, z) and translations [21,3] hold the placed classes' poses and zeros elsewhere; class_one_hot is 1
    for every class placed in the frame."""
    from .. import tfrecord_io
    d = _host(depth, None)
    d = d.view(np.uint16) if d.dtype == np.int16 else d
    lab = _host(label, None)
    require(d.dtype == np.uint16 and lab.dtype == np.uint8, "depth must be uint16 (or its int16 bits) and label uint8")
    require(d.ndim == 3 and d.shape == lab.shape, "depth and label must be [F, H, W]")
    F, H, W = d.shape
    intr = _host(intrinsics, np.float32)
    require(intr.shape == (F, 5), "intrinsics must be [F, 5]")
    require(len(poses) == F and len(classes) == F and len(frame_ids) == F, "poses, classes and frame_ids: one entry per frame")
    image = bytes(H * W * 3)
    out = []
    for f in range(F):
        cls = [int(c) for c in classes[f]]
        require(len(poses[f]) == len(cls), "one pose per class of a frame")
        require(all(0 <= c < NUM_CLASS for c in cls), "classes must lie in [0, 21)")
        require(len(set(cls)) == len(cls), "a frame record holds one instance per class")
        quat, trans = np.zeros((NUM_CLASS, 4), np.float32), np.zeros((NUM_CLASS, 3), np.float32)
        one_hot = np.zeros(NUM_CLASS, np.int64)
        for c, pose in zip(cls, poses[f]):
            m = _host(pose, np.float64).reshape(4, 4)
            quat[c], trans[c], one_hot[c] = mat2quat(m[:3, :3]), m[:3, 3], 1
        out.append(tfrecord_io.encode_example({
            "image": image, "image_shape": np.array([H, W, 3], np.int64),
            "depth": np.ascontiguousarray(d[f]).astype("<u2").tobytes(), "depth_shape": np.array([H, W], np.int64),
            "label": np.ascontiguousarray(lab[f]).tobytes(), "label_shape": np.array([H, W], np.int64),
            "quaternions": quat.reshape(-1), "translations": trans.reshape(-1), "class_one_hot": one_hot,
            "seq_id": np.array([int(seq_id)], np.int64), "frame_id": np.array([int(frame_ids[f])], np.int64),
            "fx": intr[f, 0:1], "fy": intr[f, 1:2], "cx": intr[f, 2:3], "cy": intr[f, 3:4], "factor_depth": intr[f, 4:5]}))
    return out


def sample_scenes(num_frames, num_objects, num_classes, seed=DEFAULT_SEED, dataset='ycbv', device=None):
    """num_objects distinct classes per frame (a seeded numpy Generator) under poses of the existing sampler
    (sample_pose_in_frustum.sample_poses: pose i of the call is global sample i of `seed`).  -> (classes [F,K] numpy,
    poses [F,K,4,4] float64 numpy)."""
    from . import pose_score
    from . import sample_pose_in_frustum as spf
    F, K = int(num_frames), int(num_objects)
    require(F >= 1 and 1 <= K <= int(num_classes), "frames >= 1 and 1 <= objects <= the number of meshes")
    rng = np.random.default_rng(int(seed))
    classes = np.stack([np.sort(rng.permutation(int(num_classes))[:K]) for _ in range(F)])
    s = spf.sample_poses(F * K, seed, 0, dataset=dataset, device=device)
    poses = pose_score.pose_matrix(s['axisangle'], s['translation']).cpu().numpy().reshape(F, K, 4, 4)
    return classes, poses


def main(argv=None):
    parser = argparse.ArgumentParser(description="<seq>_pcnn.tfrecord frame records rendered from the *.ply meshes of a directory")
    parser.add_argument("--meshes", required=True, help="directory of *.ply files; class i is the i-th in sorted order")
    parser.add_argument("--out", required=True, help="directory to write <seq>_pcnn.tfrecord into")
    parser.add_argument("--frames", type=int, default=8)
    parser.add_argument("--objects", type=int, default=1, help="distinct classes drawn into every frame")
    parser.add_argument("--seq", type=int, default=48, help="sequence id: the file's name and every record's seq_id")
    parser.add_argument("--seed", type=int, default=DEFAULT_SEED)
    parser.add_argument("--mesh_scale", type=float, default=1.0, help="factor on the coordinates (0.001: millimetres to metres)")
    parser.add_argument("--width", type=int, default=None, help="image size [default: the camera's, 640 x 480]")
    parser.add_argument("--height", type=int, default=None)
    parser.add_argument("--frames_per_launch", type=int, default=8)
    parser.add_argument("--sensor", choices=["none", "kinect1"], default="none",
                        help="depth sensor model applied to the rendered frames (utils/depth_noise.py) [default: none]")
    parser.add_argument("--sensor_seed", type=int, default=0)
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    from .. import tfrecord_io
    from . import sample_pose_in_frustum as spf
    torch.cuda.set_device(args.gpu)
    files = mesh_models.mesh_files(args.meshes)
    require(len(files) <= NUM_CLASS, "a frame record holds at most 21 classes")
    packed = mesh_models.pack_meshes(files, args.mesh_scale)
    cam = spf.camera_parameters('ycbv')
    W = int(args.width) if args.width else int(cam['width'])
    H = int(args.height) if args.height else int(cam['height'])
    # another image size is the same view at another resolution: focal lengths and principal point scale with it
    sx, sy = W / cam['width'], H / cam['height']
    row = [cam['fx'] * sx, cam['fy'] * sy, cam['cx'] * sx, cam['cy'] * sy, FACTOR_DEPTH]
    classes, poses = sample_scenes(args.frames, args.objects, len(files), seed=args.seed)
    payloads, dropped = [], 0
    for lo in range(0, args.frames, max(args.frames_per_launch, 1)):
        hi = min(lo + max(args.frames_per_launch, 1), args.frames)
        intr = np.array([row] * (hi - lo), np.float32)
        inst = [[(int(c), int(c) + 1, poses[f, k]) for k, c in enumerate(classes[f])] for f in range(lo, hi)]
        sensor = dict(sensor=args.sensor, sensor_seed=args.sensor_seed, first_frame=lo) if args.sensor != "none" else {}
        out = render_frames(packed, inst, intr, H, W, **sensor)
        dropped += int(out['dropped'].sum())
        payloads += frame_records(out['depth'], out['label'], intr, poses[lo:hi], classes[lo:hi], args.seq,
                                  list(range(lo, hi)))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, str(args.seq).zfill(4) + "_pcnn.tfrecord")
    tfrecord_io.write_records(path, payloads)
    for i, f in enumerate(files):
        print("class %d: %s" % (i, os.path.basename(f)))
    print("%d frames of %d x %d with %d objects each written to %s (%d triangles dropped at the near plane or guard band)"
          % (args.frames, W, H, args.objects, path, dropped))
    return 0


if __name__ == "__main__":
    main()
