"""Fused models: a triangle mesh of an object that has no CAD model, from posed depth views of it.  The views are summed
into a truncated signed distance volume in the object's frame (cloudaae_tsdf_integrate; csrc/tsdf.hip), the volume is cut into
triangles by marching tetrahedra on the voxel centres (cloudaae_tsdf_count / cloudaae_tsdf_emit) and the triangles' vertices
are welded by their edge keys.  The mesh is what mesh_models.pack_meshes, render.render_frames, models_from_meshes and
symmetry.find_symmetries take.  The poses are the caller's: a record's, a turntable's, track_objects'.  The definition is in
DESIGN.md ("Fused models").

    vol = volume_for(aabb, 0.002)                                  # or Volume(origin, voxel, (nx, ny, nz))
    integrate(vol, depth, intrinsics, poses)                        # any number of calls, any order of the frames
    vertices, triangles = extract_mesh(vol)                         # float32 [V,3], int32 [T,3] on the device
    vertices, triangles, vol = fuse_frames(depth, label, intrinsics, poses, want, 0.002)
    mesh_models.write_ply("model.ply", vertices, triangles)

    python -m cloudaae_amd.utils.fuse --files REC_pcnn.tfrecord --target_cls C --voxel 0.002 --out model.ply [--every N]
        [--simplify METRES]
"""
import argparse

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from . import render
from .frame_inputs import depth_frames, host, on_device, record_intrinsics

# choices, not measurements on data
FRONT_VOXELS = 4.0        # the truncation in front of a surface, and the deep band's far end behind it
BEHIND_VOXELS = 1.5       # the near band's far end behind a surface
MARGIN = 4                # voxels around the box of volume_for

MAX_DIM = 512
MAX_VOXELS = 1 << 27
MAX_FRAMES = 1 << 19      # per call; per voxel over all calls the int32 sums hold 2^19 votes


class Volume(object):
    """nx x ny x nz voxels of side `voxel` (metres) in the object's frame, the low corner of voxel (0, 0, 0) at `origin`; the
    centre of voxel (i, j, k) is origin + (i + 0.5, j + 0.5, k + 0.5) voxel.  state [nz,ny,nx,4] int32 on the device: (acc,
    cnt, acc_deep, cnt_deep), zeros to begin with."""

    def __init__(self, origin, voxel, dims, device=None):
        self.origin = tuple(float(o) for o in np.asarray(origin, np.float64).reshape(3))
        self.voxel = float(voxel)
        self.dims = tuple(int(n) for n in dims)
        require(len(self.dims) == 3 and all(2 <= n <= MAX_DIM for n in self.dims) and
                self.dims[0] * self.dims[1] * self.dims[2] <= MAX_VOXELS,
                "dims must be (nx, ny, nz), each in [2, 512], with nx ny nz <= 2^27")
        require(all(np.isfinite(self.origin)) and np.isfinite(self.voxel) and self.voxel > 0.0,
                "the origin must be finite and the voxel finite and positive")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        nx, ny, nz = self.dims
        self.state = torch.zeros((nz, ny, nx, 4), dtype=torch.int32, device=self.device)


def volume_for(aabb, voxel, margin=MARGIN, device=None):
    """The Volume around a box aabb [2,3] (low and high corner, metres) with `margin` voxels on every side."""
    box = host(aabb, np.float64)
    require(box.shape == (2, 3) and np.all(np.isfinite(box)) and np.all(box[1] >= box[0]), "aabb must be a finite [2, 3] box, low <= high")
    s, margin = float(voxel), int(margin)
    require(np.isfinite(s) and s > 0.0 and margin >= 0, "voxel must be positive and margin >= 0")
    cells = np.ceil((box[1] - box[0]) / s)
    require(np.all(cells + 2 * margin <= MAX_DIM), "the box needs more than 512 voxels along an axis: choose a larger voxel")
    dims = tuple(int(max(n, 2)) for n in cells.astype(np.int64) + 2 * margin)
    return Volume(box[0] - margin * s, s, dims, device)


def _frames(dev, depth, intrinsics, poses, label, want):
    """The frames of a call as contiguous tensors on `dev`, shapes checked: (depth, intr, poses, label or None, want or None)."""
    dt = depth_frames(depth, dev)
    require(dt.device == dev, "the frames must be on the volume's device")
    F = int(dt.shape[0])
    require(1 <= F <= MAX_FRAMES, "1 <= F <= 2^19 frames per call")
    intr = on_device(intrinsics, torch.float32, dev, (F, 5), "intrinsics")
    pose = on_device(poses, torch.float64, dev, (F, 4, 4), "poses")
    require((label is None) == (want is None), "label and want come together")
    lab = wnt = None
    if label is not None:
        require(isinstance(label, np.ndarray) or label.dtype == torch.uint8, "label must be uint8")
        lab = on_device(label, torch.uint8, dev, tuple(dt.shape), "label")
        wnt = on_device(np.asarray(want, np.int64).astype(np.int32) if not isinstance(want, torch.Tensor) else want, torch.int32, dev,
                        (F,), "want")
    return dt, intr, pose, lab, wnt


def integrate(volume, depth, intrinsics, poses, label=None, want=None, front=None, behind=None, z_near=render.Z_NEAR):
    """cloudaae_tsdf_integrate: adds F frames to volume.state.  depth [F,H,W] uint16 (numpy, or a device tensor holding the
    bits as int16); intrinsics [F,5] float32 (fx, fy, cx, cy, factor_depth); poses [F,4,4] float64, model -> camera; label
    [F,H,W] uint8 with want [F]: a pixel of frame f is used when want[f] == 0 or label == want[f] (neither given: every pixel
    with a depth).  front (default 4 voxels) and behind (default 1.5 voxels) in metres, front > behind > 0.  The sums are
    integers: any split of the frames over calls and any order gives the same state bit for bit; a voxel holds 2^19 votes,
    beyond that the int32 sums wrap -- the caller's concern.  No read-back.  -> volume."""
    require(isinstance(volume, Volume), "volume must be a Volume")
    dt, intr, pose, lab, wnt = _frames(volume.device, depth, intrinsics, poses, label, want)
    F, H, W = (int(v) for v in dt.shape)
    front = FRONT_VOXELS * volume.voxel if front is None else float(front)
    behind = BEHIND_VOXELS * volume.voxel if behind is None else float(behind)
    nx, ny, nz = volume.dims
    ox, oy, oz = volume.origin
    with torch.cuda.device(volume.device):
        _lib.check(_lib.lib().cloudaae_tsdf_integrate(nx, ny, nz, ox, oy, oz, volume.voxel, ptr(volume.state), F, H, W, ptr(dt),
                                                      ptr(lab), ptr(wnt), ptr(intr), ptr(pose), front, behind, float(z_near),
                                                      stream()), "cloudaae_tsdf_integrate")
    return volume


def extract_triangles(volume, min_count=1):
    """cloudaae_tsdf_count, torch.cumsum, cloudaae_tsdf_emit.  -> (tri_pos [T,3,3] float64, tri_key [T,3] int64, tri_count
    [cells] uint8) on the device, triangles in the order cell, tetrahedron, triangle.  One read-back: T."""
    require(isinstance(volume, Volume), "volume must be a Volume")
    require(int(min_count) >= 1, "min_count must be >= 1")
    nx, ny, nz = volume.dims
    ox, oy, oz = volume.origin
    dev = volume.device
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    L = _lib.lib()
    count = _lib.empty((cells,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.cloudaae_tsdf_count(nx, ny, nz, ptr(volume.state), int(min_count), ptr(count), stream()), "cloudaae_tsdf_count")
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(ends[-1])
        offset = (ends - count).contiguous()
        pos = _lib.empty((total, 3, 3), dtype=torch.float64, device=dev)
        key = _lib.empty((total, 3), dtype=torch.int64, device=dev)
        if total:
            _lib.check(L.cloudaae_tsdf_emit(nx, ny, nz, ox, oy, oz, volume.voxel, ptr(volume.state), int(min_count), ptr(offset),
                                            total, ptr(pos), ptr(key), stream()), "cloudaae_tsdf_emit")
    return pos, key, count


def weld(tri_pos, tri_key):
    """Triangles with one position and one key per corner -> (vertices [V,3] float32 in ascending key order, triangles [T,3]
    int32 in the given order).  Every occurrence of a key carries the same position bits, so any one of them is taken."""
    T = int(tri_key.shape[0])
    dev = tri_key.device
    if T == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    keys, inverse = torch.unique(tri_key.reshape(-1), sorted=True, return_inverse=True)
    first = torch.zeros((int(keys.numel()),), dtype=torch.int64, device=dev)
    first.scatter_(0, inverse, torch.arange(3 * T, dtype=torch.int64, device=dev))
    return tri_pos.reshape(-1, 3)[first].to(torch.float32), inverse.reshape(T, 3).to(torch.int32)


def extract_mesh(volume, min_count=1, simplify=None):
    """-> (vertices [V,3] float32, triangles [T,3] int32) on the device: what mesh_models.pack_meshes takes as a mesh.  An
    empty surface gives two empty tensors.  Surfaces no view saw stay open; zero-area triangles (a vertex exactly on a voxel
    centre) are kept.  simplify: a cell side in metres -- the mesh goes through simplify.simplify_mesh with its defaults
    ("Simplified meshes"); None: the mesh as cut."""
    pos, key, _ = extract_triangles(volume, min_count)
    vertices, triangles = weld(pos, key)
    if simplify is not None:
        from .simplify import simplify_mesh
        vertices, triangles = simplify_mesh(vertices, triangles, simplify)
    return vertices, triangles


def used_points_aabb(depth, label, intrinsics, poses, want):
    """The box of the used pixels back-projected into the object's frame, in torch on the frames' device: p_cam = ((u - cx) dm
    / fx, (v - cy) dm / fy, dm), dm = d / factor_depth; p_obj = R^T (p_cam - t).  -> [2,3] float64 (host; one read-back)."""
    F, H, W = (int(v) for v in depth.shape)
    dev = depth.device
    d = (depth.to(torch.int32) & 0xFFFF).to(torch.float64)
    used = d != 0
    if label is not None:
        w = want.view(F, 1, 1)
        used &= (w == 0) | (label.to(torch.int32) == w)
    k = intrinsics.to(torch.float64)
    dm = d / k[:, 4].view(F, 1, 1)
    u = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    v = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    cam = torch.stack([(u - k[:, 2].view(F, 1, 1)) * dm / k[:, 0].view(F, 1, 1), (v - k[:, 3].view(F, 1, 1)) * dm / k[:, 1].view(F, 1, 1),
                       dm], dim=-1)                                                   # [F,H,W,3]
    R, t = poses[:, :3, :3], poses[:, :3, 3]
    obj = torch.einsum('fij,fhwi->fhwj', R, cam - t.view(F, 1, 1, 3))
    big = torch.full_like(obj, float('inf'))
    m = used.unsqueeze(-1)
    box = torch.stack([torch.where(m, obj, big).amin(dim=(0, 1, 2)), torch.where(m, obj, -big).amax(dim=(0, 1, 2))]).cpu().numpy()
    require(np.all(np.isfinite(box)), "no pixel of the frames is used: nothing to fuse")
    return box


def fuse_frames(depth, label, intrinsics, poses, want, voxel, aabb=None, min_count=1, front=None, behind=None, z_near=render.Z_NEAR,
                simplify=None):
    """One object from F posed frames: the volume around `aabb` (default: the box of the used pixels back-projected into the
    object's frame, one read-back), all frames integrated, the mesh extracted (simplify: as in extract_mesh).  label and want
    may both be None.  -> (vertices [V,3] float32, triangles [T,3] int32, volume)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if not isinstance(depth, torch.Tensor) else depth.device
    dt, intr, pose, lab, wnt = _frames(dev, depth, intrinsics, poses, label, want)
    if aabb is None:
        aabb = used_points_aabb(dt, lab, intr, pose, wnt)
    volume = volume_for(aabb, voxel, device=dev)
    integrate(volume, dt, intr, pose, lab, wnt, front=front, behind=behind, z_near=z_near)
    vertices, triangles = extract_mesh(volume, min_count, simplify)
    return vertices, triangles, volume


def mesh_counts(vertices, triangles):
    """(vertices, triangles, boundary edges: used by one triangle only, connected components) of a welded mesh, on the host."""
    t = np.asarray(triangles.cpu() if isinstance(triangles, torch.Tensor) else triangles, np.int64).reshape(-1, 3)
    V = int(vertices.shape[0])
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    _, cnt = np.unique(np.minimum(e[:, 0], e[:, 1]) * max(V, 1) + np.maximum(e[:, 0], e[:, 1]), return_counts=True)
    comp = np.arange(V)
    while len(e):
        low = np.minimum(comp[e[:, 0]], comp[e[:, 1]])
        new = comp.copy()
        np.minimum.at(new, e[:, 0], low)
        np.minimum.at(new, e[:, 1], low)
        new = new[new]
        if np.array_equal(new, comp):
            break
        comp = new
    used = np.unique(t)
    return V, len(t), int((cnt == 1).sum()), len(np.unique(comp[used])) if len(used) else 0


def class_frames(path, target_cls, every=1):
    """One class of a <seq>_pcnn.tfrecord: every `every`-th frame of the file that shows the class, in file order -> (depth
    [F,H,W] uint16, label [F,H,W] uint8, intrinsics [F,5] float32, the record's poses of the class [F,4,4] float64, the
    frames' records)."""
    from .. import tfrecord_io
    from .track import record_poses
    require(every >= 1, "--every must be >= 1")
    frames = [fr for fr in list(tfrecord_io.read_frames(path))[::every] if bool(fr["class_one_hot"][target_cls])]
    require(len(frames) >= 1, "no frame of %s shows class %d" % (path, target_cls))
    depth = np.stack([fr["depth"] for fr in frames])
    label = np.stack([fr["label"] for fr in frames]).astype(np.uint8)
    poses = np.concatenate([record_poses(fr, [target_cls]) for fr in frames])
    return depth, label, record_intrinsics(frames), poses, frames


def main(argv=None):
    parser = argparse.ArgumentParser(description="fuse one class of a <seq>_pcnn.tfrecord into a mesh from the record's labels and poses")
    parser.add_argument("--files", required=True, help="one <seq>_pcnn.tfrecord; its frames are taken in file order")
    parser.add_argument("--target_cls", type=int, required=True, help="the class to fuse (its label in the frames is class + 1)")
    parser.add_argument("--voxel", type=float, default=0.002, help="voxel side in metres")
    parser.add_argument("--out", required=True, help="the PLY file to write")
    parser.add_argument("--every", type=int, default=1, help="take every N-th frame")
    parser.add_argument("--simplify", type=float, default=None, metavar="METRES", help="simplify the mesh on cells of this side")
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    from . import mesh_models
    torch.cuda.set_device(args.gpu)
    c = args.target_cls
    depth, label, intr, poses, frames = class_frames(args.files, c, args.every)
    vertices, triangles, volume = fuse_frames(depth, label, intr, poses, np.full(len(frames), c + 1, np.int32), args.voxel,
                                              simplify=args.simplify)
    mesh_models.write_ply(args.out, vertices, triangles)
    print("%d frames into %d x %d x %d voxels of %g m" % ((len(frames),) + volume.dims + (volume.voxel,)))
    print("%d vertices, %d triangles, %d boundary edges, %d components written to %s" % (mesh_counts(vertices, triangles) + (args.out,)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
