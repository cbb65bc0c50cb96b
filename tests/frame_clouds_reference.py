"""NumPy restatement of DESIGN.md, "Rendered training clouds": cloudaae_frame_clouds (mask, ranks, strata, the fill rule,
the fp32 back-projection of "Frame segments") and cloudaae_rendered_scene (the instance arrays of two frames per sample
with strided bases).  Written from the definition, with integer arithmetic for everything but the back-projection,
which is float32 operation by operation (NumPy rounds each correctly, as the device does without fma)."""
import numpy as np

from pose_sampling_reference import object_occluder, philox4x32, pick
from render_reference import render

STREAM_STRATUM, STREAM_REDRAW = 23, 24
MAX_INDEX = 1 << 39


def backproject(u, v, d, intr):
    """Pixels (u, v) of depth d (uint16) -> [n,3] float32: dm = float(d) / factor, x = ((u - cx) dm) / fx, y likewise."""
    fx, fy, cx, cy, factor = (np.float32(k) for k in np.asarray(intr, np.float32).reshape(5))
    dm = np.asarray(d).astype(np.float32) / factor
    x = ((np.asarray(u).astype(np.float32) - cx) * dm) / fx
    y = ((np.asarray(v).astype(np.float32) - cy) * dm) / fy
    return np.stack([x, y, dm], axis=-1).astype(np.float32)


def draws(seed, g, rows, stream):
    """q_j = word 0 of philox4x32(seed, g 2^24 + j, stream), j = 0 .. rows-1, as Python-int friendly uint64."""
    ctr = np.uint64(int(g) << 24) + np.arange(rows, dtype=np.uint64)
    return philox4x32(seed, ctr, stream)[:, 0].astype(np.uint64)


def strata(n, rows):
    """s_j = floor(j n / rows), j = 0 .. rows."""
    return (np.arange(rows + 1, dtype=np.int64) * int(n)) // int(rows)


def stratum_of(r, n, rows):
    """The hint: the stratum of rank r is floor(((r + 1) rows - 1) / n)."""
    return ((np.asarray(r, np.int64) + 1) * int(rows) - 1) // int(n)


def select(n, rows, seed, g):
    """-> (ranks [rows] of the masked pixels that become the rows, num_distinct, row_src [rows]); n >= 1."""
    n, rows = int(n), int(rows)
    j = np.arange(rows, dtype=np.int64)
    if n >= rows:
        s = strata(n, rows)
        q = draws(seed, g, rows, STREAM_STRATUM)
        ranks = s[:-1] + ((q * (s[1:] - s[:-1]).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        return ranks, rows, j.astype(np.int32)
    q = draws(seed, g, rows, STREAM_REDRAW)
    src = pick(q, n)
    row_src = np.where(j < n, j, src)
    return row_src.copy(), n, row_src.astype(np.int32)


def frame_cloud(depth, label, intr, want, g, rows, seed, fallback=None):
    """One cloud of one frame: depth [H,W] uint16, label [H,W] uint8.  -> (cloud [rows,3] float32, n, num_distinct,
    row_src [rows] int32)."""
    H, W = depth.shape
    fb = np.zeros(3, np.float32) if fallback is None else np.asarray(fallback, np.float32).reshape(3)
    mask = ((label.astype(np.int64) == int(want)) & (depth != 0)).reshape(-1)
    pix = np.flatnonzero(mask)                     # pixel order: their ranks are their positions here
    n = len(pix)
    if n == 0 or not (0 <= int(g) < MAX_INDEX):
        return np.tile(fb, (rows, 1)), 0, 1, np.zeros(rows, np.int32)
    ranks, distinct, row_src = select(n, rows, seed, g)
    p = pix[ranks]
    return backproject(p % W, p // W, depth.reshape(-1)[p], intr), n, distinct, row_src


def frame_clouds(depth, label, intrinsics, frame_of, want, index, rows, seed, fallback=None):
    """The whole call: depth [F,H,W] uint16, label [F,H,W] uint8, intrinsics [F,5].  -> dict(cloud [C,rows,3],
    num_pixels [C] int32, num_distinct [C] int64, row_src [C,rows] int32)."""
    depth = np.asarray(depth)
    depth = depth.view(np.uint16) if depth.dtype == np.int16 else depth
    F = depth.shape[0]
    C = len(frame_of)
    cloud = np.zeros((C, rows, 3), np.float32)
    num_pixels, num_distinct = np.zeros(C, np.int32), np.zeros(C, np.int64)
    row_src = np.zeros((C, rows), np.int32)
    for c in range(C):
        fb = None if fallback is None else np.asarray(fallback, np.float32)[c]
        f = int(frame_of[c])
        if 0 <= f < F:
            out = frame_cloud(depth[f], np.asarray(label)[f], np.asarray(intrinsics)[f], want[c], index[c], rows, seed, fb)
        else:
            out = frame_cloud(np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint8), np.ones(5, np.float32), want[c],
                              index[c], rows, seed, fb)
        cloud[c], num_pixels[c], num_distinct[c], row_src[c] = out
    return dict(cloud=cloud, num_pixels=num_pixels, num_distinct=num_distinct, row_src=row_src)


def rendered_scene(class_id, mesh_index, rot_mat64, translation, seed, first_index, max_v, max_t, classes, dataset='ycbv',
                   camera=None):
    """cloudaae_rendered_scene: -> dict(inst_offsets [2B+1], inst_mesh, inst_label [3B], inst_pose [3B,16] float64,
    vert_base, tri_base [3B+1], occluder_class [B], occluder_centre [B,3] float32)."""
    class_id = np.asarray(class_id, np.int64)
    mesh_index = np.asarray(mesh_index, np.int64)
    B = len(class_id)
    R = np.asarray(rot_mat64, np.float64).reshape(B, 3, 3)
    t = np.asarray(translation, np.float32).reshape(B, 3)
    dummy = np.zeros((int(max(classes)) + 1, 1, 6), np.float32)        # the class and the centre do not read the models
    occ = object_occluder(dummy, B, seed, first_index, classes, R, t, per=1, dataset=dataset, camera=camera)
    ok = (class_id >= 0) & (class_id < len(mesh_index))
    target = np.where(ok, mesh_index[np.clip(class_id, 0, len(mesh_index) - 1)], -1)
    pose = np.zeros((3 * B, 4, 4), np.float64)
    pose[:, 3, 3] = 1.0
    for k in range(3):
        pose[k::3, :3, :3] = R
    pose[0::3, :3, 3] = t.astype(np.float64)
    pose[1::3, :3, 3] = t.astype(np.float64)
    pose[2::3, :3, 3] = occ['centre'].astype(np.float64)
    mesh = np.stack([target, target, mesh_index[occ['occ_class']]], axis=1).reshape(-1)
    offs = np.empty(2 * B + 1, np.int64)
    offs[0:2 * B:2] = 3 * np.arange(B)
    offs[1:2 * B:2] = 3 * np.arange(B) + 1
    offs[2 * B] = 3 * B
    j = np.arange(3 * B + 1, dtype=np.int64)
    return dict(inst_offsets=offs.astype(np.int32), inst_mesh=mesh.astype(np.int32),
                inst_label=np.tile(np.array([1, 1, 2], np.int32), B), inst_pose=pose.reshape(3 * B, 16),
                vert_base=(j * max_v).astype(np.int32), tri_base=(j * max_t).astype(np.int32),
                occluder_class=occ['occ_class'], occluder_centre=occ['centre'])


def render_strided(meshes, scene, intrinsics, height, width, z_near=0.05):
    """render_reference.render given the scene's own bases: every instance is padded to the largest mesh with vertices
    and triangles that cannot be drawn (a vertex behind the camera; the renderer treats ranks past a mesh's counts as
    absent, so the padding must leave depth, label and rank of every pixel as the device writes them)."""
    max_v = max(len(m[0]) for m in meshes)
    max_t = max(len(m[1]) for m in meshes)
    padded = []
    for v, t in ((m[0], m[1]) for m in meshes):
        v, t = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(t, np.int64).reshape(-1, 3)
        pv = np.concatenate([v, np.full((max_v - len(v), 3), np.nan, np.float32)])
        pt = np.concatenate([t, np.full((max_t - len(t), 3), -1, np.int64)])
        padded.append((pv, pt))
    offs = scene['inst_offsets']
    frames = []
    for f in range(len(offs) - 1):
        frames.append([(int(scene['inst_mesh'][j]), int(scene['inst_label'][j]), scene['inst_pose'][j].reshape(4, 4))
                       for j in range(offs[f], offs[f + 1])])
    return render(padded, frames, intrinsics, height, width, z_near)
