"""Object models from triangle meshes: what the reference ships ready-made as obj_models.tfrecords ([2048,6] records of
21 YCB objects), built here from PLY meshes on the GPU.  cloudaae_mesh_weights turns triangle areas into integer weights
and their exact cumulative sums, cloudaae_mesh_sample draws area-uniform surface points with colours and face normals,
cloudaae_ragged_fps thins them to the model and cloudaae_mesh_gather_rows collects the rows.  The definition is in
DESIGN.md ("Mesh sampling"); a model is a function of (seed, mesh id) alone.

    v, t, c = read_ply("obj_000001.ply", scale=0.001)                       # BOP meshes are in millimetres
    models, normals = models_from_meshes(paths, return_normals=True)       # [S,2048,6] f32, [S,2048,3] f64 (device)
    write_obj_models("obj_models.tfrecords", models)                       # what --data_dir / load_object_models read
    write_ply("model.ply", vertices, triangles)                            # e.g. a mesh fused by utils/fuse.py

    python -m cloudaae_amd.utils.mesh_models --meshes DIR --out FILE [--scale 0.001] [--seed N]
"""
import argparse
import glob
import os

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

STREAM = 20                      # the Philox stream of the draws (csrc/mesh_sample.hip)
DEFAULT_SEED = 123456789
NUM_POINT = 2048                 # points of a model record (tfrecord_io.read_and_decode_obj_model)
OVERSAMPLE = 16
MAX_TRIANGLES = 1 << 24          # per mesh
MAX_INDEX = 1 << 40              # global sample indices lie below

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


# ---- PLY -------------------------------------------------------------------------------------------------------------
def _ply_header(data):
    """-> (format, [(element name, count, [(property name, type) or (name, count type, item type)])], body offset)."""
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file (no ply / end_header)")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError("PLY header is cut short")
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if not elements:
                raise ValueError("PLY property before any element")
            types = w[2:4] if w[1] == "list" else w[1:2]
            for ty in types:
                if ty not in _PLY_TYPES:
                    raise ValueError("unknown PLY type %r" % ty)
            elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]) if w[1] == "list"
                                   else (w[2], _PLY_TYPES[w[1]]))
        else:
            raise ValueError("unknown PLY header line %r" % line)
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("PLY format %r is not supported (ascii and binary_little_endian are)" % fmt)
    return fmt, elements, nl + 1


def _ply_binary_element(data, pos, count, props):
    """-> ({scalar property: array}, {list property: list of arrays}, new pos)."""
    if all(len(p) == 2 for p in props):
        dt = np.dtype([(name, "<" + ty) for name, ty in props])
        if pos + count * dt.itemsize > len(data):
            raise ValueError("PLY file is cut short")
        rows = np.frombuffer(data, dt, count, pos)
        return {name: rows[name] for name, _ in props}, {}, pos + count * dt.itemsize
    # lists: when every row has the counts of the first one, the element is a fixed record after all
    first, p = [], pos
    for prop in props:
        if len(prop) == 2:
            p += np.dtype(prop[1]).itemsize
            first.append(None)
        else:
            cdt = np.dtype("<" + prop[1])
            if count and p + cdt.itemsize > len(data):          # (an element without rows, as write_ply's faces of an empty mesh)
                raise ValueError("PLY file is cut short")
            k = int(np.frombuffer(data, cdt, 1, p)[0]) if count else 0
            first.append(k)
            p += cdt.itemsize + k * np.dtype(prop[2]).itemsize
    fields = []
    for prop, k in zip(props, first):
        if len(prop) == 2:
            fields.append((prop[0], "<" + prop[1]))
        else:
            fields += [(prop[0] + "#n", "<" + prop[1]), (prop[0], "<" + prop[2], (k,))]
    dt = np.dtype(fields)
    if pos + count * dt.itemsize <= len(data):
        rows = np.frombuffer(data, dt, count, pos)
        if all(np.all(rows[prop[0] + "#n"] == k) for prop, k in zip(props, first) if len(prop) == 3):
            scalars = {prop[0]: rows[prop[0]] for prop in props if len(prop) == 2}
            lists = {prop[0]: list(rows[prop[0]]) for prop in props if len(prop) == 3}
            return scalars, lists, pos + count * dt.itemsize
    scalars = {prop[0]: [] for prop in props if len(prop) == 2}
    lists = {prop[0]: [] for prop in props if len(prop) == 3}
    for _ in range(count):
        for prop in props:
            if len(prop) == 2:
                dt = np.dtype("<" + prop[1])
                if pos + dt.itemsize > len(data):
                    raise ValueError("PLY file is cut short")
                scalars[prop[0]].append(np.frombuffer(data, dt, 1, pos)[0])
                pos += dt.itemsize
            else:
                cdt, idt = np.dtype("<" + prop[1]), np.dtype("<" + prop[2])
                if pos + cdt.itemsize > len(data):
                    raise ValueError("PLY file is cut short")
                k = int(np.frombuffer(data, cdt, 1, pos)[0])
                pos += cdt.itemsize
                if k < 0 or pos + k * idt.itemsize > len(data):
                    raise ValueError("PLY file is cut short")
                lists[prop[0]].append(np.frombuffer(data, idt, k, pos))
                pos += k * idt.itemsize
    return {k: np.array(v) for k, v in scalars.items()}, lists, pos


def _ply_ascii_element(lines, row, count, props):
    if row + count > len(lines):
        raise ValueError("PLY file is cut short")
    scalars = {prop[0]: [] for prop in props if len(prop) == 2}
    lists = {prop[0]: [] for prop in props if len(prop) == 3}
    for line in lines[row:row + count]:
        w, p = line.split(), 0
        try:
            for prop in props:
                if len(prop) == 2:
                    scalars[prop[0]].append(float(w[p]))
                    p += 1
                else:
                    k = int(w[p])
                    if k < 0 or p + 1 + k > len(w):
                        raise IndexError
                    lists[prop[0]].append(np.array([int(x) for x in w[p + 1:p + 1 + k]], np.int64))
                    p += 1 + k
        except (IndexError, ValueError):
            raise ValueError("PLY file is cut short or malformed: %r" % line)
    return {k: np.array(v, np.float64) for k, v in scalars.items()}, lists, row + count


def read_ply(path, scale=1.0):
    """A PLY mesh -> (vertices [V,3] float32 = the file's x y z times `scale`, triangles [T,3] int32, colors [V,3]
    float32 in 0..1 or None).  ASCII and binary_little_endian; x y z float or double; red green blue uchar (divided by
    255) or float; other vertex properties and other elements are skipped by their declared size; faces are the list
    vertex_indices / vertex_index with any integer count and index types, polygons split as a fan (0, i, i+1).  A file
    that ends early raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, elements, pos = _ply_header(data)
    lines = None
    if fmt == "ascii":
        lines = [ln for ln in data[pos:].decode("ascii", "replace").splitlines() if ln.strip()]
        pos = 0
    found = {}
    for name, count, props in elements:
        if fmt == "ascii":
            scalars, lists, pos = _ply_ascii_element(lines, pos, count, props)
        else:
            scalars, lists, pos = _ply_binary_element(data, pos, count, props)
        found[name] = (count, dict(props_of=props), scalars, lists)
    if "vertex" not in found:
        raise ValueError("PLY file without a vertex element")
    nv, meta, sc, _ = found["vertex"]
    for k in "xyz":
        if k not in sc:
            raise ValueError("PLY vertex element without %s" % k)
    vertices = (np.stack([np.asarray(sc[k], np.float64) for k in "xyz"], axis=1).reshape(nv, 3)
                * float(scale)).astype(np.float32)
    colors = None
    if all(k in sc for k in ("red", "green", "blue")):
        types = {p[0]: p[1] for p in meta["props_of"] if len(p) == 2}
        cols = []
        for k in ("red", "green", "blue"):
            x = np.asarray(sc[k], np.float64)
            cols.append(x / 255.0 if types[k] == "u1" else x)
        colors = np.stack(cols, axis=1).reshape(nv, 3).astype(np.float32)
    triangles = np.zeros((0, 3), np.int64)
    if "face" in found:
        _, _, _, lists = found["face"]
        key = "vertex_indices" if "vertex_indices" in lists else "vertex_index" if "vertex_index" in lists else None
        if key is None:
            raise ValueError("PLY face element without vertex_indices / vertex_index")
        faces = [np.asarray(x, np.int64) for x in lists[key]]
        sizes = set(len(x) for x in faces)
        if len(sizes) == 1 and min(sizes) >= 3:          # the usual file: one polygon size
            poly, k = np.stack(faces), min(sizes)
            triangles = np.stack([np.stack([poly[:, 0], poly[:, i], poly[:, i + 1]], axis=1) for i in range(1, k - 1)],
                                 axis=1).reshape(-1, 3)
        else:                                            # the file's face order, each polygon's fan in order
            fans = [[x[0], x[i], x[i + 1]] for x in faces for i in range(1, len(x) - 1)]
            triangles = np.array(fans, np.int64).reshape(-1, 3)
    if triangles.size and (triangles.min() < -(1 << 31) or triangles.max() >= (1 << 31)):
        raise ValueError("PLY vertex index outside int32")
    triangles = triangles.astype(np.int32)
    return vertices, triangles, colors


def write_ply(path, vertices, triangles):
    """(vertices [V,3], triangles [T,3]; arrays or tensors) -> a binary_little_endian PLY file with float x y z and faces as
    `list uchar int vertex_indices`: what read_ply reads back, the float32 coordinates bit for bit."""
    v = np.asarray(vertices.detach().cpu() if isinstance(vertices, torch.Tensor) else vertices)
    t = np.asarray(triangles.detach().cpu() if isinstance(triangles, torch.Tensor) else triangles)
    require(v.ndim == 2 and v.shape[1] == 3, "vertices must be [V, 3]")
    require(t.ndim == 2 and t.shape[1] == 3 and t.dtype.kind in "iu", "triangles must be an integer [T, 3]")
    require(t.size == 0 or (t.min() >= 0 and t.max() < len(v)), "a triangle names a vertex outside the mesh")
    faces = np.zeros(len(t), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"], faces["i"] = 3, t
    header = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x",
                        "property float y", "property float z", "element face %d" % len(t),
                        "property list uchar int vertex_indices", "end_header"]) + "\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        f.write(faces.tobytes())


# ---- meshes on the device ------------------------------------------------------------------------------------------------
class PackedMeshes(object):
    """S meshes packed for the kernels: vert_offsets, tri_offsets [S+1] int32; vertices [V,3] float32; colors [V,3]
    float32 or None; triangles [T,3] int32 (indices local to their mesh) -- device tensors; num_triangles [S] (host)."""


def _as_mesh(m, scale):
    if isinstance(m, (str, bytes, os.PathLike)):
        return read_ply(m, scale)
    require(isinstance(m, (tuple, list)) and len(m) in (2, 3), "a mesh is a path or (vertices, triangles[, colors])")
    v = np.asarray(m[0].cpu() if isinstance(m[0], torch.Tensor) else m[0])
    t = np.asarray(m[1].cpu() if isinstance(m[1], torch.Tensor) else m[1])
    c = m[2] if len(m) == 3 else None
    require(v.ndim == 2 and v.shape[1] == 3, "vertices must be [V, 3]")
    require(t.ndim == 2 and t.shape[1] == 3 and t.dtype.kind in "iu", "triangles must be an integer [T, 3]")
    if c is not None:
        c = np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, np.float32)
        require(c.shape == v.shape, "colors must be [V, 3] like the vertices")
    if float(scale) != 1.0:
        v = v.astype(np.float64) * float(scale)
    return v.astype(np.float32), t.astype(np.int32), c


def pack_meshes(meshes, scale=1.0, device=None):
    """[path or (vertices, triangles[, colors])] -> PackedMeshes on `device`.  Colours are kept only when every mesh
    has them (a mesh without gets zeros otherwise -- then all get zeros)."""
    if isinstance(meshes, PackedMeshes):
        return meshes
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    require(len(meshes) >= 1, "no mesh given")
    ms = [_as_mesh(m, scale) for m in meshes]
    nt = np.array([len(m[1]) for m in ms], np.int64)
    nv = np.array([len(m[0]) for m in ms], np.int64)
    require(nt.max() <= MAX_TRIANGLES, "a mesh has more than 2^24 triangles")
    require(nt.sum() >= 1 and nv.sum() >= 1, "the meshes hold no triangle")
    require(nt.sum() <= (1 << 28) and nv.sum() <= (1 << 28), "more than 2^28 vertices or triangles in all")
    p = PackedMeshes()
    p.num_triangles, p.num_vertices = nt, nv
    p.vert_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)).to(device)
    p.tri_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(nt)]).astype(np.int32)).to(device)
    p.vertices = torch.from_numpy(np.ascontiguousarray(np.concatenate([m[0] for m in ms]))).to(device)
    p.triangles = torch.from_numpy(np.ascontiguousarray(np.concatenate([m[1] for m in ms]))).to(device)
    p.colors = None
    if all(m[2] is not None for m in ms):
        p.colors = torch.from_numpy(np.ascontiguousarray(np.concatenate([m[2] for m in ms]))).to(device)
    p.device = device
    return p


def mesh_weights(packed):
    """cloudaae_mesh_weights -> dict(weights, cum [T] (int64 tensors holding the uint64 values: all below 2^57),
    a2max [S] float64, invalid [S] int32), on the device."""
    p = packed
    S, V, T = len(p.num_triangles), int(p.vertices.shape[0]), int(p.triangles.shape[0])
    dev = p.device
    weights = _lib.empty((T,), dtype=torch.int64, device=dev)
    cum = _lib.empty((T,), dtype=torch.int64, device=dev)
    a2max = _lib.empty((S,), dtype=torch.float64, device=dev)
    invalid = _lib.empty((S,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.cloudaae_mesh_weights_workspace_bytes(T))
    require(nbytes > 0, "triangle count outside the kernel's limits")
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.check(L.cloudaae_mesh_weights(S, ptr(p.vert_offsets), ptr(p.tri_offsets), V, T, ptr(p.vertices), ptr(p.triangles),
                                       ptr(weights), ptr(cum), ptr(a2max), ptr(invalid), ptr(ws), nbytes, stream()),
               "cloudaae_mesh_weights")
    return dict(weights=weights, cum=cum, a2max=a2max, invalid=invalid)


def sample_meshes(meshes, n, seed=DEFAULT_SEED, first_index=0, mesh_ids=None, return_normals=False, cum=None, scale=1.0,
                  device=None):
    """n area-uniform surface samples of every mesh: sample j is global sample first_index + j of mesh id mesh_ids[i]
    (default i), so a launch may be split, and a mesh sampled alone under its id gives its samples in the batch.
    meshes: PackedMeshes or what pack_meshes takes.  cum: cumulative weights to draw by (default: the areas', from
    mesh_weights).  Returns dict(xyzrgb [S,n,6] float32, tri [S,n] int32 (-1: the mesh has no area), normal [S,n,3]
    float64 (with return_normals: the face's unit normal, its sign the winding's), cum, packed)."""
    require(int(n) >= 1, "n must be >= 1")
    require(0 <= int(first_index) and int(first_index) + int(n) <= MAX_INDEX, "sample indices must lie in [0, 2^40)")
    p = pack_meshes(meshes, scale, device)
    S, V, T = len(p.num_triangles), int(p.vertices.shape[0]), int(p.triangles.shape[0])
    require(S * int(n) <= (1 << 28), "more than 2^28 samples in one call")
    dev = p.device
    ids = None
    if mesh_ids is not None:
        host = np.asarray(mesh_ids.cpu() if isinstance(mesh_ids, torch.Tensor) else mesh_ids, np.int64).reshape(-1)
        require(len(host) == S, "one mesh id per mesh")
        require(host.min() >= 0 and host.max() < (1 << 24), "mesh ids must lie in [0, 2^24)")
        ids = torch.from_numpy(host.astype(np.int32)).to(dev)
    if cum is None:
        cum = mesh_weights(p)['cum']
    require(isinstance(cum, torch.Tensor) and cum.dtype == torch.int64 and cum.numel() == T,
            "cum must be an int64 device tensor with one entry per triangle")
    xyzrgb = _lib.empty((S, int(n), 6), dtype=torch.float32, device=dev)
    tri = _lib.empty((S, int(n)), dtype=torch.int32, device=dev)
    normal = _lib.empty((S, int(n), 3), dtype=torch.float64, device=dev) if return_normals else None
    _lib.check(_lib.lib().cloudaae_mesh_sample(S, ptr(p.vert_offsets), ptr(p.tri_offsets), V, T, ptr(p.vertices),
                                               ptr(p.colors), ptr(p.triangles), ptr(cum), ptr(ids), int(n),
                                               int(first_index), int(seed) % (1 << 64), ptr(xyzrgb), ptr(tri), ptr(normal),
                                               stream()), "cloudaae_mesh_sample")
    out = dict(xyzrgb=xyzrgb, tri=tri, cum=cum, packed=p)
    if return_normals:
        out['normal'] = normal
    return out


def gather_rows(src, idx, cols=None):
    """cloudaae_mesh_gather_rows: src [S,R,C] (float32 / int32 / float64 / int64), idx [S,k] int32 local to the set, or
    None with cols: the first `cols` columns of every row, repacked.  -> [S,k,cols]."""
    require(src.dim() == 3 and src.is_contiguous(), "src must be a contiguous [S, R, C] tensor")
    S, R, C = (int(v) for v in src.shape)
    cols = C if cols is None else int(cols)
    require(1 <= cols <= C, "cols must lie in [1, C]")
    item = src.element_size()
    require(item in (4, 8), "rows of 4- or 8-byte elements only")
    if idx is not None:
        require(idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == S, "idx must be an int32 [S, k] tensor")
    k = int(idx.shape[1]) if idx is not None else R
    out = _lib.empty((S, k, cols), dtype=src.dtype, device=src.device)
    _lib.check(_lib.lib().cloudaae_mesh_gather_rows(S, k, ptr(idx), R, ptr(src), C, cols, item, ptr(out), cols, stream()),
               "cloudaae_mesh_gather_rows")
    return out


def models_from_meshes(meshes_or_paths, num_point=NUM_POINT, oversample=OVERSAMPLE, seed=DEFAULT_SEED, scale=1.0,
                       return_normals=False, mesh_ids=None, device=None, details=False):
    """One object model per mesh: oversample * num_point surface samples, thinned to num_point by farthest point
    sampling from sample 0 (cloudaae_ragged_fps), the six columns (and the normals) of the picked rows gathered.
    -> models [S,num_point,6] float32 (device), and with return_normals also normals [S,num_point,3] float64: the
    obj_normals that evaluate_batch(icp={'estimation': 'point_to_plane'}) takes.  The same (seed, mesh id) gives the same
    model whatever else is in the batch.  A mesh without area raises ValueError (one read-back of a total per mesh).
    details: return the dict with idx [S,num_point] and the samples too."""
    from . import segment
    require(int(num_point) >= 1 and int(oversample) >= 1, "num_point and oversample must be >= 1")
    n = int(num_point) * int(oversample)
    p = pack_meshes(meshes_or_paths, scale, device)
    S = len(p.num_triangles)
    w = mesh_weights(p)
    last = torch.from_numpy(np.maximum(np.cumsum(p.num_triangles) - 1, 0)).to(p.device)
    totals = w['cum'][last].cpu().numpy()
    for i in range(S):
        if p.num_triangles[i] == 0 or totals[i] == 0:
            raise ValueError("mesh %d has no triangle with an area" % i)
    s = sample_meshes(p, n, seed=seed, mesh_ids=mesh_ids, return_normals=return_normals, cum=w['cum'])
    xyz = gather_rows(s['xyzrgb'], None, cols=3)
    offsets = torch.from_numpy((np.arange(S + 1, dtype=np.int64) * n).astype(np.int32)).to(p.device)
    idx, _ = segment.ragged_fps(offsets, xyz.view(S * n, 3), int(num_point), np.zeros(S, np.int32))
    models = gather_rows(s['xyzrgb'], idx)
    normals = gather_rows(s['normal'], idx) if return_normals else None
    if details:
        return dict(models=models, normals=normals, idx=idx, samples=s, weights=w)
    return (models, normals) if return_normals else models


def write_obj_models(path, models, labels=None):
    """A TFRecord file of object models in the schema tfrecord_io.read_and_decode_obj_model reads: per model the
    features model (2048 * 6 floats) and label (int64; default: the model's position)."""
    from .. import tfrecord_io
    m = np.asarray(models.detach().cpu() if isinstance(models, torch.Tensor) else models)
    require(m.ndim == 3 and m.shape[1:] == (NUM_POINT, 6), "models must be [S, 2048, 6] (the record's size)")
    m = m.astype(np.float32)
    labels = np.arange(len(m)) if labels is None else np.asarray(labels)
    require(labels.shape == (len(m),) and labels.dtype.kind in "iu", "labels must be one integer per model")
    tfrecord_io.write_records(path, [tfrecord_io.encode_example({"model": m[i].reshape(-1), "label": np.array([labels[i]], np.int64)})
                                     for i in range(len(m))])


def mesh_files(directory):
    """The *.ply files of a directory in sorted order: class i is file i."""
    files = sorted(glob.glob(os.path.join(directory, "*.ply")))
    require(len(files) >= 1, "no *.ply file in %s" % directory)
    return files


def main(argv=None):
    parser = argparse.ArgumentParser(description="object models (obj_models.tfrecords) from the *.ply meshes of a directory")
    parser.add_argument("--meshes", required=True, help="directory of *.ply files; class i is the i-th in sorted order")
    parser.add_argument("--out", required=True, help="the TFRecord file to write")
    parser.add_argument("--scale", type=float, default=1.0, help="factor on the coordinates (0.001: millimetres to metres)")
    parser.add_argument("--seed", type=int, default=DEFAULT_SEED)
    parser.add_argument("--oversample", type=int, default=OVERSAMPLE)
    parser.add_argument("--gpu", type=int, default=0)
    args = parser.parse_args(argv)
    files = mesh_files(args.meshes)
    torch.cuda.set_device(args.gpu)
    models = models_from_meshes(files, oversample=args.oversample, seed=args.seed, scale=args.scale)
    write_obj_models(args.out, models)
    for i, f in enumerate(files):
        print("class %d: %s" % (i, os.path.basename(f)))
    print("%d models written to %s" % (len(files), args.out))


if __name__ == "__main__":
    main()
