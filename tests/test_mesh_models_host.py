"""CPU: the PLY reader, the object-model writer and the argument checks of cloudaae_amd/utils/mesh_models.py, and the
NumPy restatement of DESIGN.md "Mesh sampling" (tests/mesh_models_reference.py) checked for what it claims: exact
integer weights, barycentric coordinates that are non-negative and sum to 1, and area-uniform draws."""
import os
import struct

import numpy as np
import pytest

import mesh_models_reference as R

SOUP_SEED, DRAW_SEED = 1, 3          # the chi-square below: chosen once so that it passes (statistic 205.87 of 266.39)


def _mm():
    from cloudaae_amd.utils import mesh_models
    return mesh_models


# ---- writers of test files -------------------------------------------------------------------------------------------
def _header(fmt, nv, nf, vertex_props, face_prop="property list uchar int vertex_indices", extra=()):
    lines = ["ply", "format %s 1.0" % fmt, "comment made by the test", "element vertex %d" % nv] + list(vertex_props)
    for name, count, props in extra:
        lines += ["element %s %d" % (name, count)] + list(props)
    lines += ["element face %d" % nf, face_prop, "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _write_ascii(path, v, faces, colors=None):
    props = ["property float x", "property float y", "property float z"]
    if colors is not None:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    body = []
    for i, p in enumerate(v):
        row = ["%r" % float(x) for x in p]
        if colors is not None:
            row += ["%d" % c for c in colors[i]]
        body.append(" ".join(row))
    for f in faces:
        body.append(" ".join(["%d" % len(f)] + ["%d" % i for i in f]))
    with open(path, "wb") as fh:
        fh.write(_header("ascii", len(v), len(faces), props) + ("\n".join(body) + "\n").encode("ascii"))


def _write_binary(path, v, faces, colors=None, coord="float", extra_prop=False, count_type="uchar", index_type="int",
                  face_name="vertex_indices", float_colors=False, other_element=False):
    cfmt = {"float": "f", "double": "d"}[coord]
    ifmt = {"uchar": "B", "ushort": "H", "int": "i", "uint": "I", "short": "h"}
    props = ["property %s x" % coord, "property %s y" % coord]
    if extra_prop:
        props.append("property double quality")           # between y and z: skipped by its declared size
    props.append("property %s z" % coord)
    if colors is not None:
        props += ["property %s %s" % ("float" if float_colors else "uchar", k) for k in ("red", "green", "blue")]
    if extra_prop:
        props.append("property ushort flags")
    extra = [("camera", 2, ["property float cx", "property short id"])] if other_element else []
    out = _header("binary_little_endian", len(v), len(faces), props,
                  "property list %s %s %s" % (count_type, index_type, face_name), extra)
    for i, p in enumerate(v):
        out += struct.pack("<2" + cfmt, p[0], p[1])
        if extra_prop:
            out += struct.pack("<d", 1e300)
        out += struct.pack("<" + cfmt, p[2])
        if colors is not None:
            out += struct.pack("<3f", *colors[i]) if float_colors else struct.pack("<3B", *colors[i])
        if extra_prop:
            out += struct.pack("<H", 65535)
    if other_element:
        out += struct.pack("<fh", 1.5, -3) * 2
    for f in faces:
        out += struct.pack("<" + ifmt[count_type], len(f)) + struct.pack("<%d%s" % (len(f), ifmt[index_type]), *f)
    with open(path, "wb") as fh:
        fh.write(out)
    return len(out)


def _quad_cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32) * np.float32(0.37) + np.float32(0.1)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    colors = (np.arange(24).reshape(8, 3) * 11 % 256).astype(np.uint8)
    fan = np.array([[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)], np.int32)
    return v, quads, colors, fan


# ---- PLY -------------------------------------------------------------------------------------------------------------
def test_ply_ascii_quads_and_uchar_colours(tmp_path):
    v, quads, colors, fan = _quad_cube()
    _write_ascii(tmp_path / "a.ply", v, quads, colors)
    gv, gt, gc = _mm().read_ply(tmp_path / "a.ply")
    assert gv.dtype == np.float32 and gt.dtype == np.int32 and gc.dtype == np.float32
    assert np.array_equal(gv, v) and np.array_equal(gt, fan)
    assert np.array_equal(gc, (colors.astype(np.float64) / 255.0).astype(np.float32))
    # no colours, triangles
    _write_ascii(tmp_path / "b.ply", v, [tuple(t) for t in fan])
    gv, gt, gc = _mm().read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(gv, v) and np.array_equal(gt, fan) and gc is None


@pytest.mark.parametrize("coord, count_type, index_type, face_name",
                         [("float", "uchar", "int", "vertex_indices"), ("double", "ushort", "uint", "vertex_index"),
                          ("float", "int", "short", "vertex_indices")])
def test_ply_binary(tmp_path, coord, count_type, index_type, face_name):
    v, quads, colors, fan = _quad_cube()
    path = tmp_path / "c.ply"
    _write_binary(path, v, quads, colors, coord=coord, extra_prop=True, count_type=count_type, index_type=index_type,
                  face_name=face_name, other_element=True)
    gv, gt, gc = _mm().read_ply(path)
    assert np.array_equal(gv, v) and np.array_equal(gt, fan)
    assert np.array_equal(gc, (colors.astype(np.float64) / 255.0).astype(np.float32))


def test_ply_mixed_polygons_float_colours_and_scale(tmp_path):
    v, quads, colors, fan = _quad_cube()
    faces = [quads[0], (0, 4, 5), (2, 3, 7, 6, 4), (1, 5)]                # a quad, a triangle, a pentagon, a stray edge
    want = np.array([[0, 1, 3], [0, 3, 2], [0, 4, 5], [2, 3, 7], [2, 7, 6], [2, 6, 4]], np.int32)
    fc = (colors.astype(np.float32) / np.float32(300.0))
    _write_binary(tmp_path / "d.ply", v.astype(np.float64) * 1000.0, faces, fc, coord="double", float_colors=True)
    gv, gt, gc = _mm().read_ply(tmp_path / "d.ply", scale=0.001)
    assert np.array_equal(gt, want) and np.array_equal(gc, fc)
    assert np.array_equal(gv, (v.astype(np.float64) * 1000.0 * 0.001).astype(np.float32))
    assert np.abs(gv - v).max() <= np.spacing(np.float32(0.5))


def test_ply_truncated_file_raises(tmp_path):
    v, quads, colors, _ = _quad_cube()
    n = _write_binary(tmp_path / "e.ply", v, quads, colors)
    data = open(tmp_path / "e.ply", "rb").read()
    assert len(data) == n
    for cut in (n - 1, n - 17 * 6 + 3, n - 17 * 6 - 5, data.index(b"end_header") + 3, 40):
        with open(tmp_path / "f.ply", "wb") as fh:
            fh.write(data[:cut])
        with pytest.raises(ValueError):
            _mm().read_ply(tmp_path / "f.ply")
    _write_ascii(tmp_path / "g.ply", v, quads, colors)
    text = open(tmp_path / "g.ply", "rb").read()
    with open(tmp_path / "h.ply", "wb") as fh:
        fh.write(text[:-30])
    with pytest.raises(ValueError):
        _mm().read_ply(tmp_path / "h.ply")
    with open(tmp_path / "i.ply", "wb") as fh:
        fh.write(b"solid not a ply\n")
    with pytest.raises(ValueError):
        _mm().read_ply(tmp_path / "i.ply")


# ---- object-model records --------------------------------------------------------------------------------------------------
def test_written_object_models_read_back_bit_equal(tmp_path):
    from cloudaae_amd import tfrecord_io
    rng = np.random.default_rng(5)
    models = rng.standard_normal((3, 2048, 6)).astype(np.float32)
    models[0, 0, 0] = np.float32(-0.0)
    models[1, 7, 3] = np.float32(1e-42)                       # a subnormal keeps its bits too
    _mm().write_obj_models(str(tmp_path / "m.tfrecords"), models)
    got, labels = tfrecord_io.read_and_decode_obj_model(str(tmp_path / "m.tfrecords"))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), models.view(np.uint32))
    assert np.array_equal(labels, [0, 1, 2])
    import torch
    _mm().write_obj_models(str(tmp_path / "n.tfrecords"), torch.from_numpy(models[:2]), labels=[20, 4])
    got, labels = tfrecord_io.read_and_decode_obj_model(str(tmp_path / "n.tfrecords"))
    assert np.array_equal(got.view(np.uint32), models[:2].view(np.uint32)) and np.array_equal(labels, [20, 4])
    assert list(tfrecord_io.tf_record_iterator(str(tmp_path / "n.tfrecords"), verify=True))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_lattice_weights_are_exact():
    v, t = R.lattice(300, seed=2)
    w = R.mesh_weights(v, t)
    a2 = w['a2']
    assert set(a2.tolist()) <= {1.0, 2.0, 4.0, 8.0, 16.0} and w['invalid'] == 0
    assert np.array_equal(w['weights'], (a2 / a2.max() * 2.0 ** 32).astype(np.uint64))
    assert int(w['weights'].max()) == 1 << 32 and w['W'] == sum(int(x) for x in w['weights'])
    assert np.array_equal(w['cum'], np.cumsum(w['weights'], dtype=np.uint64))


def test_degenerate_triangles_get_no_weight():
    v, t, _ = R.soup(200, seed=SOUP_SEED, degenerate=True)
    w = R.mesh_weights(v, t)
    assert w['invalid'] == 3                                   # zero area, repeated vertex, index out of range
    assert list(w['weights'][:4]) == [0, 0, 0, 0]              # and the one 2^-40 of the largest
    assert w['a2'][3] == w['a2max'] * 2.0 ** -40 and np.all(w['weights'][4:] > 0)
    s = R.sample_mesh(v, t, 5000, seed=9)
    assert s['tri'].min() >= 4
    empty = R.sample_mesh(v, t[:3], 10, seed=9)
    assert np.all(empty['tri'] == -1) and not empty['xyzrgb'].any() and not empty['normal'].any()


def test_restatement_is_area_uniform():
    from scipy import stats
    T, n = 200, 200000
    v, t, c = R.soup(T, seed=SOUP_SEED)
    w = R.mesh_weights(v, t)
    s = R.sample_mesh(v, t, n, seed=DRAW_SEED, colors=c)
    share = w['weights'].astype(np.float64) / float(w['W'])
    counts = np.bincount(s['tri'], minlength=T)
    chi2 = float((((counts - n * share) ** 2) / (n * share)).sum())
    limit = float(stats.chi2.ppf(0.999, T - 1))
    print("chi-square of %d draws over %d triangles: %.3f (99.9 %% quantile %.3f)" % (n, T, chi2, limit))
    assert chi2 < limit
    # the weights are the areas to 2^-32 of the largest
    area = w['a2'] / w['a2'].sum()
    assert np.abs(share - area).max() < 2.0 ** -30
    b = s['bary']
    assert b.min() >= 0.0 and np.abs(b.sum(axis=1) - 1.0).max() <= 2.0 ** -52
    # every point lies in its triangle's plane and every colour between its corners'
    nrm, a2, _ = R.triangle_normals(v, t)
    d = np.einsum('ij,ij->i', s['xyzrgb'][:, :3].astype(np.float64) - v[t[s['tri'], 0]].astype(np.float64),
                  nrm[s['tri']] / a2[s['tri']][:, None])
    assert np.abs(d).max() < 1e-6
    corner = c[t[s['tri']]]
    assert np.all(s['xyzrgb'][:, 3:] >= corner.min(axis=1) - 1e-6) and np.all(s['xyzrgb'][:, 3:] <= corner.max(axis=1) + 1e-6)
    assert np.abs(np.linalg.norm(s['normal'], axis=1) - 1.0).max() < 1e-15


def test_restatement_draws_depend_on_seed_mesh_and_index_only():
    v, t, c = R.soup(50, seed=4)
    one = R.sample_mesh(v, t, 100, seed=11, first_index=0, mesh_id=5, colors=c)
    a = R.sample_mesh(v, t, 30, seed=11, first_index=0, mesh_id=5, colors=c)
    b = R.sample_mesh(v, t, 70, seed=11, first_index=30, mesh_id=5, colors=c)
    for k in ('xyzrgb', 'tri', 'normal'):
        assert np.array_equal(one[k], np.concatenate([a[k], b[k]]))
    other = R.sample_mesh(v, t, 100, seed=11, first_index=0, mesh_id=6, colors=c)
    assert not np.array_equal(one['tri'], other['tri'])


# ---- argument checks -----------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks(tmp_path):
    import torch
    mm = _mm()
    v, t, c = R.cube()
    with pytest.raises(ValueError):
        mm.write_obj_models(str(tmp_path / "x.tfrecords"), np.zeros((2, 1024, 6), np.float32))
    with pytest.raises(ValueError):
        mm.write_obj_models(str(tmp_path / "x.tfrecords"), np.zeros((2, 2048, 6), np.float32), labels=[1])
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t)], 0, device="cpu")
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t)], 16, first_index=(1 << 40) - 15, device="cpu")
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t)], 16, first_index=-1, device="cpu")
    with pytest.raises(ValueError):
        mm.pack_meshes([], device="cpu")
    with pytest.raises(ValueError):
        mm.pack_meshes([(v[:, :2], t)], device="cpu")
    with pytest.raises(ValueError):
        mm.pack_meshes([(v, t.astype(np.float32))], device="cpu")
    with pytest.raises(ValueError):
        mm.pack_meshes([(v, t, c[:4])], device="cpu")
    with pytest.raises(ValueError):
        mm.pack_meshes([(v, np.zeros((0, 3), np.int32))], device="cpu")
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t), (v, t)], 4, mesh_ids=[3], device="cpu")
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t)], 4, mesh_ids=[1 << 24], device="cpu")
    with pytest.raises(ValueError):
        mm.sample_meshes([(v, t)], 4, cum=torch.zeros(3, dtype=torch.int64), device="cpu")
    with pytest.raises(ValueError):
        mm.models_from_meshes([(v, t)], num_point=0, device="cpu")
    with pytest.raises(ValueError):
        mm.gather_rows(torch.zeros((2, 4, 6)), None, cols=7)
    with pytest.raises(ValueError):
        mm.mesh_files(str(tmp_path))
    # packing keeps colours only when every mesh has them, scales the coordinates, and nothing runs off the GPU
    p = mm.pack_meshes([(v, t, c), (v, t)], scale=2.0, device="cpu")
    assert p.colors is None and list(p.tri_offsets) == [0, 12, 24] and list(p.vert_offsets) == [0, 8, 16]
    assert np.array_equal(p.vertices.numpy()[:8], v * 2)
    from cloudaae_amd import _lib
    with pytest.raises(_lib.HipLibraryError):
        mm.mesh_weights(p)
    assert int(_lib.lib().cloudaae_mesh_weights_workspace_bytes(0)) == -1
    assert int(_lib.lib().cloudaae_mesh_weights_workspace_bytes(1 << 29)) == -1
    assert int(_lib.lib().cloudaae_mesh_weights_workspace_bytes(257)) >= 2 * 8 * 257 + 2 * 8 * 2


def test_training_flags_need_sampled_poses():
    from cloudaae_amd import train_cloudAAE_ycbv as T
    args = T.parse_arg_groups(T.get_training_argparser(), [])['mi355x']
    assert args['meshes'] == '' and args['mesh_scale'] == 1.0
    with pytest.raises(SystemExit):
        T.main(['--meshes', os.path.dirname(__file__), '--poses', 'records'])
