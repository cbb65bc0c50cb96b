"""GPU: cloudaae_mesh_weights, cloudaae_mesh_sample and cloudaae_mesh_gather_rows through the C ABI against the NumPy
restatement of DESIGN.md "Mesh sampling" (tests/mesh_models_reference.py), the object model built from them, and a short
training run on models made from PLY files.

What is integer in the definition is compared for equality: weights of the lattice meshes (every A2 a power of two),
cumulative sums, W, invalid counts, triangle indices (the restatement is fed the kernel's own cum, so a weight that
differed by one could not move a draw).  What is floating point has the bound its arithmetic gives: a weight is
floor(x 2^32) of a quotient of two correctly rounded square roots, so it may differ by 1 where a library's sqrt or
division is 1 ulp off (|dw| <= 1); a point is products and sums of exactly widened fp32 values in a fixed order, rounded
once (1 ulp of fp32); a normal is three quotients by one square root (1e-15).  Equality is expected in all three and was
measured on MI355X (profiles/notes_mesh_models.md): 0 weights, 0 coordinates and 0 normal components differ.  Every
test prints its figures before it asserts."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_models_reference as R
import segment_reference as SR

pytestmark = pytest.mark.gpu

B = 256                    # MS_SCAN_BLOCK of csrc/mesh_sample.hip: triangles per block of the scan
GUARD = 4                  # rows kept before and after every output
FILL = 0xA5


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side."""

    def __init__(self, rows, cols, dtype, dev):
        item = torch.empty((), dtype=dtype).element_size()
        self.rb = cols * item
        self.full = torch.full(((rows + 2 * GUARD) * self.rb,), FILL, dtype=torch.uint8, device=dev)
        self.view = self.full[GUARD * self.rb:(GUARD + rows) * self.rb].view(dtype).view(rows, cols)
        self.rows = rows

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        full = self.full.cpu().numpy()
        edge = GUARD * self.rb
        assert np.all(full[:edge] == FILL) and np.all(full[edge + self.rows * self.rb:] == FILL), "guard rows were written"
        return self.view.cpu().numpy()


class Packed(object):
    def __init__(self, meshes, dev):
        vo, to, v, t, c = R.pack(meshes)
        self.S, self.V, self.T = len(meshes), len(v), len(t)
        self.host = (vo, to, v, t, c)
        self.vo, self.to = torch.from_numpy(vo).to(dev), torch.from_numpy(to).to(dev)
        self.v, self.t = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
        self.c = torch.from_numpy(c).to(dev) if c is not None else None
        self.dev = dev

    def mesh(self, i):
        vo, to, v, t, c = self.host
        return v[vo[i]:vo[i + 1]], t[to[i]:to[i + 1]], (c[vo[i]:vo[i + 1]] if c is not None else None)


def run_weights(hip, p):
    L = hip.lib()
    w, cum = Guarded(p.T, 1, torch.int64, p.dev), Guarded(p.T, 1, torch.int64, p.dev)
    a2max, invalid = Guarded(p.S, 1, torch.float64, p.dev), Guarded(p.S, 1, torch.int32, p.dev)
    nbytes = int(L.cloudaae_mesh_weights_workspace_bytes(p.T))
    assert nbytes > 0
    ws = Guarded(nbytes // 8, 1, torch.int64, p.dev)
    hip.check(L.cloudaae_mesh_weights(p.S, p.vo.data_ptr(), p.to.data_ptr(), p.V, p.T, p.v.data_ptr(), p.t.data_ptr(), w.ptr(),
                                      cum.ptr(), a2max.ptr(), invalid.ptr(), ws.ptr(), nbytes, hip.stream()),
              "cloudaae_mesh_weights")
    torch.cuda.synchronize()
    ws.numpy()
    return dict(weights=w.numpy().view(np.uint64).ravel(), cum=cum.numpy().view(np.uint64).ravel(),
                a2max=a2max.numpy().ravel(), invalid=invalid.numpy().ravel(), cum_dev=cum.view)


def run_sample(hip, p, cum_dev, n, seed, first=0, mesh_ids=None, normals=True):
    L = hip.lib()
    xyzrgb, tri = Guarded(p.S * n, 6, torch.float32, p.dev), Guarded(p.S * n, 1, torch.int32, p.dev)
    normal = Guarded(p.S * n, 3, torch.float64, p.dev) if normals else None
    ids = torch.tensor(mesh_ids, dtype=torch.int32, device=p.dev) if mesh_ids is not None else None
    hip.check(L.cloudaae_mesh_sample(p.S, p.vo.data_ptr(), p.to.data_ptr(), p.V, p.T, p.v.data_ptr(), hip.ptr(p.c),
                                     p.t.data_ptr(), cum_dev.data_ptr(), hip.ptr(ids), n, first, seed, xyzrgb.ptr(), tri.ptr(),
                                     normal.ptr() if normals else None, hip.stream()), "cloudaae_mesh_sample")
    torch.cuda.synchronize()
    out = dict(xyzrgb=xyzrgb.numpy().reshape(p.S, n, 6), tri=tri.numpy().reshape(p.S, n))
    if normals:
        out['normal'] = normal.numpy().reshape(p.S, n, 3)
    return out


def per_mesh(p, values):
    to = p.host[1]
    return [values[to[i]:to[i + 1]] for i in range(p.S)]


# ---- weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, B - 1, B, B + 1, B * B + 1])
def test_weights_of_lattice_meshes_are_exact(hip, dev, T):
    """Three ragged meshes, the middle one empty; the mesh of T triangles starts at packed triangle B + 3, so its blocks
    of the scan straddle the mesh's start, and B * B + 1 takes the scan of the block sums into a second round."""
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    p = Packed([R.lattice(B + 3, seed=1), empty, R.lattice(T, seed=2)], dev)
    got = run_weights(hip, p)
    for i in range(p.S):
        v, t, _ = p.mesh(i)
        want = R.mesh_weights(v, t)
        assert np.array_equal(per_mesh(p, got['weights'])[i], want['weights'])
        assert np.array_equal(per_mesh(p, got['cum'])[i], want['cum'])
        if len(t):
            assert int(per_mesh(p, got['cum'])[i][-1]) == want['W'] > 0
        assert got['invalid'][i] == want['invalid'] == 0 and got['a2max'][i] == want['a2max']
    assert got['a2max'][1] == 0.0


@pytest.fixture(scope="module")
def general(dev):
    ico_v, ico_t = R.icosphere(3)
    ico_c = np.random.default_rng(8).uniform(0, 1, ico_v.shape).astype(np.float32)
    return Packed([(ico_v, ico_t, ico_c), R.soup(200, seed=1, degenerate=True)], dev)


def test_weights_of_general_meshes(hip, general):
    p = general
    assert p.host[1][1] == 1280
    got = run_weights(hip, p)
    differ = 0
    for i in range(p.S):
        v, t, _ = p.mesh(i)
        want = R.mesh_weights(v, t)
        w = per_mesh(p, got['weights'])[i]
        d = np.abs(w.astype(np.int64) - want['weights'].astype(np.int64))
        differ += int((d != 0).sum())
        print("mesh %d: %d of %d weights differ from the restatement (largest difference %d); a2max %r against %r; invalid %d"
              % (i, (d != 0).sum(), len(w), d.max(), got['a2max'][i], want['a2max'], got['invalid'][i]))
        assert d.max() <= 1
        assert got['invalid'][i] == want['invalid']
        assert abs(got['a2max'][i] - want['a2max']) <= np.spacing(want['a2max'])
        # the scan is the exact integer scan of the kernel's own weights
        run, own = 0, []
        for x in w:
            run += int(x)
            own.append(run)
        assert np.array_equal(per_mesh(p, got['cum'])[i], np.array(own, np.uint64))
    w = per_mesh(p, got['weights'])[1]
    assert got['invalid'][1] == 3 and list(w[:4]) == [0, 0, 0, 0] and np.all(w[4:] > 0)     # 2^-40 of the largest: no weight
    print("weights that differ in all: %d" % differ)


# ---- draws ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(dev):
    """Six meshes with colours: a cube, an icosphere, the degenerate soup, a soup without any valid triangle (W = 0),
    a lattice and a plain soup."""
    ico_v, ico_t = R.icosphere(2)
    rng = np.random.default_rng(12)
    sv, st, sc = R.soup(200, seed=1, degenerate=True)
    lv, lt = R.lattice(B + 1, seed=3)
    meshes = [R.cube(), (ico_v, ico_t, rng.uniform(0, 1, ico_v.shape).astype(np.float32)), (sv, st, sc),
              (sv, st[:3], sc), (lv, lt, rng.uniform(0, 1, lv.shape).astype(np.float32)), R.soup(64, seed=6)]
    return Packed(meshes, dev)


@pytest.fixture(scope="module")
def batch_weights(hip, batch):
    return run_weights(hip, batch)


def _ulp32(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_draws_equal_the_restatement(hip, batch, batch_weights, n):
    p, seed, first = batch, 2024, 7
    got = run_sample(hip, p, batch_weights['cum_dev'], n, seed, first)
    unequal = unequal_n = 0
    for i in range(p.S):
        v, t, c = p.mesh(i)
        want = R.sample_mesh(v, t, n, seed, first, mesh_id=i, colors=c, cum=per_mesh(p, batch_weights['cum'])[i])
        assert np.array_equal(got['tri'][i], want['tri'])
        unequal += int((got['xyzrgb'][i].view(np.uint32) != want['xyzrgb'].view(np.uint32)).sum())
        unequal_n += int((got['normal'][i] != want['normal']).sum())
        assert np.all(_ulp32(got['xyzrgb'][i], want['xyzrgb']))
        assert np.abs(got['normal'][i] - want['normal']).max() <= 1e-15
    print("n = %d: %d of %d xyzrgb values and %d of %d normal components differ from the restatement"
          % (n, unequal, got['xyzrgb'].size, unequal_n, got['normal'].size))
    # the mesh without a valid triangle: zeros and -1
    assert np.all(got['tri'][3] == -1) and not got['xyzrgb'][3].any() and not got['normal'][3].any()
    assert got['tri'][2].min() >= 4                                   # the soup's four weightless triangles: never drawn
    # without colours and without normals: the same points, zero colours
    bare = Packed([p.mesh(i)[:2] for i in range(p.S)], p.dev)
    plain = run_sample(hip, bare, batch_weights['cum_dev'], n, seed, first, normals=False)
    assert np.array_equal(plain['xyzrgb'][:, :, :3], got['xyzrgb'][:, :, :3]) and not plain['xyzrgb'][:, :, 3:].any()
    assert np.array_equal(plain['tri'], got['tri'])


def test_draws_do_not_depend_on_the_launch(hip, batch, batch_weights):
    p, seed = batch, 31
    cum = batch_weights['cum_dev']
    one = run_sample(hip, p, cum, 1000, seed, 0)
    again = run_sample(hip, p, cum, 1000, seed, 0)
    a, b = run_sample(hip, p, cum, 300, seed, 0), run_sample(hip, p, cum, 700, seed, 300)
    for k in ('xyzrgb', 'tri', 'normal'):
        assert np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)), k
        assert np.array_equal(one[k].view(np.uint8), np.concatenate([a[k], b[k]], axis=1).view(np.uint8)), k
    # mesh 5 alone under its id
    alone = Packed([p.mesh(5)], p.dev)
    w = run_weights(hip, alone)
    assert np.array_equal(w['cum'], per_mesh(p, batch_weights['cum'])[5])
    got = run_sample(hip, alone, w['cum_dev'], 1000, seed, 0, mesh_ids=[5])
    zero = run_sample(hip, alone, w['cum_dev'], 1000, seed, 0)
    for k in ('xyzrgb', 'tri', 'normal'):
        assert np.array_equal(got[k][0].view(np.uint8), one[k][5].view(np.uint8)), k
    assert not np.array_equal(zero['tri'][0], one['tri'][5])
    # far into the index range and with the largest seed: still the restatement's triangles
    v, t, c = p.mesh(5)
    far = run_sample(hip, alone, w['cum_dev'], 65, (1 << 64) - 1, (1 << 40) - 65, mesh_ids=[(1 << 24) - 1])
    want = R.sample_mesh(v, t, 65, (1 << 64) - 1, (1 << 40) - 65, mesh_id=(1 << 24) - 1, colors=c, cum=w['cum'])
    assert np.array_equal(far['tri'][0], want['tri']) and np.array_equal(far['xyzrgb'][0], want['xyzrgb'])


def test_caller_weights_and_bad_arguments(hip, batch, batch_weights):
    """cum is an input: all the weight on one triangle draws that triangle only; a weight on a triangle whose index
    lies outside its mesh gives zeros and -1 instead of a read past the vertices."""
    L = hip.lib()
    p = Packed([batch.mesh(2)], batch.dev)
    own = np.zeros(p.T, np.uint64)
    own[10:] = 5
    got = run_sample(hip, p, torch.from_numpy(own.view(np.int64)).to(p.dev), 200, 1)
    assert np.all(got['tri'] == 10)
    own[:2], own[2:] = 0, 7                                  # triangle 2 has the out-of-range index
    got = run_sample(hip, p, torch.from_numpy(own.view(np.int64)).to(p.dev), 200, 1)
    assert np.all(got['tri'] == -1) and not got['xyzrgb'].any() and not got['normal'].any()
    own[:] = np.arange(1, p.T + 1, dtype=np.uint64) * np.uint64(3)
    got = run_sample(hip, p, torch.from_numpy(own.view(np.int64)).to(p.dev), 500, 1)
    want = R.sample_mesh(*p.mesh(0)[:2], 500, 1, colors=p.mesh(0)[2], cum=own)
    assert np.array_equal(got['tri'][0], want['tri']) and (want['tri'] == -1).sum() > 0
    assert np.array_equal(got['xyzrgb'][0], want['xyzrgb'])
    x = torch.zeros(64, dtype=torch.int64, device=p.dev)
    args = [p.vo.data_ptr(), p.to.data_ptr(), p.V, p.T, p.v.data_ptr(), None, p.t.data_ptr(), x.data_ptr(), None]
    assert L.cloudaae_mesh_sample(1, *args, 0, 0, 0, x.data_ptr(), x.data_ptr(), None, hip.stream()) != 0
    assert L.cloudaae_mesh_sample(1, *args, 2, (1 << 40) - 1, 0, x.data_ptr(), x.data_ptr(), None, hip.stream()) != 0
    assert L.cloudaae_mesh_sample(0, *args, 2, 0, 0, x.data_ptr(), x.data_ptr(), None, hip.stream()) != 0
    assert L.cloudaae_mesh_sample(1, *args, 2, 0, 0, None, x.data_ptr(), None, hip.stream()) != 0
    assert b"cloudaae_mesh_sample" in L.cloudaae_last_error()
    assert L.cloudaae_mesh_gather_rows(1, 2, None, 1, x.data_ptr(), 1, 1, 4, x.data_ptr(), 1, hip.stream()) != 0
    assert L.cloudaae_mesh_gather_rows(1, 2, None, 4, x.data_ptr(), 1, 1, 2, x.data_ptr(), 1, hip.stream()) != 0
    assert L.cloudaae_mesh_weights(1, p.vo.data_ptr(), p.to.data_ptr(), p.V, p.T, p.v.data_ptr(), p.t.data_ptr(), x.data_ptr(),
                                   x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 8, hip.stream()) != 0


def test_gather_rows(hip, dev):
    from cloudaae_amd.utils import mesh_models as mm
    rng = np.random.default_rng(3)
    src = rng.standard_normal((3, 50, 6)).astype(np.float32)
    idx = rng.integers(0, 50, (3, 17)).astype(np.int32)
    idx[1, 4], idx[2, 0] = -1, 50
    want = np.stack([src[s][np.clip(idx[s], 0, 49)] for s in range(3)])
    want[1, 4], want[2, 0] = 0, 0
    L = hip.lib()
    for dtype, t in ((np.float32, torch.float32), (np.float64, torch.float64)):
        x = torch.from_numpy(src.astype(dtype)).to(dev)
        out = Guarded(3 * 17, 6, t, dev)
        hip.check(L.cloudaae_mesh_gather_rows(3, 17, torch.from_numpy(idx).to(dev).data_ptr(), 50, x.data_ptr(), 6, 6,
                                              x.element_size(), out.ptr(), 6, hip.stream()), "cloudaae_mesh_gather_rows")
        torch.cuda.synchronize()
        assert np.array_equal(out.numpy().reshape(3, 17, 6), want.astype(dtype))
    # a column range through the strides: the first three of six columns into rows of four, the fourth left alone
    x = torch.from_numpy(src).to(dev)
    out = Guarded(3 * 50, 4, torch.float32, dev)
    hip.check(L.cloudaae_mesh_gather_rows(3, 50, None, 50, x.data_ptr(), 6, 3, 4, out.ptr(), 4, hip.stream()),
              "cloudaae_mesh_gather_rows")
    torch.cuda.synchronize()
    got = out.numpy().reshape(3, 50, 4)
    assert np.array_equal(got[:, :, :3], src[:, :, :3]) and np.all(got[:, :, 3].view(np.uint32) == 0xA5A5A5A5)
    assert np.array_equal(mm.gather_rows(x, None, cols=3).cpu().numpy(), src[:, :, :3])


# ---- the model -----------------------------------------------------------------------------------------------------------
def test_model_of_a_cube(hip, dev):
    from cloudaae_amd.utils import mesh_models as mm
    d = mm.models_from_meshes([R.cube()], num_point=2048, oversample=4, seed=77, return_normals=True, device=dev, details=True)
    models, normals, idx = d['models'].cpu().numpy(), d['normals'].cpu().numpy(), d['idx'].cpu().numpy()
    samples, sn = d['samples']['xyzrgb'].cpu().numpy(), d['samples']['normal'].cpu().numpy()
    assert models.shape == (1, 2048, 6) and models.dtype == np.float32 and normals.shape == (1, 2048, 3)
    assert normals.dtype == np.float64 and samples.shape == (1, 8192, 6)
    xyz = models[0, :, :3].astype(np.float64)
    on_face = np.minimum(np.abs(xyz), np.abs(xyz - 1.0)) <= 1e-6
    assert np.all(on_face.any(axis=1)) and xyz.min() >= 0.0 and xyz.max() <= 1.0
    assert np.array_equal(models[0, :, 3:], models[0, :, :3])              # the cube's colours are its coordinates
    # the picked rows: the restated FPS on the kernel's samples, from sample 0
    want = SR.fps(samples[0, :, :3], 2048, 0)
    assert np.array_equal(idx[0], want) and len(set(want.tolist())) == 2048
    assert np.array_equal(models[0], samples[0][idx[0]]) and np.array_equal(normals[0], sn[0][idx[0]])
    # the normals are the faces' axes: one component +-1 along the coordinate that lies on the face, outward
    axis = np.abs(normals[0]).argmax(axis=1)
    assert np.all(np.abs(normals[0]).sum(axis=1) == 1.0) and np.all(on_face[np.arange(2048), axis])
    outward = np.where(xyz[np.arange(2048), axis] > 0.5, 1.0, -1.0)
    assert np.array_equal(normals[0][np.arange(2048), axis], outward)
    assert len(set(axis.tolist())) == 3 and set(outward.tolist()) == {1.0, -1.0}
    # a model is a function of (seed, mesh id): the cube as mesh 1 of a batch and alone under id 1
    ico = R.icosphere(1)
    ico = (ico[0], ico[1], np.zeros_like(ico[0]))
    both = mm.models_from_meshes([ico, R.cube()], num_point=256, oversample=4, seed=5, device=dev)
    alone = mm.models_from_meshes([R.cube()], num_point=256, oversample=4, seed=5, mesh_ids=[1], device=dev)
    assert torch.equal(both[1], alone[0]) and not torch.equal(both[1], both[0])
    with pytest.raises(ValueError):
        mm.models_from_meshes([R.cube(), (R.cube()[0], np.zeros((2, 3), np.int32))], num_point=64, device=dev)


# ---- training --------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, t, c):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue", "element face %d" % len(t),
            "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r %d %d %d" % (tuple(float(x) for x in p) + tuple(int(x) for x in q)) for p, q in zip(v, c)]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


def test_training_on_models_from_meshes(dev, tmp_path, capsys):
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    meshes = tmp_path / "meshes"
    os.makedirs(meshes)
    cv, ct, _ = R.cube()
    iv, it = R.icosphere(2)
    # millimetres, as BOP meshes are: a 10 cm box and a ball of 5 cm radius
    _write_ply(meshes / "obj_000002.ply", (cv - np.float32(0.5)) * np.float32(100.0), ct, np.full((len(cv), 3), 200))
    _write_ply(meshes / "obj_000001.ply", iv * np.float32(50.0), it, np.full((len(iv), 3), 50))
    # the command line: class i is file i in sorted order
    mm.main(["--meshes", str(meshes), "--out", str(tmp_path / "obj_models.tfrecords"), "--scale", "0.001", "--oversample", "2"])
    models, labels = tfrecord_io.read_and_decode_obj_model(str(tmp_path / "obj_models.tfrecords"))
    assert models.shape == (2, 2048, 6) and list(labels) == [0, 1]
    radius = np.linalg.norm(models[:, :, :3], axis=2)
    assert np.all(radius[0] <= 0.05 + 1e-6) and radius[0].min() > 0.045 and radius[1].max() > 0.08
    assert np.allclose(models[0, :, 3:], 50 / 255.0) and np.allclose(models[1, :, 3:], 200 / 255.0)
    capsys.readouterr()

    def run(tag):
        T.main(['--poses', 'sampled', '--meshes', str(meshes), '--mesh_scale', '0.001', '--classes', '0,1', '--steps', '2',
                '--num_point', '256', '--batch_size', '8', '--max_epoch', '1', '--deterministic', '--log_dir',
                str(tmp_path / tag)])
        out = capsys.readouterr().out
        rows = re.findall(r"epoch 0 batch (\d+) xyz_loss (\S+) trans_loss (\S+) axag_loss (\S+)", out)
        assert [int(r[0]) for r in rows] == [0, 1], out[-2000:]
        return rows
    first = run("a")
    print(first)
    assert np.all(np.isfinite(np.array([[float(x) for x in r[1:]] for r in first])))
    assert run("b") == first
