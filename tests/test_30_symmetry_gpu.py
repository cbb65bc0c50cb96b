"""GPU: cloudaae_transform_hausdorff through the C ABI against the NumPy restatement of DESIGN.md "Object symmetries"
(tests/symmetry_reference.py), bit for bit; then utils/symmetry.py by its outcome on small analytic meshes, and the
effect of the found sets on MSSD and on the evaluation.

The score has no summation: minima and maxima of fp64 expressions written in the definition's order and one correctly
rounded square root, so every comparison with the restatement is an equality of the float64 bits.  Outputs sit between
guard rows.  The kernel's tiles: 128 queries and 4 candidates per workgroup, 1024 targets per LDS tile."""
import json
import math
import os

import numpy as np
import pytest
import torch

import symmetry_reference as SR

pytestmark = pytest.mark.gpu

GUARD = 4
FILL = 0xA5
R_GROUP = 4                # candidates of a workgroup (csrc/symmetry.hip)
LDS_TILE = 1024            # targets staged at a time
TARGETS, QUERIES = 4096, 512


class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_26_bop_score_gpu.py)."""

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


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _d(a, ty, dev):
    return torch.from_numpy(np.ascontiguousarray(a, ty)).to(dev)


def launch(hip, dev, q, t, T, limit2, ws=None, out=None):
    """cloudaae_transform_hausdorff on rows as given (their last dimension is the stride) -> ([c] float64, workspace)."""
    L = hip.lib()
    c = len(T)
    g = [_d(q, np.float32, dev), _d(t, np.float32, dev), _d(T, np.float64, dev)]
    out = out or Guarded(c, 1, torch.float64, dev)
    assert int(L.cloudaae_transform_hausdorff_workspace_bytes(c)) == 8 * c
    ws = ws or Guarded(c, 1, torch.int64, dev)
    hip.check(L.cloudaae_transform_hausdorff(c, len(q), g[0].data_ptr(), q.shape[1], len(t), g[1].data_ptr(), t.shape[1],
                                             g[2].data_ptr(), float(limit2), out.ptr(), ws.ptr(), hip.stream()),
              "cloudaae_transform_hausdorff")
    torch.cuda.synchronize()
    ws.numpy()
    return out.numpy().ravel().copy(), ws


def _poses(rng, c, spread=0.3):
    T = np.tile(np.eye(4), (c, 1, 1))
    for i in range(c):
        T[i, :3, :3] = SR.rotation(rng.standard_normal(3), rng.uniform(0.0, spread))
        T[i, :3, 3] = rng.standard_normal(3) * 0.02 * spread
    return T


def _same_bits(got, want):
    return torch.equal(torch.from_numpy(got.copy()).view(torch.int64), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int64))


# m, n, c, row length: one point each; partial tiles on both sides; one target more than an LDS tile; a single candidate, a
# partial candidate group and 257; rows of six floats
SHAPES = [(1, 1, 1, 3), (129, 65, R_GROUP + 1, 3), (70, LDS_TILE + 1, 3, 3), (257, 300, 257, 6), (64, 2 * LDS_TILE + 7, 1, 6)]


@pytest.mark.parametrize("m,n,c,row", SHAPES)
def test_kernel_equals_the_restatement(hip, dev, m, n, c, row):
    rng = np.random.default_rng(1000 * m + n + c)
    q = (rng.standard_normal((m, row)) * 0.05).astype(np.float32)
    t = (rng.standard_normal((n, row)) * 0.05).astype(np.float32)
    t[n // 2, :3] = q[m // 2, :3]                                   # a query equal to a target
    T = _poses(rng, c)
    T[0] = np.eye(4)
    h2 = SR.squared_hausdorff(q, t, T)
    want = np.sqrt(h2)
    got, ws = launch(hip, dev, q, t, T, np.inf)
    print("m %d n %d c %d: %d of %d differ; score 0 %r" % (m, n, c, int((got != want).sum()), c, float(got[0])))
    assert _same_bits(got, want) and np.isfinite(got).all()
    if m == 1:
        assert (got[0] == 0.0) == (n == 1)
    # limit2 equal to one candidate's H2 exactly: that one stays finite, the larger ones do not
    k = int(np.argsort(h2)[len(h2) // 2])
    got_k, _ = launch(hip, dev, q, t, T, h2[k], ws=ws)              # the same workspace again
    assert _same_bits(got_k, SR.hausdorff_scores(q, t, T, h2[k])) and np.isfinite(got_k[k])
    assert int(np.isinf(got_k).sum()) == int((h2 > h2[k]).sum())
    got_0, _ = launch(hip, dev, q, t, T, 0.0, ws=ws)
    assert _same_bits(got_0, SR.hausdorff_scores(q, t, T, 0.0)) and int(np.isfinite(got_0).sum()) == int((h2 == 0.0).sum())
    again, _ = launch(hip, dev, q, t, T, np.inf, ws=ws)
    assert _same_bits(again, want)


def test_zero_distance_and_the_wrapper(hip, dev):
    """Queries that are targets under the identity score exactly 0; the wrapper takes strided rows, an array of
    transforms and a limit in metres."""
    from cloudaae_amd.utils import symmetry as S
    rng = np.random.default_rng(30)
    t = (rng.standard_normal((200, 6)) * 0.05).astype(np.float32)
    q = t[::3].copy()
    T = _poses(rng, 9)
    T[4] = np.eye(4)
    want = SR.hausdorff_scores(q, t, T)
    limit = float(np.sort(want)[5])
    got = S.hausdorff_scores(_d(q, np.float32, dev), _d(t, np.float32, dev)[:, :3], T, limit).cpu().numpy()
    assert want[4] == 0.0 and _same_bits(got, SR.hausdorff_scores(q, t, T, limit * limit))
    assert np.isfinite(got).sum() in (5, 6)                          # limit * limit against H2: the sixth by rounding


def test_argument_errors_write_nothing(hip, dev):
    L = hip.lib()
    q, t = _d(np.zeros((8, 3)), np.float32, dev), _d(np.ones((5, 3)), np.float32, dev)
    T = _d(np.tile(np.eye(4), (2, 1, 1)), np.float64, dev)
    out, ws = Guarded(2, 1, torch.float64, dev), Guarded(2, 1, torch.int64, dev)
    wb = L.cloudaae_transform_hausdorff_workspace_bytes
    assert wb(1) == 8 and wb(1 << 20) == 8 << 20 and wb(0) == -1 and wb((1 << 20) + 1) == -1

    def call(c=2, m=8, qs=3, n=5, ts=3, qp=q.data_ptr(), tp=t.data_ptr(), Tp=T.data_ptr(), limit2=np.inf, o=out.ptr(),
             w=ws.ptr()):
        return L.cloudaae_transform_hausdorff(c, m, qp, qs, n, tp, ts, Tp, limit2, o, w, hip.stream())
    assert call(c=0) != 0
    assert b"cloudaae_transform_hausdorff" in L.cloudaae_last_error()
    assert call(c=(1 << 20) + 1) != 0 and call(m=0) != 0 and call(n=0) != 0 and call(m=(1 << 24) + 1) != 0
    assert call(qs=2) != 0 and call(ts=2) != 0
    assert call(qp=None) != 0 and call(tp=None) != 0 and call(Tp=None) != 0 and call(o=None) != 0 and call(w=None) != 0
    assert call(limit2=-1.0) != 0 and call(limit2=float("nan")) != 0
    torch.cuda.synchronize()
    for buf in (out, ws):
        assert np.all(buf.numpy().view(np.uint8) == FILL)            # nothing was written, guards included
    assert call() == 0
    torch.cuda.synchronize()
    assert out.numpy().ravel().tolist() == [math.sqrt(3.0)] * 2      # (0,0,0) against (1,1,1)


# ---- the search ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def found(hip, dev):
    """find_symmetries of the five solids, as meshes through mesh_models, in one batch of draws."""
    from cloudaae_amd.utils import symmetry as S
    meshes = [SR.solid(name)[:2] for name in SR.SOLIDS]
    results = S.symmetries_of_meshes(meshes, num_targets=TARGETS, num_queries=QUERIES, device=dev)
    for name, r in zip(SR.SOLIDS, results):
        print("%s: kind %s transforms %d orders %s closed %s epsilon %.5f h0 %.5f steps %d"
              % (name, r["kind"], len(r["transforms"]), r["orders"].tolist(), r["closed"], r["epsilon"], r["h0"], r["steps"]))
    return dict(zip(SR.SOLIDS, results))


@pytest.mark.parametrize("name", ["box", "square_prism", "tri_prism", "l_solid"])
def test_finite_groups_are_found_member_by_member(found, name):
    r = found[name]
    v, t, group, centre, axis = SR.solid(name)
    T = r["transforms"]
    assert T.dtype == np.float64 and np.array_equal(T[0], np.eye(4))
    assert len(T) == SR.EXPECTED_COUNT[name], (name, len(T), r["orders"])
    assert r["kind"] == ("none" if name == "l_solid" else "finite") and r["closed"]
    dist = SR.angles_deg(T[:, :3, :3], group)
    match = dist.argmin(axis=1)
    print("%s: rotation distance to the matched element, degrees: %s" % (name, np.round(dist.min(axis=1), 3).tolist()))
    assert sorted(match.tolist()) == list(range(len(group)))          # one to one
    assert dist.min(axis=1).max() <= 3.0
    # every member keeps the centre where the sample's centroid is
    assert np.abs(np.einsum("nij,j->ni", T[:, :3, :3], r["centre"]) + T[:, :3, 3] - r["centre"]).max() < 1e-12
    assert np.abs(r["centre"] - centre).max() < 0.005


def test_cylinder_is_axial(found):
    r = found["cylinder"]
    v, t, group, centre, axis = SR.solid("cylinder")
    assert r["kind"] == "axial" and r["continuous"].tolist() == [True, False] and r["orders"].tolist() == [120, 2]
    tilt = math.degrees(math.acos(min(1.0, abs(float(r["axes"][0] @ axis)))))
    print("cylinder: axis off by %.3f degrees, %d steps" % (tilt, r["steps"]))
    assert tilt <= 2.0
    assert abs(float(r["axes"][1] @ r["axes"][0])) < 1e-12            # the half-turn's axis is perpendicular
    n = r["steps"]
    assert len(r["transforms"]) == 2 * n and np.array_equal(r["transforms"][0], np.eye(4))
    # r_max is the farthest target from the FOUND axis through the FOUND centre: at least the 24-gon's inradius, at most
    # the radius plus what the axis' tilt (over the half-height) and the centre's offset add; n grows with r_max
    half, radius = SR.CYLINDER[0], SR.CYLINDER[1]
    lo = radius * math.cos(math.pi / SR.CYLINDER[2])
    hi = radius + half * math.sin(math.radians(tilt)) + float(np.linalg.norm(r["centre"] - centre))
    assert SR.discretisation_count(lo, r["diameter"]) <= n <= SR.discretisation_count(hi, r["diameter"])
    flips = SR.angles_deg(r["transforms"][n:, :3, :3], np.eye(3)[None]).ravel()
    assert np.allclose(flips, 180.0, atol=1e-5)


# ---- what it changes ---------------------------------------------------------------------------------------------------------
def test_quarter_turn_of_the_square_prism_scores_as_correct(hip, dev, found):
    from cloudaae_amd.utils import bop_score as B
    from cloudaae_amd.utils import symmetry as S
    r = found["square_prism"]
    v, t, group, centre, axis = SR.solid("square_prism")
    model = _d(SR.sample_surface(v, t, 1024, 7)[None], np.float32, dev)
    G = np.eye(4)
    G[:3, :3] = SR.rotation((0.3, -0.5, 0.8), 0.9)
    G[:3, 3] = (0.05, -0.02, 0.9)
    quarter = SR.about(group[1], centre)                               # the prism's true quarter-turn
    est = _d((G @ quarter)[None], np.float64, dev)
    gt = _d(G[None], np.float64, dev)
    plain = float(B.mssd_mspd(model, est, gt, symmetries=None)["mssd"][0, 0])
    aware = float(B.mssd_mspd(model, est, gt, symmetries=[r["transforms"]])["mssd"][0, 0])
    print("square prism: MSSD %.5f without the set, %.5f with it; diameter %.4f" % (plain, aware, r["diameter"]))
    assert plain > 0.3 * r["diameter"]
    assert aware < S.TOL * r["diameter"] + r["h0"]


def _write_ply(path, v, t):
    rows = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
            "element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    rows += ["%r %r %r" % tuple(float(x) for x in p) for p in v]
    rows += ["3 %d %d %d" % tuple(f) for f in t]
    with open(path, "w") as fh:
        fh.write("\n".join(rows) + "\n")


def test_command_line_file_changes_only_mssd_and_mspd(hip, dev, tmp_path, capsys):
    """Two meshes (the L-shaped solid, the square prism), four rendered frames as in tests/test_26_bop_score_gpu.py; the
    JSON the command line writes goes through load_symmetries into evaluate_batch(bop=...)."""
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd import train_cloudAAE_ycbv as T
    from cloudaae_amd.utils import mesh_models as mm
    from cloudaae_amd.utils import pose_score, render
    from cloudaae_amd.utils import symmetry as S
    os.makedirs(str(tmp_path / "meshes"))
    for i, name in enumerate(("l_solid", "square_prism")):
        v, t = SR.solid(name)[:2]
        _write_ply(str(tmp_path / "meshes" / ("obj_%06d.ply" % (i + 1))), (v - SR.MOTION_T.astype(np.float32)) * np.float32(1000.0), t)
    out_json = str(tmp_path / "symmetries.json")
    assert S.main(["--meshes", str(tmp_path / "meshes"), "--mesh_scale", "0.001", "--out", out_json]) == 0
    printed = capsys.readouterr().out
    assert "symmetry class 0 kind none transforms 1 " in printed and "symmetry class 1 kind finite transforms 8 " in printed
    sets = S.load_symmetries(out_json)
    assert sorted(sets) == [0, 1] and sets[0].shape == (1, 4, 4) and sets[1].shape == (8, 4, 4)
    data = json.load(open(out_json))["classes"]
    assert data[1]["kind"] == "finite" and sorted(data[1]["orders"]) == [2, 2, 2, 2, 4] and data[1]["name"] == "obj_000002.ply"

    render.main(["--meshes", str(tmp_path / "meshes"), "--out", str(tmp_path / "data"), "--frames", "4", "--objects", "2",
                 "--seq", "48", "--seed", "11", "--mesh_scale", "0.001", "--width", "160", "--height", "120"])
    files = mm.mesh_files(str(tmp_path / "meshes"))
    models = mm.models_from_meshes(files, scale=0.001, oversample=2, device=dev)
    packed = mm.pack_meshes(files, 0.001, dev)
    frames = tfrecord_io.read_frames(str(tmp_path / "data" / "0048_pcnn.tfrecord"), verify=True)
    N = 128
    el = E.element_from_frames(frames, 1, N, models, seed=4, device=dev, keep_frames=True)
    assert el is not None
    B = len(el['class_id'])
    diam = pose_score.model_diameter(models[:, :, :3].contiguous())
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    tensors = {k: v for k, v in el.items() if isinstance(v, torch.Tensor)}
    bop = dict(meshes=packed, mesh_index=None, diameters=diam)
    plain = E.evaluate_batch(graph, tensors, bop=dict(bop))
    aware = E.evaluate_batch(graph, tensors, bop=dict(bop, symmetries=sets))
    assert set(plain) == set(aware)
    for k, a in plain.items():
        if k.startswith(("mssd_", "mspd_")) or not isinstance(a, torch.Tensor):
            continue
        assert torch.equal(a, aware[k]), k
    print("mssd %s -> %s" % (plain["mssd_pred"].tolist(), aware["mssd_pred"].tolist()))
    assert (aware["mssd_pred"] <= plain["mssd_pred"]).all() and (aware["mspd_pred"] <= plain["mspd_pred"]).all()
    # the identity alone is what None gives
    same = E.evaluate_batch(graph, tensors, bop=dict(bop, symmetries={1: np.eye(4)[None]}))
    assert torch.equal(same["mssd_pred"], plain["mssd_pred"]) and torch.equal(same["mspd_pred"], plain["mspd_pred"])
