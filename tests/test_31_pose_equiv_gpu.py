"""GPU: cloudaae_nearest_equivalent_pose through the C ABI against the NumPy restatement of DESIGN.md "Equivalent poses"
(tests/pose_equiv_reference.py); then its place in the training step and in the evaluation.

The kernel and the restatement take the same float64 operations in the same order; what differs is the last bits of sin,
cos, atan2 and acos.  So the discrete output (member) is compared where the restatement's margin -- the gap between the
best and the second-best trace -- exceeds 1e-9, and the continuous ones to tolerances that are MEASURED, not chosen: the
restatement run in numpy.longdouble against its float64 run on these very inputs, ten times the largest difference per
output with a floor of 1e-12 (the rule of profiles/notes_icp_plane.md).  measured_tolerances() below recomputes them on
the CPU; the constants are what it returned (profiles/notes_pose_equiv.md).  Output buffers sit between guard rows."""
import math

import numpy as np
import pytest
import torch

import pose_equiv_reference as PR

pytestmark = pytest.mark.gpu

GUARD = 4
FILL = 0xA5
GAP = 1e-9                 # member is compared where the best trace leads by more
AXIAL_VALUE = 1e-6         # phi and the rotation are compared where sqrt((tau - alpha)^2 + beta^2) exceeds it
MAX_UNDECIDED = 0.02       # at most this share of the random samples may fall under either
NEAR_CLAMP = 1e-6          # within it of the clamp the angle is compared through its cosine
SEED = 31

# measured_tolerances() on the inputs of this file (in brackets the largest longdouble-against-float64 difference per output;
# ten times each lies under the floor, so every tolerance is the floor):
TOL_ROT = 1e-12            # exp(rot_equiv), entries of the matrix    [9.7e-16]
TOL_TRANS = 1e-12          # trans_equiv before its float32 rounding  [9.1e-17]; one float32 ulp is allowed on top
TOL_PHI = 1e-12            # on the circle                            [1.0e-15]
TOL_ANGLE = 1e-12          # away from the clamp                      [4.9e-14]
TOL_COS = 1e-12            # the clamped cosine                       [5.8e-16]

CLASSES = PR.example_classes()
NAME = {n: i for i, n in enumerate(PR.CLASS_NAMES)}


# ---- the inputs -------------------------------------------------------------------------------------------------------------
def _labels(rng, b):
    return PR.random_rotations(rng, b)[1], (rng.standard_normal((b, 3)) * 0.1 + [0.0, 0.0, 0.8]).astype(np.float32)


def _mixed_ids(b):
    """Every class in turn, and three ids outside the table."""
    ids = np.arange(b) % (len(CLASSES) + 3)
    return np.where(ids == len(CLASSES), -1, np.where(ids == len(CLASSES) + 1, len(CLASSES), np.where(
        ids == len(CLASSES) + 2, 2 ** 40, ids))).astype(np.int64)


def cases():
    """name -> (rot_pred float64 [b,3], rot_label, trans_label, class_id, random): the float32 runs round rot_pred."""
    rng = np.random.default_rng(SEED)
    out = {}
    for name, b, ids in (("one", 1, np.array([NAME["cube"]])), ("five", 5, np.array([3, 4, 7, 8, 0])), ("mixed", 37, _mixed_ids(37)),
                         ("mixed_again", 96, _mixed_ids(96))):
        rl, tl = _labels(rng, b)
        out[name] = (PR.random_rotations(rng, b)[1], rl, tl, ids.astype(np.int64), True)
    ids = np.arange(len(CLASSES), dtype=np.int64)
    rl, tl = _labels(rng, len(ids))
    out["equal"] = (rl.copy(), rl, tl, ids, False)                           # the prediction is the label
    rl0 = rl.copy()
    rl0[3] = 0.0
    out["zero"] = (np.zeros_like(rl), rl0, tl, ids, False)                   # the Taylor branch; one label is zero too
    # a prediction half a turn from every member: Rl R_v(pi) with v perpendicular to the group's axis (none, trivial, C2)
    u = np.array([1.0, 2.0, -1.0])
    v = np.cross(u, [0.3, -0.2, 0.9])
    ids = np.array([NAME["none"], NAME["trivial"], NAME["c2"]] * 2, np.int64)
    rl, tl = _labels(rng, len(ids))
    half = PR.rotation(v, math.pi)
    out["opposite"] = (PR.log_map(PR.exp_map(rl) @ half[None]), rl, tl, ids, False)
    # labels whose equivalent rotation Q is within 1e-3 of a half-turn: Rl = Q S^T for a member S, the prediction near Q
    ids = np.array([NAME["trivial"], NAME["cube"], NAME["icosahedral"], NAME["c64"], NAME["axial"], NAME["axial_flip"]] * 2, np.int64)
    axes = rng.standard_normal((len(ids), 3))
    axes /= np.sqrt((axes * axes).sum(axis=1))[:, None]
    q = axes * (math.pi - rng.uniform(1e-5, 9e-4, (len(ids), 1)))
    Q = PR.exp_map(q)
    Rl = np.empty_like(Q)
    rp = q.copy()
    for i, c in enumerate(ids):
        spec = CLASSES[c]
        if spec["kind"] == "finite":
            S = spec["rot"][int(rng.integers(len(spec["rot"])))]
            rp[i] = q[i] + rng.standard_normal(3) * 0.01
        else:
            S = PR.rotation(spec["axis"], 0.7)
            if spec.get("flip") is not None and i >= 6:
                S = spec["flip"] @ S
        Rl[i] = Q[i] @ S.T
    out["half_turn"] = (rp, PR.log_map(Rl), _labels(rng, len(ids))[1], ids, False)
    return out


def restate(case, is_f64, dtype=np.float64):
    rp, rl, tl, ids, _ = case
    rp = rp if is_f64 else rp.astype(np.float32)
    return rp, PR.nearest_equivalent_pose(rp, rl, tl, ids, CLASSES, dtype)


def _decided(ref, ids):
    """Samples whose member, and whose phi, the restatement decides with a margin; and the exact ties of the class with a
    repeated member, which are decided by the rule (the lower index) and are no accident of the seed."""
    member_ok = ref["gap"] > GAP
    phi_ok = member_ok & (ref["axial_value"] > AXIAL_VALUE)
    return member_ok, phi_ok, (ref["gap"] == 0.0) & (np.asarray(ids) == NAME["duplicate"])


def measured_tolerances():
    """The rule: ten times the largest |longdouble - float64| per output over every input of this file, floor 1e-12.
    Runs on the CPU (python -c 'import test_31_pose_equiv_gpu as t; print(t.measured_tolerances())')."""
    worst = dict(rot=0.0, trans=0.0, phi=0.0, angle=0.0, cos=0.0)
    undecided = total = 0
    for name, case in cases().items():
        for is_f64 in (True, False):
            _, lo = restate(case, is_f64)
            _, hi = restate(case, is_f64, np.longdouble)
            member_ok, phi_ok, tie = _decided(lo, case[3])
            if case[4]:
                undecided += int((~(phi_ok | tie)).sum())
                total += len(phi_ok)
            same = (phi_ok | tie) & (lo["member"] == hi["member"])
            if not same.any():
                continue
            away = same & (np.abs(lo["cos"]) <= PR.CLAMP - NEAR_CLAMP)
            d = lambda k, m: float(np.abs(lo[k][m].astype(np.longdouble) - hi[k][m]).max()) if m.any() else 0.0
            worst["rot"] = max(worst["rot"], float(np.abs(PR.exp_map(lo["rot_equiv"][same]).astype(np.longdouble) -
                                                          PR.exp_map(hi["rot_equiv"][same])).max()))
            worst["trans"] = max(worst["trans"], d("trans_equiv", same))
            worst["phi"] = max(worst["phi"], float(_wrapped(lo["phi"][same].astype(np.longdouble) - hi["phi"][same]).max()))
            worst["angle"] = max(worst["angle"], d("angle", away))
            worst["cos"] = max(worst["cos"], d("cos", same))
    return {k: max(10.0 * v, 1e-12) for k, v in worst.items()}, worst, undecided / max(total, 1)


def _wrapped(d):
    """|d| on the circle."""
    d = np.abs(d) % (2.0 * math.pi)
    return np.minimum(d, 2.0 * math.pi - d)


# ---- the launch ---------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """An output buffer of `rows` rows with GUARD rows of a byte pattern on either side (as in
    tests/test_30_symmetry_gpu.py)."""

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


@pytest.fixture(scope="module")
def table(dev):
    """The test classes as device arrays (index, centre, axis, rot), uploaded once."""
    index, centre, axis, rot = PR.table_arrays(CLASSES)
    return (_d(index, np.int32, dev), _d(centre, np.float64, dev), _d(axis, np.float64, dev), _d(rot, np.float64, dev))


def _outputs(b, dev):
    return dict(rot_equiv=Guarded(b, 3, torch.float64, dev), trans_equiv=Guarded(b, 3, torch.float32, dev),
                member=Guarded(b, 1, torch.int32, dev), phi=Guarded(b, 1, torch.float64, dev),
                angle=Guarded(b, 1, torch.float64, dev))


def launch(hip, dev, table, rp, rl, tl, ids):
    """cloudaae_nearest_equivalent_pose -> dict of NumPy outputs (guards checked)."""
    b = len(rp)
    is_f64 = rp.dtype == np.float64
    g = [_d(rp, rp.dtype, dev), _d(rl, np.float64, dev), _d(tl, np.float32, dev), _d(ids, np.int64, dev)]
    out = _outputs(b, dev)
    hip.check(hip.lib().cloudaae_nearest_equivalent_pose(
        b, g[0].data_ptr(), int(is_f64), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), len(CLASSES), table[0].data_ptr(),
        table[1].data_ptr(), table[2].data_ptr(), int(table[3].shape[0]), table[3].data_ptr(), out["rot_equiv"].ptr(),
        out["trans_equiv"].ptr(), out["member"].ptr(), out["phi"].ptr(), out["angle"].ptr(), hip.stream()),
        "cloudaae_nearest_equivalent_pose")
    torch.cuda.synchronize()
    return {k: (v.numpy() if k in ("rot_equiv", "trans_equiv") else v.numpy().ravel()).copy() for k, v in out.items()}


def compare(got, ref, ids, name):
    """The kernel's outputs against the restatement's; -> the number of samples left undecided."""
    member_ok, phi_ok, duplicate_tie = _decided(ref, ids)                    # an exact tie: the lower index, exactly
    sure = member_ok | duplicate_tie
    assert np.array_equal(got["member"][sure], ref["member"][sure]), (name, got["member"], ref["member"])
    same = (got["member"] == ref["member"]) & (phi_ok | duplicate_tie)
    e = dict(rot=0.0, trans=0.0, phi=0.0, angle=0.0, cos=0.0)
    if same.any():
        e["rot"] = float(np.abs(PR.exp_map(got["rot_equiv"][same]) - PR.exp_map(ref["rot_equiv"][same])).max())
        ulp = np.spacing(np.abs(ref["trans_equiv32"][same])).astype(np.float64)
        over = np.abs(got["trans_equiv"][same].astype(np.float64) - ref["trans_equiv"][same]) - ulp
        e["trans"] = float(max(over.max(), 0.0))
        e["phi"] = float(_wrapped(got["phi"][same] - ref["phi"][same]).max())
    # the angle does not depend on which of two tied members was taken
    near = np.abs(ref["cos"]) > PR.CLAMP - NEAR_CLAMP
    if (~near).any():
        e["angle"] = float(np.abs(got["angle"] - ref["angle"])[~near].max())
    e["cos"] = float(np.abs(np.cos(got["angle"]) - ref["cos"]).max())
    print("%s: b %d undecided %d errors %s" % (name, len(sure), int((~(phi_ok | duplicate_tie)).sum()),
                                              " ".join("%s %.2e" % kv for kv in e.items())))
    assert e["rot"] <= TOL_ROT and e["trans"] <= TOL_TRANS and e["phi"] <= TOL_PHI, (name, e)
    assert e["angle"] <= TOL_ANGLE and e["cos"] <= TOL_COS, (name, e)
    assert np.isfinite(got["rot_equiv"]).all() and np.isfinite(got["trans_equiv"]).all() and np.isfinite(got["angle"]).all()
    return int((~(phi_ok | duplicate_tie)).sum())


@pytest.mark.parametrize("is_f64", [True, False], ids=["f64", "f32"])
def test_kernel_equals_the_restatement(hip, dev, table, is_f64):
    undecided = total = 0
    for name, case in cases().items():
        rp, ref = restate(case, is_f64)
        got = launch(hip, dev, table, rp, case[1], case[2], case[3])
        n = compare(got, ref, case[3], name)
        if case[4]:
            undecided, total = undecided + n, total + len(rp)
        # `none`, a class id outside the table, and S* = I: the labels come back bit for bit
        ids = case[3]
        kept = (ids < 0) | (ids >= len(CLASSES)) | (ids == NAME["none"]) | (ids == NAME["trivial"])
        assert np.array_equal(got["rot_equiv"][kept], case[1][kept]) and np.array_equal(got["trans_equiv"][kept], case[2][kept])
        assert (got["member"][kept] == 0).all() and (got["phi"][kept] == 0.0).all()
        if name == "equal" and is_f64:
            assert (got["member"] == 0).all() and np.array_equal(got["rot_equiv"][:7], case[1][:7])
            assert np.abs(np.cos(got["angle"]) - PR.CLAMP).max() <= TOL_COS
        if name == "opposite":
            assert np.abs(np.cos(got["angle"]) + PR.CLAMP).max() <= TOL_COS
        if name == "half_turn":
            theta = np.sqrt((got["rot_equiv"] ** 2).sum(axis=1))
            assert (np.abs(theta - math.pi) <= 1e-3).all(), theta
    assert total >= 100 and undecided <= MAX_UNDECIDED * total, (undecided, total)


def test_an_exact_tie_goes_to_the_lower_index(hip, dev, table):
    rng = np.random.default_rng(SEED + 1)
    b = 64
    rl, tl = _labels(rng, b)
    rp = PR.random_rotations(rng, b)[1]
    ids = np.full(b, NAME["duplicate"], np.int64)
    ref = PR.nearest_equivalent_pose(rp, rl, tl, ids, CLASSES)
    got = launch(hip, dev, table, rp, rl, tl, ids)
    tied = ref["gap"] == 0.0
    assert tied.sum() >= 8 and (ref["member"][tied] == 1).all()
    assert (got["member"][tied] == 1).all() and (got["member"] != 3).all()
    compare(got, ref, ids, "duplicate")


def test_every_sample_is_independent_of_its_batch(hip, dev, table):
    """One wave per sample: a sample alone gives the bits it gives among 36 others."""
    case = cases()["mixed"]
    whole = launch(hip, dev, table, *case[:4])
    for i in (0, 3, 4, 8, 36):
        one = launch(hip, dev, table, *[a[i:i + 1] for a in case[:4]])
        for k in whole:
            assert np.array_equal(one[k][0], whole[k][i]), (i, k)


def test_argument_errors_write_nothing(hip, dev, table):
    L = hip.lib()
    b = 5
    case = cases()["five"]
    g = [_d(case[0], np.float64, dev), _d(case[1], np.float64, dev), _d(case[2], np.float32, dev), _d(case[3], np.int64, dev)]
    out = _outputs(b, dev)
    good = dict(b=b, rp=g[0].data_ptr(), is64=1, rl=g[1].data_ptr(), tl=g[2].data_ptr(), ids=g[3].data_ptr(), nc=len(CLASSES),
                index=table[0].data_ptr(), centre=table[1].data_ptr(), axis=table[2].data_ptr(), nr=int(table[3].shape[0]),
                rot=table[3].data_ptr(), o0=out["rot_equiv"].ptr(), o1=out["trans_equiv"].ptr(), o2=out["member"].ptr(),
                o3=out["phi"].ptr(), o4=out["angle"].ptr())

    def call(**kw):
        return L.cloudaae_nearest_equivalent_pose(*(list(dict(good, **kw).values()) + [hip.stream()]))
    assert call(b=0) != 0
    assert b"cloudaae_nearest_equivalent_pose" in L.cloudaae_last_error()
    assert call(b=-3) != 0 and call(is64=2) != 0 and call(nc=0) != 0 and call(nr=-1) != 0 and call(rot=None) != 0
    for k in ("rp", "rl", "tl", "ids", "index", "centre", "axis", "o0", "o1", "o2", "o3", "o4"):
        assert call(**{k: None}) != 0, k
    torch.cuda.synchronize()
    for buf in out.values():
        assert np.all(buf.numpy().view(np.uint8) == FILL)                   # nothing was written, guards included
    # a table whose entries leave its rotations is followed nowhere: with no rotations every class with members is `none`
    assert call(nr=0, rot=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out["rot_equiv"].numpy(), case[1]) and np.array_equal(out["trans_equiv"].numpy(), case[2])
    assert (out["member"].numpy().ravel() == 0).all()
    assert call() == 0
    torch.cuda.synchronize()
    ref = PR.nearest_equivalent_pose(*case[:4], CLASSES)
    assert np.array_equal(out["member"].numpy().ravel(), ref["member"])


# ---- against the code that exists -----------------------------------------------------------------------------------------------
def test_the_loss_at_the_equivalent_label_is_the_least_over_the_members(hip, dev):
    """get_rotation_error(rot_pred, rot_equiv) per sample = min over j of get_rotation_error(rot_pred, l_j), the l_j being
    the log maps of Rl G_j computed on the host."""
    from cloudaae_amd.losses.angular_distance_taylor import get_rotation_error
    from cloudaae_amd.utils import pose_equiv as PE
    tab = PE.SymmetryTable(*PR.table_arrays(CLASSES), device=dev)
    rng = np.random.default_rng(SEED + 2)
    for c in (NAME["cube"], NAME["icosahedral"], NAME["c64"]):
        b = 16
        rl, tl = _labels(rng, b)
        rp = PR.random_rotations(rng, b)[1].astype(np.float32)
        ids = np.full(b, c, np.int64)
        near = PE.nearest_equivalent_pose(_d(rp, np.float32, dev), _d(rl, np.float64, dev), _d(tl, np.float32, dev),
                                          _d(ids, np.int64, dev), tab)
        _, per = get_rotation_error(_d(rp, np.float32, dev), near["rot_equiv"])
        G = CLASSES[c]["rot"]
        labels = PR.log_map((PR.exp_map(rl)[:, None] @ G[None]).reshape(-1, 3, 3))              # [b n,3]
        _, every = get_rotation_error(_d(np.repeat(rp, len(G), axis=0), np.float32, dev), _d(labels, np.float64, dev))
        least = every.cpu().numpy().reshape(b, len(G)).min(axis=1)
        per, ang = per.cpu().numpy(), near["angle"].cpu().numpy()
        away = np.cos(least) <= PR.CLAMP - NEAR_CLAMP
        print("class %d: |per - least| %.2e |angle - least| %.2e" % (c, np.abs(per - least)[away].max(), np.abs(ang - least)[away].max()))
        assert np.abs(per - least)[away].max() <= TOL_ANGLE and np.abs(ang - least)[away].max() <= TOL_ANGLE
        assert np.abs(np.cos(per) - np.cos(least)).max() <= TOL_COS


def _graph_table(dev):
    """A table over the training graph's 21 classes: the test classes in turn."""
    from cloudaae_amd.utils import pose_equiv as PE
    return PE.SymmetryTable(*PR.table_arrays([CLASSES[c % len(CLASSES)] for c in range(21)]), device=dev)


def _elements(T, B, N, dev, n, seed):
    els = [T.synthetic_element(B, N, dev, seed=seed + i) for i in range(n)]
    for i, el in enumerate(els):
        el["noise"] = torch.randn((B, N, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(seed + i)) * 0.001
        el["class_id"] = torch.arange(B, device=dev, dtype=torch.int64) * 2 % 9 + (i % 2)         # several kinds in a batch
    return els


def _same_step(oa, ob, a, b, where):
    for k in ("xyz_loss", "trans_loss", "axag_loss", "total_loss"):
        assert float(oa[k].detach()) == float(ob[k].detach()), (where, k)
    assert torch.equal(oa["axag_loss_perSample"], ob["axag_loss_perSample"]), where
    assert torch.equal(a.store.flat_params, b.store.flat_params), where
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v), where
    assert torch.equal(a.store.flat_state, b.store.flat_state), where


@pytest.mark.parametrize("replay,steps", [(False, 1), (True, 3)], ids=["eager", "replayed"])
def test_the_step_trains_on_the_equivalent_labels(hip, dev, replay, steps):
    """Graph A has the table and the element's labels; graph B has none and is given A's reported equivalent labels: the
    same losses and the same parameters, bit for bit -- also replayed, with labels that change between the replays."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    B, N = 4, 128
    tab = _graph_table(dev)
    mk = lambda sym: T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=replay, deterministic=True,
                                  symmetries=sym)
    a, b_ = mk(tab), mk(None)
    assert torch.equal(a.store.flat_params, b_.store.flat_params)
    members = []
    for step, el in enumerate(_elements(T, B, N, dev, steps, 310)):
        oa = a.train_step(el)
        torch.cuda.synchronize()
        moved = dict(el, axisangle=oa["axisangle_equiv"].clone(), translation=oa["translation_equiv"].clone())
        ob = b_.train_step(moved)
        torch.cuda.synchronize()
        _same_step(oa, ob, a, b_, step)
        assert oa["axisangle_equiv"].dtype == torch.float64 and oa["translation_equiv"].dtype == torch.float32
        assert oa["symmetry_member"].dtype == torch.int32 and oa["symmetry_phi"].dtype == torch.float64
        assert not torch.equal(oa["axisangle_equiv"], el["axisangle"].to(torch.float64))           # something was moved
        assert "axisangle_equiv" not in ob
        members.append((oa["symmetry_member"].cpu().tolist(), oa["axisangle_equiv"].cpu().clone()))
        # the reported labels are those of the definition for the reported prediction
        ref = PR.nearest_equivalent_pose(oa["rot_pred"].detach().cpu().numpy(), el["axisangle"].cpu().numpy(),
                                         el["translation"].cpu().numpy(), el["class_id"].cpu().numpy(),
                                         [CLASSES[c % len(CLASSES)] for c in range(21)])
        sure = ref["gap"] > GAP
        assert np.array_equal(np.asarray(members[-1][0])[sure], ref["member"][sure])
    if replay:
        assert a.replay and a._plan is not None and not a._plan.foreign_ops and not b_._plan.foreign_ops
        assert len(a._plan.entries) == len(b_._plan.entries) + 1                                    # the one launch
        assert not torch.equal(members[0][1], members[1][1]) and not torch.equal(members[1][1], members[2][1])
    assert float(a.batch) == float(steps)
    b_.deterministic = False
    b_._set_mode()                                                           # (the ordinary mode for the tests that follow)


def test_without_a_table_nothing_changes(hip, dev):
    from cloudaae_amd import train_cloudAAE_ycbv as T
    B, N = 4, 128
    a = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=True, deterministic=True, symmetries=None)
    b_ = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B}, replay=True, deterministic=True)
    for step, el in enumerate(_elements(T, B, N, dev, 2, 320)):
        oa, ob = a.train_step(el), b_.train_step(el)
        torch.cuda.synchronize()
        _same_step(oa, ob, a, b_, step)
        assert set(oa) == set(ob) and "axisangle_equiv" not in oa
    assert len(a._plan.entries) == len(b_._plan.entries)
    b_.deterministic = False
    b_._set_mode()


def test_evaluation_reports_the_errors_against_the_equivalent_labels(hip, dev):
    from cloudaae_amd import evaluate_cloudAAE_ycbv as E
    from cloudaae_amd import train_cloudAAE_ycbv as T
    B, N = 6, 128
    g = torch.Generator().manual_seed(77)
    t = torch.rand((B, 3), generator=g) * torch.tensor([0.5, 0.5, 1.0]) + torch.tensor([-0.25, -0.25, 0.5])
    axag = torch.from_numpy(PR.random_rotations(np.random.default_rng(77), B)[1])
    ids = torch.tensor([NAME["none"], NAME["cube"], NAME["axial"], NAME["axial_flip"], NAME["icosahedral"], 20])
    el = dict(xyz_inlier=torch.randn((B, N + 9, 3), generator=g) * 0.05 + t[:, None, :],
              visiblePoints_org=torch.randn((B, 4 * N, 3), generator=g) * 0.05 + t[:, None, :], class_id=ids,
              translation=t.clone(), axisangle=axag, obj_batch=torch.randn((B, 300, 3), generator=g) * 0.05)
    el = {k: v.to(dev) for k, v in el.items()}
    classes = [CLASSES[c] if c < len(CLASSES) else dict(kind="none") for c in range(21)]
    from cloudaae_amd.utils import pose_equiv as PE
    tab = PE.SymmetryTable(*PR.table_arrays(classes), device=dev)
    graph = T.TrainGraph({"num_point": N, "gpu": 0}, {}, {"batch_size": B})
    plain = E.evaluate_batch(graph, el, icp=True)
    aware = E.evaluate_batch(graph, el, icp=True, symmetries=tab)
    new = {"%s%s_sym" % (k, tag) for k in ("axag_loss", "trans_loss", "axag_loss_perSample", "trans_loss_perSample")
           for tag in ("", "_icp")}
    assert set(aware) - set(plain) == new, sorted(set(aware) - set(plain))
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, aware[k]), k
    for tag in ("", "_icp"):
        per, sym = aware["axag_loss_perSample" + tag], aware["axag_loss_perSample%s_sym" % tag]
        print("rotation errors%s %s -> %s" % (tag, per.tolist(), sym.tolist()))
        assert (sym <= per).all() and (sym[1:5] < per[1:5]).any()
        assert torch.equal(sym[0], per[0]) and torch.equal(sym[5], per[5])                          # kind none
        tper, tsym = aware["trans_loss_perSample" + tag], aware["trans_loss_perSample%s_sym" % tag]
        assert torch.equal(tsym[0], tper[0]) and torch.equal(tsym[5], tper[5])
        assert abs(float(aware["axag_loss%s_sym" % tag]) - float(sym.mean())) <= 1e-6
    # replayed: the same bits, twice
    again = E.evaluate_batch(graph, el, icp=True, symmetries=tab, replay=True)
    again = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in again.items()}
    once_more = E.evaluate_batch(graph, el, icp=True, symmetries=tab, replay=True)
    for k in new:
        assert torch.equal(again[k], aware[k]) and torch.equal(once_more[k], aware[k]), k
