"""CPU: the NumPy restatement of DESIGN.md "Equivalent poses" (tests/pose_equiv_reference.py) against facts that do not
depend on it -- the minimum of the plain geodesic distance over the members, the cubic group's maximal misorientation, the
angle between the axes of an axially symmetric object -- and utils/pose_equiv.py's table: what it makes of find_symmetries
results, its round trip through a save_symmetries file and what it refuses.  The entry point of the C ABI is exported and
rejects bad arguments before it touches memory."""
import math
import os
import re

import numpy as np
import pytest

import pose_equiv_reference as PR

CLASSES = PR.example_classes()
NAME = {n: i for i, n in enumerate(PR.CLASS_NAMES)}


def _run(cls, n, seed, centre_shift=True):
    rng = np.random.default_rng(seed)
    Rp, rp = PR.random_rotations(rng, n)
    Rl, rl = PR.random_rotations(rng, n)
    tl = (rng.standard_normal((n, 3)) * 0.1 + [0.0, 0.0, 0.8]).astype(np.float32)
    out = PR.nearest_equivalent_pose(rp, rl, tl, np.full(n, cls), CLASSES)
    return rp, rl, tl, out


@pytest.mark.parametrize("name", ["trivial", "c2", "cube", "icosahedral", "c64", "duplicate"])
def test_finite_angle_is_the_least_geodesic_distance(name):
    spec = CLASSES[NAME[name]]
    rp, rl, tl, out = _run(NAME[name], 500, 11 + NAME[name])
    G = np.asarray(spec["rot"])
    labels = np.einsum("bij,njk->bnik", out["Rl"], G)                       # Rl G_j
    dist = PR.geodesic(out["Rp"][:, None], labels)                          # [b,n]
    # arccos near 0 loses half the digits: 2e-8 is sqrt(eps) scale; away from 0 the agreement is round-off
    assert np.abs(out["angle"] - dist.min(axis=1)).max() <= 2e-8
    far = dist.min(axis=1) > 0.1
    assert np.abs(out["angle"] - dist.min(axis=1))[far].max() <= 1e-13
    clear = out["gap"] > 1e-9
    assert np.array_equal(out["member"][clear], dist.argmin(axis=1)[clear])
    assert clear.mean() > 0.98 or name == "duplicate"                       # (whose quarter turn ties with its copy)
    assert (out["phi"] == 0.0).all()


def test_the_lower_index_wins_an_exact_tie():
    rp, rl, tl, out = _run(NAME["duplicate"], 400, 5)
    assert set(out["member"].tolist()) == {0, 1, 2}                          # member 3 repeats member 1 and never wins
    assert (out["gap"][out["member"] == 1] == 0.0).all() and (out["member"] == 1).sum() > 50


def test_cube_group_misorientation_bound():
    """No pose is farther than 2 atan(sqrt(23 - 16 sqrt 2)) = 62.7994 degrees from the nearest of the cube's 24."""
    bound = 2.0 * math.atan(math.sqrt(23.0 - 16.0 * math.sqrt(2.0)))
    assert abs(math.degrees(bound) - 62.7994) < 1e-4
    rp, rl, tl, out = _run(NAME["cube"], 100000, 2024)
    worst = float(np.degrees(out["angle"].max()))
    print("largest angle over 1e5 poses: %.4f degrees" % worst)
    assert worst <= 62.80 and worst > 55.0


def test_axial_angle_is_the_angle_between_the_axes():
    rp, rl, tl, out = _run(NAME["axial"], 2000, 3)
    a = CLASSES[NAME["axial"]]["axis"]
    pa, la = out["Rp"] @ a, out["Rl"] @ a
    want = np.arctan2(np.sqrt((np.cross(pa, la) ** 2).sum(axis=1)), (pa * la).sum(axis=1))
    big = want > 0.05
    assert np.abs(out["angle"] - want)[big].max() <= 1e-13 and np.abs(out["angle"] - want).max() <= 2e-8
    assert (out["member"] == 0).all()
    # the closed form is the maximum over phi: a scan never exceeds it, and the chosen phi reaches it
    K = PR.skew(a)
    M = np.einsum("bji,bjk->bik", out["Rp"], out["Rl"])
    s_star = 2.0 * np.cos(out["angle"]) + 1.0
    for ph in np.linspace(-math.pi, math.pi, 181):
        R = np.eye(3) + math.sin(ph) * K + (1.0 - math.cos(ph)) * (K @ K)
        assert (np.einsum("bij,ji->b", M, R) <= s_star + 1e-12).all()
    assert np.abs(np.einsum("bij,bji->b", M, out["S"]) - s_star).max() <= 1e-13


def test_axial_with_flip_is_never_past_a_right_angle():
    rp, rl, tl, out = _run(NAME["axial_flip"], 2000, 4)
    assert out["angle"].max() <= math.pi / 2.0 + 1e-9
    assert set(out["member"].tolist()) == {0, 1}
    a = CLASSES[NAME["axial_flip"]]["axis"]
    pa, la = out["Rp"] @ a, out["Rl"] @ a
    want = np.arccos(np.clip(np.abs((pa * la).sum(axis=1)), 0.0, 1.0))      # a line has no sign
    assert np.abs(out["angle"] - want).max() <= 2e-8


@pytest.mark.parametrize("name", PR.CLASS_NAMES)
def test_the_equivalent_pose_is_the_composed_pose(name):
    rp, rl, tl, out = _run(NAME[name], 300, 40 + NAME[name])
    spec = CLASSES[NAME[name]]
    c = np.zeros(3) if spec["kind"] == "none" else np.asarray(spec["centre"])
    S = out["S"]
    assert np.abs(S @ S.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(S) - 1.0).max() <= 1e-14
    T_label = np.tile(np.eye(4), (len(rl), 1, 1))
    T_label[:, :3, :3], T_label[:, :3, 3] = out["Rl"], tl.astype(np.float64)
    T_sym = np.tile(np.eye(4), (len(rl), 1, 1))
    T_sym[:, :3, :3], T_sym[:, :3, 3] = S, c[None] - S @ c
    T = T_label @ T_sym
    assert np.abs(PR.exp_map(out["rot_equiv"]) - T[:, :3, :3]).max() <= 1e-13
    assert np.abs(out["trans_equiv"] - T[:, :3, 3]).max() <= 1e-15
    assert np.abs(out["trans_equiv32"].astype(np.float64) - T[:, :3, 3]).max() <= 2.0 ** -24 * 1.5
    # the angle left is the distance of the prediction from that pose, and no member is nearer
    dist = PR.geodesic(out["Rp"], T[:, :3, :3])
    assert np.abs(dist - out["angle"]).max() <= 2e-8
    assert (out["angle"] <= PR.geodesic(out["Rp"], out["Rl"]) + 2e-8).all()
    if spec["kind"] == "none":
        assert np.array_equal(out["rot_equiv"], rl) and np.array_equal(out["trans_equiv32"], tl)


def test_log_map_near_a_half_turn_and_at_zero():
    rng = np.random.default_rng(6)
    v = rng.standard_normal((200, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    for theta in (0.0, 1e-9, 1.0, 2.2, math.pi - 1e-3, math.pi - 1e-7, math.pi):
        R = PR.exp_map(v * theta)
        back = PR.log_map(R)
        assert np.abs(PR.exp_map(back) - R).max() <= 1e-13, theta
        assert np.abs(np.sqrt((back * back).sum(axis=1)) - theta).max() <= 1e-7, theta


def test_a_class_id_outside_the_table_is_none():
    rng = np.random.default_rng(8)
    rp, rl = PR.random_axis_angles(rng, 6), PR.random_axis_angles(rng, 6)
    tl = rng.standard_normal((6, 3)).astype(np.float32)
    out = PR.nearest_equivalent_pose(rp, rl, tl, [-1, 9, 99, 3, 0, 2 ** 40], CLASSES)
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(out["rot_equiv"][i], rl[i]) and out["member"][i] == 0 and np.array_equal(out["S"][i], np.eye(3))
    assert not np.array_equal(out["rot_equiv"][3], rl[3]) or out["member"][3] == 0


# ---- utils/pose_equiv.py: the table ---------------------------------------------------------------------------------------
def _result(kind, rot=None, axes=(), centre=(0.0, 0.0, 0.0)):
    from cloudaae_amd.utils import symmetry as S
    rot = np.eye(3)[None] if rot is None else rot
    axes = np.asarray(axes, np.float64).reshape(-1, 3)
    orders = np.array([S.ORDER_STEPS] + [2] * (len(axes) - 1), np.int64)[:len(axes)]
    return dict(kind=kind, transforms=S.about_centre(rot, centre), axes=axes, orders=orders,
                continuous=orders == S.ORDER_STEPS, closed=True, epsilon=0.01, h0=0.001, diameter=0.1,
                centre=np.asarray(centre, np.float64), steps=0)


def _hand_made():
    a = PR.TILTED_AXIS
    f = np.cross(a, [0.0, 0.0, 1.0])
    return [_result("none"),
            _result("finite", PR.cube_group(), [[0, 0, 1.0]], (0.01, 0.0, -0.02)),
            _result("axial", axes=[3.0 * a], centre=(0.0, 0.03, 0.0)),
            _result("axial", axes=[a, 2.0 * f], centre=(0.0, 0.03, 0.01)),
            _result("spherical", axes=[[0, 0, 1.0], [1.0, 0, 0]])]


def test_table_from_results_and_through_a_file(tmp_path):
    from cloudaae_amd.utils import pose_equiv as PE
    from cloudaae_amd.utils import symmetry as S
    results = _hand_made()
    table = PE.SymmetryTable.from_results(results)
    assert table.kinds() == ["none", "finite", "axial", "axial", "none"] and table.num_class == 5
    assert table.index.tolist() == [[0, 0, 0], [1, 0, 24], [2, 24, 0], [2, 24, 1], [0, 0, 0]] and table.num_rot == 25
    assert np.array_equal(table.rot[:24], PR.cube_group()) and np.array_equal(table.centre[1], [0.01, 0.0, -0.02])
    unit = PR.TILTED_AXIS / np.sqrt(PR.TILTED_AXIS @ PR.TILTED_AXIS)
    assert np.abs(table.axis[2] - unit).max() <= 1e-16 and abs(np.sqrt(table.axis[2] @ table.axis[2]) - 1.0) <= 1e-16
    F = table.rot[24]
    assert np.abs(F @ F - np.eye(3)).max() <= 1e-15 and np.abs(F @ table.axis[3] + table.axis[3]).max() <= 1e-15
    # the same table from the file save_symmetries writes; load_symmetries keeps returning the transform sets
    path = str(tmp_path / "symmetries.json")
    S.save_symmetries(path, results)
    again = PE.load_symmetry_table(path)
    for k in ("index", "centre", "axis", "rot"):
        assert np.array_equal(getattr(again, k), getattr(table, k)), k
    wide = PE.load_symmetry_table(path, num_class=21)
    assert wide.num_class == 21 and wide.kinds()[5:] == ["none"] * 16 and np.array_equal(wide.rot, table.rot)
    sets = S.load_symmetries(path)
    assert sorted(sets) == [0, 1, 2, 3, 4] and sets[1].shape == (24, 4, 4)
    # the restatement reads the same table
    index, centre, axis, rot = PR.table_arrays([dict(kind="none"), dict(kind="finite", rot=PR.cube_group(), centre=table.centre[1])])
    assert np.array_equal(index, table.index[:2]) and np.array_equal(rot, table.rot[:24])


def test_table_refuses_what_the_kernel_cannot_take(tmp_path):
    from cloudaae_amd.utils import pose_equiv as PE
    from cloudaae_amd.utils import symmetry as S
    c65 = PR.cyclic_group([0, 0, 1.0], 65)
    with pytest.raises(ValueError, match="limit is 64"):
        PE.SymmetryTable.from_results([_result("finite", c65)])
    assert PE.SymmetryTable.from_results([_result("finite", PR.cyclic_group([0, 0, 1.0], 64))]).index.tolist() == [[1, 0, 64]]
    with pytest.raises(ValueError, match="start with the identity"):
        PE.SymmetryTable.from_results([_result("finite", PR.cube_group()[1:])])
    with pytest.raises(ValueError, match="not zero"):
        PE.SymmetryTable.from_results([_result("axial", axes=[[0.0, 0.0, 0.0]])])
    with pytest.raises(ValueError):
        PE.SymmetryTable.from_results([_result("axial")])                   # no axis at all
    with pytest.raises(ValueError):
        PE.SymmetryTable.from_results([_result("finite", 2.0 * PR.cube_group())])
    with pytest.raises(ValueError):
        PE.SymmetryTable.from_results([_result("none")], num_class=1, classes=[1])
    # the same through a file
    path = str(tmp_path / "bad.json")
    S.save_symmetries(path, [_result("none"), _result("finite", c65)])
    with pytest.raises(ValueError, match="limit is 64"):
        PE.load_symmetry_table(path)
    # and the arrays given directly: an entry that leaves the rotations
    with pytest.raises(ValueError, match="leave"):
        PE.SymmetryTable([[1, 20, 5]], np.zeros((1, 3)), np.zeros((1, 3)), PR.cube_group())
    with pytest.raises(ValueError):
        PE.SymmetryTable([[2, 0, 2]], np.zeros((1, 3)), [[0, 0, 1.0]], PR.cube_group())


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    from cloudaae_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    return _lib.lib()._cdll             # typed from the header, without the recording wrapper


def test_entry_point_is_declared_and_rejects_bad_arguments(cdll):
    from cloudaae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cloudaae_hip.h")).read()
    assert "cloudaae_nearest_equivalent_pose" in header.split("#define CLOUDAAE_ABI_VERSION")[0]
    assert int(re.search(r"#define\s+CLOUDAAE_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    for word, value in (("NONE", PR.NONE), ("FINITE", PR.FINITE), ("AXIAL", PR.AXIAL), ("MAX_MEMBERS", PR.MAX_MEMBERS)):
        assert int(re.search(r"#define\s+CLOUDAAE_SYMMETRY_%s\s+(\d+)" % word, header).group(1)) == value
    decl = re.search(r"int cloudaae_nearest_equivalent_pose\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == len(_lib._SIGNATURES["cloudaae_nearest_equivalent_pose"]) == 18
    # a pointer that would fault if read: every refusal comes before the launch
    p = 0x1000
    good = dict(b=4, rot_pred=p, is64=0, rot_label=p, trans_label=p, class_id=p, num_class=3, index=p, centre=p, axis=p,
                num_rot=5, rot=p, rot_equiv=p, trans_equiv=p, member=p, phi=p, angle=p)

    def call(**kw):
        a = dict(good, **kw)
        return cdll.cloudaae_nearest_equivalent_pose(*(list(a.values()) + [None]))
    for kw in (dict(b=0), dict(b=-1), dict(b=(1 << 24) + 1), dict(is64=2), dict(num_class=0), dict(num_rot=-1),
               dict(rot=None), dict(rot_pred=None), dict(rot_label=None), dict(trans_label=None), dict(class_id=None),
               dict(index=None), dict(centre=None), dict(axis=None), dict(rot_equiv=None), dict(trans_equiv=None),
               dict(member=None), dict(phi=None), dict(angle=None)):
        assert call(**kw) != 0, kw
        assert b"cloudaae_nearest_equivalent_pose" in cdll.cloudaae_last_error(), kw
