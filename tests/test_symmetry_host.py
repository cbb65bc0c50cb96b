"""CPU: the NumPy restatement of DESIGN.md "Object symmetries" (tests/symmetry_reference.py) and the host side of
cloudaae_amd/utils/symmetry.py, anchored on cases worked by hand; then the margins of the acceptance rule on the test
solids, which is what lets tests/test_30_symmetry_gpu.py ask for exact member counts.

Margins, as measured with the restatement (4096 targets, 512 queries, the seeds below; epsilon = h0 + 0.02 diameter):
    box 0.10 / 0.075 / 0.05         true <= 0.64 epsilon, far >= 1.44 epsilon
    square prism 0.10, 0.07         true <= 0.66 epsilon, far >= 1.38 epsilon
    triangular prism 0.07, 0.08     true <= 0.66 epsilon, far >= 1.59 epsilon
    L-shaped solid                  (identity alone)      far >= 2.18 epsilon
    cylinder 0.08, 0.05             true <= 0.66 epsilon  (its ring of half-turn axes defeats "far from the group")
The box first planned (0.1 / 0.05 / 0.025) was replaced by a less flat one: a turn of 15 degrees about its long axis lifts a
corner of the 0.05 x 0.025 section by 0.012 m only, which is epsilon itself.  The square prism's half-edge went from
0.06 to 0.07 for the same reason (far 1.13 epsilon at 0.06 with one of three seeds).  h0 is the maximum of 512 nearest
distances and varies by a quarter from seed to seed; with an unlucky draw (h0 0.0111 instead of 0.0085) the square
prism's far margin falls to 1.02, so the seeds here are fixed and the GPU test does not rest on the far margin: the
order sweep and the sharpening decide there.
"""
import math

import numpy as np
import pytest

import symmetry_reference as SR
from cloudaae_amd.utils import symmetry as S

TARGETS, QUERIES = 4096, 512               # what tests/test_30_symmetry_gpu.py draws from the meshes
TARGET_SEED, QUERY_SEED = 101, 201
HALF = (0.3, 0.2, 0.1)                     # the hand-worked box's half-edges


def _corners():
    return np.array([[sx * HALF[0], sy * HALF[1], sz * HALF[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)],
                    np.float32)


def _half_turn(axis):
    T = np.eye(4)
    for k in range(3):
        if k != axis:
            T[k, k] = -1.0                 # exact: a permutation of the corners with signs
    return T


def test_corners_of_a_box_under_its_half_turns_score_zero():
    p = _corners()
    T = np.stack([_half_turn(a) for a in range(3)])
    assert np.array_equal(SR.squared_hausdorff(p, p, T), np.zeros(3))
    assert np.array_equal(SR.hausdorff_scores(p, p, T, 0.0), np.zeros(3))      # limit2 = 0 keeps an exact hit


def test_quarter_turn_by_hand_and_the_limit():
    """A quarter-turn about z sends the corner (x, y, z) to (-y, x, z): (0.3, 0.2) -> (-0.2, 0.3), whose nearest corner
    is (-0.3, 0.2) at squared distance 0.1^2 + 0.1^2; every corner is as far.  The float32 coordinates widened are not
    the decimal ones, so the expected value is formed from them in the definition's order."""
    p = _corners()
    a, b = float(np.float32(0.3)), float(np.float32(0.2))
    T = np.eye(4)
    T[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    dx, dy = -b - (-a), a - b
    h2 = dx * dx + dy * dy
    assert abs(h2 - 0.02) < 1e-7
    got = SR.squared_hausdorff(p, p, T[None])
    assert got[0] == h2
    assert SR.hausdorff_scores(p, p, T[None], h2)[0] == math.sqrt(h2)          # limit2 = H2 exactly: finite
    assert SR.hausdorff_scores(p, p, T[None], np.nextafter(h2, 0.0))[0] == np.inf
    assert SR.hausdorff_scores(p, p, T[None], np.nextafter(h2, 1.0))[0] == math.sqrt(h2)
    fast = SR.hausdorff_scores_fast(p, p, T[None])
    assert fast[0] == math.sqrt(h2)


def test_order_rule_on_hand_made_masks():
    L = SR.ORDER_STEPS
    for rule in (SR.order_from_mask, S.order_from_mask):
        none = np.zeros(L - 1, bool)
        assert rule(none) == 1
        assert rule(np.ones(L - 1, bool)) == L                                 # every angle: a continuous axis
        half = none.copy()
        half[60 - 1] = True
        assert rule(half) == 2
        near = half.copy()
        near[[58, 60]] = True                                                  # 177 and 183 degrees pass too: still 2
        assert rule(near) == 2
        quarter = none.copy()
        quarter[[29, 59, 89]] = True
        assert rule(quarter) == 4
        quarter[59] = False                                                    # a quarter-turn without its square: none
        assert rule(quarter) == 1
        third = none.copy()
        third[[39, 79]] = True
        assert rule(third) == 3
        six = none.copy()
        six[[19, 39, 59, 79, 99]] = True
        assert rule(six) == 6
        six[19] = False                                                        # 60 degrees fails: orders 2 and 3 remain, 3 wins
        assert rule(six) == 3
        almost = np.ones(L - 1, bool)
        almost[6] = False                                                      # 21 degrees fails: every even step still passes
        assert rule(almost) == 60


def test_discretisation_count():
    for rule in (SR.discretisation_count, S.discretisation_count):
        # r_max 0.05, diameter 0.2, 1 %: 2 * 0.05 * sin(pi / n) <= 0.002  <=>  n >= pi / asin(0.02) = 157.07
        assert rule(0.05, 0.2, 0.01) == 158
        assert 2 * 0.05 * math.sin(math.pi / 158) <= 0.002 < 2 * 0.05 * math.sin(math.pi / 157)
        assert rule(0.001, 0.2, 0.01) == 2                                     # a needle: the half-turn is enough
        assert rule(0.1, 0.2, 1.0) == 2 and rule(0.1, 0.2, 0.9) == 3      # sin(pi / 3) = 0.866
    assert S.discretisation_count(0.0, 0.2) == 2


def test_rotation_helpers_agree_with_the_restatement():
    rng = np.random.default_rng(3)
    axes = rng.standard_normal((5, 3))
    ang = rng.uniform(0.3, 3.0, 5)
    c = np.array([0.1, -0.2, 0.3])
    T = S.rotations_about(axes, ang, c)
    for i in range(5):
        want = SR.about(SR.rotation(axes[i], ang[i]), c)
        assert np.allclose(T[i], want, atol=1e-15)
        a = S.rotation_axis(T[i, :3, :3])
        assert np.allclose(a, axes[i] / np.linalg.norm(axes[i]), atol=1e-12)
    half = S.rotations_about(axes[0], math.pi, c)[0, :3, :3]                   # no skew part: the line, either sign
    assert abs(abs(float(S.rotation_axis(half) @ axes[0]) / np.linalg.norm(axes[0])) - 1.0) < 1e-12
    assert np.allclose(S.rotation_distance_deg(T[:, :3, :3], T[:, :3, :3]).diagonal(), 0.0, atol=1e-5)
    assert abs(S.rotation_distance_deg(np.eye(3)[None], T[:1, :3, :3])[0, 0] - math.degrees(ang[0])) < 1e-9
    assert np.array_equal(S.fibonacci_hemisphere(64), SR.fibonacci_hemisphere(64))
    assert S.is_closed(np.stack([_half_turn(a)[:3, :3] for a in range(3)] + [np.eye(3)]))
    assert not S.is_closed(np.stack([np.eye(3), SR.rotation((0, 0, 1), math.pi / 2)]))


def test_solids_are_what_they_say():
    counts = {"box": 12, "square_prism": 12, "tri_prism": 8, "cylinder": 92, "l_solid": 20}
    for name in SR.SOLIDS:
        v, t, g, centre, axis = SR.solid(name)
        assert len(t) == counts[name] and t.max() < len(v) and v.dtype == np.float32
        assert np.allclose(SR.surface_centroid(v.astype(np.float64), t), centre, atol=1e-6)
        # every group element maps the vertex set onto itself (float32 vertices: to 1e-6)
        if name != "cylinder":
            for r in g:
                moved = (v.astype(np.float64) - centre) @ r.T + centre
                d = np.sqrt(((moved[:, None] - v.astype(np.float64)[None]) ** 2).sum(axis=2)).min(axis=1)
                assert d.max() < 1e-6, name
            assert len(g) == SR.EXPECTED_COUNT[name]
        assert np.abs(SR.MOTION_R).max() < 0.9                    # no coordinate axis stays one


@pytest.fixture(scope="module", params=SR.SOLIDS)
def sampled(request):
    v, t, g, centre, axis = SR.solid(request.param)
    targets = SR.sample_surface(v, t, TARGETS, TARGET_SEED)
    queries = SR.sample_surface(v, t, QUERIES, QUERY_SEED)
    return request.param, v, g, targets, queries


def test_margins_of_the_acceptance_rule(sampled):
    name, v, g, targets, queries = sampled
    c = targets.astype(np.float64).mean(axis=0)
    d = SR.diameter_of(v)
    h0 = float(SR.hausdorff_scores_fast(queries, targets, np.eye(4)[None])[0])
    eps = h0 + 0.02 * d
    true = SR.hausdorff_scores_fast(queries, targets, np.stack([SR.about(r, c) for r in g]))
    cand, R = SR.coarse_candidates(2048, c)
    far = SR.hausdorff_scores_fast(queries, targets, cand)[SR.angles_deg(R, g).min(axis=1) > 15.0]
    print("%s: diameter %.4f h0 %.5f epsilon %.5f true max %.5f (%.2f epsilon) far min %.5f (%.2f epsilon) of %d"
          % (name, d, h0, eps, true.max(), true.max() / eps, far.min(), far.min() / eps, len(far)))
    assert true.max() <= 0.9 * eps
    if name != "cylinder":
        assert len(far) > 4000 and far.min() >= 1.1 * eps


def test_restated_procedure_on_the_box_and_the_l():
    """Without sharpening (the restatement has none) a true axis can be found twice, so the box's count is bounded, not
    fixed; its kind and orders, and the L-shaped solid's lone identity, do not depend on that."""
    for name in ("box", "l_solid"):
        v, t, g, centre, axis = SR.solid(name)
        r = SR.find_symmetries(SR.sample_surface(v, t, TARGETS, TARGET_SEED), SR.sample_surface(v, t, QUERIES, QUERY_SEED),
                               SR.diameter_of(v))
        print(name, r["kind"], r["count"], r["orders"])
        if name == "box":
            assert r["kind"] == "finite" and set(r["orders"]) == {2} and 4 <= r["count"] <= 7, r
        else:
            assert (r["kind"], r["count"], r["orders"]) == ("none", 1, []), r
