"""CPU: the NumPy restatement of DESIGN.md "Pose proposals" (tests/ppf_reference.py) anchored on hand-computed values,
on the bookkeeping of the pair table, on a known pose that it must recover, and on its tie rules.  The GPU tests
(tests/test_33_ppf_gpu.py) compare the kernels with this restatement."""
import numpy as np

import pose_verify_reference as V
import ppf_reference as P
import render_reference as R


def oriented_points(vertices, triangles, n, seed):
    """n area-weighted surface samples of a mesh with their faces' unit normals (the winding's sign), float32 points;
    samples inside another part of the mesh's union (the L prism is two boxes that share a block) are drawn again."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    cr = np.cross(b - a, c - a)
    area = np.sqrt((cr * cr).sum(axis=1))
    lo = [v[:8].min(axis=0), v[8:].min(axis=0)]
    hi = [v[:8].max(axis=0), v[8:].max(axis=0)]
    pts, nrm = [], []
    while len(pts) < n:
        t = rng.choice(len(triangles), p=area / area.sum())
        u, w = rng.random(2)
        if u + w > 1.0:
            u, w = 1.0 - u, 1.0 - w
        p = a[t] + u * (b[t] - a[t]) + w * (c[t] - a[t])
        other = 1 if t < 12 else 0
        if np.all(p > lo[other] + 1e-9) and np.all(p < hi[other] - 1e-9):
            continue
        pts.append(p)
        nrm.append(cr[t] / area[t])
    return np.asarray(pts, np.float32), np.asarray(nrm, np.float64)


def prism_model(n=128, seed=3):
    v, t = V.l_prism()
    xyz, nrm = oriented_points(v, t, n, seed)
    d = xyz[:, None].astype(np.float64) - xyz[None].astype(np.float64)
    return xyz, nrm, float(np.sqrt((d * d).sum(axis=2)).max())


def posed_scene(xyz, nrm, gt, seed, clutter=0.2):
    """The model points whose normals face the camera at the origin under the pose gt, moved by it, then a fifth as many
    clutter points around them with normals towards the camera.  -> (points [N,3] float32, normals [N,3])."""
    rng = np.random.default_rng(seed)
    p = xyz.astype(np.float64) @ gt[:3, :3].T + gt[:3, 3]
    n = nrm @ gt[:3, :3].T
    seen = (n * -p).sum(axis=1) > 0.0
    p, n = p[seen], n[seen]
    k = int(round(clutter * len(p)))
    cp = p.mean(axis=0) + rng.uniform(-0.12, 0.12, (k, 3))
    cn = rng.standard_normal((k, 3))
    cn /= np.sqrt((cn * cn).sum(axis=1, keepdims=True))
    cn = np.where(((cn * -cp).sum(axis=1) > 0.0)[:, None], cn, -cn)
    order = rng.permutation(len(p) + k)
    return np.concatenate([p, cp])[order].astype(np.float32), np.concatenate([n, cn])[order]


def test_the_prism_model_is_oriented_outward():
    v, _ = V.l_prism()
    xyz, nrm, diam = prism_model()
    assert xyz.shape == (128, 3) and abs(np.sqrt((nrm * nrm).sum(axis=1)) - 1.0).max() < 1e-15
    # a step along the normal leaves both boxes
    out = xyz.astype(np.float64) + 1e-4 * nrm
    inside = [np.all((out > v[s].min(axis=0)) & (out < v[s].max(axis=0)), axis=1) for s in (slice(0, 8), slice(8, 16))]
    assert not (inside[0] | inside[1]).any()
    assert 0.15 < diam < 0.20


def test_frame_takes_the_normal_onto_x_on_both_branches():
    rng = np.random.default_rng(0)
    n = rng.standard_normal((200, 3))
    n /= np.sqrt((n * n).sum(axis=1, keepdims=True))
    n = np.concatenate([n, [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [-1e-300, 1.0, 0.0]]])
    Q = P.frame(n)
    assert (n[:, 0] < 0).sum() > 50 and (n[:, 0] >= 0).sum() > 50
    assert np.abs(Q @ np.swapaxes(Q, 1, 2) - np.eye(3)).max() < 1e-15
    assert np.abs(np.linalg.det(Q) - 1.0).max() < 1e-15
    assert np.abs(np.einsum("kij,kj->ki", Q, n) - [1.0, 0.0, 0.0]).max() < 1e-15
    assert np.array_equal(Q[200], np.eye(3)) and np.array_equal(Q[201], np.diag([-1.0, -1.0, 1.0]))


def test_a_hand_computed_pair():
    cos_edges, alpha_edges, alpha_cs = P.tables(15, 30)
    assert len(cos_edges) == 14 and len(alpha_edges) == 14 and alpha_cs.shape == (30, 2)
    assert np.all(np.diff(cos_edges) < 0) and np.all(np.diff(alpha_edges) < 0)
    # 3.5 cm apart along x, both normals +z: distance bin 3 of 1 cm; both normals at 90 degrees to d (bin 7 of 12 degrees),
    # the normals parallel (bin 0)
    up = np.array([0.0, 0.0, 1.0])
    key, d = P.pair_key(np.zeros(3, np.float32), up, np.array([0.035, 0, 0], np.float32), up, 0.01, 20, 15, cos_edges)
    assert int(key) == ((3 * 15 + 7) * 15 + 7) * 15 + 0 == 11805
    # Q(+z) = rows (0,0,1), (0,1,0), (-1,0,0): d = (x, 0, 0) has the in-plane direction (0, -1)
    ok, uy, uz = P.direction(P.frame(up), d)
    assert bool(ok) and (float(uy), float(uz)) == (0.0, -1.0)
    # the skips: the same point; 20 distance bins end at 20 cm; d along the normal has no in-plane direction
    assert int(P.pair_key(np.zeros(3, np.float32), up, np.zeros(3, np.float32), up, 0.01, 20, 15, cos_edges)[0]) == -1
    assert int(P.pair_key(np.zeros(3, np.float32), up, np.array([0.25, 0, 0], np.float32), up, 0.01, 20, 15, cos_edges)[0]) == -1
    assert int(P.pair_key(np.zeros(3, np.float32), up, np.array([0.15, 0, 0], np.float32), up, 0.01, 20, 15, cos_edges)[0]) >= 0
    k, d = P.pair_key(np.zeros(3, np.float32), up, np.array([0, 0, 0.05], np.float32), up, 0.01, 20, 15, cos_edges)
    assert int(k) == ((5 * 15 + 0) * 15 + 0) * 15 + 0 and not bool(P.direction(P.frame(up), d)[0])
    # angle bins: the ends, and a cosine exactly on an edge belongs to the bin that starts there
    assert P.angle_bin([1.0, 1.5, -1.0, -1.5, cos_edges[3], np.nextafter(cos_edges[3], 2.0)], cos_edges).tolist() == [0, 0, 14, 14, 4, 3]
    # the rotation bins: alpha = 0 is the lower edge of bin n_alpha / 2, pi and -pi fall into the last and the first
    for ca, sa, want in ((1.0, 0.0, 15), (1.0, -0.0, 15), (1.0, -1e-9, 14), (-1.0, 0.0, 29), (-1.0, -1e-9, 0), (0.0, 1.0, 22), (0.0, -1.0, 7)):
        q = int(P.angle_bin(ca, alpha_edges))
        assert (15 + q if sa >= 0.0 else 14 - q) == want


def test_every_ordered_pair_is_in_the_csr_once_or_is_a_stated_skip():
    xyz, nrm, diam = prism_model(64, seed=5)
    flat = (np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 2) * 0.01).astype(np.float32)
    flat = np.concatenate([flat, np.zeros((30, 1), np.float32)], axis=1)
    sets = [(xyz, nrm), (flat, np.tile([0.0, 0.0, 1.0], (30, 1)))]
    model = P.make_model(sets, [diam, 0.03])                   # the patch is larger than its "diameter": pairs past n_dist
    n_key = 20 * 15 ** 3
    bs, ref, dirs = model["bucket_start"], model["entry_ref"], model["entry_dir"]
    assert bs.shape == (2, n_key + 1) and bs[0, 0] == 0 and bs[0, -1] == bs[1, 0] and bs[1, -1] == len(ref)
    assert np.all(np.diff(bs, axis=1) >= 0)
    for s, (x, n) in enumerate(sets):
        key, r, d = model["pairs"][s]
        M = len(x)
        seen = np.zeros((M, M), np.int64)
        for k in np.nonzero(np.diff(bs[s]))[0]:
            lo, hi = bs[s, k], bs[s, k + 1]
            rows, cols = np.nonzero(key == k)                  # (r, i) in pair order, as the stable sort leaves them
            assert len(rows) == hi - lo and np.array_equal(ref[lo:hi], rows) and np.array_equal(dirs[lo:hi], d[rows, cols])
            seen[rows, cols] += 1
        kept = key >= 0
        assert np.array_equal(seen, kept.astype(np.int64))
        # what is not kept is a stated skip: the diagonal, a coincident pair, a pair past the last distance bin, or a
        # pair without an in-plane direction
        xd = x.astype(np.float64)
        dist = np.sqrt((((xd[None] - xd[:, None]) ** 2)).sum(axis=2))
        far = dist / model["dist_step"][s] >= 20
        for a, b in zip(*np.nonzero(~kept)):
            dd = xd[b] - xd[a]
            assert a == b or dist[a, b] == 0 or far[a, b] or not P.direction(P.frame(n[a]), dd)[0], (s, a, b)
        assert kept.sum() > 0 and (s == 0 or far.sum() > 0)
    # the flat patch: every kept pair has both normals at 90 degrees to d and parallel to each other
    keys = np.unique(model["pairs"][1][0])
    assert set((keys[keys >= 0] % 15 ** 3).tolist()) == {(7 * 15 + 7) * 15}


def test_a_known_pose_is_recovered():
    xyz, nrm, diam = prism_model(128, seed=3)
    model = P.make_model([(xyz, nrm)], [diam])
    gt = R.pose_matrix([0.5, -0.4, 0.3], [-0.02, 0.01, 0.5])
    scene, normals = posed_scene(xyz, nrm, gt, seed=1)
    n_model = int(round(len(scene) / 1.2))
    assert 30 <= n_model <= 128 and len(scene) - n_model == int(round(0.2 * n_model))
    r = P.propose(model, scene[None], normals[None], np.ones((1, len(scene))), [0], top=4, ref_step=5, peaks=2)
    tt2, rot_bound = P.thresholds([diam])
    dist, trace = P.pose_errors(r["pose"][0, 0], gt)
    print("top cluster: score %d, %.4f m (threshold %.4f) and trace %.4f (bound %.4f) from the truth; scores %s"
          % (r["score"][0, 0], dist, np.sqrt(tt2[0]), trace, rot_bound, r["score"][0].tolist()))
    assert r["valid"][0, 0] == 1 and dist * dist <= tt2[0] and trace >= rot_bound


def test_peaks_break_ties_by_the_lower_cell():
    """A flat 3 x 3 patch voted for by itself: symmetric, so many cells tie."""
    g = (np.stack(np.meshgrid(np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 2) * 0.01).astype(np.float32)
    flat = np.concatenate([g, np.zeros((9, 1), np.float32)], axis=1)
    up = np.tile([0.0, 0.0, 1.0], (9, 1))
    model = P.make_model([(flat, up)], [0.05], n_alpha=6)
    scene = flat + np.float32(0.5)
    v = P.vote(scene[None], up[None], np.ones((1, 9)), [0], model, ref_step=1, peaks=4)
    assert v["acc"].shape == (1, 9, 9, 6) and v["acc"].sum() > 0
    ties = 0
    for j in range(9):
        a = v["acc"][0, j].reshape(-1)
        order = sorted(range(len(a)), key=lambda c: (-int(a[c]), c))[:4]
        ties += int(a[order[0]] == a[order[1]])
        for k, c in enumerate(order):
            assert v["votes"][0, j, k] == a[c] and (a[c] == 0 or (v["model_index"][0, j, k], v["bin"][0, j, k]) == (c // 6, c % 6))
    assert ties > 0
    # the scene is the model moved by (0.5, 0.5, 0.5): the corner's best pose is that translation or one of the patch's
    # own symmetries; its rotation keeps +z
    T = v["pose"][0, 0, 0]
    assert abs(T[2, 2] - 1.0) < 1e-12 and abs(T[2, 3] - 0.5) < 1e-12


def test_clusters_join_the_first_near_enough_and_rank_by_score_then_founding_order():
    tt2, rot_bound = P.thresholds([0.2])                       # 2 cm, 12 degrees
    def pose(angle_deg, x):
        return R.pose_matrix([0.0, 0.0, np.radians(angle_deg)], [x, 0.0, 0.0])
    # equal votes: visited in index order.  0 founds A; 1 (5 degrees, 1 cm from A) joins A; 2 (13 degrees from A) founds B;
    # 3 is near both A and B (7 and 6 degrees) and joins A, the first; 4 is 3 cm off and founds C; 5 has no votes
    poses = np.stack([pose(0, 0), pose(5, 0.01), pose(13, 0), pose(7, 0), pose(0, 0.03), pose(0, 0)])[None]
    votes = np.array([[5, 5, 5, 5, 5, 0]])
    r = P.cluster(votes, poses, [0], tt2, rot_bound, top=4)
    assert r["members"][0] == [(0, [0, 1, 3]), (2, [2]), (4, [4])]
    assert r["score"].tolist() == [[15, 5, 5, 0]] and r["valid"].tolist() == [[1, 1, 1, 0]]
    assert np.array_equal(r["pose"][0, 1], poses[0, 2]) and np.array_equal(r["pose"][0, 3], np.eye(4))
    # more votes are visited first: candidate 2 founds the first cluster, then 0 (13 degrees off) founds the second; 1 and
    # 3 are near both (8 and 6 degrees from 2) and join the one founded first
    r = P.cluster(np.array([[5, 5, 9, 5, 5, 0]]), poses, [0], tt2, rot_bound, top=2)
    assert r["members"][0] == [(2, [2, 1, 3]), (0, [0])] and r["score"].tolist() == [[19, 5]]
    # a class outside the table has no cluster
    assert not P.cluster(votes, poses, [3], tt2, rot_bound, top=2)["valid"].any()
