"""CPU: the NumPy restatement of DESIGN.md "Pose sampling" (tests/pose_sampling_reference.py) -- its Philox against known
vectors, the statistics of the restated draws, the keep / replace rule, invariance to how the samples are batched -- and
the argument checks of cloudaae_sample_poses / cloudaae_random_object_occluder (C ABI revision 602), which must fail
before they touch memory."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import pose_sampling_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")
ALL = list(range(21))

# seeds and sizes of tests/test_21_pose_sampling_gpu.py's exact comparison: the restatement alone must exclude none
GPU_CASES = [('ycbv', 11, 0, 4096), ('linemod', 12, 1 << 33, 4096)]
# philox4x32(seed = 0x0123456789ABCDEF, ctr = 2^32 + 5, stream) of csrc/philox.h: computed with the restatement, whose
# rounds reproduce the three known-answer vectors of Random123 below; the GPU file checks the kernels' raw words
# (streams 16 and 17) and the padding draws of cloudaae_hidden_point_removal (stream 7) against the same function
WRAPPER_SEED, WRAPPER_CTR = 0x0123456789ABCDEF, (1 << 32) + 5
# share of translations replaced by the frustum middle over 10^6 draws of seed 1 (profiles/notes_pose_sampling.md)
REPLACED_SHARE = {'ycbv': 0.776892, 'linemod': 0.430024}


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_symbols_and_signatures(cdll):
    from cloudaae_amd import _lib
    I, U, P, F = ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_float
    want = {"cloudaae_sample_poses": [I, U, U, I, P, I] + [F] * 10 + [P] * 9,
            "cloudaae_random_object_occluder": [I, U, U, I, I, P, I, P, P, P, I, F, F, F, P, P, P, P]}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudaae_hip.h")).read(), flags=re.S)
    for fn, sig in want.items():
        assert _lib._SIGNATURES[fn] == sig
        f = getattr(cdll, fn)
        assert list(f.argtypes) == sig and f.restype is ctypes.c_int
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % fn, header).group(1)
        assert len(decl.split(",")) == len(sig), decl
    assert _lib.ABI_VERSION == 602 and cdll.cloudaae_version() == 602


_X = 0x1000          # a fake, never dereferenced address: every call below must fail in validation


def _ints(*v):
    return (ctypes.c_int * max(len(v), 1))(*v)


def _sp(**kw):
    a = dict(b=4, first=0, seed=1, n_classes=2, classes=_ints(0, 20), nmodels=21, wnear=0.719, wfar=1.438, near=0.5, far=1.0,
             fx=1066.778, fy=1067.487, cx=312.9869, cy=241.3109, width=640.0, height=480.0, class_id=_X, axisangle=_X,
             rot=_X, rot32=None, trans=_X, in_fov=_X, drawn=None, raw=None)
    a.update(kw)
    return list(a.values()) + [None]


def _oo(**kw):
    a = dict(b=4, first=0, seed=1, nmodels=21, npts=2048, models=_X, n_classes=2, classes=_ints(0, 20), rot=_X, trans=_X,
             per=512, wnear=0.719, hnear=0.558, near=0.5, occ=_X, occ_class=None, raw=None)
    a.update(kw)
    return list(a.values()) + [None]


_S, _O = "cloudaae_sample_poses", "cloudaae_random_object_occluder"


@pytest.mark.parametrize("fn, args, needle", [
    (_S, _sp(b=0), "b must"), (_S, _sp(b=-3), "b must"),
    (_S, _sp(n_classes=0), "empty class list"), (_S, _sp(n_classes=-1), "empty class list"),
    (_S, _sp(classes=None), "null"), (_S, _sp(classes=_ints(0, 21)), "class id outside"),
    (_S, _sp(classes=_ints(-1, 3)), "class id outside"), (_S, _sp(nmodels=0), "nmodels"),
    (_S, _sp(n_classes=129, classes=_ints(*([0] * 129))), "longer than 128"),
    (_S, _sp(far=0.5), "far must be > near"), (_S, _sp(far=0.4), "far must be > near"),
    (_S, _sp(far=float("nan")), "far must be > near"),
    (_S, _sp(width=0.0), "width and height"), (_S, _sp(height=-480.0), "width and height"),
    (_S, _sp(width=float("nan")), "width and height"), (_S, _sp(fx=float("inf")), "finite"),
] + [(_S, _sp(**{k: None}), "null") for k in ("class_id", "axisangle", "rot", "trans", "in_fov")] + [
    (_O, _oo(b=0), "b must"), (_O, _oo(b=-1), "b must"), (_O, _oo(per=0), "per must"),
    (_O, _oo(per=2049), "per above the model's points"), (_O, _oo(npts=100), "per above the model's points"),
    (_O, _oo(n_classes=0), "empty class list"), (_O, _oo(classes=None), "null"),
    (_O, _oo(classes=_ints(3, 21)), "class id outside"), (_O, _oo(nmodels=0), "nmodels"),
    (_O, _oo(near=float("nan")), "finite"),
] + [(_O, _oo(**{k: None}), "null") for k in ("models", "rot", "trans", "occ")])
def test_invalid_arguments_are_rejected(cdll, fn, args, needle):
    from cloudaae_amd import _lib
    rc = getattr(_lib.lib(), fn)(*args)
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert fn in msg and needle in msg, msg


def test_philox_known_vectors():
    """Random123's known answers for Philox4x32-10 (counter, key -> output), then the wrapper of csrc/philox.h."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for c, k, want in kat:
        got = R.philox_rounds(np.array([c], np.uint64), np.array([k], np.uint64))[0]
        assert [int(v) for v in got] == want
    # the wrapper: counter = (ctr low, ctr high, stream, 0x9E3779B9), key = (seed low, seed high)
    for stream in (7, 16):
        got = R.philox4x32(WRAPPER_SEED, [WRAPPER_CTR], stream)[0]
        want = R.philox_rounds(np.array([[5, 1, stream, 0x9E3779B9]], np.uint64), np.array([[0x89ABCDEF, 0x01234567]], np.uint64))[0]
        assert np.array_equal(got, want)
    # u01: 24 bits, never 0; the top value rounds to 1.0 in fp32
    assert R.u01(np.uint32(0)) == np.float32(0.5 / 16777216) and R.u01(np.uint32(0xFFFFFFFF)) == np.float32(1.0)
    assert np.array_equal(R.pick(np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32), 21), [0, 10, 10, 20])


def padding_rows_follow_philox(row_src, num_vis, seed):
    """An existing integer use of philox4x32 (csrc/synth.hip, hpr_gather_kernel): output row r >= num_vis of cloud h
    repeats visible row r0 % num_vis, r0 the first word of philox4x32(seed, h << 32 | r, 7)."""
    for h in range(row_src.shape[0]):
        nv, rows = int(num_vis[h]), row_src.shape[1]
        assert 0 < nv < rows and np.array_equal(row_src[h, :nv], np.arange(nv))
        r = np.arange(nv, rows, dtype=np.uint64)
        words = R.philox4x32(seed, (np.uint64(h) << np.uint64(32)) | r, 7)
        assert np.array_equal(row_src[h, nv:], (words[:, 0] % np.uint32(nv)).astype(np.int32))


def test_philox_reproduces_a_recorded_device_draw():
    """The known vector of an existing use: the batch stored by the record path on the GPU (tests/golden/
    small_data_records_b4.npz, seed 5; the target's removal runs with seed + 1) holds ~1000 padding draws per cloud."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "small_data_records_b4.npz"))
    padding_rows_follow_philox(gold['visiblePoints_org_src'], gold['num_vis_point_org'], int(gold['seed']) + 1)


def test_rotation_statistics():
    n = 200000
    a = R.sample_poses(n, 5, 0, ALL)
    ax = a['axisangle']
    angle_abs = np.linalg.norm(ax, axis=1)
    axis = ax / angle_abs[:, None]                      # +- the drawn axis; the sign is the angle's, independent of it
    # the drawn axis itself: recover the sign from z = u (the axis' z) and the restated angle's sign
    r = a['raw']
    sign = np.where(R.u01(r[:, 3]) * np.float32(2) - np.float32(1) < 0, -1.0, 1.0)
    axis = axis * sign[:, None]
    se = np.sqrt(1.0 / 3.0 / n)                         # a uniform unit vector: each component has variance 1/3
    assert np.all(np.abs(axis.mean(0)) < 5 * se), axis.mean(0)
    z2 = axis[:, 2] ** 2                                # z ~ U(-1,1): E z^2 = 1/3, Var z^2 = 1/5 - 1/9
    assert abs(z2.mean() - 1.0 / 3.0) < 5 * np.sqrt((1.0 / 5 - 1.0 / 9) / n)
    angle = angle_abs * sign                            # U(-pi, pi): mean 0, variance pi^2/3, Var x^2 = pi^4 (1/5 - 1/9)
    assert abs(angle.mean()) < 5 * np.sqrt(np.pi ** 2 / 3 / n)
    assert abs(angle.var() - np.pi ** 2 / 3) < 5 * np.sqrt(np.pi ** 4 * (1.0 / 5 - 1.0 / 9) / n)
    assert angle_abs.max() <= float(np.float32(np.pi)) * (1 + 1e-6)
    # classes: uniform over the list, and only the list
    for classes in (ALL, [3, 7, 20]):
        c = R.sample_poses(n, 5, 0, classes)['class_id']
        assert set(np.unique(c)) == set(classes)
        p = 1.0 / len(classes)
        for k in classes:
            assert abs((c == k).mean() - p) < 5 * np.sqrt(p * (1 - p) / n)
    # the rotation matrix of the drawn axis-angle is a rotation by that angle
    Rm = a['rot_mat64'][:1000]
    assert np.allclose(Rm @ Rm.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    assert np.allclose((np.trace(Rm, axis1=1, axis2=2) - 1) / 2, np.cos(angle_abs[:1000]), atol=1e-6)


@pytest.mark.parametrize("dataset", ["ycbv", "linemod"])
def test_kept_translations_project_inside_and_replaced_ones_are_the_middle(dataset):
    a = R.sample_poses(300000, 9, 12345, ALL, dataset)
    c = R.camera_constants(dataset)
    keep, t = a['in_fov'], a['translation']
    assert t.dtype == np.float32 and 0 < keep.sum() < len(keep)
    x, y, z = (t[keep][:, k] for k in range(3))
    u = (c['fx'] * x + c['cx'] * z) / z
    v = (c['fy'] * y + c['cy'] * z) / z
    assert np.all((u > 0) & (u < c['width']) & (v > 0) & (v < c['height']))
    middle = np.array([0.0, 0.0, (c['far'] + c['near']) / np.float32(2)], np.float32)
    assert np.all(t[~keep] == middle[None, :])
    assert np.array_equal(t[keep], a['drawn'][keep][:, :3])
    # the draws before replacement: N(0, (Wnear+Wfar)/7) twice and N((far+near)/2, (far-near)/7)
    d = a['drawn'].astype(np.float64)
    n = len(d)
    sxy, sz = float(c['wnear'] + c['wfar']) / 7, float(c['far'] - c['near']) / 7
    assert abs(d[:, 0].mean()) < 5 * sxy / np.sqrt(n) and abs(d[:, 1].mean()) < 5 * sxy / np.sqrt(n)
    assert abs(d[:, 2].mean() - float(middle[2])) < 5 * sz / np.sqrt(n)
    for col, s in ((0, sxy), (1, sxy), (2, sz)):
        assert abs(d[:, col].var() - s * s) < 5 * s * s * np.sqrt(2.0 / n)


@pytest.mark.parametrize("dataset", ["ycbv", "linemod"])
def test_replaced_share(dataset):
    n = 1000000
    share = 1.0 - R.sample_poses(n, 1, 0, ALL, dataset)['in_fov'].mean()
    print("replaced share %s seed 1: %.6f" % (dataset, share))
    assert abs(share - REPLACED_SHARE[dataset]) < 5e-7            # the figure of the notes
    other = 1.0 - R.sample_poses(n, 2, 0, ALL, dataset)['in_fov'].mean()
    print("replaced share %s seed 2: %.6f" % (dataset, other))
    p = REPLACED_SHARE[dataset]
    assert abs(other - p) < 5 * np.sqrt(2 * p * (1 - p) / n)      # both are estimates: the difference's standard error


def test_invariance_to_the_batch_split():
    one = R.sample_poses(256, 77, 0, ALL)
    keys = ('raw', 'class_id', 'axisangle', 'rot_mat64', 'translation', 'in_fov', 'drawn')

    def cat(parts):
        return {k: np.concatenate([p[k] for p in parts]) for k in keys}
    eight = cat([R.sample_poses(32, 77, 32 * s, ALL) for s in range(8)])
    # 4 ranks x 2 steps of a global batch of 128: rank r of step s draws g = s * 128 + r * 32 + i
    parts = {}
    for s in range(2):
        for r in range(4):
            g0 = R.global_index(s, 128, r, 32)
            parts[g0] = R.sample_poses(32, 77, g0, ALL)
    ranks = cat([parts[g0] for g0 in sorted(parts)])
    assert sorted(parts) == list(range(0, 256, 32))
    for k in keys:
        assert np.array_equal(one[k], eight[k], equal_nan=True) and np.array_equal(one[k], ranks[k], equal_nan=True), k
    # the same holds for the occluder, and another seed or stream gives other words
    models = np.random.default_rng(0).standard_normal((21, 600, 6)).astype(np.float32) * 0.05
    o1 = R.object_occluder(models, 256, 77, 0, ALL, one['rot_mat64'], one['translation'])
    o8 = [R.object_occluder(models, 32, 77, 32 * s, ALL, one['rot_mat64'][32 * s:32 * s + 32],
                            one['translation'][32 * s:32 * s + 32]) for s in range(8)]
    assert np.array_equal(o1['occluder'], np.concatenate([o['occluder'] for o in o8]))
    assert not np.array_equal(one['raw'], R.sample_poses(256, 78, 0, ALL)['raw'])
    assert len({tuple(w) for w in np.concatenate([one['raw'][:, :4], one['raw'][:, 4:], o1['raw'][:, :4], o1['raw'][:, 4:]])}) == 1024


def test_sampled_poses_index_ranges():
    """Every rank draws its own range of g: disjoint, and together the whole of [0, steps * global batch)."""
    from cloudaae_amd import train_cloudAAE_ycbv as T
    seen = []
    for rank in range(4):
        sp = T.SampledPoses(1000, 128, rank, 4)
        assert sp.steps_per_epoch() == 7 and len(sp) == 7 * 32
        for epoch in range(2):
            for b in range(sp.steps_per_epoch()):
                g0 = sp.first_index(epoch, b)
                assert g0 == R.global_index(epoch * 7 + b, 128, rank, 32)
                seen.extend(range(g0, g0 + 32))
    assert sorted(seen) == list(range(2 * 7 * 128))


def test_defaults_of_get_small_data_are_the_record_path():
    from cloudaae_amd import train_cloudAAE_ycbv as T
    p = inspect.signature(T.get_small_data).parameters
    assert p['occluder'].default == 'spherical' and p['dataset'].default == 'ycbv' and p['rows'].default is None
    args = T.parse_arg_groups(T.get_training_argparser(), [])['mi355x']
    assert (args['poses'], args['occluder'], args['dataset'], args['epoch_size']) == ('records', 'spherical', 'ycbv', 381553)


def test_gpu_cases_exclude_nothing_and_tolerances_are_measurable():
    """The seeds of the GPU file's exact comparison: no restated pixel within 1e-4 px of an image edge, so the GPU file's
    exclusion list is empty before the GPU is asked; and the measured tolerances have the size of fp32 rounding."""
    for dataset, seed, first, n in GPU_CASES:
        a = R.sample_poses(n, seed, first, ALL, dataset)
        assert (R.edge_distance(a['drawn'], dataset) < 1e-4).sum() == 0
    from cloudaae_amd import train_cloudAAE_ycbv as T
    models = T.synthetic_object_models().numpy()
    for dataset in ("ycbv", "linemod"):
        tol = R.float_tolerances(21, 65536, dataset, models, ALL)
        print("tolerances %s: %r" % (dataset, tol))
        for k, v in tol.items():
            assert 4 * 2.0 ** -24 * 0.25 <= v < 1e-3, (k, v)
