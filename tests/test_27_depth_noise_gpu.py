"""GPU: cloudaae_depth_normals and cloudaae_depth_sensor_noise (csrc/depth_noise.hip) against the NumPy restatement of
DESIGN.md "Sensor noise" (tests/depth_noise_reference.py), on frames rendered by utils/render.render_frames.

The comparison rule is fixed on the CPU by tests/test_depth_noise_host.py: a pixel is settled when, in the restatement
with the float64 normal2, no decision (a lateral offset or a disparity against a half-integer, theta against theta_drop,
z'' factor + 0.5 against an integer) lies within the measured margin of its point.  At every settled pixel depth and
label equal the float32 restatement exactly; the counts agree within the number of unsettled pixels; z_noisy agrees
within a relative 1e-6 (the resolution of the fp32 normal2) wherever both have depth; the unsettled share is <= 2 %.
The shapes are the smallest at which the kernel can still go wrong: 37 x 70 (a partial last wave, every border clamp)
with one frame and 48 x 64 with three."""
import math

import numpy as np
import pytest
import torch

import depth_noise_reference as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def frames(hip, dev):
    """name -> (depth uint16 numpy, label, intr, device depth int16, device label): rendered by render_frames, and
    equal to the restatement's rendering that the host test measured the rule on."""
    from cloudaae_amd.utils import render
    out = {}
    for name, (meshes, fr, intr, H, W) in D.scenes().items():
        r = render.render_frames([m[:2] for m in meshes], fr, intr, H, W, device=dev)
        depth = r['depth'].cpu().numpy().view(np.uint16)
        want = D.rendered(name)
        assert np.array_equal(depth, want[0]) and np.array_equal(r['label'].cpu().numpy(), want[1]), name
        out[name] = (depth, want[1], intr, r['depth'], r['label'])
    return out


def _apply(fr, params, seed=0, first_frame=0):
    from cloudaae_amd.utils import depth_noise
    r = depth_noise.apply(fr[3], fr[4], fr[2], params, seed=seed, first_frame=first_frame, return_z=True)
    torch.cuda.synchronize()
    return dict(depth=r['depth'].cpu().numpy().view(np.uint16), label=r['label'].cpu().numpy(),
                counts=r['counts'].cpu().numpy(), z_noisy=r['z_noisy'].cpu().numpy())


@pytest.mark.parametrize("name", list(D.scenes()))
def test_normals_equal_the_restatement(frames, name):
    from cloudaae_amd.utils import depth_noise
    fr = frames[name]
    got = depth_noise.depth_normals(fr[3], fr[4], fr[2])
    want = D.depth_normals(fr[0], fr[1], fr[2])
    tol_n, tol_t = D.slope_tolerance()
    normals, theta = got['normals'].cpu().numpy(), got['theta'].cpu().numpy()
    flat = (fr[0] != 0) & ~normals.any(axis=-1)
    err_n, err_t = np.abs(normals.astype(np.float64) - want['normals']).max(), np.abs(theta.astype(np.float64) - want['theta']).max()
    print("%s: flat %s, normals off by %.3e (tolerance %.3e), theta by %.3e (%.3e)"
          % (name, want['flat_counts'].tolist(), err_n, tol_n, err_t, tol_t))
    assert np.array_equal(flat, want['flat']) and np.array_equal(got['flat_counts'].cpu().numpy(), want['flat_counts'])
    assert err_n <= tol_n and err_t <= tol_t
    assert not normals[fr[0] == 0].any() and not theta[fr[0] == 0].any()
    length = np.sqrt((normals.astype(np.float64) ** 2).sum(axis=-1))[(fr[0] != 0) & ~want['flat']]
    assert np.abs(length - 1.0).max() < 1e-6 and normals[..., 2].max() <= 0.0      # towards the camera


@pytest.mark.parametrize("name", list(D.scenes()))
def test_preset_none_returns_its_input(frames, name):
    fr = frames[name]
    got = _apply(fr, 'none', seed=9, first_frame=5)
    assert np.array_equal(got['depth'], fr[0]) and np.array_equal(got['label'], fr[1])
    assert np.array_equal(got['counts'][:, 0], (fr[0] != 0).reshape(len(fr[0]), -1).sum(axis=1))
    assert not got['counts'][:, 1:].any()


@pytest.mark.parametrize("case", D.CASES, ids=["%s-%s" % c[:2] for c in D.CASES])
def test_sensor_equals_the_restatement_at_settled_pixels(frames, case):
    name, stage, seed, first = case
    fr = frames[name]
    got = _apply(fr, D.STAGES[stage], seed=seed, first_frame=first)
    r32, r64 = D.case_results(case)
    un = D.unsettled(r64, D.STAGES[stage], D.measured_margin())
    share = un.sum() / float((fr[0] != 0).sum())
    bad_d, bad_l = (got['depth'] != r32['depth']) & ~un, (got['label'] != r32['label']) & ~un
    both = (got['z_noisy'] != 0) & (r32['z_noisy'] != 0)
    rel = (np.abs(got['z_noisy'] - r32['z_noisy'])[both] / np.abs(r32['z_noisy'][both])).max()
    print("%s %s: unsettled %d (%.2f %%), depth differs at %d settled pixels (and %d unsettled), label at %d, counts %s "
          "against %s, z_noisy off by %.2e relative"
          % (name, stage, un.sum(), 100 * share, bad_d.sum(), ((got['depth'] != r32['depth']) & un).sum(), bad_l.sum(),
             got['counts'].tolist(), r32['counts'].tolist(), rel))
    assert share <= D.UNSETTLED_CAP
    assert not bad_d.any() and not bad_l.any()
    assert np.abs(got['counts'].astype(np.int64) - r32['counts']).sum() <= un.sum()
    assert np.array_equal(got['z_noisy'] != 0, r32['z_noisy'] != 0) or un.any()
    assert rel <= 1e-6


def test_deterministic_and_independent_of_the_launch_split(frames):
    fr = frames['planes_48x64']
    a, b = _apply(fr, 'kinect1', seed=3), _apply(fr, 'kinect1', seed=3)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for f in range(3):
        one = _apply(tuple(x[f:f + 1] for x in fr), 'kinect1', seed=3, first_frame=f)
        for k in a:
            assert np.array_equal(a[k][f], one[k][0]), (k, f)
    other = _apply(fr, 'kinect1', seed=4)
    assert not np.array_equal(other['depth'], a['depth']) and not np.array_equal(other['z_noisy'], a['z_noisy'])
    shifted = _apply(fr, 'kinect1', seed=3, first_frame=1)
    assert not np.array_equal(shifted['depth'][0], a['depth'][0])


def _plane(dev, rot, H=48, W=64, z=0.8, focal=60.0, half=8.0):
    from cloudaae_amd.utils import render
    import render_reference as RR
    intr = np.array([[focal, focal, 31.5, 23.5, 10000.0]], np.float32)
    r = render.render_frames([D.plane_mesh(half)], [[(0, 1, RR.pose_matrix(rot, [0.0, 0.0, z]))]], intr, H, W, device=dev)
    return r['depth'], r['label'], intr


def test_axial_noise_has_the_stated_spread(hip, dev):
    """A fronto-parallel plane at 0.8 m, the axial stage alone: the standard deviation of depth_out - clean over the
    interior pixels lies within 5 % of sigma_z(0.8, theta) averaged over those pixels' theta (the sampling error at
    about 2000 pixels is 1.6 %, the depth unit adds (1/12) / 12^2 / 2 < 0.1 %)."""
    from cloudaae_amd.utils import depth_noise
    depth, label, intr = _plane(dev, [0.0, 0.0, 0.0])
    p = D.STAGES['axial']
    got = depth_noise.apply(depth, label, intr, p, seed=21)
    theta = depth_noise.depth_normals(depth, label, intr)['theta'].cpu().numpy()[0, 4:-4, 4:-4].astype(np.float64)
    clean = depth.cpu().numpy().view(np.uint16)[0, 4:-4, 4:-4].astype(np.float64)
    noisy = got['depth'].cpu().numpy().view(np.uint16)[0, 4:-4, 4:-4].astype(np.float64)
    assert np.all(clean == 8000) and clean.size >= 2000
    sigma = (p['a0'] + p['a1'] * (0.8 - p['z0']) ** 2) + (p['a2'] / math.sqrt(0.8)) * theta ** 2 / (math.pi / 2 - theta) ** 2
    want, have = sigma.mean() * 10000.0, (noisy - clean).std()
    print("axial spread: %.3f units, stated %.3f (%.2f %% off), mean shift %.3f" % (have, want, 100 * (have / want - 1),
                                                                                  (noisy - clean).mean()))
    assert abs(have / want - 1.0) <= 0.05
    assert abs((noisy - clean).mean()) <= 4.0 * want / math.sqrt(clean.size)
    assert got['counts'].cpu().numpy().tolist() == [[48 * 64, 0, 0, 0]]


def test_a_plane_past_theta_drop_returns_nothing(hip, dev):
    from cloudaae_amd.utils import depth_noise
    # a long lens: the viewing rays stay within 0.06 rad of the axis, so every theta is near the tilt of 1.35 rad
    # (and a plane small enough to stay in front of the near plane: the renderer does not clip)
    depth, label, intr = _plane(dev, [0.0, 1.35, 0.0], z=1.0, focal=600.0, half=0.9)
    with_depth = int((depth != 0).sum())
    theta = depth_noise.depth_normals(depth, label, intr)['theta'].cpu().numpy()[0]
    d = depth.cpu().numpy()[0] != 0
    assert with_depth > 500
    got = depth_noise.apply(depth, label, intr, dict(D.NONE, theta_drop=1.2), seed=1)
    counts = got['counts'].cpu().numpy()[0]
    dropped_all = theta[d].min() > 1.2
    print("tilted plane: %d pixels with depth, counts %s, smallest theta %.3f" % (with_depth, counts.tolist(), theta[d].min()))
    assert dropped_all and not got['depth'].any()
    assert counts.tolist() == [with_depth, with_depth, 0, 0]
    assert torch.equal(got['label'], label)


def test_render_frames_with_a_sensor_feeds_extract_segments(hip, dev):
    """An icosphere that fills the frame, rendered with sensor='kinect1': clean_depth is the render without a sensor,
    and extract_segments yields the object's segment from the noisy frame."""
    from cloudaae_amd.utils import render, segment
    import mesh_models_reference as MR
    import render_reference as RR
    v, t = MR.icosphere(3)
    mesh = [((v * np.float32(0.12)), t)]
    intr = np.array([[250.0, 250.0, 79.5, 59.5, 10000.0]], np.float32)
    inst = [[(0, 4, RR.pose_matrix([0.3, 0.2, 0.1], [0.0, 0.0, 0.7]))]]
    clean = render.render_frames(mesh, inst, intr, 120, 160, device=dev)
    noisy = render.render_frames(mesh, inst, intr, 120, 160, device=dev, sensor='kinect1', sensor_seed=6, first_frame=2)
    assert torch.equal(noisy['clean_depth'], clean['depth']) and 'clean_depth' not in clean
    assert not torch.equal(noisy['depth'], clean['depth'])
    counts = noisy['sensor_counts'].cpu().numpy()[0]
    assert counts[0] == int((clean['depth'] != 0).sum()) and counts[1] > 0
    seg = segment.extract_segments(noisy['depth'], noisy['label'], intr, classes=[[3]])
    ref = segment.extract_segments(clean['depth'], clean['label'], intr, classes=[[3]])
    print("points after the filters: %s with the sensor, %s without"
          % (seg.num_point_after_filter.tolist(), ref.num_point_after_filter.tolist()))
    assert bool(seg.kept.all()) and bool(ref.kept.all())
    assert int(seg.offsets[-1]) > 1000
