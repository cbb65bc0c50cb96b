"""CPU: the two helpers that turn decoded frame records into arrays, frame_inputs.record_intrinsics and
track.record_poses, on two records made by hand, against the expressions they took the place of."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cloudaae_amd.utils import fuse, track  # noqa: E402
from cloudaae_amd.utils.frame_inputs import record_intrinsics  # noqa: E402


def _records():
    """Two records as tfrecord_io.decode_frame gives them (the fields the helpers read): float32 scalars, quaternions [21,4]
    (w, x, y, z; not normalised) and translations [21,3] float32."""
    rng = np.random.default_rng(47)
    out = []
    for f in range(2):
        fr = {k: np.float32(v) for k, v in zip(("fx", "fy", "cx", "cy", "factor_depth"),
                                               (1066.778 + f, 1067.487 - f, 312.9869, 241.3109 + 0.5 * f, (10000.0, 1000.0)[f]))}
        fr["quaternions"] = rng.standard_normal((21, 4)).astype(np.float32)
        fr["translations"] = rng.standard_normal((21, 3)).astype(np.float32)
        out.append(fr)
    return out


def test_record_intrinsics_is_the_row_per_record():
    frames = _records()
    got = record_intrinsics(frames)
    assert got.dtype == np.float32 and got.shape == (2, 5)
    for want in (np.array([[f["fx"], f["fy"], f["cx"], f["cy"], f["factor_depth"]] for f in frames], np.float32),
                 np.array([[fr[k] for k in ("fx", "fy", "cx", "cy", "factor_depth")] for fr in frames], np.float32)):
        assert want.dtype == got.dtype and np.array_equal(got, want)
    assert got[1].tolist() == [float(frames[1][k]) for k in ("fx", "fy", "cx", "cy", "factor_depth")]
    assert record_intrinsics(frames[:1]).shape == (1, 5)


def test_record_poses_is_the_pose_per_class():
    frames = _records()
    classes = [3, 0, 20]
    for fr in frames:
        got = track.record_poses(fr, classes)
        want = np.tile(np.eye(4), (len(classes), 1, 1))
        for i, c in enumerate(classes):
            want[i, :3, :3], want[i, :3, 3] = track.quat2mat(fr["quaternions"][c]), fr["translations"][c]
        assert got.dtype == np.float64 and got.shape == (3, 4, 4) and np.array_equal(got, want)
        assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)))
        assert np.abs(got[:, :3, :3] @ got[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
        assert np.array_equal(got[:, :3, 3], fr["translations"][classes].astype(np.float64))
    # one class over the frames, as fuse.class_frames stacks them
    c = 7
    want = np.tile(np.eye(4), (len(frames), 1, 1))
    for f, fr in enumerate(frames):
        want[f, :3, :3], want[f, :3, 3] = track.quat2mat(fr["quaternions"][c]), fr["translations"][c]
    got = np.concatenate([track.record_poses(fr, [c]) for fr in frames])
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert track.record_poses(frames[0], []).shape == (0, 4, 4)


def test_class_frames_reads_both_from_a_record_file(tmp_path):
    """Three frames of 4 x 6 written as records; class 3 is in the first and the last."""
    from cloudaae_amd import tfrecord_io
    from cloudaae_amd.utils import render
    rng = np.random.default_rng(48)
    depth = rng.integers(500, 900, (3, 4, 6)).astype(np.uint16)
    label = rng.integers(0, 5, (3, 4, 6)).astype(np.uint8)
    intr = np.array([[100.0 + f, 101.0, 3.0, 2.0 + f, 1000.0] for f in range(3)], np.float32)

    def pose():
        q = rng.standard_normal(4)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = track.quat2mat(q), rng.standard_normal(3)
        return T
    path = str(tmp_path / "0048_pcnn.tfrecord")
    tfrecord_io.write_records(path, render.frame_records(depth, label, intr, [[pose(), pose()], [pose()], [pose()]],
                                                         [[3, 5], [5], [3]], 48, [0, 1, 2]))
    d, lab, k, poses, frames = fuse.class_frames(path, 3)
    assert [int(fr["frame_id"]) for fr in frames] == [0, 2]
    assert np.array_equal(d, depth[[0, 2]]) and np.array_equal(lab, label[[0, 2]]) and lab.dtype == np.uint8
    assert k.dtype == np.float32 and np.array_equal(k, intr[[0, 2]])
    want = np.tile(np.eye(4), (2, 1, 1))
    for f, fr in enumerate(frames):
        want[f, :3, :3], want[f, :3, 3] = track.quat2mat(fr["quaternions"][3]), fr["translations"][3]
    assert poses.dtype == np.float64 and poses.shape == (2, 4, 4) and np.array_equal(poses, want)
