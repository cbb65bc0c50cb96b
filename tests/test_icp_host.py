"""CPU: the ICP entry point of the C ABI (revision 602) is exported and rejects bad arguments before it touches
the GPU; the NumPy restatement (tests/icp_reference.py) recovers a known pose."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cloudaae_amd", "libcloudaae_hip.so")


@pytest.fixture(scope="module")
def cdll():
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, as the product does)
    from cloudaae_amd import _lib
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    return _lib.lib()._cdll


def test_abi_revision_and_export(cdll):
    from cloudaae_amd import _lib
    assert _lib.ABI_VERSION == 602
    assert cdll.cloudaae_version() == 602
    assert hasattr(cdll, "cloudaae_icp_point_to_point") and hasattr(cdll, "cloudaae_f64_to_f32")


# a fake, never dereferenced address: every call below must fail in validation, before any HIP runtime call
_X = 0x1000


def _args(**kw):
    a = dict(b=1, m=2048, src=_X, sps=6, scs=2048 * 6, n=1024, dst=_X, dps=3, dcs=1024 * 3, rot=_X, trans=_X,
             radius=0.01, decay=0.9, rounds=10, max_it=30, rf=1e-6, rr=1e-6, T=_X, rot_out=_X, trans_out=_X, fit=_X,
             rmse=_X, its=_X)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("bad, needle", [
    (dict(b=0), "b, m and n"), (dict(m=0), "b, m and n"), (dict(n=0), "b, m and n"),
    (dict(n=4097), "limit"), (dict(m=4097), "limit"),
    (dict(rounds=-1), "rounds"), (dict(max_it=-1), "max_iteration"),
    (dict(radius=0.0), "radius"), (dict(radius=-0.01), "radius"),
    (dict(decay=0.0), "decay"), (dict(decay=1.5), "decay"), (dict(decay=-0.9), "decay"),
    (dict(src=None), "null"), (dict(dst=None), "null"), (dict(rot=None), "null"), (dict(trans=None), "null"),
    (dict(T=None), "null"), (dict(rot_out=None), "null"), (dict(trans_out=None), "null"), (dict(fit=None), "null"),
    (dict(rmse=None), "null"), (dict(its=None), "null"),
])
def test_invalid_arguments_are_rejected(cdll, bad, needle):
    from cloudaae_amd import _lib
    rc = cdll.cloudaae_icp_point_to_point(*_args(**bad))
    assert rc != 0
    msg = cdll.cloudaae_last_error().decode()
    assert "cloudaae_icp_point_to_point" in msg and needle in msg, msg
    assert _lib.ABI_VERSION == 602


def test_restatement_recovers_a_known_pose():
    """Case 2 of the GPU tests: the whole posed model as the scene, noise-free, initial pose 2 deg / 3 mm off.  The
    scene is stored in fp32 (6e-8 m at 0.8 m), which bounds how closely the truth can be recovered."""
    import icp_reference as R
    from cloudaae_amd import tfrecord_io
    models, _ = tfrecord_io.read_and_decode_obj_model(os.path.join(ROOT, "tests", "golden", "obj_model_first1.tfrecords"))
    rng = np.random.default_rng(5)
    rot = R.log_map(R.rodrigues(rng.standard_normal(3)))
    trans = np.array([0.01, -0.02, 0.8])
    sc, r0, t0 = R.scene(models[0][:, :3], rot, trans, 2048, 0.0, rng, 2.0, 0.003)
    T, fit, rmse, its = R.refine(models[0], sc, r0, t0)
    assert fit == 1.0 and rmse < 1e-7
    assert np.abs(T - R.initial_transform(rot, trans)).max() < 1e-7
    assert len(its) == 10 and its.min() >= 1
