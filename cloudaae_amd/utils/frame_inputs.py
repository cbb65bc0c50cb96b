"""Frame inputs: the checks and uploads that the modules working on depth frames share -- depth images as their uint16 bits,
intrinsics rows, int32 columns, float64 poses -- so that one input is accepted, refused and worded the same way by every
binding it reaches.  Nothing here launches a kernel.
"""
import numpy as np
import torch

from .._lib import require

DEPTH_TYPES = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())


def check_depth(t, name, dims):
    """A depth tensor of `dims` dimensions as the kernels read it, contiguous."""
    require(isinstance(t, torch.Tensor) and t.dim() == dims and t.dtype in DEPTH_TYPES,
            "%s must be an int16 (the uint16 bits, as render_frames returns them) or uint16 tensor of %d dimensions"
            % (name, dims))
    return t.contiguous()


def upload_depth(depth, device):
    """uint16 depth (numpy, or a tensor holding the bits as int16) on `device`, contiguous, the same bits."""
    if isinstance(depth, np.ndarray):
        require(depth.dtype == np.uint16, "depth must be uint16")
        return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device)
    require(depth.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)), "depth must be uint16")
    return depth.to(device).contiguous()


def depth_frames(depth, device, name="depth", dims=3):
    """What the loops take as depth: a numpy array is uploaded to `device`, a tensor stays where it is; then check_depth."""
    return check_depth(upload_depth(depth, device) if isinstance(depth, np.ndarray) else depth, name, dims)


def upload_intrinsics(intrinsics, device):
    """float32 intrinsics (a float32 tensor, or anything numpy takes) on `device`, contiguous."""
    if isinstance(intrinsics, torch.Tensor):
        require(intrinsics.dtype == torch.float32, "intrinsics must be float32")
        return intrinsics.to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(intrinsics, np.float32))).to(device)


def check_int32(t, name, shape, dev):
    require(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == shape and t.device == dev,
            "%s must be an int32 %s tensor on the inputs' device" % (name, list(shape)))
    return t.contiguous()


def check_poses(t, name, dims, B, dev):
    """float64 [B,4,4] (3 in dims) or [B,P,4,4] (4 in dims) on `dev`, contiguous."""
    require(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() in dims and tuple(t.shape[-2:]) == (4, 4) and
            int(t.shape[0]) == B and t.device == dev, "%s must be a float64 [B, %s4, 4] tensor on the inputs' device"
            % (name, "P, " if 4 in dims else ""))
    return t.contiguous()


def host(x, dtype):
    """A tensor (read back) or anything numpy takes, as a numpy array of `dtype`."""
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype)


def on_device(x, dtype, dev, shape=None, name=None):
    """A tensor or an array as a contiguous tensor of `dtype` on `dev`; with `shape`, checked against it under `name`."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.to(device=dev, dtype=dtype).contiguous()
    if shape is not None:
        require(tuple(t.shape) == shape, "%s must be %s" % (name, list(shape)))
    return t


def record_intrinsics(frames):
    """Decoded frame records (tfrecord_io.decode_frame) -> float32 [F,5] on the host: each record's intrinsics row."""
    return np.array([[fr[k] for k in ("fx", "fy", "cx", "cy", "factor_depth")] for fr in frames], np.float32)


def intrinsics_per_frame(intrinsics, F):
    """Intrinsics [5] or [F,5] -> float32 [F,5] on the host, one row per frame."""
    return np.ascontiguousarray(np.broadcast_to(host(intrinsics, np.float32).reshape(-1, 5), (F, 5)))
