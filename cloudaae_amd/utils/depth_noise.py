"""A structured-light depth sensor's noise on depth / label frames, and the per-pixel normal map it is built on: the
stage between render.render_frames and segment.extract_segments (cloudaae_depth_sensor_noise and cloudaae_depth_normals,
csrc/depth_noise.hip).  The definition is in DESIGN.md ("Sensor noise"); the constants of the 'kinect1' preset are those
of Nguyen, Izadi and Lovell (2012) as recalled, not checked.  The reference has no sensor model; nothing here is matched
to it.

    out = render.render_frames(meshes, instances, intrinsics, 480, 640)
    noisy = apply(out['depth'], out['label'], intrinsics, 'kinect1', seed=1)
    r = segment.extract_segments(noisy['depth'], noisy['label'], intrinsics, classes=[[0, 1], ...])      # no host copy
"""
import math

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream

PARAMS = ('sigma_l', 'a0', 'a1', 'z0', 'a2', 'theta_max', 'theta_drop', 'p_drop', 'baseline', 'disparity_step')
PRESETS = {
    # returns its input bit for bit
    'none': dict(sigma_l=0.0, a0=0.0, a1=0.0, z0=0.0, a2=0.0, theta_max=0.0, theta_drop=math.pi, p_drop=0.0, baseline=0.0,
                 disparity_step=0.0),
    # Kinect v1 (as recalled, not checked): lateral sigma in pixels, axial sigma_z = a0 + a1 (z - z0)^2 + (a2 / sqrt(z))
    # theta^2 / (pi/2 - theta)^2 in metres, angles in radians, baseline in metres, disparity step in pixels
    'kinect1': dict(sigma_l=0.8, a0=0.0012, a1=0.0019, z0=0.4, a2=0.0001, theta_max=1.45, theta_drop=1.40, p_drop=0.005,
                    baseline=0.075, disparity_step=0.125),
}
MAX_FRAME = 1 << 40


def sensor_params(preset='kinect1', **overrides):
    """The parameter block of a preset ('none', 'kinect1') with `overrides`, validated: a dict of floats with the keys
    PARAMS."""
    require(preset in PRESETS, "unknown sensor preset %r (known: %s)" % (preset, ", ".join(sorted(PRESETS))))
    unknown = sorted(set(overrides) - set(PARAMS))
    require(not unknown, "unknown sensor parameter(s): %s" % ", ".join(unknown))
    p = dict(PRESETS[preset])
    p.update({k: float(v) for k, v in overrides.items()})
    require(all(math.isfinite(p[k]) for k in PARAMS), "sensor parameters must be finite")
    require(p['sigma_l'] >= 0.0, "sigma_l must be >= 0")
    require(0.0 <= p['theta_max'] < math.pi / 2, "theta_max must lie in [0, pi / 2)")
    require(0.0 <= p['p_drop'] <= 1.0, "p_drop must lie in [0, 1]")
    require(p['disparity_step'] >= 0.0, "disparity_step must be >= 0")
    return p


def _frames(depth, label, intrinsics):
    """Device tensors of the three inputs: depth [F,H,W] int16 (uint16 bits; a uint16 array is taken too), label uint8,
    intrinsics [F,5] float32 (host intrinsics are checked for factor_depth > 0 on the way)."""
    if not isinstance(depth, torch.Tensor):
        d = np.ascontiguousarray(depth)
        require(d.dtype in (np.uint16, np.int16), "depth must be uint16 (or its int16 bits)")
        depth = torch.from_numpy(d.view(np.int16))
    if not isinstance(label, torch.Tensor):
        label = torch.from_numpy(np.ascontiguousarray(label, np.uint8))
    require(depth.dtype == torch.int16 and label.dtype == torch.uint8,
            "depth must be int16 (the uint16 bit pattern) and label uint8")
    require(depth.dim() == 3 and depth.shape == label.shape, "depth and label must be [F, H, W]")
    F = int(depth.shape[0])
    if not isinstance(intrinsics, torch.Tensor):
        k = np.ascontiguousarray(intrinsics, np.float32)
        require(k.shape == (F, 5), "intrinsics must be [F, 5], one row per frame")
        require(bool(np.all(k[:, 4] > 0.0)), "factor_depth must be > 0")
        intrinsics = torch.from_numpy(k)
    require(tuple(intrinsics.shape) == (F, 5), "intrinsics must be [F, 5], one row per frame")
    dev = depth.device if depth.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return (depth.to(dev).contiguous(), label.to(dev).contiguous(),
            intrinsics.to(device=dev, dtype=torch.float32).contiguous())


def depth_normals(depth, label, intrinsics):
    """The slope at every pixel.  -> dict of device tensors: normals [F,H,W,3] float32 (unit, towards the camera; zeros
    where there is no depth or the pixel is flat), theta [F,H,W] float32 (the angle between normal and viewing ray, in
    [0, pi/2]), flat_counts [F] int32 (pixels with depth but without a slope).  No read-back."""
    depth, label, intr = _frames(depth, label, intrinsics)
    F, H, W = (int(x) for x in depth.shape)
    dev = depth.device
    normals = _lib.empty((F, H, W, 3), dtype=torch.float32, device=dev)
    theta = _lib.empty((F, H, W), dtype=torch.float32, device=dev)
    flat = _lib.empty((F,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_depth_normals(F, H, W, ptr(depth), ptr(label), ptr(intr), ptr(normals), ptr(theta),
                                                     ptr(flat), stream()), "cloudaae_depth_normals")
    return dict(normals=normals, theta=theta, flat_counts=flat)


def apply(depth, label, intrinsics, sensor, seed=0, first_frame=0, return_z=False):
    """The sensor model on F frames.  sensor: a preset's name or a dict of sensor_params.  Frame f of the call has the
    global index first_frame + f: the same (seed, global index) gives the same frame whatever F or the launch split.
    -> dict of device tensors: depth [F,H,W] int16 (the uint16 bits, the form extract_segments and bop_score.vsd take),
    label [F,H,W] uint8, counts [F,4] int32 (pixels with input depth; dropped by angle; dropped by chance; lost to range
    or disparity) and, with return_z, z_noisy [F,H,W] float64 (the depth after the axial noise, before dropout, disparity
    steps and quantisation; 0 where there is no depth).  No read-back."""
    p = sensor_params(sensor) if isinstance(sensor, str) else sensor_params('none', **dict(sensor))
    depth, label, intr = _frames(depth, label, intrinsics)
    F, H, W = (int(x) for x in depth.shape)
    require(0 <= int(first_frame) and int(first_frame) + F <= MAX_FRAME, "global frame indices must lie below 2^40")
    dev = depth.device
    depth_out = _lib.empty((F, H, W), dtype=torch.int16, device=dev)
    label_out = _lib.empty((F, H, W), dtype=torch.uint8, device=dev)
    counts = _lib.empty((F, 4), dtype=torch.int32, device=dev)
    z = _lib.empty((F, H, W), dtype=torch.float64, device=dev) if return_z else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cloudaae_depth_sensor_noise(F, H, W, ptr(depth), ptr(label), ptr(intr), int(seed) % (1 << 64),
                                                          int(first_frame), *[p[k] for k in PARAMS], ptr(depth_out),
                                                          ptr(label_out), ptr(counts), ptr(z), stream()),
                   "cloudaae_depth_sensor_noise")
    out = dict(depth=depth_out, label=label_out, counts=counts)
    if return_z:
        out['z_noisy'] = z
    return out
