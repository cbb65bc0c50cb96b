"""Surface normals from the covariance of a radius neighbourhood -- cloudaae_estimate_normals (csrc/normals.hip).
The definition is in DESIGN.md ("Surface normals")."""
import ctypes

import torch

from .. import _lib
from .._lib import ptr, require, stream
from .icp import _points

_offsets = {}      # (device, S, K) -> [S+1] int32 offsets of S sets of K points (kept: recorded plans hold their address)


def uniform_offsets(S, K, device):
    """offsets [S+1] int32 of S packed sets of K points each.  One tensor per shape and device, made by a fill
    that takes no device tensor, so a recorded evaluation pass may ask for it."""
    key = (str(device), int(S), int(K))
    if key not in _offsets:
        _offsets[key] = torch.arange(0, (int(S) + 1) * int(K), int(K), dtype=torch.int32, device=device)
    return _offsets[key]


def estimate_normals(xyz, radius, queries=None, offsets=None, min_neighbors=3, viewpoint=None):
    """Normals of `queries` from their neighbours within `radius` in the support sets `xyz` (float32, one GPU).
    xyz [S,K,>=3] (S sets of K points; rows wider than 3 are read in place: obj_batch [B,2048,6]) or, with
    offsets [S+1] int32, the packed sets xyz [M,>=3].  queries [S,Q,>=3]; None = the support itself (batched form
    only).  viewpoint: three numbers; an estimated normal is flipped to face it.
    Returns (normals [S,Q,3] f64 unit vectors, eigenvalues [S,Q,3] f64 ascending, count [S,Q] int32).  A query
    with fewer than min_neighbors (>= 3) neighbours gets (0, 0, 1), zeros and its count.  Only the library's kernels
    run (outputs and workspace from _lib.empty), so the call records into a StepPlan and replays."""
    require(isinstance(xyz, torch.Tensor) and xyz.dtype == torch.float32, "xyz must be a float32 tensor")
    if not xyz.is_cuda:
        raise _lib.HipLibraryError("cloudaae_amd ops run on the GPU only; got a %s tensor" % xyz.device)
    dev = xyz.device
    if offsets is None:
        sp, sps, scs, K = _points(xyz, "xyz")
        S = int(xyz.shape[0])
        require(S >= 1 and K >= 1, "xyz must hold at least one set of at least one point")
        require(S == 1 or scs == K * sps, "the sets of a batched xyz must follow each other without gaps")
        M = S * K
        offsets = uniform_offsets(S, K, dev)
        if queries is None:
            queries = xyz
    else:
        require(xyz.dim() == 2 and xyz.shape[1] >= 3 and xyz.stride(1) == 1 and xyz.shape[0] >= 1,
                "a packed xyz must be [M, >=3] with contiguous coordinates")
        require(isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int32 and offsets.dim() == 1 and
                offsets.numel() >= 2 and offsets.device == dev and offsets.is_contiguous(),
                "offsets must be a contiguous int32 [S+1] tensor on xyz's device")
        require(queries is not None, "packed support sets need queries [S, Q, >=3]")
        sp, sps, M = xyz.data_ptr(), int(xyz.stride(0)), int(xyz.shape[0])
        S = int(offsets.numel()) - 1
    qp, qps, qss, Q = _points(queries, "queries")
    require(int(queries.shape[0]) == S and queries.device == dev and Q >= 1,
            "queries must be [S, Q, >=3] on xyz's device")
    vp = None
    if viewpoint is not None:
        v = [float(c) for c in (viewpoint.tolist() if isinstance(viewpoint, torch.Tensor) else viewpoint)]
        require(len(v) == 3, "viewpoint must hold three numbers")
        vp = (ctypes.c_double * 3)(*v)
    L = _lib.lib()
    nbytes = int(L.cloudaae_estimate_normals_workspace_bytes(S, M))
    require(nbytes > 0, "support above the kernel's limit")
    ws = _lib.empty((nbytes,), dtype=torch.uint8, device=dev)
    normals = _lib.empty((S, Q, 3), dtype=torch.float64, device=dev)
    eig = _lib.empty((S, Q, 3), dtype=torch.float64, device=dev)
    count = _lib.empty((S, Q), dtype=torch.int32, device=dev)
    _lib.check(L.cloudaae_estimate_normals(S, offsets.data_ptr(), sp, sps, M, Q, qp, qps, qss, float(radius),
                                           int(min_neighbors), vp, ptr(normals), ptr(eig), count.data_ptr(), ptr(ws),
                                           nbytes, stream()), "cloudaae_estimate_normals")
    return normals, eig, count
