"""Object candidates from unlabelled depth frames on the GPU: the dominant support plane by hypothesis voting, the
foreground that stands on it, its connected components in the depth image and their ordered table as a label image in
the convention extract_segments takes (0 = none, component k = value k + 1) -- cloudaae_depth_plane,
cloudaae_depth_foreground, cloudaae_depth_components and cloudaae_component_labels; and, in front of the components when
asked for, the cut along the concave creases of the foreground that separates objects that touch --
cloudaae_depth_creases.  The definitions are in DESIGN.md ("Depth components", "Creases").

    s = segment_depth(depth, intrinsics, seed=0)                  # DepthSegments, one read-back of the table
    s = segment_depth(depth, intrinsics, seed=0, creases=True)    # touching objects cut apart at their creases
    k, iou = match_components(s.label, record_label, depth, 10)   # the component that is the record's value 10
"""
import math

import numpy as np
import torch

from .. import _lib
from .._lib import ptr, require, stream
from .frame_inputs import upload_depth, upload_intrinsics

# choices, not measurements
N_HYP = 256
STRIDE = 4
TOL = 0.01                # metres: half the thickness of the plane's slab
MAX_HEIGHT = 0.5          # metres above the plane
MIN_PLANE_PERCENT = 10    # of the tested pixels
JUMP = 0.02               # metres between 4-neighbours of one component
MIN_PIXELS = 200
MAX_COMPONENTS = 32
STEP = 3                  # pixels from a pixel to the two ends of its chord
SMOOTH = 1                # the box of the integer smoothing is (2 SMOOTH + 1)^2 pixels
ANGLE = 30.0              # degrees a fold must deviate from flat


class DepthSegments(object):
    """The result of segment_depth.  Device tensors: label [F,H,W] uint8, root [F,H,W] int32, fg [F,H,W] uint8, plane
    [F,4] float64, plane_hyp [F] int32, count [F,n_hyp] int32, tested [F] int32, jump_units [F] int32 (what `jump` became
    per frame).  Host arrays (numpy, one read-back): n_components, n_candidates [F]; comp_root, comp_size
    [F,max_components]; comp_box [F,max_components,4].  With creases: crease, fg_cut [F,H,W] uint8 (device; fg stays the
    uncut image, the components are those of fg_cut) and n_crease [F] (host, the same read-back)."""


def jump_units(jump, factor_depth):
    """floor(jump * factor_depth + 0.5) in float64 per frame, as pose_verify's tau_units."""
    return np.array([int(math.floor(float(jump) * float(fd) + 0.5)) for fd in np.asarray(factor_depth).reshape(-1)], np.int32)


def find_creases(depth, fg, intrinsics, jump_units, step=STEP, smooth=SMOOTH, angle=ANGLE, n_crease=None):
    """depth [F,H,W] uint16 (numpy, or a tensor holding the bits as int16), fg [F,H,W] uint8, intrinsics [F,5] float32,
    jump_units [F] int32 (device tensors, or numpy) -> dict of device tensors: crease, tested, fg_cut [F,H,W] uint8,
    n_crease [F] int32 (written into the given tensor when there is one) and smooth_map [F,H,W] int32 holding the bits of
    the kernel's uint32 (S << 8) | n.  angle is in degrees; cos(angle)^2 is formed here, once."""
    device = fg.device if isinstance(fg, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    d = upload_depth(depth, device)
    intr = upload_intrinsics(intrinsics, device)
    g = (fg if isinstance(fg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fg))).to(device).contiguous()
    ju = (jump_units if isinstance(jump_units, torch.Tensor)
          else torch.from_numpy(np.ascontiguousarray(jump_units, np.int32))).to(device).contiguous()
    require(d.dim() == 3 and g.shape == d.shape and g.dtype == torch.uint8, "depth and fg must be [F, H, W], fg uint8")
    F, H, W = (int(v) for v in d.shape)
    require(tuple(intr.shape) == (F, 5) and tuple(ju.shape) == (F,) and ju.dtype == torch.int32,
            "intrinsics must be [F, 5] and jump_units [F] int32")
    require(1 <= int(step) <= 8 and 0 <= int(smooth) <= 7, "step must lie in [1, 8] and smooth in [0, 7]")
    c = math.cos(math.radians(float(angle)))
    L = _lib.lib()
    r = dict(crease=torch.empty((F, H, W), dtype=torch.uint8, device=device),
             tested=torch.empty((F, H, W), dtype=torch.uint8, device=device),
             fg_cut=torch.empty((F, H, W), dtype=torch.uint8, device=device),
             n_crease=torch.empty((F,), dtype=torch.int32, device=device) if n_crease is None else n_crease)
    nbytes = int(L.cloudaae_depth_creases_workspace_bytes(F, H, W))
    require(nbytes > 0, "frame batch above the kernel's limit")
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=device)
    _lib.check(L.cloudaae_depth_creases(F, H, W, d.data_ptr(), ptr(g), ptr(intr), ptr(ju), int(step), int(smooth), c * c,
                                        ptr(r["crease"]), ptr(r["tested"]), ptr(r["fg_cut"]), r["n_crease"].data_ptr(), ptr(ws),
                                        nbytes, stream()), "cloudaae_depth_creases")
    r["smooth_map"] = ws[:F * H * W].view(F, H, W)          # the workspace's first F H W words
    return r


def segment_depth(depth, intrinsics, seed=0, first_frame=0, n_hyp=N_HYP, stride=STRIDE, tol=TOL, max_height=MAX_HEIGHT,
                  min_plane_percent=MIN_PLANE_PERCENT, jump=JUMP, min_pixels=MIN_PIXELS, max_components=MAX_COMPONENTS,
                  device=None, creases=None):
    """depth [F,H,W] uint16 (numpy, or a tensor holding the bits as int16), intrinsics [F,5] float32 (fx, fy, cx, cy,
    factor_depth) -> DepthSegments.  Frame f draws its plane hypotheses from (seed, first_frame + f), so a frame's result
    does not depend on the batch it arrives in.  Raises when a bounded walk of the component kernels hit its bound.
    creases: None (nothing changes), True (the defaults) or a dict with any of step, smooth, angle: find_creases runs after
    the foreground and the components are those of its fg_cut."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    d = upload_depth(depth, device)
    intr = upload_intrinsics(intrinsics, device)
    require(d.dim() == 3, "depth must be [F, H, W]")
    F, H, W = (int(v) for v in d.shape)
    require(tuple(intr.shape) == (F, 5), "intrinsics must be [F, 5]")
    require(F >= 1, "no frame to segment")
    K = int(max_components)
    L = _lib.lib()
    st = stream()
    r = DepthSegments()
    r.count = torch.empty((F, int(n_hyp)), dtype=torch.int32, device=device)
    r.tested = torch.empty((F,), dtype=torch.int32, device=device)
    r.plane = torch.empty((F, 4), dtype=torch.float64, device=device)
    r.plane_hyp = torch.empty((F,), dtype=torch.int32, device=device)
    _lib.check(L.cloudaae_depth_plane(F, H, W, d.data_ptr(), ptr(intr), int(seed) % (1 << 64), int(first_frame), int(n_hyp),
                                      int(stride), float(tol), int(min_plane_percent), ptr(r.count), ptr(r.tested),
                                      ptr(r.plane), ptr(r.plane_hyp), st), "cloudaae_depth_plane")
    r.fg = torch.empty((F, H, W), dtype=torch.uint8, device=device)
    _lib.check(L.cloudaae_depth_foreground(F, H, W, d.data_ptr(), ptr(intr), ptr(r.plane), ptr(r.plane_hyp), float(tol),
                                           float(max_height), ptr(r.fg), st), "cloudaae_depth_foreground")
    cut = None if creases is None or creases is False else ({} if creases is True else dict(creases))
    # one read-back buffer: status | n_components | n_candidates | comp_root | comp_size | comp_box (| n_crease)
    host = torch.empty((3 * F + 6 * F * K + (F if cut is not None else 0),), dtype=torch.int32, device=device)
    status, n_comp, n_cand = host[:F], host[F:2 * F], host[2 * F:3 * F]
    comp_root = host[3 * F:3 * F + F * K]
    comp_size = host[3 * F + F * K:3 * F + 2 * F * K]
    comp_box = host[3 * F + 2 * F * K:3 * F + 6 * F * K]
    factor = (intrinsics[:, 4].cpu().numpy() if isinstance(intrinsics, torch.Tensor)       # (a tensor costs a second read-back)
              else np.asarray(intrinsics, np.float32)[:, 4])
    ju = torch.from_numpy(jump_units(jump, factor.astype(np.float64))).to(device)
    r.root = torch.empty((F, H, W), dtype=torch.int32, device=device)
    nbytes = int(L.cloudaae_depth_components_workspace_bytes(F, H, W))
    require(nbytes > 0, "frame batch above the kernel's limit")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    fg = r.fg
    if cut is not None:
        c = find_creases(d, r.fg, intr, ju, n_crease=host[3 * F + 6 * F * K:], **cut)
        r.crease, r.fg_cut = c["crease"], c["fg_cut"]
        fg = r.fg_cut
    _lib.check(L.cloudaae_depth_components(F, H, W, d.data_ptr(), ptr(fg), ptr(ju), ptr(r.root), status.data_ptr(), ptr(ws),
                                           nbytes, st), "cloudaae_depth_components")
    r.label = torch.empty((F, H, W), dtype=torch.uint8, device=device)
    nbytes = int(L.cloudaae_component_labels_workspace_bytes(F, H, W))
    ws2 = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    _lib.check(L.cloudaae_component_labels(F, H, W, ptr(r.root), int(min_pixels), K, ptr(r.label), n_comp.data_ptr(),
                                           n_cand.data_ptr(), comp_root.data_ptr(), comp_size.data_ptr(), comp_box.data_ptr(),
                                           ptr(ws2), nbytes, st), "cloudaae_component_labels")
    h = host.cpu().numpy()                                   # the one read-back
    bad = np.nonzero(h[:F])[0]
    if len(bad):
        raise _lib.HipLibraryError("cloudaae_depth_components: a bounded walk hit its bound in frame %d (status %d)"
                                   % (int(bad[0]), int(h[bad[0]])))
    r.n_components, r.n_candidates = h[F:2 * F].copy(), h[2 * F:3 * F].copy()
    r.comp_root = h[3 * F:3 * F + F * K].reshape(F, K).copy()
    r.comp_size = h[3 * F + F * K:3 * F + 2 * F * K].reshape(F, K).copy()
    r.comp_box = h[3 * F + 2 * F * K:3 * F + 6 * F * K].reshape(F, K, 4).copy()
    if cut is not None:
        r.n_crease = h[3 * F + 6 * F * K:].copy()
    r.jump_units = ju
    return r


def match_components(found_label, other_label, depth, value):
    """Per frame, the component of found_label [F,H,W] uint8 with the largest IoU against the pixels with other_label ==
    value and depth != 0 (device tensors; depth as int16 bits or numpy uint16).  The contingency counts come from
    torch.bincount; the comparison is exact in integers (n_k union_j > n_j union_k, ties to the lowest k).  Returns
    (k [F] int64 numpy, 0 when nothing overlaps; iou [F] float64 numpy)."""
    device = found_label.device
    d = upload_depth(depth, device)
    other = other_label if isinstance(other_label, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(other_label))
    other = other.to(device)
    F = int(found_label.shape[0])
    found = found_label.reshape(F, -1).to(torch.int64)
    target = ((other.reshape(F, -1) == int(value)) & (d.reshape(F, -1) != 0)).to(torch.int64)
    frame = torch.arange(F, device=device, dtype=torch.int64)[:, None]
    cells = torch.bincount(((frame * 256 + found) * 2 + target).reshape(-1), minlength=F * 512).reshape(F, 256, 2).cpu().numpy()
    ks, ious = np.zeros(F, np.int64), np.zeros(F, np.float64)
    for f in range(F):
        n_target = int(cells[f, :, 1].sum())
        best, best_n, best_u = 0, 0, 1
        for k in range(1, 256):
            n = int(cells[f, k, 1])
            u = int(cells[f, k, 0]) + n_target                 # |k| + |target| - n = (both k's cells) + (target - n)
            if n > 0 and n * best_u > best_n * u:
                best, best_n, best_u = k, n, u
        ks[f], ious[f] = best, (float(best_n) / float(best_u) if best else 0.0)
    return ks, ious
