"""Float64 NumPy restatement of DESIGN.md "Pose scores": ADD, ADD-S, the model diameter and the data-set summary.  A
yardstick for cloudaae_pose_score / cloudaae_cloud_diameter / cloudaae_pose_matrix and utils/pose_score.py, written
from the definition only.  Transforms are taken element by element in the stated order (no `@`: BLAS may fuse)."""
import numpy as np

from icp_reference import apply, initial_transform          # p = ((T00 x + T01 y) + T02 z) + T03; T0 = [Rodrigues | t]

SYMMETRIC_CLASSES = (12, 15, 18, 19, 20)


def pose_matrix(rot, trans):
    """T0 of "Pose refinement" from an axis-angle (float32 or float64, promoted exactly) and a float32 translation."""
    return initial_transform(np.asarray(rot).astype(np.float64), np.asarray(trans, np.float32).astype(np.float64))


def block_sum(v):
    """The stated order: blocks of 64 consecutive terms (the last one padded with zeros), each folded as a binary
    tree (64 -> 32 -> ... -> 1: the upper half added onto the lower), the blocks' sums added in ascending order."""
    v = np.asarray(v, np.float64)
    pad = (-len(v)) % 64
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, 64)
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = v[:, :h] + v[:, h:]
    total = v[0, 0]
    for t in range(1, len(v)):
        total = total + v[t, 0]
    return total


def nn_d2(G, E, rows=256):
    """min_j ((dx^2 + dy^2) + dz^2), d = G_i - E_j, in row blocks."""
    out = np.empty(len(G))
    for s in range(0, len(G), rows):
        g = G[s:s + rows]
        dx = g[:, 0:1] - E[None, :, 0]
        dy = g[:, 1:2] - E[None, :, 1]
        dz = g[:, 2:3] - E[None, :, 2]
        out[s:s + rows] = ((dx * dx + dy * dy) + dz * dz).min(axis=1)
    return out


def score(model, est, gt):
    """One sample and one pose: model [M,>=3] float32, est and gt [4,4] float64.  Returns (ADD, ADD-S, nn_d2 [M])."""
    X = np.asarray(model)[:, :3].astype(np.float64)
    G, E = apply(np.asarray(gt, np.float64), X), apply(np.asarray(est, np.float64), X)
    d = G - E
    add = block_sum(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])) / len(X)
    nn = nn_d2(G, E)
    return add, block_sum(np.sqrt(nn)) / len(X), nn


def diameter(model, rows=256):
    X = np.asarray(model)[:, :3].astype(np.float64)
    far = 0.0
    for s in range(0, len(X), rows):
        g = X[s:s + rows]
        dx = g[:, 0:1] - X[None, :, 0]
        dy = g[:, 1:2] - X[None, :, 1]
        dz = g[:, 2:3] - X[None, :, 2]
        far = max(far, float(((dx * dx + dy * dy) + dz * dz).max()))
    return np.sqrt(far)


def auc(d, limit=0.1):
    """VOCap of the YCB-Video toolbox as DESIGN.md states it (as recalled, not checked), written as its loops."""
    d = [float(x) for x in d]
    n = len(d)
    kept = sorted(x for x in d if x <= limit)
    if not kept:
        return 0.0
    mrec = [0.0] + kept + [limit]
    mpre = [0.0] + [(k + 1) / n for k in range(len(kept))]
    mpre.append(mpre[-1])
    for i in range(1, len(mpre)):
        mpre[i] = max(mpre[i], mpre[i - 1])
    area = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            area += (mrec[i] - mrec[i - 1]) * mpre[i]
    return area / limit


def summarize(d, diameter=None, limit=0.1):
    d = np.asarray(d, np.float64)
    n = len(d)
    out = {"n": n, "auc": auc(d, limit), "acc_2cm": sum(1 for x in d if x < 0.02) / n if n else 0.0}
    if diameter is not None:
        dm = np.broadcast_to(np.asarray(diameter, np.float64), d.shape)
        out["acc_0.1d"] = sum(1 for x, m in zip(d, dm) if x < 0.1 * m) / n if n else 0.0
    return out


def add_s_pick(class_id, add, adds, symmetric=SYMMETRIC_CLASSES):
    """ADD(-S): ADD-S for the symmetric classes, ADD otherwise."""
    return np.array([s if int(c) in symmetric else a for c, a, s in zip(class_id, add, adds)], np.float64)


def lattice(n=4, spacing=0.01, origin=(0.0, 0.0, 0.0)):
    """n^3 points of a cubic lattice centred on `origin` (float32: pick spacing and origin exactly representable)."""
    k = (np.arange(n) - (n - 1) / 2.0) * spacing
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin)
    return g.astype(np.float32)
