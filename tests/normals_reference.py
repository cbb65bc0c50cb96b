"""Float64 NumPy restatement of cloudaae_estimate_normals ("Surface normals"): brute-force radius
neighbours, the covariance about their mean in two passes, numpy.linalg.eigh.  A yardstick for the GPU kernel, written
from the definition only.  `reverse` takes every sum over the neighbours in descending instead of ascending index
order: the difference between the two is the measure of what the order of a sum may change."""
import numpy as np


def _seqsum(a):
    return np.cumsum(a, axis=0)[-1]


def neighbours(support, q, radius):
    """Indices (ascending) of the support points with ((dx^2 + dy^2) + dz^2) < r^2, r = (double)(float)radius."""
    r = np.float64(np.float32(radius))
    dx, dy, dz = q[0] - support[:, 0], q[1] - support[:, 1], q[2] - support[:, 2]
    return np.nonzero(((dx * dx + dy * dy) + dz * dz) < r * r)[0]


def estimate_normals(support, radius, queries=None, min_neighbors=3, viewpoint=None, reverse=False):
    """support [M,>=3], queries [K,>=3] (None: the support), float32 promoted exactly.  Returns (normals [K,3],
    eigenvalues [K,3] ascending, count [K] int32).  count < min_neighbors: (0, 0, 1) and zeros.  With a viewpoint v
    an estimated normal is flipped when n . (q - v) > 0; without one the sign is eigh's."""
    support = np.asarray(support, np.float64)[:, :3]
    queries = support if queries is None else np.asarray(queries, np.float64)[:, :3]
    K = len(queries)
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (K, 1))
    eig = np.zeros((K, 3))
    count = np.zeros(K, np.int32)
    for i, q in enumerate(queries):
        idx = neighbours(support, q, radius)
        count[i] = len(idx)
        if len(idx) < min_neighbors:
            continue
        p = support[idx[::-1] if reverse else idx]
        mu = _seqsum(p) / len(p)
        e = p - mu
        C = _seqsum(e[:, :, None] * e[:, None, :]) / len(p)
        w, V = np.linalg.eigh(C)
        n = V[:, 0] / np.linalg.norm(V[:, 0])
        if viewpoint is not None:
            d = q - np.asarray(viewpoint, np.float64)
            if (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] > 0.0:
                n = -n
        normals[i] = n
        eig[i] = w
    return normals, eig, count


def relative_gap(eig):
    """(lambda1 - lambda0) / lambda2 per query (0 where lambda2 is 0): how well the smallest eigenvector is defined."""
    top = eig[:, 2]
    return np.where(top > 0.0, (eig[:, 1] - eig[:, 0]) / np.where(top > 0.0, top, 1.0), 0.0)
