"""Float64 restatement of the validation metrics for the metric tests, written from the algorithm's description (the contract
of the reference's utils/tools/tf_approxmatch.* and nn_distance.*), not from its source:

  nn_distance(xyz1, xyz2)              brute-force nearest neighbours both ways: squared distances and indices
  approx_match(xyz1, xyz2, n, m)       [b, m, n] approximate EMD assignment (ten levels of three all-pairs passes)
  match_cost(xyz1, xyz2, match)        [b] sum of match[l, k] |xyz2[l] - xyz1[k]|

``dtype=np.float32`` evaluates the same expressions in float32 (np.exp standing in for __expf): the size of the rounding the
GPU kernels should show, used to pick the tests' error bars."""
import numpy as np

LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]  # -4^7 ... -4^-1, then 0


def _pad3(x):
    x = np.asarray(x)
    return np.concatenate([x, np.zeros(x.shape[:-1] + (1,), x.dtype)], -1) if x.shape[-1] == 2 else x


def sqdist(a, b, dtype=np.float64):
    """[n, m] squared distances between the rows of a [n, 3] and b [m, 3]."""
    a, b = _pad3(a).astype(dtype), _pad3(b).astype(dtype)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def nn_distance(xyz1, xyz2):
    """-> (dist1 [b, n], idx1, dist2 [b, m], idx2) in float64; equal distances go to the lowest index (np.argmin)."""
    out = [[], [], [], []]
    for a, b in zip(xyz1, xyz2):
        d = sqdist(a, b)
        out[0].append(d.min(1))
        out[1].append(d.argmin(1))
        out[2].append(d.min(0))
        out[3].append(d.argmin(0))
    return tuple(np.stack(o) for o in out)


def multipliers(ni, mi):
    """(multiL, multiR): the larger set's points carry 1, the smaller set's the INTEGER quotient of the counts."""
    return (1, ni // mi) if ni >= mi else (mi // ni, 1)


def approx_match_one(x1, x2, dtype=np.float64):
    """match [m, n] of one item: x1 [n, 3], x2 [m, 3]."""
    ni, mi = len(x1), len(x2)
    d2 = sqdist(x1, x2, dtype)  # [n, m]
    ml, mr = multipliers(ni, mi)
    remainL = np.full(ni, ml, dtype)
    remainR = np.full(mi, mr, dtype)
    match = np.zeros((mi, ni), dtype)
    eps = dtype(1e-9)
    for level in LEVELS:
        e = np.exp(dtype(level) * d2)
        ratioL = remainL / (eps + e @ remainR)                        # A
        s = remainR * (e.T @ ratioL)                                   # B
        ratioR = np.minimum(remainR / (s + eps), dtype(1)) * remainR
        remainR = np.maximum(dtype(0), remainR - s)
        w = e * ratioL[:, None] * ratioR[None, :]                      # C
        match += w.T
        remainL = np.maximum(dtype(0), remainL - w.sum(1))
    return match


def approx_match(xyz1, xyz2, n=None, m=None, dtype=np.float64):
    """[b, m, n]; n / m: per-batch counts (rows / columns past them are 0)."""
    b, N, M = len(xyz1), xyz1.shape[1], xyz2.shape[1]
    n = [N] * b if n is None else list(n)
    m = [M] * b if m is None else list(m)
    out = np.zeros((b, M, N), dtype)
    for i in range(b):
        if n[i] and m[i]:
            out[i, :m[i], :n[i]] = approx_match_one(xyz1[i, :n[i]], xyz2[i, :m[i]], dtype)
    return out


def match_cost(xyz1, xyz2, match):
    """[b] = sum_{l,k} match[l, k] |xyz2[l] - xyz1[k]|."""
    return np.array([(np.asarray(mt, np.float64) * np.sqrt(sqdist(a, b)).T).sum() for a, b, mt in zip(xyz1, xyz2, match)])


def match_abs_scale(xyz1, xyz2, n=None, m=None):
    """Scale of the element-wise bar on match: the float64 match itself plus 1/64 of its largest entry per item (entries near
    zero come out of differences of O(max) terms: remainR - s, remainL - sum w)."""
    ref = approx_match(xyz1, xyz2, n, m)
    return ref, np.abs(ref) + np.abs(ref).max(axis=(1, 2), keepdims=True) / 64
