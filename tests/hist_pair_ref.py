"""What evaluation_helper.compare_dist computes on the way to its KL value, in numpy, for the tests of dmcf_hist_pair_ragged:
the two percentiles and the two integer histograms, with the host function's own expressions (np.percentile on the float32
concatenation, the float32 bin width, astype("int32"), np.clip, np.ravel_multi_index, np.bincount)."""
import numpy as np


def lerp(a, b, g):
    """numpy's _lerp on float32 scalars."""
    a, b, g = np.float32(a), np.float32(b), np.float32(g)
    d = b - a
    r = a + d * g
    if g >= np.float32(0.5):
        r = b - d * (np.float32(1) - g)
    return r


def percentiles_and_counts(x, y, bin_size=25):
    """-> (percentiles [2, dim], counts of x [(per + 1)^dim], counts of y): the intermediate values of compare_dist(x, y)."""
    assert x.shape == y.shape
    cnt, dim = x.shape
    per = int((cnt // bin_size) ** (1 / dim))
    both = np.concatenate((x, y), axis=0)
    min_v = np.percentile(both, 5, axis=0)
    max_v = np.percentile(both, 95, axis=0)
    with np.errstate(divide="ignore"):
        bin_w = (max_v - min_v + 1e-6) / per
    shape = (per + 1,) * dim

    def hist(v):
        idx = np.clip(((v - min_v) / bin_w).astype("int32"), 0, per)
        return np.bincount(np.ravel_multi_index(tuple(idx.T), shape), minlength=int(np.prod(shape)))

    return np.stack([min_v, max_v]), hist(x), hist(y)


def kl_from_numpy_counts(x, y, bin_size=25):
    from dmcf_amd.utils.evaluation_helper import _kl_from_counts
    _, cx, cy = percentiles_and_counts(x, y, bin_size)
    return _kl_from_counts(cx, cy)
