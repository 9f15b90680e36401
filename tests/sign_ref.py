"""Sign reweighting restated in numpy (include/dqmc_hip.h "sign reweighting"): what the signed accumulators hold, the
rule for a sign of 0, and the jackknife of the ratio <O s> / <s> over walkers.  Shared by test_sign_reference.py (CPU)
and test_gpu_sign.py.

Samples x [T, W, E] (T measurement points, W walkers, E elements) and signs s [T, W] in {+1, -1, 0}; s = 0 marks a
walker whose determinant could not be signed at that point."""
import numpy as np

SECTIONS = ("greens", "correlations", "pairing", "susceptibilities", "time_displaced")  # DQMC_RED_* order


def weighted_sums(x, s):
    """-> (sum of s x [E], sum of s, samples kept, samples left out per walker [W]).  A sample with s = 0 is not read:
    its x may be anything, NaN included, and it counts nowhere but in the last entry."""
    x, s = np.asarray(x, dtype=np.float64), np.asarray(s)
    acc = np.zeros(x.shape[2])
    for t in range(x.shape[0]):
        for w in range(x.shape[1]):  # measurement points in order, walkers in order: the order of the device sums
            if s[t, w] != 0:
                acc += float(s[t, w]) * x[t, w]
    return acc, float(s.sum()), int((s != 0).sum()), (s == 0).sum(axis=0)


def signed_mean(x, s):
    """<O s> / <s>; ZeroDivisionError when the signs cancel"""
    acc, S, _, _ = weighted_sums(x, s)
    if S == 0:
        raise ZeroDivisionError("the sum of signs is 0")
    return acc / S


def walker_sums(x, s):
    """-> (sx [W, E], sw [W]): each walker's sums of s x and of s over the measurement points (level 0 of its binners; a
    left-out sample enters both as 0)"""
    x, s = np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64)
    kept = np.where(s[:, :, None] != 0, x, 0.0)
    return (s[:, :, None] * kept).sum(axis=0), s.sum(axis=0)


def jackknife_ratio(sx, sw):
    """ratio = sum_w sx_w / sum_w sw_w and its delete-one jackknife error over the W walkers, written out walker by walker:
    r_w = the ratio without walker w, error^2 = (W - 1) / W sum_w (r_w - mean_w r_w)^2"""
    sx, sw = np.asarray(sx, dtype=np.float64), np.asarray(sw, dtype=np.float64)
    W = len(sw)
    if W < 2:
        raise ValueError("needs two walkers")
    if sw.sum() == 0:
        raise ValueError("the signs cancel")
    reps = []
    for w in range(W):
        keep = [v for v in range(W) if v != w]
        den = sw[keep].sum()
        if den == 0:
            raise ValueError("the signs cancel without walker %d" % w)
        reps.append(sx[keep].sum(axis=0) / den)
    reps = np.array(reps)
    return sx.sum(axis=0) / sw.sum(), np.sqrt((W - 1) / W * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0))


def sign_products(case):
    """the per-walker products of the per-block signs of one entry of tests/golden/logdet_sizes.json"""
    return np.array(case["sign"]).prod(axis=1)
