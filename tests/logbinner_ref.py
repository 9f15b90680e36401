"""A plain numpy LogBinner, written from the contract in include/dqmc_hip.h ("error bars") and independent of the
product: the reference the device binners are compared with (test infrastructure, float64 throughout).

One binner per element of a vector observable: L = ceil(log2(capacity + 1)) levels, each with x_sum, x2_sum, a one-value
compressor and a count.  push(x): for l = 0, 1, ...: sums of level l take x; if the level's compressor is empty, x waits
there and the push ends, else the pair's average is carried to level l + 1."""
import numpy as np

DEFAULT_CAPACITY = 100000


class LogBinnerRef:
    def __init__(self, n_elements, capacity=DEFAULT_CAPACITY):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.capacity = int(capacity)
        self.L = int(np.ceil(np.log2(self.capacity + 1)))
        self.E = int(n_elements)
        self.x_sum = np.zeros((self.L, self.E))
        self.x2_sum = np.zeros((self.L, self.E))
        self.c = np.zeros((self.L, self.E))
        self.full = np.zeros(self.L, dtype=bool)     # compressor of level l holds a value
        self.count = np.zeros(self.L, dtype=np.int64)

    def push(self, x):
        if self.count[0] >= self.capacity:
            raise OverflowError("the binner has reached its capacity of %d" % self.capacity)
        x = np.array(x, dtype=np.float64).reshape(self.E)
        for l in range(self.L):
            self.x_sum[l] += x
            self.x2_sum[l] += x * x
            self.count[l] += 1
            if not self.full[l]:
                self.c[l] = x
                self.full[l] = True
                return
            x = 0.5 * (self.c[l] + x)
            self.full[l] = False
        raise AssertionError("a pair completed on the top level")  # impossible within the capacity

    # ---- per-level statistics
    def reliable_level(self):
        ok = np.nonzero(self.count >= 32)[0]
        return int(ok[-1]) if ok.size else 0

    def mean(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.x_sum[0] / float(self.count[0])

    def varN(self, level):
        return varN_from_sums(self.x_sum[level], self.x2_sum[level], int(self.count[level]))

    def std_error(self, level=None):
        level = self.reliable_level() if level is None else level
        return np.sqrt(np.maximum(self.varN(level), 0.0))  # (np.maximum keeps a NaN)

    def tau(self, level=None):
        level = self.reliable_level() if level is None else level
        with np.errstate(invalid="ignore", divide="ignore"):
            return 0.5 * (self.varN(level) / self.varN(0) - 1.0)


def varN_from_sums(x_sum, x2_sum, n):
    """var / n with var = x2_sum/(n-1) - x_sum^2/(n(n-1)); NaN below two samples"""
    x_sum, x2_sum = np.asarray(x_sum, dtype=np.float64), np.asarray(x2_sum, dtype=np.float64)
    if n < 2:
        return np.full(x_sum.shape, np.nan)
    return (x2_sum / (n - 1.0) - x_sum * x_sum / (n * (n - 1.0))) / n


def combine_walkers(binners, level=None):
    """W independent chains -> dict(mean, std_error, std_error_walkers, tau, level): mean = sum_w mean_w / W,
    std_error = sqrt(sum_w varN_w(l)) / W, tau = (sum_w varN_w(l) / sum_w varN_w(0) - 1)/2, std_error_walkers =
    sqrt(sum_w (mean_w - mean)^2 / (W (W - 1))) (NaN for one walker)"""
    W = len(binners)
    level = binners[0].reliable_level() if level is None else level
    means = np.stack([b.mean() for b in binners])
    vl = np.sum([b.varN(level) for b in binners], axis=0)
    v0 = np.sum([b.varN(0) for b in binners], axis=0)
    mean = means.sum(axis=0) / W
    with np.errstate(invalid="ignore", divide="ignore"):
        sew = np.sqrt(((means - mean) ** 2).sum(axis=0) / (W * (W - 1.0))) if W >= 2 else np.full(mean.shape, np.nan)
        return dict(mean=mean, std_error=np.sqrt(np.maximum(vl, 0.0)) / W, std_error_walkers=sew,
                    tau=0.5 * (vl / v0 - 1.0), level=level, sum_varN_level=vl, sum_varN_0=v0, means=means)


def ar1_series(phi, length, rng, burn=200):
    """x_t = phi x_{t-1} + e_t with unit normal e_t, started from its stationary law after `burn` steps; its
    integrated autocorrelation time in the convention tau = (varN(l -> inf) / varN(0) - 1)/2 is phi / (1 - phi)"""
    e = rng.standard_normal(length + burn)
    x = np.empty(length + burn)
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, length + burn):
        x[t] = phi * x[t - 1] + e[t]
    return x[burn:]
