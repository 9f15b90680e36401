"""A plain numpy restatement of the Ising flavor's per-walker binner, written from the contract in include/dqmc_hip.h
("error bars of the MC flavor") on top of logbinner_ref.LogBinnerRef and independent of the product (test
infrastructure, float64 throughout).

Elements [E, E2, M, M2] with M = |M|; next to x_sum and x2_sum every level keeps xy_sum[2], the sum of the products of
the level's two values of the pairs (E, E2) and (M, M2), taken exactly where x2_sum takes the squares.  Per level with
n = count: covN = (xy_sum/(n-1) - x_sum y_sum/(n(n-1)))/n, NaN below two samples, and the delta method gives the error
of a fluctuation observable scale (<x2> - <x>^2):  var = scale^2 (varN(x2) - 4 <x> covN(x, x2) + 4 <x>^2 varN(x))."""
import numpy as np

from logbinner_ref import DEFAULT_CAPACITY, LogBinnerRef, varN_from_sums

PAIRS = ((0, 1), (2, 3))


class IsingBinnerRef(LogBinnerRef):
    """the binners of n_walkers chains that measure at the same sweeps: LogBinnerRef over 4 n_walkers elements
    (walker-major), read back per walker"""

    def __init__(self, capacity=DEFAULT_CAPACITY, n_walkers=1):
        super().__init__(4 * n_walkers, capacity)
        self.W = int(n_walkers)
        self.xy_sum = np.zeros((self.L, self.W, 2))

    def push_EM(self, E, M):
        """one measurement of every walker: integer E and M, arrays of n_walkers (or scalars for one walker)"""
        e = np.asarray(E, dtype=np.float64).reshape(self.W)
        m = np.abs(np.asarray(M, dtype=np.float64).reshape(self.W))
        self.push(np.stack([e, e * e, m, m * m], axis=1))

    def push(self, x):
        """LogBinnerRef.push with the cross sums: the value a level receives is rebuilt from the compressors the
        push is about to consume"""
        x = np.array(x, dtype=np.float64).reshape(self.E)
        if self.count[0] < self.capacity:
            v = x.copy()
            for l in range(self.L):
                vv = v.reshape(self.W, 4)
                for q, (a, b) in enumerate(PAIRS):
                    self.xy_sum[l, :, q] += vv[:, a] * vv[:, b]
                if not self.full[l]:
                    break
                v = 0.5 * (self.c[l] + v)
        super().push(x)

    # ---- one walker's view
    def sums(self, walker, level):
        """(x_sum[4], x2_sum[4], xy_sum[2], count) of one level of one walker"""
        k = slice(4 * walker, 4 * walker + 4)
        return self.x_sum[level, k], self.x2_sum[level, k], self.xy_sum[level, walker], int(self.count[level])

    def mean_w(self, walker):
        return self.mean()[4 * walker:4 * walker + 4]

    def varN_w(self, walker, level):
        return self.varN(level)[4 * walker:4 * walker + 4]

    def covN_w(self, walker, level):
        xs, _, xy, n = self.sums(walker, level)
        return np.array([covN_from_sums(xs[a], xs[b], xy[q], n) for q, (a, b) in enumerate(PAIRS)])

    def tau_w(self, walker, level=None):
        return self.tau(level)[4 * walker:4 * walker + 4]

    def fluctuation(self, walker, scale, pair, level=None):
        """(value, variance of the value clamped at 0) of scale (<x2> - <x>^2) for pair 0 (E, E2) or 1 (M, M2)"""
        level = self.reliable_level() if level is None else level
        a, b = PAIRS[pair]
        mean, vN = self.mean_w(walker), self.varN_w(walker, level)
        var = delta_variance(scale, mean[a], vN[a], vN[b], self.covN_w(walker, level)[pair])
        return scale * (mean[b] - mean[a] * mean[a]), var


def covN_from_sums(x_sum, y_sum, xy_sum, n):
    if n < 2:
        return np.nan
    return (xy_sum / (n - 1.0) - x_sum * y_sum / (n * (n - 1.0))) / n


def delta_variance(scale, x, varN_x, varN_x2, covN_x_x2):
    var = scale * scale * (varN_x2 - 4.0 * x * covN_x_x2 + 4.0 * x * x * varN_x)
    return np.maximum(var, 0.0)  # (np.maximum keeps a NaN)


def from_series(E, M, capacity=DEFAULT_CAPACITY):
    """E, M: [n_measurements][n_walkers] (or 1-D for one walker)"""
    E, M = np.asarray(E), np.asarray(M)
    if E.ndim == 1:
        E, M = E[:, None], M[:, None]
    b = IsingBinnerRef(capacity, E.shape[1])
    for e, m in zip(E, M):
        b.push_EM(e, m)
    return b


def pool(values, variances):
    """W chains of one beta: mean = sum mean_w / W, std_error = sqrt(sum var_w) / W, std_error_walkers =
    sqrt(sum (mean_w - mean)^2 / (W (W - 1)))"""
    v, q = np.asarray(values, dtype=np.float64), np.asarray(variances, dtype=np.float64)
    W = float(len(v))
    mean = v.sum() / W
    with np.errstate(invalid="ignore", divide="ignore"):
        sew = np.sqrt(((v - mean) ** 2).sum() / (W * (W - 1.0))) if W >= 2 else np.nan
    return mean, np.sqrt(np.maximum(q.sum(), 0.0)) / W, sew


__all__ = ["IsingBinnerRef", "covN_from_sums", "delta_variance", "from_series", "pool", "varN_from_sums"]
