"""Restatement of the q-state engine's binner (csrc/qstate.hip, qs_bin_push) in numpy, written from the definition in
include/dqmc_hip.h ("Binner" of the q-state section) on top of tests/logbinner_ref.py and independent of the product:

  elements    [E, E2, |M|, M2, M2, M4] with the values the sums use: e = E_int 2^-30, e e, sqrt(m2), m2, m2, m2 m2,
              m2 = x x + y y
  pairs       (2 p, 2 p + 1): (E, E2), (|M|, M2), (M2, M4); xy_sum[l][p] takes the product of the pair's two level-l values
              wherever x2_sum[l] takes the squares
  levels      LogBinnerRef's: L = ceil(log2(capacity + 1)), count[l] = T >> l, the push stops at the first level whose
              compressor is empty (the number of trailing 1-bits of the pushes before it)
  finish      mean = x_sum[0] / T, varN and covN = (q/(n - 1) - a b/(n (n - 1)))/n at the level, tau = (varN/varN0 - 1)/2

`QsBinnerRef` holds the binners of all W walkers of a handle as one LogBinnerRef over 6 W elements (element-major, as the
device lays them out), so a push is one vector operation.  Shared by test_qstate_tempering_host.py (CPU) and the GPU tests."""
import numpy as np

from logbinner_ref import LogBinnerRef

Q30 = 2.0 ** 30
N_ELEM, N_PAIRS = 6, 3
SQRT_ELEMENTS = (2,)       # |M|: inherits the device's sqrt
SQRT_PAIRS = (1,)          # (|M|, M2)


def sample(E, Mx, My):
    """[6][W]: the pushed values of every walker from its exact integers"""
    e = np.asarray(E).astype(np.float64) / Q30
    x, y = np.asarray(Mx).astype(np.float64) / Q30, np.asarray(My).astype(np.float64) / Q30
    m2 = x * x + y * y
    return np.stack([e, e * e, np.sqrt(m2), m2, m2, m2 * m2])


class QsBinnerRef(LogBinnerRef):
    def __init__(self, W, capacity):
        super().__init__(N_ELEM * W, capacity)
        self.W = W
        self.xy_sum = np.zeros((self.L, N_PAIRS * W))
        self.T = 0

    def push(self, x):
        """LogBinnerRef.push with the cross sums: the same levels, the same carries"""
        if self.count[0] >= self.capacity:
            raise OverflowError("the binner has reached its capacity of %d" % self.capacity)
        x = np.array(x, dtype=np.float64).reshape(N_ELEM, self.W)
        for l in range(self.L):
            flat = x.reshape(-1)
            self.x_sum[l] += flat
            self.x2_sum[l] += flat * flat
            self.xy_sum[l] += (x[0::2] * x[1::2]).reshape(-1)
            self.count[l] += 1
            if not self.full[l]:
                self.c[l] = flat
                self.full[l] = True
                self.T += 1
                return
            x = 0.5 * (self.c[l].reshape(N_ELEM, self.W) + x)
            self.full[l] = False
        raise AssertionError("a pair completed on the top level")

    def push_measurement(self, E, Mx, My):
        self.push(sample(E, Mx, My))

    def clear(self):
        for a in (self.x_sum, self.x2_sum, self.xy_sum, self.c):
            a[:] = 0.0
        self.full[:] = False
        self.count[:] = 0
        self.T = 0

    def level(self, w, l):
        """(x_sum[6], x2_sum[6], xy_sum[3], count) of one level of one walker"""
        return (self.x_sum[l].reshape(N_ELEM, self.W)[:, w].copy(), self.x2_sum[l].reshape(N_ELEM, self.W)[:, w].copy(),
                self.xy_sum[l].reshape(N_PAIRS, self.W)[:, w].copy(), int(self.count[l]))

    def finish(self, w, level=None):
        """the fields of dqmc_qs_binned, formula by formula"""
        level = self.reliable_level() if level is None else level
        xs0, x20, _, n0 = self.level(w, 0)
        xs, x2, xy, nl = self.level(w, level)
        assert n0 == self.T and nl == self.T >> level
        with np.errstate(invalid="ignore", divide="ignore"):
            varN = np.array([cov_n(xs[k], xs[k], x2[k], nl) for k in range(N_ELEM)])
            varN0 = np.array([cov_n(xs0[k], xs0[k], x20[k], n0) for k in range(N_ELEM)])
            return {"mean": xs0 / float(n0), "varN": varN, "varN0": varN0, "tau": 0.5 * (varN / varN0 - 1.0),
                    "covN": np.array([cov_n(xs[2 * p], xs[2 * p + 1], xy[p], nl) for p in range(N_PAIRS)]),
                    "count": nl, "level": level}


def cov_n(a, b, q, n):
    if n < 2:
        return float("nan")
    n = float(n)
    return (q / (n - 1.0) - a * b / (n * (n - 1.0))) / n
