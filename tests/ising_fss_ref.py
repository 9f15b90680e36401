"""A plain numpy restatement of the Ising flavor's finite-size-scaling measurement, written from the contract in
include/dqmc_hip.h ("finite-size-scaling observables") and independent of the product (test infrastructure).

  tables   cos_q30[k][i] = llround(cos(k . r_i) 2^30), sin_q30 likewise (int32)
  F        Fc_k = sum_i s_i cos_q30[k][i], Fs_k likewise, in int64 (exact)
  S_k      ((double)Fc (double)Fc + (double)Fs (double)Fs) * (1 / (N 2^60)), every operation rounded on its own
  M4       m2 * m2 with m2 = (double)(M M)
  binner   LogBinnerRef over the elements [M2, M4, S_0 ..] with the cross sums of (M2, M4) and (M2, S_k), taken where
           x2_sum takes the squares (as ising_binner_ref does for (E, E2) and (M, M2))
  U4       1 - <M4> / (3 <M2>^2);  xi_k = sqrt(<M2> / (N <S_k>) - 1) / (2 sin(|k| / 2)); errors by the delta method"""
import numpy as np

from logbinner_ref import DEFAULT_CAPACITY, LogBinnerRef, varN_from_sums


def reciprocal(lattice_vectors):
    """rows b_j with a_i . b_j = 2 pi delta_ij"""
    A = np.array(lattice_vectors, dtype=float)  # rows a_i
    return 2.0 * np.pi * np.linalg.inv(A).T     # A B^T = 2 pi I


def llround(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int64)


def q30(positions, k_vectors):
    """(cos_q30, sin_q30) as int64 [n_k][N]"""
    r = np.array(positions, dtype=float)
    k = np.array(k_vectors, dtype=float).reshape(-1, r.shape[1])
    ph = k @ r.T
    return llround(np.cos(ph) * 2.0 ** 30), llround(np.sin(ph) * 2.0 ** 30)


def F(conf, table):
    """sum_i s_i table[k][i] in int64, for every k"""
    return np.asarray(table, dtype=np.int64) @ np.asarray(conf, dtype=np.int64).reshape(-1)


def S(conf, cos_q30, sin_q30):
    N = np.asarray(conf).size
    fc, fs = F(conf, cos_q30).astype(np.float64), F(conf, sin_q30).astype(np.float64)
    return (fc * fc + fs * fs) * np.float64(1.0 / (N * 2.0 ** 60))


def M2_M4(conf):
    M = int(np.asarray(conf, dtype=np.int64).sum())
    m2 = np.float64(M * M)
    return m2, m2 * m2


def values(conf, cos_q30, sin_q30):
    """[M2, M4, S_0 ..] of one configuration"""
    m2, m4 = M2_M4(conf)
    return np.concatenate([[m2, m4], S(conf, cos_q30, sin_q30)]) if len(cos_q30) else np.array([m2, m4])


class FssBinnerRef(LogBinnerRef):
    """one walker's FSS section: elements [M2, M4, S_0 ..], pairs (M2, element 1 + q)"""

    def __init__(self, n_k, capacity=DEFAULT_CAPACITY):
        super().__init__(2 + n_k, capacity)
        self.xy_sum = np.zeros((self.L, 1 + n_k))

    def push(self, x):
        x = np.array(x, dtype=np.float64).reshape(self.E)
        if self.count[0] < self.capacity:
            v = x.copy()
            for l in range(self.L):
                self.xy_sum[l] += v[0] * v[1:]
                if not self.full[l]:
                    break
                v = 0.5 * (self.c[l] + v)
        super().push(x)

    def covN(self, level):
        n = int(self.count[level])
        if n < 2:
            return np.full(self.E - 1, np.nan)
        xs = self.x_sum[level]
        return (self.xy_sum[level] / (n - 1.0) - xs[0] * xs[1:] / (n * (n - 1.0))) / n


def binder(M2, M4):
    return 1.0 - M4 / (3.0 * M2 * M2)


def xi(M2, S_k, N, knorm):
    return np.sqrt(M2 / (N * S_k) - 1.0) / (2.0 * np.sin(0.5 * knorm))


def fd_variance(f, x, y, vx, vy, cov, h=1e-6):
    """first-order variance of f(x, y) with the gradient by central differences (relative step h)"""
    gx = (f(x * (1 + h), y) - f(x * (1 - h), y)) / (2 * h * x)
    gy = (f(x, y * (1 + h)) - f(x, y * (1 - h))) / (2 * h * y)
    return gx * gx * vx + gy * gy * vy + 2.0 * gx * gy * cov


__all__ = ["FssBinnerRef", "F", "M2_M4", "S", "binder", "fd_variance", "llround", "q30", "reciprocal", "values",
           "varN_from_sums", "xi"]
