"""A plain numpy restatement of the q-state engine's scaling measurement, written from the definition in
include/dqmc_hip.h ("Scaling" of the q-state section) and independent of the product (test infrastructure).

  tables   cos_q30[k][i] = llround(cos(k . r_i) 2^30), sin_q30 likewise
  exact    Ac[t] = sum_{i: s_i = t} cos_q30[k][i], As[t] likewise, int64, over the N sites
  fp64     for (u, A) = (c_q30, Ac), (c_q30, As), (s_q30, Ac), (s_q30, As): F = +0.0, then F = F + u[t] * A[t] for
           t = 0 .. q - 1, every operation an IEEE double operation of its own (numpy scalars: no fused multiply-add)
  S_k      ((((F1 F1 + F2 F2) + F3 F3) + F4 F4)) * inv, inv = 1.0 / (N 2^120)
  m2       x x + y y with (x, y) = (Mx, My) 2^-30, the value of the engine's measurement
  binner   LogBinnerRef over the elements [M2, S_0 ..] with the cross sums of (M2, S_k), taken where x2_sum takes the
           squares
  xi_k     sqrt(<M2> / (N <S_k>) - 1) / (2 sin(|k| / 2)); its error by the delta method"""
import numpy as np

from logbinner_ref import DEFAULT_CAPACITY, LogBinnerRef, combine_walkers  # noqa: F401

Q30 = 2.0 ** 30


def llround(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int64)


def q30(positions, k_vectors):
    """(cos_q30, sin_q30) as int64 [n_k][N]"""
    r = np.array(positions, dtype=float)
    k = np.array(k_vectors, dtype=float).reshape(-1, r.shape[1])
    ph = k @ r.T
    return llround(np.cos(ph) * Q30), llround(np.sin(ph) * Q30)


def state_tables(q):
    """(c_q30, s_q30) int64 [q]"""
    ang = 2.0 * np.pi * np.arange(q) / q
    return llround(np.cos(ang) * Q30), llround(np.sin(ang) * Q30)


def state_sums(conf, q, table):
    """A[k][t] = sum_{i: s_i = t} table[k][i], int64 [n_k][q]"""
    conf = np.asarray(conf, dtype=np.int64).reshape(-1)
    table = np.asarray(table, dtype=np.int64)
    assert table.shape[1] == conf.size
    return np.stack([table[:, conf == t].sum(axis=1) for t in range(q)], axis=1)


def amplitudes(conf, c_q30, s_q30, cos_q30, sin_q30):
    """F[k][4] = (F1, F2, F3, F4) of every wave vector, the ordered fp64 contraction over the states"""
    q = len(c_q30)
    Ac, As = state_sums(conf, q, cos_q30), state_sums(conf, q, sin_q30)
    out = np.zeros((len(Ac), 4))
    for k in range(len(Ac)):
        for j, (u, A) in enumerate(((c_q30, Ac[k]), (c_q30, As[k]), (s_q30, Ac[k]), (s_q30, As[k]))):
            F = np.float64(0.0)
            for t in range(q):
                F = F + np.float64(int(u[t])) * np.float64(int(A[t]))
            out[k, j] = F
    return out


def S(conf, c_q30, s_q30, cos_q30, sin_q30):
    """S_k of one configuration, float64 [n_k]"""
    N = np.asarray(conf).size
    inv = np.float64(1.0) / (np.float64(N) * np.float64(2.0 ** 120))
    F = amplitudes(conf, c_q30, s_q30, cos_q30, sin_q30)
    return np.array([((((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) + f[3] * f[3])) * inv for f in F], dtype=np.float64)


def order_parameter(conf, c_q30, s_q30):
    conf = np.asarray(conf, dtype=np.int64).reshape(-1)
    return int(np.asarray(c_q30, dtype=np.int64)[conf].sum()), int(np.asarray(s_q30, dtype=np.int64)[conf].sum())


def m2(conf, c_q30, s_q30):
    Mx, My = order_parameter(conf, c_q30, s_q30)
    x, y = np.float64(Mx) * np.float64(1.0 / Q30), np.float64(My) * np.float64(1.0 / Q30)
    return x * x + y * y


def values(conf, c_q30, s_q30, cos_q30, sin_q30):
    """[M2, S_0 ..] of one configuration"""
    return np.concatenate([[m2(conf, c_q30, s_q30)], S(conf, c_q30, s_q30, cos_q30, sin_q30)])


class ScalingBinnerRef(LogBinnerRef):
    """one walker's scaling section: elements [M2, S_0 ..], pairs (M2, S_k)"""

    def __init__(self, n_k, capacity=DEFAULT_CAPACITY):
        super().__init__(1 + n_k, capacity)
        self.xy_sum = np.zeros((self.L, n_k))

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


def xi(M2, S_k, N, knorm):
    with np.errstate(invalid="ignore"):  # NaN where S(0) < S_k
        return np.sqrt(M2 / (N * S_k) - 1.0) / (2.0 * np.sin(0.5 * knorm))


def fd_variance(f, x, y, vx, vy, cov, h=1e-6):
    """first-order variance of f(x, y) with the gradient by central differences (relative step h)"""
    gx = (f(x * (1 + h), y) - f(x * (1 - h), y)) / (2 * h * x)
    gy = (f(x, y * (1 + h)) - f(x, y * (1 - h))) / (2 * h * y)
    return gx * gx * vx + gy * gy * vy + 2.0 * gx * gy * cov


# ---- the physics check at beta = 0, shared by the host test (the restatement alone) and the device test
HOT_Q, HOT_L, HOT_W, HOT_MEAS, HOT_SEED = 3, 8, 64, 200, 777


def pooled(binners, element, level=None):
    """(mean, std_error) of one element pooled over independent walkers, by the rules of binned_scaling"""
    c = combine_walkers(binners, level)
    return float(c["mean"][element]), float(c["std_error"][element])
