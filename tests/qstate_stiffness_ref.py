"""A plain numpy restatement of the q-state engine's stiffness measurement (the helicity modulus), written from the
definition in include/dqmc_hip.h ("Stiffness" of the q-state section) and independent of the product (test
infrastructure).  The configurations come from the chain restatement of tests/qstate_ref.py.

  tables   d1_q30[d] = llround(J d1[d] 2^30) for d <= q / 2, d1_q30[(q - d) % q] = -d1_q30[d] (0 where d is its own
           mirror); d2_q30 likewise, mirrored with the same sign.  Clock model: d1 = sin(2 pi d / q), d2 = cos(2 pi d / q)
  exact    I_c = sum over the slots (i, k) of class c of d1_q30[(s_i - s_j) mod q], j = neighs[k, i]; K_c with d2_q30;
           int64, the slots of class -1 left out
  fp64     per direction mu: G = +0.0, then G = G + x[mu][c] * float(I_c) for c = 0 .. n_c - 1; F = +0.0, then
           F = F + (x[mu][c] * x[mu][c]) * float(K_c); J = G * 2^-30, T = F * 2^-30, J2 = J * J: every operation an IEEE
           double operation of its own (numpy scalars: no fused multiply-add)
  sums     sum_T += T, sum_J += J, sum_J2 += J2, one rounding each per measurement, in measurement order
  binner   LogBinnerRef over the elements [T_0, J2_0, T_1, J2_1 ..] with the cross sums of the pairs (2 p, 2 p + 1),
           taken where x2_sum takes the squares
  Upsilon  (<T> - beta <J2>) / N; its error by the delta method with the gradient (1 / N, -beta / N)"""
import functools
import math

import numpy as np

import qstate_ref
from logbinner_ref import DEFAULT_CAPACITY, LogBinnerRef  # noqa: F401

Q30 = 2.0 ** 30


def llround(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int64)


def twist_q30(q, d1, d2, J=1.0):
    """(d1_q30, d2_q30) int64 [q]"""
    a, b = np.zeros(q, dtype=np.int64), np.zeros(q, dtype=np.int64)
    for d in range(q // 2 + 1):
        m = (q - d) % q
        a[d] = 0 if m == d else int(llround(J * d1[d] * Q30))
        a[m] = -a[d]
        b[d] = b[m] = int(llround(J * d2[d] * Q30))
    return a, b


def clock_twist(q):
    """(d1, d2) fp64 [q] of the clock model: sin and cos of 2 pi d / q, d <= q / 2 computed, the rest mirrored"""
    d1, d2 = np.zeros(q), np.zeros(q)
    for d in range(q // 2 + 1):
        m = (q - d) % q
        d2[d] = d2[m] = math.cos(2.0 * math.pi * d / q)
        if m != d:
            d1[d] = math.sin(2.0 * math.pi * d / q)
            d1[m] = -d1[d]
    return d1, d2


def class_sums(conf, neighs, slot_class, q, d1_q30, d2_q30, n_c):
    """(I, K) int64 [..., n_c] of the configurations conf [..., N]; neighs [z][N] 1-based, slot_class [z][N]"""
    conf = np.asarray(conf, dtype=np.int64)
    nb = np.asarray(neighs, dtype=np.int64) - 1
    cls = np.asarray(slot_class, dtype=np.int64)
    I = np.zeros(conf.shape[:-1] + (n_c,), dtype=np.int64)
    K = np.zeros(conf.shape[:-1] + (n_c,), dtype=np.int64)
    for k in range(nb.shape[0]):
        d = (conf - conf[..., nb[k]]) % q          # [..., N]: s_i - s_j of slot (i, k)
        for c in range(n_c):
            on = cls[k] == c
            if on.any():
                I[..., c] += np.asarray(d1_q30, dtype=np.int64)[d[..., on]].sum(axis=-1)
                K[..., c] += np.asarray(d2_q30, dtype=np.int64)[d[..., on]].sum(axis=-1)
    return I, K


def contract(I, K, x):
    """(T, J, J2) float64 [n_dir] of one sample, operation by operation"""
    x = np.asarray(x, dtype=np.float64)
    T, J, J2 = np.zeros(len(x)), np.zeros(len(x)), np.zeros(len(x))
    scale = np.float64(1.0 / Q30)
    for mu in range(len(x)):
        G, F = np.float64(0.0), np.float64(0.0)
        for c in range(x.shape[1]):
            xc = np.float64(x[mu, c])
            G = G + xc * np.float64(int(I[c]))
            F = F + (xc * xc) * np.float64(int(K[c]))
        Jv = G * scale
        T[mu], J[mu], J2[mu] = F * scale, Jv, Jv * Jv
    return T, J, J2


def elements(T, J2):
    """[T_0, J2_0, T_1, J2_1 ..]"""
    return np.stack([T, J2], axis=1).reshape(-1)


class Measurer:
    """what one handle's walkers `ws` accumulate, fed one configuration per walker and measurement"""

    def __init__(self, l, q, twist, x, slot_class, ws, J=1.0, capacity=None):
        self.neighs, self.cls, self.x, self.q = np.asarray(l.neighs), np.asarray(slot_class), np.asarray(x, dtype=np.float64), q
        self.d1, self.d2 = twist_q30(q, twist[0], twist[1], J)
        self.n_dir, self.n_c = self.x.shape
        self.ws, self.n = list(ws), 0
        self.sum_T = {w: np.zeros(self.n_dir) for w in self.ws}
        self.sum_J = {w: np.zeros(self.n_dir) for w in self.ws}
        self.sum_J2 = {w: np.zeros(self.n_dir) for w in self.ws}
        self.sample = {w: None for w in self.ws}
        self.bins = {w: StiffnessBinnerRef(self.n_dir, capacity) for w in self.ws} if capacity else None

    def take(self, conf_of):
        self.n += 1
        for w in self.ws:
            I, K = class_sums(conf_of(w), self.neighs, self.cls, self.q, self.d1, self.d2, self.n_c)
            T, J, J2 = contract(I, K, self.x)
            self.sum_T[w] = self.sum_T[w] + T
            self.sum_J[w] = self.sum_J[w] + J
            self.sum_J2[w] = self.sum_J2[w] + J2
            self.sample[w] = (I, K)
            if self.bins:
                self.bins[w].push(elements(T, J2))


class StiffnessBinnerRef(LogBinnerRef):
    """one walker's stiffness section: elements [T_0, J2_0, ..], pairs (2 p, 2 p + 1)"""

    def __init__(self, n_dir, capacity=DEFAULT_CAPACITY):
        super().__init__(2 * n_dir, capacity)
        self.xy_sum = np.zeros((self.L, n_dir))

    def push(self, x):
        x = np.array(x, dtype=np.float64).reshape(self.E)
        if self.count[0] < self.capacity:
            v = x.copy()
            for l in range(self.L):
                self.xy_sum[l] += v[0::2] * v[1::2]
                if not self.full[l]:
                    break
                v = 0.5 * (self.c[l] + v)
        super().push(x)

    def covN(self, level):
        n = int(self.count[level])
        if n < 2:
            return np.full(self.E // 2, np.nan)
        xs = self.x_sum[level]
        return (self.xy_sum[level] / (n - 1.0) - xs[0::2] * xs[1::2] / (n * (n - 1.0))) / n


def upsilon(T, J2, beta, N):
    return (T - beta * J2) / N


def upsilon_var(vT, vJ2, cov, beta, N):
    """first-order variance of Upsilon from the variances of the means of T and J2 and their covariance"""
    gT, gJ = 1.0 / N, -beta / N
    v = gT * gT * vT + gJ * gJ * vJ2 + 2.0 * gT * gJ * cov
    return max(v, 0.0) if v == v else v


def binned_upsilon(b, mu, beta, N, level=None):
    """(Upsilon_mu, its variance) of one walker's binner"""
    level = b.reliable_level() if level is None else level
    m, v, c = b.mean(), b.varN(level), b.covN(level)
    return upsilon(m[2 * mu], m[2 * mu + 1], beta, N), upsilon_var(v[2 * mu], v[2 * mu + 1], c[mu], beta, N)


def pooled_upsilon(binners, mu, beta, N, level=None):
    """(mean, std_error) over independent walkers of equal beta: Upsilon per walker first, sqrt(sum_w var_w) / W"""
    per = [binned_upsilon(b, mu, beta, N, level) for b in binners]
    W = float(len(per))
    return float(sum(p[0] for p in per) / W), math.sqrt(max(sum(p[1] for p in per), 0.0)) / W


# ---- the identity Upsilon = (1/N) d^2F/dphi^2 by enumeration
def twisted_lnZ(l, q, slot_class, xs, beta, phi, J=1.0):
    """ln Z(phi) of the clock model with the bond (i, j) of a counted slot at -J cos(theta_i - theta_j - phi x_c), all q^N
    states in float64; xs[c] the projection of class c on the twist direction"""
    st = qstate_ref.all_states(len(l), q)
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    cls = np.asarray(slot_class)
    E = np.zeros(len(st))
    for k in range(nb.shape[0]):
        for i in range(nb.shape[1]):
            c = cls[k, i]
            if c >= 0:
                E -= J * np.cos(2.0 * np.pi * (st[:, i] - st[:, nb[k, i]]) / q - phi * xs[c])
    a = -beta * E
    top = a.max()
    return float(top + np.log(np.exp(a - top).sum()))


def upsilon_exact(l, q, slot_class, x, beta, J=1.0):
    """Upsilon_mu [n_dir] of the clock model from the restatement's per-configuration T and J over all q^N states,
    Boltzmann-weighted with the engine's integer energy"""
    st = qstate_ref.all_states(len(l), q)
    e_q30, _, _ = qstate_ref.tables(q, qstate_ref.clock_table(q), J)
    E = qstate_ref.state_energies_q30(l, q, e_q30, st).astype(np.float64) / Q30
    wgt = np.exp(-beta * (E - E.min()))
    wgt /= wgt.sum()
    d1, d2 = twist_q30(q, *clock_twist(q), J)
    x = np.asarray(x, dtype=np.float64)
    I, K = class_sums(st, l.neighs, slot_class, q, d1, d2, x.shape[1])
    out = np.zeros(len(x))
    for mu in range(len(x)):
        Jm = (I.astype(np.float64) @ x[mu]) / Q30
        Tm = (K.astype(np.float64) @ (x[mu] * x[mu])) / Q30
        out[mu] = (wgt @ Tm - beta * (wgt @ (Jm * Jm))) / len(l)
    return out


# ---- the physics check: clock q = 6 on SquareLattice(8), shared by the host test (the restatement alone) and the device
PHYS_Q, PHYS_L, PHYS_THERM, PHYS_SWEEPS, PHYS_SEED, PHYS_REF_W = 6, 8, 500, 2000, 2024, 8


@functools.lru_cache(maxsize=2)
def physics_reference(beta):
    """(Upsilon_x, err_x, Upsilon_y, err_y) from PHYS_REF_W walkers of the chain restatement (local sweeps only: the
    same stationary distribution as the device's sweeps with cluster moves), PHYS_THERM sweeps unmeasured and then
    PHYS_SWEEPS measured ones, binned per walker and pooled"""
    import __graft_entry__ as g
    pkg = g.load_package()
    l = pkg.lattices.SquareLattice(PHYS_L)
    slot_class, _, x = pkg.lattices.bond_classes(l, True)
    W = PHYS_REF_W
    wk = qstate_ref.Walkers(l, PHYS_Q, qstate_ref.clock_table(PHYS_Q), [beta] * W, [PHYS_SEED + w for w in range(W)])
    d1, d2 = twist_q30(PHYS_Q, *clock_twist(PHYS_Q))
    bins = [StiffnessBinnerRef(2, PHYS_SWEEPS) for _ in range(W)]
    for s in range(PHYS_THERM + PHYS_SWEEPS):
        wk.sweep()
        if s >= PHYS_THERM:
            I, K = class_sums(wk.c, l.neighs, slot_class, PHYS_Q, d1, d2, x.shape[1])
            for w in range(W):
                T, _, J2 = contract(I[w], K[w], x)
                bins[w].push(elements(T, J2))
    ux, ex = pooled_upsilon(bins, 0, beta, len(l))
    uy, ey = pooled_upsilon(bins, 1, beta, len(l))
    return ux, ex, uy, ey
