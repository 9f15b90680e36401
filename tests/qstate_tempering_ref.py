"""Restatement of the q-state engine's replica exchange (csrc/qstate.hip, qs_exchange_kernel) in numpy, written from the
definition in include/dqmc_hip.h ("Replica exchange", "Order inside a sweep") on top of tests/qstate_ref.py,
tests/qstate_cluster_ref.py and tests/qstate_binner_ref.py and independent of the product:

  ladders     W / R ladders of R consecutive slots; a slot keeps beta, w, key, every cursor, sums, series, binner, counters
  round x     tries the pairs (a, a + 1) with ladder-local i = x mod 2, i + 2, .. while i + 1 < R; x += 1
  decision    d = E_a - E_b (int), db = beta_a - beta_b (fp64): swap if db == 0 or d == 0 or they have the same sign; else
              p = 1.0, p = p * t[j] over the set bits j of |d| ascending, t[j] = exp(-(|db| 2^(j - 30))) (math.exp: the C
              library's, as the product's host code calls it; the scaling by ldexp is exact), j < J, and swap iff
              u1 of P(key_a; 0, low32(x), 7, high32(x)) < p
  J           the smallest integer with 2^J > 2 n_bonds max |e_q30|
  swap        the configurations, E_int, Mx, My and the replica label (at first the slot's ladder-local index)
  counters    prop_exchange[a] += 1 per try, acc_exchange[a] += 1 per swap
  sweep i     colour passes; cluster move iff cluster_rate > 0 and i % cluster_rate == 0; round iff k > 0, R >= 2 and
              i % k == 0; measurement iff i > thermalization and i % measure_rate == 0 (sums, series, then the binner)
  launch cut  a dqmc_qs_sweep call as launches: one ends at every sweep with a round and at the work bound"""
import math

import numpy as np

import qstate_binner_ref as bref
import qstate_cluster_ref as cref
import qstate_ref as ref

DOMAIN_EXCHANGE = 7
_M32 = np.uint64(0xFFFFFFFF)


def exchange_bits(n_bonds, e_q30):
    bound = 2 * int(n_bonds) * max(abs(int(e)) for e in e_q30)
    J = 0
    while 2 ** J <= bound:
        J += 1
    return J


def pair_table(db, J):
    return [math.exp(-math.ldexp(abs(float(db)), j - 30)) for j in range(J)]


def product(t, abs_d):
    p = 1.0
    for j in range(len(t)):
        if (abs_d >> j) & 1:
            p = p * t[j]
    return p


def rule(db, d):
    """'swap' where the rule swaps without a draw, else 'decide'"""
    return "swap" if db == 0.0 or d == 0 or (db > 0.0) == (d > 0) else "decide"


def tried_pairs(x, R, W):
    """the lower slots of the pairs round x tries"""
    return [lad * R + i for lad in range(W // R) for i in range(x % 2, R - 1, 2)] if R >= 2 else []


def measurements_in(first, last, therm, rate):
    return sum(1 for i in range(first, last + 1) if i > therm and i % rate == 0)


def launch_cut(n, first, therm, rate, k, chunk, T0):
    """[(n_sweeps, first, defer_last, T_at_start)]: sweep by sweep, a launch is closed behind a sweep with a round or when
    it holds `chunk` sweeps"""
    out, start, T = [], first, T0
    for i in range(first, first + n):
        rnd = k > 0 and i % k == 0
        if rnd or i - start + 1 == max(chunk, 1) or i == first + n - 1:
            out.append((i - start + 1, start, bool(rnd and i > therm and i % rate == 0), T))
            T += measurements_in(start, i, therm, rate)
            start = i + 1
    return out


class TemperingWalkers(cref.ClusterWalkers):
    """qstate_cluster_ref.ClusterWalkers with ladders, the exchange round and (binner=capacity) the binner"""

    def __init__(self, *args, binner=None, **kwargs):
        self.bin = None
        super().__init__(*args, **kwargs)
        self.J = exchange_bits(len(self.bonds), self.e_q30)
        self.R = self.k = 0
        self.x = 0
        W = self.W
        self.replica = np.zeros(W, dtype=np.int64)
        self.prop_exchange = np.zeros(W, dtype=np.int64)
        self.acc_exchange = np.zeros(W, dtype=np.int64)
        self.decided = {"acc": 0, "rej": 0, "free": 0}  # (for the tests' own use: what the rounds so far decided how)
        if binner is not None:
            self.bin = bref.QsBinnerRef(W, binner)

    def set_exchange(self, R, k):
        assert R < 2 or self.W % R == 0
        self.R, self.k, self.x = (R if R >= 2 else 0), k, 0
        self.replica = np.arange(self.W, dtype=np.int64) % max(self.R, 1) if self.R else np.zeros(self.W, dtype=np.int64)
        self.prop_exchange[:] = 0
        self.acc_exchange[:] = 0

    def set_beta(self, w, beta):
        self.betas[w] = float(beta)
        self.w[w] = ref.weights(self.e_q30, beta).reshape(-1)

    def exchange(self):
        x = self.x
        for a in tried_pairs(x, self.R, self.W):
            b = a + 1
            d = int(self.E[a]) - int(self.E[b])
            db = float(self.betas[a]) - float(self.betas[b])
            self.prop_exchange[a] += 1
            if rule(db, d) == "swap":
                swap = True
                self.decided["free"] += 1
            else:
                assert abs(d) < 2 ** self.J
                p = product(pair_table(db, self.J), abs(d))
                u1, _ = ref.philox_two(self.keys[a], 0, np.uint64(x) & _M32, DOMAIN_EXCHANGE, np.uint64(x) >> np.uint64(32))
                swap = bool(float(u1) < p)
                self.decided["acc" if swap else "rej"] += 1
            if swap:
                self.acc_exchange[a] += 1
                self.c[[a, b]] = self.c[[b, a]]
                for arr in (self.E, self.Mx, self.My, self.replica):
                    arr[a], arr[b] = arr[b], arr[a]
        self.x += 1

    def measure(self):
        super().measure()
        if self.bin is not None:
            self.bin.push_measurement(self.E, self.Mx, self.My)

    def reset_accumulators(self):
        super().reset_accumulators()
        if self.bin is not None:
            self.bin.clear()

    def run(self, first, n, thermalization, measure_rate, cluster_rate=0):
        for i in range(first, first + n):
            self.sweep()
            if cluster_rate > 0 and i % cluster_rate == 0:
                self.cluster_move()
            if self.k > 0 and self.R >= 2 and i % self.k == 0:
                self.exchange()
            if i > thermalization and i % measure_rate == 0:
                self.measure()

    def exchange_stats(self, w):
        return {"prop_exchange": int(self.prop_exchange[w]), "acc_exchange": int(self.acc_exchange[w]),
                "replica": int(self.replica[w]), "rounds": int(self.x)}


def exchange_matrix(E_q30, beta_a, beta_b, J):
    """P[(i, j) -> (j, i)] of one try of a pair whose slots hold the states i (at beta_a) and j (at beta_b), with the
    restated p: [S][S] acceptance probabilities"""
    S = len(E_q30)
    db = float(beta_a) - float(beta_b)
    t = pair_table(db, J)
    A = np.ones((S, S))
    for i in range(S):
        for j in range(S):
            d = int(E_q30[i]) - int(E_q30[j])
            if rule(db, d) == "decide":
                A[i, j] = product(t, abs(d))
    return A


# ---- the physics check: 3 x 3 Potts q = 3, R = 4 betas around beta_c, 64 ladders, a round every second sweep, binner on
PHYS_Q, PHYS_L, PHYS_R, PHYS_LADDERS, PHYS_K = 3, 3, 4, 64, 2
PHYS_BETAS = [0.85, 0.95, 1.05, 1.15]  # beta_c = ln(1 + sqrt 3) = 1.005
PHYS_THERM, PHYS_SWEEPS, PHYS_SEED = 200, 2000, 7100


def exact_energy_per_site(l, q, beta):
    return ref.qstate_exact(l, q, ref.potts_table(q), beta)["E"] / len(l)
