"""Restatement of the Ising flavor's replica exchange (csrc/ising.hip, include/dqmc_hip.h dqmc_mc_set_exchange) and of
run! with it, in numpy on top of ising_wolff_ref.py (its Philox, its cluster move, and its Walker as the yardstick of the
local sweep), vectorised over the walkers of a handle: pair selection by the round's parity, the acceptance
probability by the product rule over the host's exp table, the swap of configuration, E, M and label, and the order
local sweep, cluster move, exchange round, measurement.  Shared by test_ising_tempering.py (CPU) and
test_gpu_ising_tempering.py."""
import math

import numpy as np

import ising_wolff_ref as R

_M32 = 0xFFFFFFFF


def pair_table(beta_a, beta_b, n_bonds):
    """(sign of beta_a - beta_b, [q[j] = exp(-2 |beta_a - beta_b| 2^j), j < J]) with 2^J > n_bonds, from the host's libm"""
    db = float(beta_a) - float(beta_b)
    J = 0
    while (1 << J) <= n_bonds:
        J += 1
    return (db > 0) - (db < 0), [math.exp(-2.0 * abs(db) * float(1 << j)) for j in range(J)]


def product_rule(q, d):
    """p = 1.0, then p = p * q[j] for every set bit j of |d|, ascending"""
    p, ad = 1.0, abs(int(d))
    assert ad < (1 << len(q))
    for j in range(len(q)):
        if (ad >> j) & 1:
            p = p * q[j]
    return p


def exchange_uniform(key, x):
    """the round's uniform of a pair: the key of its lower slot, counter words (low32(x), high32(x), 2, 0)"""
    return float(R.philox4_uniform(int(key), x & _M32, x >> 32, 2, 0))


def philox_keys(keys, index):
    """Philox4x32-10 as R.philox4_uniform, with one key per element (c2 = c3 = 0)"""
    keys = np.asarray(keys, dtype=np.uint64)
    index = np.asarray(index, dtype=np.uint64)
    m32 = np.uint64(_M32)
    c = [index & m32, index >> np.uint64(32), np.zeros_like(index), np.zeros_like(index)]
    k0, k1 = keys & m32, keys >> np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    bits = ((c[0] >> np.uint64(5)) << np.uint64(26)) | (c[1] >> np.uint64(6))
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)


class Ladders:
    """all walkers of one MC handle: slot w keeps beta, key, cursors, sums, series and counters; configurations, E, M and
    the replica label move.  n_replicas < 2: no exchange."""

    def __init__(self, l, betas, keys, n_replicas=0, series_capacity=0):
        self.N = len(l)
        self.neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
        self.bonds0 = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
        self.W = W = len(betas)
        self.R = int(n_replicas) if n_replicas >= 2 else 0
        assert self.R == 0 or W % self.R == 0
        self.keys = np.array([int(k) for k in keys], dtype=np.uint64)
        idx = np.arange(self.N, dtype=np.uint64)
        self.c = np.stack([np.where(R.local_uniform(int(k), idx) < 0.5, -1, 1) for k in keys]).astype(np.int64)
        self.draw = np.full(W, self.N, dtype=np.uint64)
        self.E = np.array([R.energy(c, self.bonds0) for c in self.c], dtype=np.int64)
        self.betas = np.zeros(W)
        self.thr = np.zeros((W, 8))
        self.pairs = [None] * W
        for w, b in enumerate(betas):
            self.betas[w] = float(b)
        for w in range(W):
            self.set_beta(w, betas[w])
        self.cap = series_capacity
        self.serE, self.serM = [[] for _ in range(W)], [[] for _ in range(W)]
        self.sums = np.zeros((W, 4))  # sum_E, sum_E2, sum_absM, sum_M2
        self.n_meas = 0
        self.acc_local = np.zeros(W, dtype=np.int64)
        self.prop_local = 0
        self.gs = [dict(prop_global=0, acc_global=0, sum_cluster_size=0, moves_drawn=0) for _ in range(W)]
        self.replica = np.arange(W) % self.R if self.R else np.zeros(W, dtype=np.int64)
        self.prop_x = np.zeros(W, dtype=np.int64)
        self.acc_x = np.zeros(W, dtype=np.int64)
        self.rounds = 0
        # draw-decided exchanges by parity of the round: [parity] -> [refused, accepted]
        self.drawn = [[0, 0], [0, 0]]

    def set_beta(self, w, beta):
        self.betas[w] = float(beta)
        self.thr[w] = [math.exp(-float(beta) * 2.0 * k) for k in range(1, 9)]
        for a in (w - 1, w):
            if self.R and a >= 0 and a % self.R + 1 < self.R:
                self.pairs[a] = pair_table(self.betas[a], self.betas[a + 1], len(self.bonds0))

    # ---- the moves
    def sweep(self):
        c, nb = self.c, self.neighs0
        for i in range(self.N):
            k = c[:, i] * c[:, nb[:, i]].sum(axis=1)  # dE / 2
            accept = k <= 0
            idx = np.flatnonzero(k > 0)
            if len(idx):
                u = philox_keys(self.keys[idx], self.draw[idx])
                accept[idx] = u < self.thr[idx, k[idx] - 1]
                self.draw[idx] += np.uint64(1)
            self.E += np.where(accept, 2 * k, 0)
            c[accept, i] = -c[accept, i]
            self.acc_local += accept
        self.prop_local += self.N

    def global_move(self):
        for w in range(self.W):
            g = self.gs[w]
            self.c[w], size = R.wolff_move(self.c[w], self.neighs0, int(self.keys[w]), g["moves_drawn"],
                                           R.wolff_p(self.betas[w]))
            self.E[w] = R.energy(self.c[w], self.bonds0)
            g["moves_drawn"] += 1
            g["prop_global"] += 1
            g["acc_global"] += int(size > 1)
            g["sum_cluster_size"] += size

    def exchange_round(self):
        x = self.rounds
        for a in range(self.W):
            i = a % self.R
            if i % 2 != x % 2 or i + 1 >= self.R:
                continue
            b = a + 1
            sgn, q = self.pairs[a]
            assert (self.E[a] - self.E[b]) % 2 == 0
            d = int(self.E[a] - self.E[b]) // 2
            if sgn == 0 or d == 0 or (d > 0) == (sgn > 0):
                swap = True
            else:
                swap = exchange_uniform(self.keys[a], x) < product_rule(q, d)
                self.drawn[x % 2][int(swap)] += 1
            self.prop_x[a] += 1
            if swap:
                self.acc_x[a] += 1
                self.c[[a, b]] = self.c[[b, a]]
                self.E[[a, b]] = self.E[[b, a]]
                self.replica[[a, b]] = self.replica[[b, a]]
        self.rounds = x + 1

    def measure(self):
        E = self.E.astype(np.float64)
        M = np.abs(self.c.sum(axis=1)).astype(np.float64)
        self.sums += np.stack([E, E * E, M, M * M], axis=1)
        self.n_meas += 1
        for w in range(self.W):
            if len(self.serE[w]) < self.cap:
                self.serE[w].append(int(self.E[w]))
                self.serM[w].append(int(M[w]))

    def run(self, first, last, therm, measure_rate, global_rate=0, exchange_rate=0):
        """sweeps first..last (1-based global indices): local sweep, cluster move, exchange round, measurement"""
        for g in range(first, last + 1):
            self.sweep()
            if global_rate and g % global_rate == 0:
                self.global_move()
            if self.R and exchange_rate and g % exchange_rate == 0:
                self.exchange_round()
            if g > therm and g % measure_rate == 0:
                self.measure()

    # ---- what the device reports
    def stats(self, w):
        s = self.sums[w]
        return dict(sum_E=s[0], sum_E2=s[1], sum_absM=s[2], sum_M2=s[3], n_meas=self.n_meas,
                    acc_local=int(self.acc_local[w]), prop_local=self.prop_local, uniforms_used=int(self.draw[w]),
                    energy=int(self.E[w]), magnetization=int(self.c[w].sum()))

    def exchange_stats(self, w):
        return dict(prop_exchange=int(self.prop_x[w]), acc_exchange=int(self.acc_x[w]), replica=int(self.replica[w]),
                    rounds=self.rounds)
