"""Restatement of the Ising flavor's Wolff cluster move (csrc/ising.hip, include/dqmc_hip.h dqmc_mc_global_move) and
of run! with it (MC.jl:230-283), in numpy: Philox4x32-10 with four counter words, the move as the header defines it,
and sweep + move + measurement for one walker.  Shared by test_ising_wolff.py (CPU) and test_gpu_ising_wolff.py."""
import math
from collections import deque

import numpy as np

_M32 = 0xFFFFFFFF


def philox4_uniform(key, c0, c1=0, c2=0, c3=0):
    """Philox4x32-10, key = the 64-bit seed, counter words (c0, c1, c2, c3) (scalars or arrays), made into a uniform in
    [0, 1) from 53 bits of the output as kernels.h philox_uniform does"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(_M32) for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key & _M32), np.uint64((key >> 32) & _M32)
    m32 = np.uint64(_M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    bits = ((c[0] >> np.uint64(5)) << np.uint64(26)) | (c[1] >> np.uint64(6))
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)


def local_uniform(key, index):
    """the walker's local stream (c2 = c3 = 0): draw `index`"""
    index = np.asarray(index, dtype=np.uint64)
    return philox4_uniform(key, index & np.uint64(_M32), index >> np.uint64(32), 0, 0)


def wolff_p(beta):
    """1 - exp(-2 beta) with the host's libm, as dqmc_mc_set_beta computes it"""
    return 1.0 - math.exp(-2.0 * beta)


def wolff_seed(key, m, N):
    u = float(philox4_uniform(key, 0, m & _M32, 1, m >> 32))
    return min(N - 1, int(math.floor(u * N)))


def active_slots(conf, neighs0, key, m, p):
    """[N][z] bool: slot (i, k) is active iff s_i == s_{neighs[k, i]} and u(m, 1 + 8 i + k) < p"""
    z, N = neighs0.shape
    t = 1 + 8 * np.arange(N, dtype=np.uint64)[:, None] + np.arange(z, dtype=np.uint64)[None, :]
    u = philox4_uniform(key, t, m & _M32, 1, m >> 32)
    return (conf[:, None] == conf[neighs0.T]) & (u < p)


def wolff_cluster(conf, neighs0, key, m, p):
    """the move's cluster: the sites reachable from the seed through active slots (sorted 0-based indices)"""
    N = len(conf)
    act = active_slots(conf, neighs0, key, m, p)
    seed = wolff_seed(key, m, N)
    inc = np.zeros(N, dtype=bool)
    inc[seed] = True
    todo = deque([seed])
    while todo:
        i = todo.popleft()
        for k in range(neighs0.shape[0]):
            j = int(neighs0[k, i])
            if act[i, k] and not inc[j]:
                inc[j] = True
                todo.append(j)
    return np.flatnonzero(inc)


def wolff_move(conf, neighs0, key, m, p):
    """global_move on a copy of conf: returns (new conf, cluster size)"""
    c = np.array(conf, dtype=np.int64)
    cl = wolff_cluster(c, neighs0, key, m, p)
    c[cl] = -c[cl]
    return c, len(cl)


def energy(conf, bonds0):
    return -int(np.sum(conf[bonds0[:, 0]] * conf[bonds0[:, 1]]))


class Walker:
    """one walker of MC with cluster_moves: sweep(mc), global_move every `global_rate`-th sweep, run!'s measurement
    (MC.jl:230-283), counters as dqmc_mc_get_stats / dqmc_mc_get_global_stats report them"""

    def __init__(self, l, beta, key, conf=None, series_capacity=0):
        self.N = len(l)
        self.neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
        self.nb = [list(self.neighs0[:, i]) for i in range(self.N)]
        self.bonds0 = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
        self.beta, self.key = beta, key
        self.p = wolff_p(beta)
        self._block = (-1, None)
        self.draw = 0
        if conf is None:
            self.c = np.where(local_uniform(key, np.arange(self.N)) < 0.5, -1, 1).astype(np.int64)
            self.draw = self.N
        else:
            self.c = np.asarray(conf, dtype=np.int64).copy()
        self.E = energy(self.c, self.bonds0)
        self.thr = [math.exp(-beta * 2.0 * k) for k in range(1, 9)]
        self.cap = series_capacity
        self.serE, self.serM = [], []
        self.st = dict(sum_E=0.0, sum_E2=0.0, sum_absM=0.0, sum_M2=0.0, n_meas=0, acc_local=0, prop_local=0)
        self.gs = dict(prop_global=0, acc_global=0, sum_cluster_size=0, moves_drawn=0)

    def _u(self, index):
        b = index >> 12
        if self._block[0] != b:
            self._block = (b, local_uniform(self.key, np.arange(b << 12, (b + 1) << 12)))
        return float(self._block[1][index & 4095])

    def sweep(self):
        c = self.c
        for i in range(self.N):
            k = int(c[i]) * sum(int(c[j]) for j in self.nb[i])  # dE / 2
            self.st["prop_local"] += 1
            accept = k <= 0
            if k > 0:
                accept = self._u(self.draw) < self.thr[k - 1]
                self.draw += 1
            if accept:
                self.E += 2 * k
                c[i] = -c[i]
                self.st["acc_local"] += 1

    def global_move(self):
        m = self.gs["moves_drawn"]
        self.c, size = wolff_move(self.c, self.neighs0, self.key, m, self.p)
        self.E = energy(self.c, self.bonds0)
        self.gs["moves_drawn"] = m + 1
        self.gs["prop_global"] += 1
        self.gs["acc_global"] += int(size > 1)
        self.gs["sum_cluster_size"] += size
        return size

    def measure(self):
        M = abs(int(self.c.sum()))
        self.st["sum_E"] += self.E
        self.st["sum_E2"] += float(self.E) * self.E
        self.st["sum_absM"] += M
        self.st["sum_M2"] += float(M) * M
        self.st["n_meas"] += 1
        if len(self.serE) < self.cap:
            self.serE.append(self.E)
            self.serM.append(M)

    def run(self, first, last, therm, measure_rate, global_rate):
        """sweeps first..last (1-based global indices) as run! takes them"""
        for i in range(first, last + 1):
            self.sweep()
            if global_rate and i % global_rate == 0:
                self.global_move()
            if i > therm and i % measure_rate == 0:
                self.measure()

    def stats(self):
        r = dict(self.st)
        r.update(uniforms_used=self.draw, energy=self.E, magnetization=int(self.c.sum()))
        return r
