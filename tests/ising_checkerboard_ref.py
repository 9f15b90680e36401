"""Restatement of the Ising flavor's checkerboard sweep (csrc/ising_cb.inl, include/dqmc_hip.h dqmc_mc_set_update) in
numpy, vectorised per colour class, written from the header's definition and independent of the product:

  colouring   greedy_colouring(l): in site order, the smallest colour not used by an already-coloured neighbour j < i
  sweep       colours 0 .. C - 1 in order; within a colour every site from the configuration as it stood when the colour
              began: dE = 2 s_i sum_k s_{neighs[k, i]}, accepted iff dE <= 0 or u_cb(s, i) < thr[dE / 2 - 1]
  u_cb(s, i)  ising_wolff_ref.philox4_uniform(key, i, low32(s), 3, high32(s)), s = the slot's checkerboard sweeps so far

on top of ising_wolff_ref (Philox, the cluster move, the sequential Walker), ising_tempering_ref (Ladders: the exchange
round, the order of a sweep's parts), ising_binner_ref and ising_fss_ref.  Walker and Ladders take `update`, which may
be switched between sweeps as dqmc_mc_set_update allows.  Shared by test_ising_checkerboard.py (CPU) and
test_gpu_ising_checkerboard.py."""
import functools
import math

import numpy as np

import ising_binner_ref as B
import ising_fss_ref as F
import ising_tempering_ref as T
import ising_wolff_ref as R

_M32 = 0xFFFFFFFF


def greedy_colouring(l):
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    N = nb.shape[1]
    colour = [-1] * N
    for i in range(N):
        if i in nb[:, i]:
            raise ValueError("site %d lists itself as a neighbour" % i)
        used = {colour[j] for j in nb[:, i] if j < i}
        colour[i] = min(c for c in range(len(used) + 1) if c not in used)
    return np.array(colour, dtype=np.int64)


def is_valid(l, colour):
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    colour = np.asarray(colour)
    return bool(np.all(colour[nb] != colour[None, :]))


def classes(colour):
    """the sites of every colour, ascending"""
    colour = np.asarray(colour)
    return [np.flatnonzero(colour == c) for c in range(int(colour.max()) + 1)]


def u_cb(key, s, i):
    """the uniform of site(s) i (0-based) in the slot's checkerboard sweep s"""
    return R.philox4_uniform(int(key), np.asarray(i, dtype=np.uint64), s & _M32, 3, s >> 32)


def u_cb_keys(keys, s, i):
    """u_cb with one key and one cursor per element (the same ten rounds, restated for arrays of keys)"""
    keys, s = np.asarray(keys, dtype=np.uint64), np.asarray(s, dtype=np.uint64)
    m32 = np.uint64(_M32)
    c = [np.asarray(i, dtype=np.uint64) & m32, s & m32, np.full(keys.shape, 3, dtype=np.uint64), s >> np.uint64(32)]
    k0, k1 = keys & m32, keys >> np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    bits = ((c[0] >> np.uint64(5)) << np.uint64(26)) | (c[1] >> np.uint64(6))
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)


class Walker(R.Walker):
    """ising_wolff_ref.Walker whose local sweep is the checkerboard sweep while update == "checkerboard"; `s` is the
    checkerboard sweep cursor (sweeps_drawn)"""

    def __init__(self, l, beta, key, conf=None, series_capacity=0, colouring=None, update="checkerboard"):
        super().__init__(l, beta, key, conf=conf, series_capacity=series_capacity)
        self.classes = classes(greedy_colouring(l) if colouring is None else colouring)
        self.update = update
        self.s = 0

    def sweep(self):
        if self.update == "sequential":
            return super().sweep()
        c, thr = self.c, np.array(self.thr)
        for idx in self.classes:
            k = c[idx] * c[self.neighs0[:, idx]].sum(axis=0)  # dE / 2, all from the state before the colour
            accept = k <= 0
            need = np.flatnonzero(k > 0)
            if len(need):
                accept[need] = u_cb(self.key, self.s, idx[need]) < thr[k[need] - 1]
            self.E += int(2 * k[accept].sum())
            c[idx[accept]] = -c[idx[accept]]
            self.st["acc_local"] += int(accept.sum())
        self.st["prop_local"] += self.N
        self.s += 1


class Ladders(T.Ladders):
    """ising_tempering_ref.Ladders (all walkers of a handle, with or without exchange) with the checkerboard sweep,
    vectorised over the walkers; optionally the binner and the FSS sums of every measurement.  The cursor `s` stays with
    the slot under exchange."""

    def __init__(self, l, betas, keys, n_replicas=0, series_capacity=0, colouring=None, update="checkerboard",
                 binning_capacity=None, fss_tables=None):
        super().__init__(l, betas, keys, n_replicas=n_replicas, series_capacity=series_capacity)
        self.classes = classes(greedy_colouring(l) if colouring is None else colouring)
        self.update = update
        self.s = np.zeros(self.W, dtype=np.int64)
        self.binner = B.IsingBinnerRef(binning_capacity, self.W) if binning_capacity else None
        self.fss_tables = fss_tables  # (cos_q30, sin_q30) or None
        if fss_tables is not None:
            n_k = len(fss_tables[0])
            self.fss_n = 0
            self.fss_sums = np.zeros((self.W, 2 + n_k))  # running sums of [M2, M4, S_0 ..]
            self.fss_binners = [F.FssBinnerRef(n_k, binning_capacity) for _ in range(self.W)] if binning_capacity else None

    def sweep(self):
        if self.update == "sequential":
            return super().sweep()
        c, nb = self.c, self.neighs0
        for idx in self.classes:
            k = c[:, idx] * c[:, nb[:, idx]].sum(axis=1)  # [W][class]
            accept = k <= 0
            ww, jj = np.nonzero(k > 0)
            if len(ww):
                u = u_cb_keys(self.keys[ww], self.s[ww], idx[jj])
                accept[ww, jj] = u < self.thr[ww, k[ww, jj] - 1]
            self.E += np.where(accept, 2 * k, 0).sum(axis=1)
            sub = c[:, idx]
            sub[accept] = -sub[accept]
            c[:, idx] = sub
            self.acc_local += accept.sum(axis=1)
        self.prop_local += self.N
        self.s += 1

    def measure(self):
        super().measure()
        if self.binner is not None:
            self.binner.push_EM(self.E, self.c.sum(axis=1))
        if self.fss_tables is not None:
            self.fss_n += 1
            for w in range(self.W):
                v = F.values(self.c[w], *self.fss_tables)
                self.fss_sums[w] = self.fss_sums[w] + v
                if self.fss_binners is not None:
                    self.fss_binners[w].push(v)


# ---- 4x4 against exact enumeration: one run of the restatement, shared by the CPU and the GPU test
ENUM_BETAS = (0.2, 0.44, 0.7)
ENUM_WB, ENUM_THERM, ENUM_SWEEPS, ENUM_SEED = 512, 200, 2000, 1234


def exact_4x4(l, beta):
    """<E>, <E2>, <|M|>, <M2> of the 4x4 periodic Ising model by enumeration of its 2^16 states"""
    bits = (np.arange(1 << 16)[:, None] >> np.arange(16)) & 1
    s = (2 * bits - 1).astype(np.float64)
    b = np.asarray(l.bonds)[:, :2] - 1
    E = -(s[:, b[:, 0]] * s[:, b[:, 1]]).sum(axis=1)
    wgt = np.exp(-beta * (E - E.min()))
    wgt /= wgt.sum()
    M = np.abs(s.sum(axis=1))
    return {"E": float(wgt @ E), "E2": float(wgt @ E ** 2), "M": float(wgt @ M), "M2": float(wgt @ M ** 2)}


@functools.lru_cache(maxsize=1)
def enum_run():
    """the defined chain on SquareLattice(4): 512 walkers at each of ENUM_BETAS, keys ENUM_SEED + w, 200 + 2000 sweeps,
    every sweep past thermalization measured.  Returns (lattice, Ladders)."""
    import __graft_entry__ as g
    l = g.load_package().lattices.SquareLattice(4)
    betas = np.repeat(ENUM_BETAS, ENUM_WB)
    lad = Ladders(l, betas, [ENUM_SEED + w for w in range(len(betas))])
    lad.run(1, ENUM_THERM + ENUM_SWEEPS, ENUM_THERM, 1)
    return l, lad


def check_enum(per_walker_sums, n_meas, l):
    """the rule of test_gpu_ising_wolff.py: per beta, the means of E, E2, |M|, M2 over the walkers lie within 4.5
    cross-walker standard errors of the enumeration.  per_walker_sums: [3 * 512][4]"""
    sums = np.asarray(per_walker_sums, dtype=np.float64)
    for bi, beta in enumerate(ENUM_BETAS):
        ex = exact_4x4(l, beta)
        v = sums[bi * ENUM_WB:(bi + 1) * ENUM_WB] / n_meas
        for q, name in enumerate(("E", "E2", "M", "M2")):
            mean, se = v[:, q].mean(), v[:, q].std(ddof=1) / math.sqrt(ENUM_WB)
            print(beta, name, mean, ex[name], (mean - ex[name]) / se)
            assert abs(mean - ex[name]) <= 4.5 * se, (beta, name, mean, ex[name], se)
