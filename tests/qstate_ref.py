"""Restatement of the q-state (Potts, clock) engine (csrc/qstate.hip) in numpy, written from the definition in
include/dqmc_hip.h ("the classical MC flavor with q-state models") and independent of the product:

  tables      e_q30[d] = llround(J e[d] 2^30) for d <= q / 2, mirrored; c_q30 / s_q30 = llround(cos / sin(2 pi s / q) 2^30)
  uniforms    P(key; c0, c1, c2, c3) = Philox4x32-10 -> (u1, u2) from the output words (o0, o1) and (o2, o3)
  domains     c2 = 4: the sweep, counter (site, low32(s), 4, high32(s)); c2 = 5: the initial configuration, counter
              (site, low32(r), 5, high32(r)), state = min(q - 1, (int)(u1 q))
  sweep       colours in order, every site of a colour from the configuration as it stood when the colour began:
              t = (s + 1 + min(q - 2, (int)(u1 (q - 1)))) mod q, dE_int = sum_k (e_q30[a_k] - e_q30[b_k]),
              p = 1.0 then p = p * w[a_k][b_k] for k = 0 .. z - 1, accept iff dE_int <= 0 or u2 < p
  w           w[a][b] = exp(-beta ((e_q30[a] - e_q30[b]) 2^-30)) by the host's libm (math.exp: the C library's exp, as
              the product's host code calls it; numpy's own exp may differ in the last bit)
  domain      beta is accepted iff beta z range <= 700, range = (max e_q30 - min e_q30) 2^-30: every partial p is finite
  measure     e = E_int 2^-30, x = Mx 2^-30, y = My 2^-30, m2 = x x + y y; sum_E += e, sum_E2 += e e, sum_M2 += m2,
              sum_M4 += m2 m2, sum_absM += sqrt(m2), one rounding each, in the order of the measurements

`Walkers` is every walker of a handle, vectorised over walkers and over the sites of a colour.  qstate_exact enumerates a
tiny lattice.  Shared by test_qstate_host.py (CPU) and test_gpu_qstate.py."""
import functools
import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
Q30 = 2.0 ** 30
DOMAIN_SWEEP, DOMAIN_CONF = 4, 5


def llround(x):
    """half away from zero, as C's llround"""
    x = np.asarray(x, dtype=np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def potts_table(q):
    e = np.zeros(q)
    e[0] = 1.0
    return e


def clock_table(q):
    e = np.zeros(q)
    for d in range(q // 2 + 1):
        e[d] = e[(q - d) % q] = math.cos(2.0 * math.pi * d / q)
    return e


def tables(q, e, J=1.0):
    e = np.asarray(e, dtype=np.float64)
    e_q30 = np.zeros(q, dtype=np.int64)
    for d in range(q // 2 + 1):
        e_q30[d] = e_q30[(q - d) % q] = llround(J * e[d] * Q30)
    ang = 2.0 * np.pi * np.arange(q) / q
    return e_q30, llround(np.cos(ang) * Q30), llround(np.sin(ang) * Q30)


def weights(e_q30, beta):
    """w[a][b] of one walker, [q][q] fp64"""
    q = len(e_q30)
    w = np.zeros((q, q))
    for a in range(q):
        for b in range(q):
            w[a, b] = math.exp(-float(beta) * (float(int(e_q30[a]) - int(e_q30[b])) / Q30))
    return w


BETA_DOMAIN = 700.0


def beta_in_domain(beta, z, e_q30):
    """the header's domain of the acceptance product: fl(fl(beta z) range) <= 700 with the exact
    range = (max e_q30 - min e_q30) 2^-30.  Inside it every partial product of z table entries is finite and non-zero."""
    rng = float(int(max(e_q30)) - int(min(e_q30))) / Q30
    return float(beta) * float(z) * rng <= BETA_DOMAIN


def domain_edge(z, e_q30):
    """(the largest beta inside the domain, the smallest outside)"""
    rng = float(int(max(e_q30)) - int(min(e_q30))) / Q30
    b = BETA_DOMAIN / (float(z) * rng)
    while beta_in_domain(b, z, e_q30):
        b = math.nextafter(b, math.inf)
    while not beta_in_domain(b, z, e_q30):
        b = math.nextafter(b, 0.0)
    return b, math.nextafter(b, math.inf)


def philox_two(keys, c0, c1, c2, c3):
    """(u1, u2) of Philox4x32-10, one key per element (arrays broadcast against the counter words)"""
    keys = np.asarray(keys, dtype=np.uint64)
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)]
    keys, *c = np.broadcast_arrays(keys, *c)
    k0, k1 = keys & _M32, keys >> np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    scale = 1.0 / 9007199254740992.0
    u1 = (((c[0] >> np.uint64(5)) << np.uint64(26)) | (c[1] >> np.uint64(6))).astype(np.float64) * scale
    u2 = (((c[2] >> np.uint64(5)) << np.uint64(26)) | (c[3] >> np.uint64(6))).astype(np.float64) * scale
    return u1, u2


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
    colour = np.asarray(colour)
    return [np.flatnonzero(colour == c) for c in range(int(colour.max()) + 1)]


def local_rule(s, t, sj, e_q30, w):
    """(dE_int, p) of the proposal s -> t of one site with neighbour states sj[z] (repeated neighbours repeated) under
    the table w[q][q]: the header's rule for one site, in scalar form"""
    q = len(e_q30)
    dE, p = 0, 1.0
    for x in sj:
        a, b = (int(s) - int(x)) % q, (int(t) - int(x)) % q
        dE += int(e_q30[a]) - int(e_q30[b])
        p = p * float(w[a, b])
    return dE, p


class Walkers:
    """all walkers of one handle: states c[W][N], E, Mx, My as exact integers, the fp64 sums, the series, the counters
    and the two cursors s (sweeps) and r (initial configurations) per walker"""

    def __init__(self, l, q, e, betas, keys, J=1.0, colouring=None, series_capacity=0, rand=True):
        self.N, self.q = len(l), int(q)
        self.e_q30, self.c_q30, self.s_q30 = tables(q, e, J)
        self.nb = np.asarray(l.neighs, dtype=np.int64) - 1  # [z][N]
        self.bonds = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
        self.z = self.nb.shape[0]
        self.betas = np.atleast_1d(np.asarray(betas, dtype=np.float64))
        self.W = len(self.betas)
        self.keys = np.array([int(k) for k in keys], dtype=np.uint64)
        assert len(self.keys) == self.W
        self.w = np.stack([weights(self.e_q30, b) for b in self.betas]).reshape(self.W, q * q)
        self.set_colouring(greedy_colouring(l) if colouring is None else colouring, l)
        self.cap = series_capacity
        self.c = np.zeros((self.W, self.N), dtype=np.int64)
        self.s = np.zeros(self.W, dtype=np.uint64)
        self.r = np.zeros(self.W, dtype=np.uint64)
        self.prop_local = np.zeros(self.W, dtype=np.int64)
        self.acc_local = np.zeros(self.W, dtype=np.int64)
        self.max_acc_dE = np.zeros(self.W, dtype=np.int64)  # (no counter of the engine: the largest accepted |dE_int|)
        self.reset_accumulators()
        if rand:
            self.rand_conf()
        else:
            self.observables()

    def set_colouring(self, colour, l=None):
        colour = np.asarray(colour, dtype=np.int64)
        assert np.all(colour[self.nb] != colour[None, :]), "invalid colouring"
        self.classes = classes(colour)

    def reset_accumulators(self):
        W = self.W
        self.sum_E, self.sum_E2, self.sum_absM = np.zeros(W), np.zeros(W), np.zeros(W)
        self.sum_M2, self.sum_M4 = np.zeros(W), np.zeros(W)
        self.n_meas = 0
        self.ser = [[] for _ in range(W)]

    def observables(self, w=None):
        """E_int, Mx, My from scratch, of every walker or of walker w"""
        b, q = self.bonds, self.q
        E = -self.e_q30[(self.c[:, b[:, 0]] - self.c[:, b[:, 1]]) % q].sum(axis=1)
        Mx, My = self.c_q30[self.c].sum(axis=1), self.s_q30[self.c].sum(axis=1)
        if w is None:
            self.E, self.Mx, self.My = E, Mx, My
        else:
            self.E[w], self.Mx[w], self.My[w] = E[w], Mx[w], My[w]

    def rand_conf(self):
        i = np.arange(self.N, dtype=np.uint64)[None, :]
        r = self.r[:, None]
        u1, _ = philox_two(self.keys[:, None], i, r & _M32, DOMAIN_CONF, r >> np.uint64(32))
        self.c = np.minimum(self.q - 1, (u1 * float(self.q)).astype(np.int64))
        self.r = self.r + np.uint64(1)
        self.observables()

    def set_conf(self, w, conf):
        self.c[w] = np.asarray(conf, dtype=np.int64).reshape(-1)
        self.observables(w)

    def sweep(self):
        c, q = self.c, self.q
        rows = np.arange(self.W)[:, None]
        s = self.s[:, None]
        for idx in self.classes:
            so = c[:, idx]                                            # [W][n]
            u1, u2 = philox_two(self.keys[:, None], idx[None, :].astype(np.uint64), s & _M32, DOMAIN_SWEEP,
                                s >> np.uint64(32))
            t = (so + 1 + np.minimum(q - 2, (u1 * float(q - 1)).astype(np.int64))) % q
            dE = np.zeros(so.shape, dtype=np.int64)
            p = np.ones(so.shape)
            for k in range(self.z):
                sj = c[:, self.nb[k, idx]]
                a, b = (so - sj) % q, (t - sj) % q
                dE += self.e_q30[a] - self.e_q30[b]
                p = p * self.w[rows, a * q + b]
            accept = (dE <= 0) | (u2 < p)
            self.E += np.where(accept, dE, 0).sum(axis=1)
            self.Mx += np.where(accept, self.c_q30[t] - self.c_q30[so], 0).sum(axis=1)
            self.My += np.where(accept, self.s_q30[t] - self.s_q30[so], 0).sum(axis=1)
            c[:, idx] = np.where(accept, t, so)
            self.acc_local += accept.sum(axis=1)
            self.max_acc_dE = np.maximum(self.max_acc_dE, np.where(accept, np.abs(dE), 0).max(axis=1))
        self.prop_local += self.N
        self.s = self.s + np.uint64(1)

    def measure(self):
        e = self.E.astype(np.float64) / Q30
        x, y = self.Mx.astype(np.float64) / Q30, self.My.astype(np.float64) / Q30
        m2 = x * x + y * y
        self.sum_E = self.sum_E + e
        self.sum_E2 = self.sum_E2 + e * e
        self.sum_M2 = self.sum_M2 + m2
        self.sum_M4 = self.sum_M4 + m2 * m2
        self.sum_absM = self.sum_absM + np.sqrt(m2)
        self.n_meas += 1
        for w in range(self.W):
            if len(self.ser[w]) < self.cap:
                self.ser[w].append((int(self.E[w]), int(self.Mx[w]), int(self.My[w])))

    def run(self, first, n, thermalization, measure_rate):
        """n sweeps with global indices first, first + 1, ..: measure iff i > thermalization and i % measure_rate == 0"""
        for i in range(first, first + n):
            self.sweep()
            if i > thermalization and i % measure_rate == 0:
                self.measure()

    def stats(self, w):
        """the fields of dqmc_qs_stats that compare with ==, and sum_absM apart (1e-13 relative)"""
        return {"energy_q30": int(self.E[w]), "mx_q30": int(self.Mx[w]), "my_q30": int(self.My[w]),
                "sum_E": float(self.sum_E[w]), "sum_E2": float(self.sum_E2[w]), "sum_M2": float(self.sum_M2[w]),
                "sum_M4": float(self.sum_M4[w]), "n_meas": self.n_meas, "prop_local": int(self.prop_local[w]),
                "acc_local": int(self.acc_local[w]), "sweeps_drawn": int(self.s[w]), "confs_drawn": int(self.r[w]),
                "n_series": len(self.ser[w])}, float(self.sum_absM[w])


def all_states(N, q):
    """[q^N][N]: every configuration, site 0 the fastest digit"""
    idx = np.arange(q ** N)
    return np.stack([(idx // q ** i) % q for i in range(N)], axis=1)


def state_energies_q30(l, q, e_q30, states):
    b = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
    return -np.asarray(e_q30)[(states[:, b[:, 0]] - states[:, b[:, 1]]) % q].sum(axis=1)


def qstate_exact(lattice, q, e, beta, J=1.0):
    """exact <E>, <E2>, <M2> of a tiny lattice by enumeration of its q^N states, under the Boltzmann weight of
    E_int 2^-30 and with M2 = (Mx^2 + My^2) 2^-60: the quantities the engine measures"""
    e_q30, c_q30, s_q30 = tables(q, e, J)
    st = all_states(len(lattice), q)
    E = state_energies_q30(lattice, q, e_q30, st).astype(np.float64) / Q30
    x, y = c_q30[st].sum(axis=1) / Q30, s_q30[st].sum(axis=1) / Q30
    wgt = np.exp(-beta * (E - E.min()))
    wgt /= wgt.sum()
    return {"E": float(wgt @ E), "E2": float(wgt @ (E * E)), "M2": float(wgt @ (x * x + y * y))}


def sweep_matrix(l, q, e_q30, beta, colouring=None):
    """the exact transition matrix [q^N][q^N] of one sweep of the defined chain: per colour the product of its
    single-site kernels; a site proposes each other state with probability 1 / (q - 1) and accepts with 1 where
    dE_int <= 0, else with min(1, p), p the product of table entries the device forms"""
    N = len(l)
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    w = weights(e_q30, beta)
    st = all_states(N, q)
    S = len(st)
    P = np.eye(S)
    for idx in classes(greedy_colouring(l) if colouring is None else colouring):
        for i in idx:
            K = np.zeros((S, S))
            for a in range(S):
                s = st[a, i]
                stay = 1.0
                for t in range(q):
                    if t == s:
                        continue
                    dE, p = local_rule(s, t, st[a, nb[:, i]], e_q30, w)
                    acc = 1.0 if dE <= 0 else min(1.0, p)
                    K[a, a + (t - s) * q ** i] += acc / (q - 1)
                    stay -= acc / (q - 1)
                K[a, a] += stay
            P = P @ K
    return P, st


# ---- the statistical check: 3 x 3 three-state Potts near its critical coupling, one run shared by both test files
STAT_Q, STAT_L, STAT_BETA = 3, 3, math.log(1.0 + math.sqrt(3.0))
STAT_W, STAT_THERM, STAT_SWEEPS, STAT_SEED = 64, 200, 3000, 4242


@functools.lru_cache(maxsize=1)
def stat_run():
    """the defined chain on SquareLattice(3), Potts q = 3: 64 walkers, keys STAT_SEED + w, 200 + 3000 sweeps, every sweep
    past thermalization measured.  Returns (lattice, Walkers)."""
    import __graft_entry__ as g
    l = g.load_package().lattices.SquareLattice(STAT_L)
    wk = Walkers(l, STAT_Q, potts_table(STAT_Q), [STAT_BETA] * STAT_W, [STAT_SEED + w for w in range(STAT_W)])
    wk.run(1, STAT_THERM + STAT_SWEEPS, STAT_THERM, 1)
    return l, wk


def stat_zscores(sum_E, sum_M2, n_meas, l):
    """z-scores of the cross-walker means of <E> and <M2> against the enumeration"""
    ex = qstate_exact(l, STAT_Q, potts_table(STAT_Q), STAT_BETA)
    out = {}
    for name, sums in (("E", sum_E), ("M2", sum_M2)):
        v = np.asarray(sums, dtype=np.float64) / n_meas
        out[name] = float((v.mean() - ex[name]) / (v.std(ddof=1) / math.sqrt(len(v))))
    return out
