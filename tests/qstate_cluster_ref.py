"""Restatement of the q-state engine's reflection cluster move (csrc/qstate.hip) in numpy, written from the definition in
include/dqmc_hip.h ("Cluster move") on top of tests/qstate_ref.py and independent of the product:

  stream      domain word c2 = 6, P(key; t, low32(m), 6, high32(m)), m = the walker's cluster moves since the seed
  seed        t = 0: i0 = min(N - 1, (int)(u1 N)); r = (2 s_i0 + 1 + min(q - 2, (int)(u2 (q - 1)))) mod q
  slot (i,k)  t = 1 + 8 i + k, u1 only; j = neighs[k, i], a = (s_i - s_j) mod q, b = (r - s_i - s_j) mod q with the states
              before the move; active iff e_q30[a] > e_q30[b] and u1 < 1.0 - w[a][b]
  cluster     the sites reachable from i0 through active slots; s_i <- (r - s_i) mod q on it
  dE_int      sum over i in C, k with neighs[k, i] outside C of e_q30[a] - e_q30[b]; dMx, dMy from the (cos, sin) tables
  counters    prop_global += 1, acc_global += (|C| > 1), sum_cluster_size += |C|, the cursor m += 1
  run         sweep i, then its move iff cluster_rate > 0 and i % cluster_rate == 0, then its measurement

The slot stream is addressed by (m, i, k), so the restatement decides all N z slots of a move at once and then follows the
active ones from the seed: whether a slot is looked at or not does not change any other.  `ClusterWalkers` is `qstate_ref.Walkers` with the move;
`cluster_matrix` is the exact transition matrix of one move on a tiny lattice.  Shared by test_qstate_cluster_host.py (CPU)
and test_gpu_qstate_cluster.py."""
import itertools

import numpy as np

import qstate_ref as ref

DOMAIN_CLUSTER = 6
_M32 = np.uint64(0xFFFFFFFF)


class ClusterWalkers(ref.Walkers):
    """qstate_ref.Walkers with the move cursor m, the global counters and the cluster move"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        W = self.W
        self.m = np.zeros(W, dtype=np.uint64)
        self.prop_global = np.zeros(W, dtype=np.int64)
        self.acc_global = np.zeros(W, dtype=np.int64)
        self.sum_cluster_size = np.zeros(W, dtype=np.int64)
        self.max_cluster_size = np.zeros(W, dtype=np.int64)  # (not a counter of the engine: for the tests' own use)
        self.n_partial = np.zeros(W, dtype=np.int64)  # (likewise: the moves with 1 < |C| < N)
        self.last_dE = np.zeros(W, dtype=np.int64)  # dE_int of every walker's last move
        self.last = None                            # the last call's walkers, cluster masks, reflections and states before

    def seed(self, w, key):
        self.keys[w] = np.uint64(key)
        self.s[w] = self.r[w] = self.m[w] = np.uint64(0)

    def cluster_move(self, w=None):
        """one move of walker w, or of every walker (None or negative).  Every slot's activity is a function of (m, i, k)
        and of the states before the move alone, so all N z slots are decided first; the cluster is then what the active
        slots connect to the seed, grown level by level for all walkers at once."""
        ws = np.arange(self.W) if w is None or w < 0 else np.array([w])
        n, q, N, z = len(ws), self.q, self.N, self.z
        s = self.c[ws]                                                   # [n][N], before the move
        keys, m = self.keys[ws], self.m[ws]
        m_lo, m_hi = m & _M32, m >> np.uint64(32)
        u1, u2 = ref.philox_two(keys, 0, m_lo, DOMAIN_CLUSTER, m_hi)
        i0 = np.minimum(N - 1, (u1 * float(N)).astype(np.int64))
        rows = np.arange(n)
        r = (2 * s[rows, i0] + 1 + np.minimum(q - 2, (u2 * float(q - 1)).astype(np.int64))) % q
        si, sj = s[:, None, :], s[:, self.nb]                           # [n][1][N], [n][z][N]
        a, b = (si - sj) % q, (r[:, None, None] - si - sj) % q
        t = (1 + 8 * np.arange(N)[None, :] + np.arange(z)[:, None]).astype(np.uint64)   # [z][N]
        u1, _ = ref.philox_two(keys[:, None, None], t[None], m_lo[:, None, None], DOMAIN_CLUSTER, m_hi[:, None, None])
        cost = self.e_q30[a] - self.e_q30[b]                             # [n][z][N]
        active = (cost > 0) & (u1 < 1.0 - self.w[ws][rows[:, None, None], a * q + b])
        target = (rows[:, None, None] * N + self.nb[None]).ravel()       # flat index of j for every slot
        inC = np.zeros((n, N), dtype=bool)
        inC[rows, i0] = True
        frontier = inC.copy()
        while frontier.any():
            hit = np.bincount(target[(active & frontier[:, None, :]).ravel()], minlength=n * N).reshape(n, N) > 0
            frontier = hit & ~inC
            inC |= frontier
        boundary = inC[:, None, :] & ~inC[:, self.nb]                    # slots of cluster sites that lead outside
        dE = np.where(boundary, cost, 0).sum(axis=(1, 2))
        new = (r[:, None] - s) % q
        self.last_dE[ws] = dE
        self.last = {"walkers": ws, "in_cluster": inC, "r": r, "before": s}
        self.E[ws] += dE
        self.Mx[ws] += np.where(inC, self.c_q30[new] - self.c_q30[s], 0).sum(axis=1)
        self.My[ws] += np.where(inC, self.s_q30[new] - self.s_q30[s], 0).sum(axis=1)
        self.c[ws] = np.where(inC, new, s)
        size = inC.sum(axis=1)
        self.prop_global[ws] += 1
        self.acc_global[ws] += size > 1
        self.sum_cluster_size[ws] += size
        self.max_cluster_size[ws] = np.maximum(self.max_cluster_size[ws], size)
        self.n_partial[ws] += (size > 1) & (size < N)
        self.m[ws] = m + np.uint64(1)

    def run(self, first, n, thermalization, measure_rate, cluster_rate=0):
        for i in range(first, first + n):
            self.sweep()
            if cluster_rate > 0 and i % cluster_rate == 0:
                self.cluster_move()
            if i > thermalization and i % measure_rate == 0:
                self.measure()

    def cluster_stats(self, w):
        return {"prop_global": int(self.prop_global[w]), "acc_global": int(self.acc_global[w]),
                "sum_cluster_size": int(self.sum_cluster_size[w]), "moves_drawn": int(self.m[w])}


def cluster_matrix(l, q, e_q30, beta):
    """(P, states): the exact transition matrix [q^N][q^N] of one cluster move on a tiny lattice.  A state's row sums over
    the seed (1 / N each), the q - 1 reflections that move the seed's state (1 / (q - 1) each) and every subset of the
    directed slots with non-zero probability p = 1.0 - w[a][b] (weights() as the device uses it): the subset's probability
    is the product of p over its slots and of 1 - p over the others, and the cluster is what the subset connects to the
    seed."""
    N = len(l)
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    z = nb.shape[0]
    w = ref.weights(e_q30, beta)
    st = ref.all_states(N, q)
    S = len(st)
    P = np.zeros((S, S))
    pw = q ** np.arange(N)
    for x in range(S):
        s = st[x]
        for i0 in range(N):
            for t in range(q - 1):
                r = (2 * int(s[i0]) + 1 + t) % q
                slots = []  # (i, j, p) with p > 0
                for i in range(N):
                    for k in range(z):
                        j = int(nb[k, i])
                        a, b = int(s[i] - s[j]) % q, int(r - s[i] - s[j]) % q
                        if e_q30[a] > e_q30[b]:
                            p = 1.0 - float(w[a, b])
                            if p > 0.0:
                                slots.append((i, j, p))
                for on in itertools.product((False, True), repeat=len(slots)):
                    prob = 1.0 / (N * (q - 1))
                    for (i, j, p), o in zip(slots, on):
                        prob *= p if o else 1.0 - p
                    C = {i0}
                    grew = True
                    while grew:
                        grew = False
                        for (i, j, p), o in zip(slots, on):
                            if o and i in C and j not in C:
                                C.add(j)
                                grew = True
                    y = s.copy()
                    for i in C:
                        y[i] = (r - s[i]) % q
                    P[x, int((y * pw).sum())] += prob
    return P, st
