"""Restatement of the SAC flavor (csrc/sac.hip) in numpy, from the definition in include/dqmc_hip.h ("the SAC flavor"):
the lane sum, the move, refresh, exchange round and measurement of one problem's ladder, and SAC.run's loop with its
window rule.  numpy's float64 arithmetic rounds every operation once and fuses nothing, which is what the header asks
for.  Shared by test_sac_reference.py (CPU) and test_gpu_sac.py."""
import math

import numpy as np

from ising_wolff_ref import philox4_uniform

_M32 = 0xFFFFFFFF


def lane_sum(t):
    """L(t) of the header: 64 lanes, lane l adds t[l], t[l + 64], .. in order, then the xor butterfly (halving)"""
    n = len(t)
    rows = np.zeros(((n + 63) // 64) * 64)
    rows[:n] = t
    rows = rows.reshape(-1, 64)
    p = rows[0].copy()
    for k in range(1, len(rows)):
        p = p + rows[k]
    while len(p) > 1:
        h = len(p) // 2
        p = p[:h] + p[h:]
    return float(p[0])


def move_uniforms(key, m, n):
    """u(m + j, 0) and u(m + j, 1) for j < n: counter words (low32(m), high32(m), t, 0)"""
    mm = np.arange(n, dtype=np.uint64) + np.uint64(m)
    lo, hi = mm & np.uint64(_M32), mm >> np.uint64(32)
    return philox4_uniform(key, lo, hi, 0, 0), philox4_uniform(key, lo, hi, 1, 0)


def exchange_uniform(key, X):
    """counter words (low32(X), high32(X), 0, 1)"""
    return float(philox4_uniform(key, X & _M32, X >> 32, 0, 1))


class Ladder:
    """the R chains of one problem: g, w [Nt], Kt [Nw][Nt], norm; thetas, seeds, windows [R]; x [R][Nd]"""

    def __init__(self, g, w, Kt, norm, thetas, seeds, x, windows):
        self.g, self.w = np.array(g, dtype=np.float64), np.array(w, dtype=np.float64)
        self.Kt = np.array(Kt, dtype=np.float64)
        self.Nw, self.Nt = self.Kt.shape
        self.theta = [float(t) for t in thetas]
        self.R = len(self.theta)
        self.key = [int(s) for s in seeds]
        self.win = [int(v) for v in np.broadcast_to(windows, (self.R,))]
        self.x = [np.array(x[r], dtype=np.int64) for r in range(self.R)]
        self.Nd = len(self.x[0])
        self.a = float(norm) / self.Nd
        self.m = [0] * self.R
        self.label = list(range(self.R))
        self.res, self.chi2 = [None] * self.R, [0.0] * self.R
        for r in range(self.R):
            self.res[r], self.chi2[r] = self.rebuild(self.x[r])
        self.rate, self.X = 0, 0
        self.prop, self.acc, self.xprop, self.xacc = ([0] * self.R for _ in range(4))
        self.drift = [0.0] * self.R
        self.reset_accumulators()

    def reset_accumulators(self):
        self.hist = [np.zeros(self.Nw, dtype=np.uint64) for _ in range(self.R)]
        self.sum, self.sum2, self.n_meas = [0.0] * self.R, [0.0] * self.R, [0] * self.R
        self.min = [math.inf] * self.R

    def rebuild(self, x):
        S = np.zeros(self.Nt)
        for d in range(len(x)):
            S = S + self.Kt[x[d]]
        res = self.a * S - self.g
        return res, lane_sum((self.w * res) * res)

    def set_exchange(self, rate):
        self.rate, self.X = rate, 0
        self.label = list(range(self.R))
        self.xprop, self.xacc = [0] * self.R, [0] * self.R

    def local_sweep(self, r):
        x, res, w, Kt, a = self.x[r], self.res[r], self.w, self.Kt, self.a
        win, theta = self.win[r], self.theta[r]
        u0, u1 = move_uniforms(self.key[r], self.m[r], self.Nd)
        n = float(2 * win + 1)
        for d in range(self.Nd):
            xo = int(x[d])
            xn = xo + int(math.floor(u0[d] * n)) - win
            self.prop[r] += 1
            if xn < 0 or xn >= self.Nw:
                continue
            D = a * (Kt[xn] - Kt[xo])
            dchi = lane_sum((w * D) * ((2.0 * res) + D))
            if dchi <= 0.0 or u1[d] < math.exp(-dchi / (2.0 * theta)):
                res = res + D
                self.chi2[r] = self.chi2[r] + dchi
                x[d] = xn
                self.acc[r] += 1
        self.res[r] = res
        self.m[r] += self.Nd

    def exchange_round(self):
        X = self.X
        for r in range(X % 2, self.R - 1, 2):
            q = (1.0 / (2.0 * self.theta[r]) - 1.0 / (2.0 * self.theta[r + 1])) * (self.chi2[r] - self.chi2[r + 1])
            swap = q >= 0.0 or exchange_uniform(self.key[r], X) < math.exp(q)
            self.xprop[r] += 1
            if swap:
                self.xacc[r] += 1
                for v in (self.x, self.res, self.chi2, self.label):
                    v[r], v[r + 1] = v[r + 1], v[r]
        self.X += 1

    def sweep(self, n_sweeps, first, thermalization=0, refresh=0):
        for i in range(first, first + n_sweeps):
            for r in range(self.R):
                self.local_sweep(r)
            if refresh > 0 and i % refresh == 0:
                for r in range(self.R):
                    self.res[r], fresh = self.rebuild(self.x[r])
                    self.drift[r] = max(self.drift[r], abs(self.chi2[r] - fresh))
                    self.chi2[r] = fresh
            if self.rate > 0 and self.R >= 2 and i % self.rate == 0:
                self.exchange_round()
            if i > thermalization:
                for r in range(self.R):
                    np.add.at(self.hist[r], self.x[r], np.uint64(1))
                    c = self.chi2[r]
                    self.sum[r] = self.sum[r] + c
                    self.sum2[r] = self.sum2[r] + c * c
                    self.min[r] = min(self.min[r], c)
                    self.n_meas[r] += 1

    def stats(self, r):
        """the fields of dqmc_sac_stats"""
        return {"chi2": self.chi2[r], "sum_chi2": self.sum[r], "sum_chi2_sq": self.sum2[r], "min_chi2": self.min[r],
                "max_drift": self.drift[r], "n_meas": self.n_meas[r], "prop": self.prop[r], "acc": self.acc[r],
                "prop_exchange": self.xprop[r], "acc_exchange": self.xacc[r], "replica": self.label[r],
                "moves_drawn": self.m[r], "rounds": self.X, "window": self.win[r]}


def adapt_window(win, prop, acc, n_omega):
    """SAC.run's rule: above 0.6 half as wide again, below 0.4 two thirds, within 1 .. n_omega"""
    rate = acc / prop if prop else 0.5
    if rate > 0.6:
        win = win + (win + 1) // 2
    elif rate < 0.4:
        win = (2 * win) // 3
    return int(min(max(win, 1), n_omega))


def run(lad, thermalization, sweeps, exchange_rate, refresh, done=0, chunks=10):
    """SAC.run on one ladder, from global sweep index done + 1 -> the sweeps done"""
    lad.set_exchange(exchange_rate)
    therm = done + thermalization
    chunk = max(1, thermalization // chunks)
    while done < therm:
        prop, acc = list(lad.prop), list(lad.acc)
        left = therm - done
        n = left if left < 2 * chunk else chunk
        lad.sweep(n, done + 1, therm, refresh)
        done += n
        for r in range(lad.R):
            lad.win[r] = adapt_window(lad.win[r], lad.prop[r] - prop[r], lad.acc[r] - acc[r], lad.Nw)
    lad.sweep(sweeps, done + 1, therm, refresh)
    return done + sweeps


def default_positions(n_deltas, n_omega):
    return [((2 * d + 1) * n_omega) // (2 * n_deltas) for d in range(n_deltas)]


def fermion_kernel(tau, omega, beta):
    """exp(-tau omega) / (1 + exp(-beta omega)) in extended range through logs: -tau omega - log1p(exp(-beta omega))"""
    tau, omega = np.asarray(tau, dtype=np.float64)[:, None], np.asarray(omega, dtype=np.float64)[None, :]
    return np.exp(-tau * omega - np.logaddexp(0.0, -beta * omega))


def two_peak_problem(Nt=24, Nw=81, beta=4.0, sigma=1e-3, seed=7, centres=(-1.5, 1.0), weights=(0.4, 0.6), width=0.25):
    """two Gaussian peaks on a fermion kernel with noise of standard deviation sigma on G(tau): -> dict(tau, omega, beta,
    G, error, A_true (grid weights summing to 1), K [Nt][Nw])"""
    tau = np.linspace(0.0, beta, Nt)
    omega = np.linspace(-4.0, 4.0, Nw)
    A = sum(wt * np.exp(-0.5 * ((omega - c) / width) ** 2) for c, wt in zip(centres, weights))
    A = A / A.sum()
    K = fermion_kernel(tau, omega, beta)
    rng = np.random.RandomState(seed)
    G = K @ A + sigma * rng.standard_normal(Nt)
    return {"tau": tau, "omega": omega, "beta": beta, "G": G, "error": np.full(Nt, sigma), "A_true": A, "K": K}
