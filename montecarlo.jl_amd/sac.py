"""The SAC flavor: stochastic analytic continuation of imaginary-time data (Sandvik, PRB 57, 10287; Beach,
cond-mat/0403055; Shao and Sandvik, Phys. Rep. 1003), `P` problems x `R` sampling temperatures batched on one device
(csrc/sac.hip; include/dqmc_hip.h, "the SAC flavor", defines every step).  The reference has no such flavor.

The host builds the kernel table, rotates data and table into the eigenbasis of the covariance, holds the loop control
and turns the histograms into spectra; every move runs on the device."""
import ctypes as C
import math

import numpy as np

from ._lib import DQMCError, SacParams, SacStats, dptr, lib

STAT_FIELDS = tuple(f for f, _ in SacStats._fields_)
WINDOW_CHUNKS = 10               # thermalisation is run in this many chunks, the windows adapted in between
ACC_LOW, ACC_HIGH = 0.4, 0.6     # the band around one half the acceptance of a chunk is steered into


def fermion_kernel(tau, omega, beta):
    """K[i, j] = exp(-tau_i omega_j) / (1 + exp(-beta omega_j)) for 0 <= tau <= beta, without overflow for either sign
    of omega: for omega < 0 it is exp((beta - tau) omega) / (1 + exp(beta omega))"""
    tau, omega = np.asarray(tau, dtype=np.float64)[:, None], np.asarray(omega, dtype=np.float64)[None, :]
    pos = omega >= 0.0
    ao = np.abs(omega)
    num = np.exp(-np.where(pos, tau, beta - tau) * ao)
    return num / (1.0 + np.exp(-beta * ao))


def boson_symmetric_kernel(tau, omega, beta):
    """K[i, j] = (exp(-tau_i omega_j) + exp(-(beta - tau_i) omega_j)) / (1 + exp(-beta omega_j)) for omega >= 0: the
    kernel of a correlator with C(tau) = C(beta - tau) whose spectral weight B(omega) = S(omega) (1 + exp(-beta omega))
    is sampled on the positive axis; K[i, j] = 1 at tau = 0 and at omega = 0"""
    tau, omega = np.asarray(tau, dtype=np.float64)[:, None], np.asarray(omega, dtype=np.float64)[None, :]
    if np.any(omega < 0.0):
        raise ValueError("boson_symmetric_kernel: omega >= 0")
    return (np.exp(-tau * omega) + np.exp(-(beta - tau) * omega)) / (1.0 + np.exp(-beta * omega))


def rotate(G, K, covariance, cut=1e-10):
    """-> (g, w, Kr): data and kernel in the eigenbasis of the covariance, C = U diag(lam) U^T: g = U^T G, Kr = U^T K,
    w = 1 / lam, so that sum_i w_i (Kr A - g)_i^2 = (K A - G)^T C^-1 (K A - G).  The eigenvalues are taken in descending
    order; those below cut * lam_max are dropped"""
    lam, U = np.linalg.eigh(np.asarray(covariance, dtype=np.float64))
    order = np.argsort(lam)[::-1]
    lam, U = lam[order], U[:, order]
    keep = lam > cut * lam[0]
    U = U[:, keep]
    return U.T @ np.asarray(G, dtype=np.float64), 1.0 / lam[keep], U.T @ np.asarray(K, dtype=np.float64)


def adapt_window(win, prop, acc, n_omega):
    """the window after a thermalisation chunk with `prop` moves of which `acc` were accepted: half as wide again above
    an acceptance of 0.6, two thirds below 0.4, within 1 .. n_omega"""
    rate = acc / prop if prop else 0.5
    if rate > ACC_HIGH:
        win = win + (win + 1) // 2
    elif rate < ACC_LOW:
        win = (2 * win) // 3
    return int(min(max(win, 1), n_omega))


def select_theta(thetas, mean_chi2, min_chi2, a=1.0):
    """the index of the largest theta with <chi2> <= chi2_min + a sqrt(2 chi2_min), chi2_min the smallest chi2 any
    replica of the ladder has measured; where no theta meets it, the one with the smallest <chi2>"""
    thetas, mean_chi2 = np.asarray(thetas, dtype=np.float64), np.asarray(mean_chi2, dtype=np.float64)
    lo = float(np.min(min_chi2))
    ok = mean_chi2 <= lo + a * math.sqrt(2.0 * max(lo, 0.0))
    if not ok.any():
        return int(np.argmin(mean_chi2))
    return int(np.argmax(np.where(ok, thetas, -np.inf)))


def default_positions(n_deltas, n_omega):
    """the flat start: delta d at grid point floor((d + 1/2) n_omega / n_deltas)"""
    return ((2 * np.arange(n_deltas, dtype=np.int64) + 1) * n_omega // (2 * n_deltas)).astype(np.uint16)


class SAC:
    """SAC(tau, G, error=... | covariance=..., kernel=fermion_kernel, omega=grid, beta=...) for G of shape [Nt] or
    [P, Nt]: P independent problems on one grid.

    `error` holds the standard errors sigma_i of G ([Nt] or [P, Nt]); `covariance` ([Nt, Nt] or [P, Nt, Nt]) is
    eigendecomposed on the host (rotate), eigenvalues below `cut` relative to the largest are dropped (weight zero where
    another problem of the batch keeps more of them), which lowers Nt.  `kernel` is a function (tau, omega, beta) or the
    table [Nt, Nw] itself.  The spectrum is `n_deltas` delta functions of weight norm / n_deltas on the grid points of
    `omega`; `thetas` are the R sampling temperatures, one ladder for every problem or [P, R].  Chain (p, r) draws from
    the Philox4x32-10 stream keyed by `seed + 16 p + r`."""

    def __init__(self, tau, G, error=None, covariance=None, kernel=fermion_kernel, omega=None, beta=None, n_deltas=256,
                 thetas=None, norm=1.0, seed=1, device_id=0, cut=1e-10, window=None):
        tau = np.asarray(tau, dtype=np.float64).reshape(-1)
        G = np.atleast_2d(np.asarray(G, dtype=np.float64))
        if omega is None:
            raise ValueError("SAC needs the frequency grid omega")
        self.omega = np.asarray(omega, dtype=np.float64).reshape(-1)
        P, Nt, Nw = G.shape[0], tau.size, self.omega.size
        if G.shape[1] != Nt:
            raise ValueError("G must have shape [Nt] or [P, Nt] with Nt = len(tau)")
        if (error is None) == (covariance is None):
            raise ValueError("give either error or covariance")
        if callable(kernel):
            if beta is None:
                raise ValueError("a kernel function needs beta")
            K = kernel(tau, self.omega, beta)
        else:
            K = np.asarray(kernel, dtype=np.float64)
        if K.shape != (Nt, Nw):
            raise ValueError("the kernel table must have shape [Nt, Nw]")
        if error is not None:
            err = np.broadcast_to(np.asarray(error, dtype=np.float64), G.shape)
            if not np.all(np.isfinite(err)) or np.any(err <= 0.0):
                raise ValueError("every error must be finite and > 0")
            rot = [(G[p], 1.0 / (err[p] * err[p]), K) for p in range(P)]
        else:
            cov = np.asarray(covariance, dtype=np.float64)
            cov = np.broadcast_to(cov, (P, Nt, Nt))
            rot = [rotate(G[p], K, cov[p], cut) for p in range(P)]
        self.n_tau = max(len(g) for g, _, _ in rot)
        self.g, self.w = np.zeros((P, self.n_tau)), np.zeros((P, self.n_tau))
        self.Kt = np.zeros((P, Nw, self.n_tau))  # grid-major
        for p, (g, w, Kr) in enumerate(rot):
            self.g[p, :len(g)], self.w[p, :len(g)], self.Kt[p, :, :len(g)] = g, w, Kr.T
        self.norm = np.broadcast_to(np.asarray(norm, dtype=np.float64), (P,)).copy()
        th = np.geomspace(20.0, 0.02, 12) if thetas is None else np.asarray(thetas, dtype=np.float64)
        self.thetas = np.broadcast_to(np.atleast_2d(th), (P, np.atleast_2d(th).shape[1])).copy()
        self.P, self.R, self.n_omega, self.n_deltas = P, self.thetas.shape[1], Nw, int(n_deltas)
        self.seed = int(seed)
        self.sweeps_done = 0
        self.thermalization = 0
        win = max(1, Nw // 10) if window is None else int(window)
        par = SacParams(P, self.n_tau, self.n_deltas, Nw, self.R, int(device_id), win, dptr(np.ascontiguousarray(self.thetas[0])))
        self._h = C.c_void_p()
        rc = lib().dqmc_sac_create(C.byref(par), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise DQMCError(rc, (lib().dqmc_sac_last_error(None) or b"").decode())
        try:
            x0 = default_positions(self.n_deltas, Nw)
            for p in range(P):
                self._c(lib().dqmc_sac_set_problem(self._h, p, dptr(np.ascontiguousarray(self.g[p])),
                                                   dptr(np.ascontiguousarray(self.w[p])),
                                                   dptr(np.ascontiguousarray(self.Kt[p])), float(self.norm[p])))
                self._c(lib().dqmc_sac_set_theta(self._h, p, dptr(np.ascontiguousarray(self.thetas[p]))))
                for r in range(self.R):
                    self._c(lib().dqmc_sac_seed(self._h, p, r, self.chain_seed(p, r)))
                    self.set_conf(p, r, x0)
        except BaseException:
            self.close()
            raise

    def chain_seed(self, p, r):
        return (self.seed + 16 * p + r) & 0xFFFFFFFFFFFFFFFF

    def _c(self, rc):
        if rc != 0:
            raise DQMCError(rc, (lib().dqmc_sac_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().dqmc_sac_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # ---- the chains
    def set_conf(self, p, r, x):
        x = np.ascontiguousarray(x, dtype=np.uint16)
        if x.shape != (self.n_deltas,):
            raise ValueError("x must hold n_deltas positions")
        self._c(lib().dqmc_sac_set_conf(self._h, p, r, x.ctypes.data_as(C.POINTER(C.c_uint16))))

    def conf(self, p, r):
        x = np.zeros(self.n_deltas, dtype=np.uint16)
        self._c(lib().dqmc_sac_get_conf(self._h, p, r, x.ctypes.data_as(C.POINTER(C.c_uint16))))
        return x

    def set_window(self, p, r, win):
        self._c(lib().dqmc_sac_set_window(self._h, p, r, int(win)))

    def set_exchange(self, rate):
        self._c(lib().dqmc_sac_set_exchange(self._h, int(rate)))

    def sweep(self, n_sweeps, thermalization=0, refresh=0):
        """n_sweeps more sweeps of every chain (dqmc_sac_sweep); the global sweep index goes on from the last call"""
        self._c(lib().dqmc_sac_sweep(self._h, int(n_sweeps), self.sweeps_done + 1, int(thermalization), int(refresh)))
        self.sweeps_done += int(n_sweeps)

    def stats(self, p, r):
        st = SacStats()
        self._c(lib().dqmc_sac_get_stats(self._h, p, r, C.byref(st)))
        return st

    def histogram(self, p, r):
        h = np.zeros(self.n_omega, dtype=np.uint64)
        self._c(lib().dqmc_sac_get_histogram(self._h, p, r, h.ctypes.data_as(C.POINTER(C.c_uint64))))
        return h

    def reset_accumulators(self):
        self._c(lib().dqmc_sac_reset_accumulators(self._h))

    # ---- the run
    def run(self, thermalization=1000, sweeps=4000, exchange_rate=1, refresh=16):
        """`thermalization` sweeps in WINDOW_CHUNKS chunks (the last one takes the remainder), each chain's window moved
        towards an acceptance near one half after every chunk (adapt_window, from the chunk's own prop and acc), then
        `sweeps` measured sweeps with the windows fixed.  An exchange round after every `exchange_rate`-th sweep (0:
        none), a refresh of res and chi2 after every `refresh`-th (0: never)."""
        self.set_exchange(exchange_rate)
        self.thermalization = therm = self.sweeps_done + int(thermalization)
        chunk = max(1, int(thermalization) // WINDOW_CHUNKS)
        while self.sweeps_done < therm:
            before = [[self.stats(p, r) for r in range(self.R)] for p in range(self.P)]
            left = therm - self.sweeps_done
            self.sweep(left if left < 2 * chunk else chunk, therm, refresh)
            for p in range(self.P):
                for r in range(self.R):
                    st = self.stats(p, r)
                    win = adapt_window(st.window, st.prop - before[p][r].prop, st.acc - before[p][r].acc, self.n_omega)
                    if win != st.window:
                        self.set_window(p, r, win)
        self.sweep(int(sweeps), therm, refresh)

    def chi2(self):
        """-> dict(mean, std, min [P, R], n_meas): <chi2>, its standard deviation over the measurements and the smallest
        measured chi2 of every slot"""
        mean, std, lo = (np.full((self.P, self.R), np.nan) for _ in range(3))
        n = 0
        for p in range(self.P):
            for r in range(self.R):
                st = self.stats(p, r)
                n = st.n_meas
                if n:
                    mean[p, r] = st.sum_chi2 / n
                    std[p, r] = math.sqrt(max(st.sum_chi2_sq / n - mean[p, r] ** 2, 0.0))
                    lo[p, r] = st.min_chi2
        return {"mean": mean, "std": std, "min": lo, "n_meas": n}

    def select_theta(self, a=1.0):
        """-> [P] indices into the ladders (select_theta)"""
        c = self.chi2()
        return np.array([select_theta(self.thetas[p], c["mean"][p], c["min"][p], a) for p in range(self.P)])

    def spectrum(self, theta=None):
        """-> dict(omega [Nw], A [P, Nw], weight [P, Nw], chi2 [P], theta [P]): of the slot `theta` (an index into the
        ladder; None: select_theta() per problem).  weight[j] = norm hist[j] / (n_meas n_deltas) is the spectral weight
        on grid point j (it sums to norm); A = weight / cell width (numpy.gradient of omega) is the density"""
        idx = self.select_theta() if theta is None else np.full(self.P, int(theta))
        c = self.chi2()
        weight = np.zeros((self.P, self.n_omega))
        for p in range(self.P):
            n = self.stats(p, int(idx[p])).n_meas
            if n == 0:
                raise DQMCError(-4, "spectrum: no measurement has been taken")
            weight[p] = self.histogram(p, int(idx[p])).astype(np.float64) * (self.norm[p] / (float(n) * self.n_deltas))
        return {"omega": self.omega.copy(), "A": weight / np.gradient(self.omega)[None, :], "weight": weight,
                "chi2": c["mean"][np.arange(self.P), idx], "theta": self.thetas[np.arange(self.P), idx]}
