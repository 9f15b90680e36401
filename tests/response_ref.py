"""Reference for the pair structure factors, the current response and the superfluid stiffness (include/dqmc_hip.h "pair
structure factors and superfluid stiffness"; test helper, numpy only).

Two things live here.

1. The transforms the device applies to a walker's sample, in numpy.longdouble, each value with the sum of the absolute
   values of its terms, so that a test can bound the device's rounding per element: pair_transform, current_transform,
   bond_kinetic.

2. Free fermions (U = 0) on a periodic Bravais lattice by two independent routes.
   Route 1, real space: the propagators as matrices, G(tau) = e^{-tau T} (1 + e^{-beta T})^{-1} and so on from an
   eigendecomposition of the hopping matrix T, and the Wick sums of pc_kernel / cc_kernel over site quadruples
   (measurement_ref: the same code the device is compared with at U != 0), then the transforms of 1.
   Route 2, band basis: T is diagonal in plane waves, eps(k) = sum_j T[0, j] e^{i k . (x_j - x_0)}; with f = 1 / (e^{beta eps}
   + 1), x_t = x_s - r_k the target of s in direction k (r = pos[src] - pos[trg], EachSitePairByDistance.directions) and
       g(r, tau) = (1/N) sum_k e^{i k r} e^{-tau eps} (1 - f)       [Gl0[a, b] = g(x_a - x_b)]
       h(r, tau) = -(1/N) sum_k e^{i k r} e^{tau eps} f             [G0l[a, b] = h(x_a - x_b)]
   the per-slice sums are, per pair direction R = r_d and with rho = r_k, tk = T[trg, src] of the bond,
       PS_l[d, k1, k2] = g(R) g(R - r_k1 + r_k2)
       CCS_l[d, k]     = S tk^2 [2 h(-R) g(R) - h(-R + rho) g(R + rho) - h(-R - rho) g(R - rho)]
   (S = 2 spin species; the product of the two mean currents vanishes, T and G00 being symmetric), and in momentum space
       P_c(q, tau)   = (1/N) sum_k g_k(tau) g_{q-k}(tau) |phi_c(q - k)|^2,     phi_c(p) = sum_k1 f_c[k1] e^{-i p r_k1}
       CCS_k(q, tau) = -(S/N) sum_p 4 tk^2 sin^2((p + q/2) . rho) f_p (1 - f_{p+q}) e^{-tau (eps_{p+q} - eps_p)}
       kbond[k]      = (S/N) tk sum_p e^{i p rho} f_p
   with sum_{l=1..M} dtau e^{-l dtau a} = dtau e^{-dtau a} expm1(-M dtau a) / expm1(-dtau a) (M dtau at a = 0): the
   engine's Riemann sum l = 1 .. slices, done exactly as a geometric series.
   CCS(q) is negative: cc_kernel sums <J J> of J = T c+c - h.c. without the i of the current j = i J.  The response of
   the stiffness formula is therefore Lambda = -CCS(q), whose longitudinal limit tends to -k_x > 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402

LD = np.longdouble


# ---- 1. the transforms of a walker's sample -------------------------------------------------------------------------
def _rows(v, Ct, St):
    """rows [r, nd] -> ([cos rows][sin rows] flat q fastest, abs sums)"""
    C, S = Ct.astype(LD), St.astype(LD)
    val = np.concatenate([(v @ C).ravel(), (v @ S).ravel()])
    ab = np.concatenate([(np.abs(v) @ np.abs(C)).ravel(), (np.abs(v) @ np.abs(S)).ravel()])
    return val, ab


def pair_transform(x, F, nd, Ct, St, scale=1.0):
    """x: the pairing sample [nd K K] flat (d fastest); F [K K, n_ch] -> (value, abs_sum, n_terms) of the sample
    [P cos: n_ch n_q][P sin: n_ch n_q]; every element is a sum of n_terms = K K nd products"""
    KK = F.shape[0]
    X = x.astype(LD).reshape(KK, nd)
    Fl = F.astype(LD)
    Z, Zab = Fl.T @ X, np.abs(Fl).T @ np.abs(X)  # [n_ch, nd]
    C, S = Ct.astype(LD), St.astype(LD)
    val = np.concatenate([(Z @ C).ravel(), (Z @ S).ravel()]) * LD(scale)
    ab = np.concatenate([(Zab @ np.abs(C)).ravel(), (Zab @ np.abs(S)).ravel()]) * abs(scale)
    return val, ab, KK * nd


def current_transform(ccs, nd, Ct, St, scale=1.0):
    """ccs [nd K_cc] flat (d fastest) -> (value, abs_sum, n_terms) of [Lambda cos: K_cc n_q][Lambda sin: K_cc n_q]"""
    val, ab = _rows(ccs.astype(LD).reshape(-1, nd), Ct, St)
    return val * LD(scale), ab * abs(scale), nd


def bond_kinetic(G, T, trg):
    """kbond[k] from Green's blocks G, hopping blocks T, targets trg [n, K] -> (value, abs_sum, n_terms)"""
    n, K = trg.shape
    fac = 2.0 if len(G) == 1 else 1.0
    val, ab = np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
    for k in range(K):
        src = np.nonzero(trg[:, k] >= 0)[0]
        t = trg[src, k]
        for b in range(len(G)):
            terms = T[b][t, src].astype(LD) * ((src == t).astype(LD) - G[b][src, t].astype(LD))
            val[k] += fac * terms.sum() / n
            ab[k] += fac * (np.abs(T[b][t, src]).astype(LD) * ((src == t) + np.abs(G[b][src, t]).astype(LD))).sum() / n
    return val, ab, n * len(G)


# ---- 2. free fermions ---------------------------------------------------------------------------------------------------
class FreeFermions:
    """U = 0 on a periodic Bravais lattice: T one n x n hopping matrix (the same for both spin species), `pairs` an
    EachSitePairByDistance, trg_loc / trg_cc the target tables [n, K] of the local / current iterators, pos the site
    positions, q [n_q, dim] the wave vectors, grid the N allowed momenta (momentum_grid)."""

    def __init__(self, T, pairs, trg_loc, trg_cc, pos, grid, q, beta, delta_tau):
        self.T = np.asarray(T, dtype=np.float64)
        self.n = self.T.shape[0]
        self.dir_of, self.nd = np.asarray(pairs.dir_of), pairs.ndirections()
        self.r = np.array(pairs.directions, dtype=np.float64)
        self.trg_loc, self.trg_cc = np.asarray(trg_loc), np.asarray(trg_cc)
        self.pos, self.grid, self.q = np.asarray(pos, dtype=np.float64), np.asarray(grid, dtype=np.float64), np.asarray(q, dtype=np.float64)
        self.beta, self.dtau = float(beta), float(delta_tau)
        self.M = int(round(beta / delta_tau))
        self.Ct, self.St = np.cos(self.r @ self.q.T), np.sin(self.r @ self.q.T)

    # route 1
    def matrices(self, l):
        """(G00, G0l, Gl0, Gll) at tau = l dtau as matrices"""
        w, V = np.linalg.eigh(self.T)
        f = 1.0 / (np.exp(self.beta * w) + 1.0)
        tau = l * self.dtau
        mk = lambda d: (V * d) @ V.T
        return mk(1.0 - f), mk(-np.exp(tau * w) * f), mk(np.exp(-tau * w) * (1.0 - f)), mk(1.0 - f)

    def real_space(self):
        """-> dict: PS_l, CCS_l (per slice, l = 1 .. M), PS, CCS (sum_l dtau), kbond, from site quadruples"""
        g00 = self.matrices(0)[0]
        steps, ps_l, ccs_l = [], [], []
        for l in range(1, self.M + 1):
            _, g0l, gl0, gll = self.matrices(l)
            steps.append(([g0l], [gl0], [gll]))
            ps_l.append(MR._quad_sum(gl0, gl0, self.dir_of, self.nd, self.trg_loc, 1.0 / self.n)[0])
            ccs_l.append(MR.cc_step([self.T], [g00], [g0l], [gl0], [gll], self.dir_of, self.nd, self.trg_cc)[0])
        sus = MR.susceptibilities([self.T], [g00], steps, self.dir_of, self.nd, self.dtau, self.trg_loc, self.trg_cc)
        kb = bond_kinetic([g00], [self.T], self.trg_cc)[0].astype(np.float64)
        return dict(PS_l=np.array(ps_l), CCS_l=np.array(ccs_l), PS=sus["PS"][0], CCS=sus["CCS"][0], kbond=kb,
                    PC=MR.pairing([g00], self.dir_of, self.nd, self.trg_loc)[0])

    def momentum_space_from_real(self, rs, channels):
        """P_c(q) (equal time and tau-integrated) and Lambda_kk(q) as the transforms of route 1's real-space sums"""
        Ct, St = self.Ct, self.St
        out = {"P": {}, "chi": {}}
        for name, f in channels.items():
            for key, X in (("P", rs["PC"]), ("chi", rs["PS"])):
                z = np.einsum("dab,a,b->d", X, f, f)
                out[key][name] = z @ Ct - 1j * (z @ St)
        out["Lambda"] = rs["CCS"].T @ Ct - 1j * (rs["CCS"].T @ St)
        return out

    # route 2
    def eps(self, k):
        """band energy at wave vectors k [..., dim]"""
        dx = self.pos - self.pos[0]
        return np.real(np.tensordot(np.exp(1j * np.tensordot(k, dx.T, axes=1)), self.T[0], axes=1))

    def _fermi(self, e):
        return 1.0 / (np.exp(self.beta * e) + 1.0)

    def _gh(self, r, tau):
        """g(r, tau), h(r, tau) for displacements r [..., dim]"""
        e = self.eps(self.grid)
        f = self._fermi(e)
        ph = np.exp(1j * np.tensordot(r, self.grid.T, axes=1))
        return np.real(ph @ (np.exp(-tau * e) * (1.0 - f))) / self.n, -np.real(ph @ (np.exp(tau * e) * f)) / self.n

    def _bond(self, trg, k):
        """(rho, tk) of direction k of a target table"""
        s = int(np.nonzero(trg[:, k] >= 0)[0][0])
        return self.r[k], self.T[trg[s, k], s]

    def _tau_sum(self, a):
        """sum_{l=1..M} dtau e^{-l dtau a}"""
        a = np.asarray(a, dtype=np.float64)
        x = -self.dtau * a
        small = np.abs(x) < 1e-300
        xs = np.where(small, 1.0, x)
        return np.where(small, self.M * self.dtau, self.dtau * np.exp(xs) * np.expm1(self.M * xs) / np.expm1(xs))

    def band_basis(self, channels):
        """-> the quantities of real_space() and momentum_space_from_real() from sums over k of Fermi factors"""
        n, nd, M = self.n, self.nd, self.M
        K, Kcc = self.trg_loc.shape[1], self.trg_cc.shape[1]
        R = self.r
        ps_l, ccs_l = np.zeros((M, nd, K, K)), np.zeros((M, nd, Kcc))
        for l in range(1, M + 1):
            tau = l * self.dtau
            gR = self._gh(R, tau)[0]
            for k1 in range(K):
                for k2 in range(K):
                    ps_l[l - 1, :, k1, k2] = gR * self._gh(R - R[k1] + R[k2], tau)[0]
            hm = self._gh(-R, tau)[1]
            for k in range(Kcc):
                rho, tk = self._bond(self.trg_cc, k)
                ccs_l[l - 1, :, k] = 2.0 * tk ** 2 * (2.0 * hm * gR - self._gh(-R + rho, tau)[1] * self._gh(R + rho, tau)[0]
                                                      - self._gh(-R - rho, tau)[1] * self._gh(R - rho, tau)[0])
        g0 = self._gh(R, 0.0)[0]
        pc = np.zeros((nd, K, K))
        for k1 in range(K):
            for k2 in range(K):
                pc[:, k1, k2] = g0 * self._gh(R - R[k1] + R[k2], 0.0)[0]
        kg = self.grid
        e, out = self.eps(kg), {"P": {}, "chi": {}}
        f = self._fermi(e)
        kb = np.zeros(Kcc)
        for k in range(Kcc):
            rho, tk = self._bond(self.trg_cc, k)
            kb[k] = 2.0 * tk * np.real(np.exp(1j * kg @ rho) @ f) / n
        lam = np.zeros((Kcc, len(self.q)), dtype=complex)
        for iq, q in enumerate(self.q):
            e2 = self.eps(q - kg)  # q - k
            f2 = self._fermi(e2)
            for name, fc in channels.items():
                phi2 = np.abs(np.exp(-1j * (q - kg) @ R[:K].T) @ fc) ** 2
                out["P"].setdefault(name, np.zeros(len(self.q), dtype=complex))[iq] = np.sum((1 - f) * (1 - f2) * phi2) / n
                out["chi"].setdefault(name, np.zeros(len(self.q), dtype=complex))[iq] = \
                    np.sum((1 - f) * (1 - f2) * phi2 * self._tau_sum(e + e2)) / n
            ep = self.eps(kg + q)
            fp = self._fermi(ep)
            for k in range(Kcc):
                rho, tk = self._bond(self.trg_cc, k)
                lam[k, iq] = -2.0 / n * np.sum(4.0 * tk ** 2 * np.sin((kg + 0.5 * q) @ rho) ** 2 * f * (1 - fp) * self._tau_sum(ep - e))
        out["Lambda"] = lam
        return dict(PS_l=ps_l, CCS_l=ccs_l, PS=self.dtau * ps_l.sum(axis=0), CCS=self.dtau * ccs_l.sum(axis=0), kbond=kb, PC=pc), out


def stiffness(kbond, Lambda, kp, km, iL, iT):
    """the host formula of DQMC.superfluid_stiffness from kbond [K_cc] and the engine-convention Lambda [K_cc, n_q]"""
    k_axis = kbond[kp] + kbond[km]
    lam = -np.real(Lambda[kp])
    return dict(k_axis=k_axis, Lambda_L=lam[iL], Lambda_T=lam[iT], rho_s=(-k_axis - lam[iT]) / 4.0, drude=-k_axis - lam[iL])


def free_fermions(pkg, lattice, beta, delta_tau, mu=0.0, t=1.0, qs=None):
    """FreeFermions of a lattice of the package `pkg` with its default iterators; -> (ff, local iterator, current iterator)"""
    n = len(lattice)
    T = np.zeros((n, n))
    for s, trg in lattice.neighbors(directed=True):
        T[trg - 1, s - 1] += -t
    T[np.diag_indices(n)] += -mu
    pairs = pkg.EachSitePairByDistance(lattice)
    loc = pkg.EachLocalQuadByDistance(lattice, pairs=pairs)
    cur = pkg.EachLocalQuadBySyncedDistance(lattice, pairs=pairs)
    from importlib import import_module
    lat = import_module(pkg.__name__ + ".lattices")
    grid = pkg.momentum_grid(lattice)[0]
    ff = FreeFermions(T, pairs, loc.trg_of, cur.trg_of, np.array(lat._positions(lattice)), grid, grid if qs is None else qs,
                      beta, delta_tau)
    return ff, loc, cur
