"""References for the DQMC global moves (include/dqmc_hip.h "global moves", csrc/logdet.hip, csrc/global_move.inl).

* slogdet_mp: sign and log|det| of I + B_M ... B_1 per block in mpmath at 60 digits, B_l = eT2 eV(l)
  (slice_matrices.jl:23-39), eV(l) = exp(+-lambda conf[:, l]) (HubbardModelAttractive.jl:100-110,
  HubbardModelRepulsive.jl:113-126).  A float64 product is no oracle at beta >= 4: its small singular values are rounding
  noise.  By default the inputs are the engine's own: the float64 eT2 of hopping_exponentials and the float64
  exp(+-lambda), taken exactly; exact=True takes exp(-dtau T) and lambda in extended precision instead (the closed-form
  tests, which compare two extended-precision numbers).
* oracle_logdet: the reference's algorithm in float64 with the CPU oracle's udt_AVX_pivot! and rdivp!: the slice chain of
  calculate_greens(mc, 0) (stack.jl:422-480), calculate_greens_AVX! (stack.jl:337-393) up to its second UDT, sum log D2 and
  the sign of det A2.  Its distance from slogdet_mp is what the tolerances of test_gpu_global_move.py are derived from.
* philox4_uniform / move_uniform, weight_ratio, decide, apply_flip: the move as the header defines it.
Shared by test_global_move_reference.py (CPU) and test_gpu_global_move.py."""
import json
import math
import os

import mpmath as mp
import numpy as np

from ising_wolff_ref import philox4_uniform

DPS = 60
FLIP_ALL, FLIP_SITE = 0, 1
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logdet_sizes.json")


def field(seed, n, M):
    """the seeded HS field of the logdet and global-move tests"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    return np.asfortranarray((2 * rng.integers(0, 2, size=(n, M)) - 1).astype(np.int8))


def golden_model(pkg, case):
    """the model of one entry of tests/golden/logdet_sizes.json (written by tools/make_logdet_golden.py)"""
    kind, L = case["lattice"]
    if kind == "cubic":
        lat = pkg.CubicLattice(3, L)
    else:
        lat = {"square": pkg.SquareLattice, "triangular": pkg.TriangularLattice}[kind](L)
    if case["model"] == "attractive":
        return pkg.HubbardModelAttractive(l=lat, U=case["U"], mu=case["mu"])
    return pkg.HubbardModelRepulsive(l=lat, U=case["U"])


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def hs_lambda(U, delta_tau):
    """lambda = acosh(exp(U dtau / 2)) as the engine computes it (float64)"""
    return math.acosh(math.exp(0.5 * U * delta_tau))


def _eT2_float(model, delta_tau):
    """the float64 hopping_matrix_exp_squared per block, by the recipe of dqmc.hopping_exponentials (stack.jl:167-181)"""
    out = []
    for T in model.hopping_matrix():
        w, V = np.linalg.eigh(-0.5 * delta_tau * T)
        eT = (V * np.exp(w)) @ V.T
        out.append(eT @ eT)
    return out


def _to_mp(a):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(a)])


def slice_inputs(model, delta_tau, exact=False):
    """-> (eT2 per block as mp matrices, e^{+lambda}, e^{-lambda}) at the working precision in force"""
    if exact:
        lam = mp.acosh(mp.exp(mp.mpf(model.U) * mp.mpf(delta_tau) / 2))
        eT2 = [mp.expm(-mp.mpf(delta_tau) * _to_mp(T)) for T in model.hopping_matrix()]
        return eT2, mp.exp(lam), mp.exp(-lam)
    lam = hs_lambda(model.U, delta_tau)
    return [_to_mp(e) for e in _eT2_float(model, delta_tau)], mp.mpf(math.exp(lam)), mp.mpf(math.exp(-lam))


def chain_mp(eT2, epl, eml, conf, block):
    """B_M ... B_1 of one block (0: exp(+lambda s), 1: exp(-lambda s))"""
    n, M = conf.shape
    P = mp.eye(n)
    for l in range(M):
        for i in range(n):  # eV(l) P: row i scaled
            up = (conf[i, l] > 0) == (block == 0)
            f = epl if up else eml
            for j in range(n):
                P[i, j] *= f
        P = eT2 * P
    return P


def slogdet_mp(model, delta_tau, conf, exact=False, with_greens=False):
    """-> (logabsdet [nb] as mpf, sign [nb]) of I + B_M ... B_1; with_greens also the inverses G_b (mp matrices)"""
    with mp.workdps(DPS):
        eT2, epl, eml = slice_inputs(model, delta_tau, exact)
        lad, sg, Gs = [], [], []
        for b in range(model.flv):
            A = mp.eye(conf.shape[0]) + chain_mp(eT2[b], epl, eml, conf, b)
            d = mp.det(A)
            lad.append(mp.log(abs(d)))
            sg.append(1 if d > 0 else -1)
            if with_greens:
                Gs.append(A ** -1)
        return (lad, sg, Gs) if with_greens else (lad, sg)


def oracle_logdet(O, model, delta_tau, safe_mult, conf):
    """float64, the reference's algorithm: -> (sum log D2 [nb], sign det A2 [nb], A2 [nb])"""
    n, M = conf.shape
    lam = hs_lambda(model.U, delta_tau)
    epl, eml = math.exp(lam), math.exp(-lam)
    lad, sg, A2s = [], [], []
    for b, eT2 in enumerate(_eT2_float(model, delta_tau)):
        cur, Dr, Tr = np.eye(n), np.ones(n), np.eye(n)
        Ur = np.eye(n)
        for k in range(M, 0, -1):  # B_k' X = eV (eT2' X)
            ev = np.where((conf[:, k - 1] > 0) == (b == 0), epl, eml)
            cur = ev[:, None] * (eT2.T @ cur)
            if k % safe_mult == 0:
                cur, Dr, T, _ = O.udt_pivot(cur * Dr[None, :], True)
                Tr = T @ Tr
        Ur, Dr, T, _ = O.udt_pivot(cur * Dr[None, :], True)
        Tr = T @ Tr
        # calculate_greens_AVX! with Ul = Tl = I, Dl = 1 up to the second UDT
        U1, D1, T1, piv = O.udt_pivot(Tr.T * Dr[None, :], False)
        Ur = O.rdivp(Ur, T1, piv)
        A2 = U1.T @ Ur + np.diag(D1)
        _, D2, _, _ = O.udt_pivot(A2, False)
        lad.append(float(np.sum(np.log(D2))))
        sg.append(int(np.linalg.slogdet(A2)[0]))
        A2s.append(A2)
    return lad, sg, A2s


def second_route_logdet(O, model, delta_tau, safe_mult, conf):
    """float64 by another stabilisation: B_M ... B_1 = U D T accumulated from the right-hand end with a pivoted QR every
    safe_mult slices (the forward chain, where oracle_logdet factors the daggered one), then, with Db = max(D, 1) and
    Ds = min(D, 1),  I + U Db Ds T = U Db (Db^-1 U' + Ds T):  logabsdet = sum log Db + log|det(Db^-1 U' + Ds T)|, the sign
    that of det U det(Db^-1 U' + Ds T), both determinants by LAPACK's LU -> (logabsdet [nb], sign [nb])"""
    n, M = conf.shape
    lam = hs_lambda(model.U, delta_tau)
    epl, eml = math.exp(lam), math.exp(-lam)
    lad, sg = [], []
    for b, eT2 in enumerate(_eT2_float(model, delta_tau)):
        cur, D, T = np.eye(n), np.ones(n), np.eye(n)
        for l in range(M):  # B_l X = eT2 (eV X)
            ev = np.where((conf[:, l] > 0) == (b == 0), epl, eml)
            cur = eT2 @ (ev[:, None] * cur)
            if (l + 1) % safe_mult == 0 or l == M - 1:
                cur, D, T1, _ = O.udt_pivot(cur * D[None, :], True)
                T = T1 @ T
        Db, Ds = np.maximum(D, 1.0), np.minimum(D, 1.0)
        s1, l1 = np.linalg.slogdet(cur.T / Db[:, None] + Ds[:, None] * T)
        s2, _ = np.linalg.slogdet(cur)
        lad.append(float(np.sum(np.log(Db)) + l1))
        sg.append(int(round(s1 * s2)))
    return lad, sg


# ---- the move ------------------------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def move_uniform(seed, m, t):
    """u(m, t): Philox4x32-10, key = seed, counter words (t, low32(m), 1, high32(m))"""
    return float(philox4_uniform(seed, t, m & _M32, 1, m >> 32))


def pick_site(u, N):
    return min(N - 1, int(math.floor(u * N)))


def apply_flip(conf, kind, site=None):
    c = conf.copy()
    if kind == FLIP_ALL:
        return -c
    c[site, :] = -c[site, :]
    return c


def weight_ratio(model, delta_tau, conf, conf_new, exact=False):
    """p of the move conf -> conf_new as an mpf: attractive exp(lambda (sum conf - sum conf')) det'^2 / det^2
    (HubbardModelAttractive.jl:113-127), repulsive det_up' det_dn' / (det_up det_dn) (HubbardModelRepulsive.jl:128-156)"""
    l0, s0 = slogdet_mp(model, delta_tau, conf, exact)
    l1, s1 = slogdet_mp(model, delta_tau, conf_new, exact)
    with mp.workdps(DPS):
        if model.flv == 1:
            lam = mp.acosh(mp.exp(mp.mpf(model.U) * mp.mpf(delta_tau) / 2)) if exact else mp.mpf(hs_lambda(model.U, delta_tau))
            dS = int(conf.astype(np.int64).sum() - conf_new.astype(np.int64).sum())
            return mp.exp(lam * dS + 2 * (l1[0] - l0[0]))
        return s0[0] * s0[1] * s1[0] * s1[1] * mp.exp((l1[0] - l0[0]) + (l1[1] - l0[1]))


def decide(p, next_uniform):
    """accept iff p > 1 || u < p, u = next_uniform() drawn only when p <= 1 (DQMC.jl:573) -> (accepted, drawn)"""
    if p > 1:
        return True, False
    return next_uniform() < p, True
