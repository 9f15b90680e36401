"""Reference for the Renyi-2 entanglement measurement (include/dqmc_hip.h "entanglement"): Grover's x(w, w') from a list of
per-walker Green's function blocks in numpy, the same in mpmath at 50 digits, and the brute-force delete-one-walker
jackknife of -log(mean).  Test infrastructure only.

mpmath's matrix product and determinant cost about 6 N_A^3 microseconds per pair in pure Python (12 s at N_A = 128), so
above MP_DIRECT_SITES sites the extended-precision value comes from det_fixed_point: the same elimination in 240-bit
fixed-point integers (72 digits) on numpy object arrays, a thousand times faster.  tests/test_entanglement_host.py holds
the two against each other at N_A = 1, 17 and 64."""
import itertools
import math

import mpmath
import numpy as np

MP_DIGITS = 50
MP_DIRECT_SITES = 17   # up to here pair_value_mp calls mpmath.det itself
FIXED_BITS = 240


def restrict(G, sites):
    """G_A[i, j] = G[a_i, a_j], the sites in the order given"""
    a = np.asarray(sites, dtype=np.int64)
    return np.asarray(G, dtype=np.float64)[np.ix_(a, a)]


def pair_matrix(Ga, Gb):
    return np.eye(Ga.shape[0]) - Ga - Gb + 2.0 * (Ga @ Gb)


def pair_value(blocks_w, blocks_v, sites):
    """x(w, w') of two walkers' lists of G blocks (one block: the determinant squared)"""
    dets = [np.linalg.det(pair_matrix(restrict(g, sites), restrict(gp, sites))) for g, gp in zip(blocks_w, blocks_v)]
    return dets[0] ** 2 if len(dets) == 1 else float(np.prod(dets))


def pair_sample(greens, sites):
    """greens: per walker a list of n x n blocks -> [W, W], x(w, w') in the strictly upper triangle, 0 elsewhere"""
    W = len(greens)
    x = np.zeros((W, W))
    for w, v in itertools.combinations(range(W), 2):
        x[w, v] = pair_value(greens[w], greens[v], sites)
    return x


def det_mpmath(Ga, Gb):
    """det(I - Ga - Gb + 2 Ga Gb) with mpmath's own product and determinant (call inside workdps)"""
    A, B = mpmath.matrix(Ga.tolist()), mpmath.matrix(Gb.tolist())
    return mpmath.det(mpmath.eye(A.rows) - A - B + 2 * (A * B))


def det_fixed_point(Ga, Gb):
    """the same determinant by Gaussian elimination with partial pivoting in fixed-point integers of FIXED_BITS
    fractional bits (the float64 inputs go in exactly, down to 2^-FIXED_BITS), as an mpf (call inside workdps)"""
    S, n = FIXED_BITS, Ga.shape[0]
    one = 1 << S
    fix = lambda X: np.array([[int(math.ldexp(float(v), S)) for v in row] for row in X], dtype=object).reshape((n, n))
    A, B = fix(Ga), fix(Gb)
    M = -A - B + 2 * (A.dot(B) // one)
    for i in range(n):
        M[i, i] += one
    sign, pivots = 1, []
    for k in range(n):
        p = max(range(k, n), key=lambda i: abs(M[i, k]))
        if M[p, k] == 0:
            return mpmath.mpf(0)
        if p != k:
            M[[k, p]] = M[[p, k]]
            sign = -sign
        piv = M[k, k]
        pivots.append(piv)
        if k < n - 1:
            l = (M[k + 1:, k] * one) // piv
            M[k + 1:, k + 1:] -= np.outer(l, M[k, k + 1:]) // one
    return sign * mpmath.fprod(mpmath.mpf(int(p)) / one for p in pivots)


def pair_value_mp(blocks_w, blocks_v, sites, direct=None):
    """pair_value at MP_DIGITS digits and more, from the float64 inputs taken exactly; returned as an mpf.  direct:
    True = mpmath.det, False = det_fixed_point, None = mpmath.det up to MP_DIRECT_SITES sites"""
    direct = len(sites) <= MP_DIRECT_SITES if direct is None else direct
    with mpmath.workdps(MP_DIGITS):
        dets = [(det_mpmath if direct else det_fixed_point)(restrict(g, sites), restrict(gp, sites))
                for g, gp in zip(blocks_w, blocks_v)]
        return dets[0] ** 2 if len(dets) == 1 else mpmath.fprod(dets)


def pair_sample_mp(greens, sites):
    """pair_sample in mpmath -> [W, W] object array of mpf (0 outside the strictly upper triangle)"""
    W = len(greens)
    x = np.zeros((W, W), dtype=object)
    for w, v in itertools.combinations(range(W), 2):
        x[w, v] = pair_value_mp(greens[w], greens[v], sites)
    return x


def reference_error(greens, sites):
    """(numpy sample, e_ref): e_ref = max over pairs of |numpy - mpmath| / |mpmath|, the float64 reference's own error"""
    x = pair_sample(greens, sites)
    xm = pair_sample_mp(greens, sites)
    W = len(greens)
    e = 0.0
    with mpmath.workdps(MP_DIGITS):
        for w, v in itertools.combinations(range(W), 2):
            e = max(e, float(abs(mpmath.mpf(float(x[w, v])) - xm[w, v]) / abs(xm[w, v])))
    return x, e


def relative_to_mp(x, xm):
    """max over pairs of |x - xm| / |xm| for a float sample x against the mpmath sample xm"""
    W = x.shape[0]
    e = 0.0
    with mpmath.workdps(MP_DIGITS):
        for w, v in itertools.combinations(range(W), 2):
            e = max(e, float(abs(mpmath.mpf(float(x[w, v])) - xm[w, v]) / abs(xm[w, v])))
    return e


def jackknife_brute(pair_sums, count):
    """(purity, S2, S2_std_error) of one subsystem's [W, W] pair sums (strictly upper triangle, or symmetric: pair (w, w')
    is read at [min, max]) by actually deleting each walker and averaging over the pairs that are left"""
    ps = np.asarray(pair_sums, dtype=np.float64)
    W = ps.shape[0]

    def mean_over(walkers):
        vals = [ps[w, v] / count for w, v in itertools.combinations(walkers, 2)]
        return sum(vals) / len(vals)

    purity = mean_over(range(W))
    s2 = [-np.log(mean_over([u for u in range(W) if u != w])) for w in range(W)]
    m = sum(s2) / W
    err = np.sqrt((W - 1) / W * sum((s - m) ** 2 for s in s2))
    return purity, -np.log(purity), err


def random_greens(rng, n):
    """a symmetric n x n matrix with spectrum in (0, 1): a generic Green's function stand-in"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.uniform(0.02, 0.98, n)
    G = (Q * lam) @ Q.T
    return 0.5 * (G + G.T)
