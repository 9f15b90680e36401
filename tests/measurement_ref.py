"""Table-driven numpy references of the measurement sums, vectorised over the n^2 (src, trg) pairs.

The formulas are the block-diagonal form of the reference's generic 2N x 2N kernels (measurements.jl:51-190, 208-219,
268-317; attractive overrides HubbardModelAttractive.jl:219-266): both Hubbard models here have block-diagonal G and T,
so every cross-spin element is zero and the functions take the per-block N x N matrices (one block: attractive, two:
repulsive).  The literal 2N x 2N restatements live in oracle/ref_test_oracle.py and tests/cc_reference.py;
tests/test_measurement_tables.py holds the two against each other.

Every function returns (value, abs_sum) per observable: abs_sum is the same sum with every factor of every product
replaced by its absolute value and every sign by +, i.e. the quantity that a rounding-error bound of the sum is
proportional to.  Factors are taken as the formulas form them, so (1 - G_ii) enters as |1 - G_ii|.

Tables: dir_of[src, trg] (0-based direction), nd directions, trg_of[src, k] (-1: no target)."""
import numpy as np


def _sum_terms(terms):
    """terms: list of (coefficient, factor, factor, ...) -> (sum of products, sum of |products|)"""
    v = a = 0.0
    for coef, *fs in terms:
        p, q = coef, abs(coef)
        for f in fs:
            p = p * f
            q = q * np.abs(f)
        v, a = v + p, a + q
    return v, a


def _bin(dir_of, nd, v, a, scale):
    d = np.asarray(dir_of).ravel()
    return (np.bincount(d, weights=np.ravel(v), minlength=nd) * scale,
            np.bincount(d, weights=np.ravel(a), minlength=nd) * scale)


def equal_time(blocks, dir_of, nd):
    """CDC, SDCx/y/z per direction (sum over the pairs of the direction / N) and Mx/y/z per site of one configuration"""
    A = blocks[0]
    n = A.shape[0]
    eye = np.eye(n)
    ii = lambda X: np.diag(X)[:, None] * np.ones((1, n))   # X[i, i] at [i, j]
    jj = lambda X: np.ones((n, 1)) * np.diag(X)[None, :]   # X[j, j] at [i, j]
    out = {}
    if len(blocks) == 1:  # HubbardModelAttractive.jl:222-236
        t = [(2.0, eye - A.T, A)]
        out["CDC"] = _bin(dir_of, nd, *_sum_terms([(4.0, 1 - ii(A), 1 - jj(A))] + t), 1.0 / n)
        for k in ("SDCx", "SDCy", "SDCz"):
            out[k] = _bin(dir_of, nd, *_sum_terms(t), 1.0 / n)
        z = np.zeros(n)
        out["Mx"] = out["My"] = out["Mz"] = (z, z)
        return out
    B = blocks[1]
    same = [(1.0, 1 - ii(A), 1 - jj(A)), (1.0, eye - A.T, A), (1.0, 1 - ii(B), 1 - jj(B)), (1.0, eye - B.T, B)]
    out["CDC"] = _bin(dir_of, nd, *_sum_terms(same + [(1.0, 1 - ii(A), 1 - jj(B)), (1.0, 1 - ii(B), 1 - jj(A))]), 1.0 / n)
    out["SDCz"] = _bin(dir_of, nd, *_sum_terms(same + [(-1.0, 1 - ii(A), 1 - jj(B)), (-1.0, 1 - ii(B), 1 - jj(A))]), 1.0 / n)
    xy = _bin(dir_of, nd, *_sum_terms([(1.0, eye - A.T, B), (1.0, eye - B.T, A)]), 1.0 / n)
    out["SDCx"] = out["SDCy"] = xy
    z = np.zeros(n)
    out["Mx"] = out["My"] = (z, z)
    out["Mz"] = (np.diag(B) - np.diag(A), np.abs(np.diag(B)) + np.abs(np.diag(A)))
    return out


def _quad_sum(A, B, dir_of, nd, trg_of, scale):
    """out[dir12, k1, k2] = sum over (s1, s2) of direction dir12 of A[s1, s2] B[trg(s1, k1), trg(s2, k2)] * scale"""
    n, K = trg_of.shape
    ok = trg_of >= 0
    tc = np.where(ok, trg_of, 0)
    val, ab = np.zeros((nd, K, K)), np.zeros((nd, K, K))
    absA, absB = np.abs(A), np.abs(B)
    for k1 in range(K):
        for k2 in range(K):
            m = np.outer(ok[:, k1], ok[:, k2])
            ix = np.ix_(tc[:, k1], tc[:, k2])
            val[:, k1, k2], ab[:, k1, k2] = _bin(dir_of, nd, A * B[ix] * m, absA * absB[ix] * m, scale)
    return val, ab


def pairing(blocks, dir_of, nd, trg_of):
    """pairing correlation [dir12, k1, k2] of one configuration: G_up[s1, s2] G_dn[t1, t2] / N"""
    A = blocks[0]
    return _quad_sum(A, blocks[-1], dir_of, nd, trg_of, 1.0 / A.shape[0])


def packed_step(g00, g0l, gl0, gll, dir_of, nd):
    """CDS, SDSx/y/z of one time step (packed kernels), sum over the pairs / N; no delta_tau yet"""
    n = g00[0].shape[0]
    ii = lambda X: np.diag(X)[:, None] * np.ones((1, n))
    jj = lambda X: np.ones((n, 1)) * np.diag(X)[None, :]
    out = {}
    if len(g00) == 1:  # HubbardModelAttractive.jl:226-241
        x = (-2.0, g0l[0].T, gl0[0])
        out["CDS"] = _bin(dir_of, nd, *_sum_terms([(4.0, 1 - ii(gll[0]), 1 - jj(g00[0])), x]), 1.0 / n)
        for k in ("SDSx", "SDSy", "SDSz"):
            out[k] = _bin(dir_of, nd, *_sum_terms([x]), 1.0 / n)
        return out
    lu, ld, zu, zd = 1 - ii(gll[0]), 1 - ii(gll[1]), 1 - jj(g00[0]), 1 - jj(g00[1])
    same = [(1.0, lu, zu), (-1.0, g0l[0].T, gl0[0]), (1.0, ld, zd), (-1.0, g0l[1].T, gl0[1])]
    out["CDS"] = _bin(dir_of, nd, *_sum_terms(same + [(1.0, lu, zd), (1.0, ld, zu)]), 1.0 / n)
    out["SDSz"] = _bin(dir_of, nd, *_sum_terms(same + [(-1.0, lu, zd), (-1.0, ld, zu)]), 1.0 / n)
    xy = _bin(dir_of, nd, *_sum_terms([(-1.0, g0l[0].T, gl0[1]), (-1.0, g0l[1].T, gl0[0])]), 1.0 / n)
    out["SDSx"] = out["SDSy"] = xy
    return out


def cc_step(T, g00, g0l, gl0, gll, dir_of, nd, trg_of):
    """current-current sums [dir12, k] of one time step / N (cc_kernel block-wise, tests/cc_reference._slice_sum with the
    t >= 0 masks): (sum_b a_b)(s1, k) (sum_b b_b)(s2, k) + sum_b cross_b; attractive 4 a b + 2 cross"""
    n, K = trg_of.shape
    nb = len(g00)
    afac, xfac = (2.0, 2.0) if nb == 1 else (1.0, 1.0)
    val, ab = np.zeros((nd, K)), np.zeros((nd, K))
    for k in range(K):
        ok = trg_of[:, k] >= 0
        t = np.where(ok, trg_of[:, k], 0)
        s = np.arange(n)
        m = np.outer(ok, ok)
        a = a_abs = b = b_abs = 0.0
        x = x_abs = 0.0
        for blk in range(nb):
            Tb = T[blk]
            tst, tts = Tb[s, t], Tb[t, s]           # T[s, trg], T[trg, s]
            av, aa = _sum_terms([(1.0, tst, gll[blk][t, s]), (-1.0, tts, gll[blk][s, t])])
            bv, ba = _sum_terms([(1.0, tst, g00[blk][t, s]), (-1.0, tts, g00[blk][s, t])])
            a, a_abs, b, b_abs = a + av, a_abs + aa, b + bv, b_abs + ba
            F, B = g0l[blk].T, gl0[blk]              # F[x, y] = G0l[y, x]
            st1, ts1, st2, ts2 = tst[:, None], tts[:, None], tst[None, :], tts[None, :]
            tt = np.ix_(t, t)
            xv, xa = _sum_terms([(-1.0, ts1, ts2, F[t, :], B[:, t]),      # - T[t1,s1] T[t2,s2] G0l[s2,t1] Gl0[s1,t2]
                                 (1.0, st1, ts2, F, B[tt]),                # + T[s1,t1] T[t2,s2] G0l[s2,s1] Gl0[t1,t2]
                                 (1.0, ts1, st2, F[tt], B),                # + T[t1,s1] T[s2,t2] G0l[t2,t1] Gl0[s1,s2]
                                 (-1.0, st1, st2, F[:, t], B[t, :])])      # - T[s1,t1] T[s2,t2] G0l[t2,s1] Gl0[t1,s2]
            x, x_abs = x + xv, x_abs + xa
        v = (afac * afac * np.outer(a, b) + xfac * x) * m
        va = (afac * afac * np.outer(a_abs, b_abs) + xfac * x_abs) * m
        val[:, k], ab[:, k] = _bin(dir_of, nd, v, va, 1.0 / n)
    return val, ab


def susceptibilities(T, g00, steps, dir_of, nd, delta_tau, trg_loc=None, trg_cc=None):
    """the time-displaced sums of one walker: sum over the steps (G0l, Gl0, Gll) (lists of per-block matrices) times
    delta_tau / N -> dict of (value, abs_sum): CDS, SDSx/y/z, PS [dir12, k1, k2] if trg_loc, CCS [dir12, k] if trg_cc"""
    n = g00[0].shape[0]
    out = {}

    def add(k, va):
        out[k] = va if k not in out else (out[k][0] + va[0], out[k][1] + va[1])

    for g0l, gl0, gll in steps:
        for k, va in packed_step(g00, g0l, gl0, gll, dir_of, nd).items():
            add(k, va)
        if trg_loc is not None:  # Gl0_up[s1, s2] Gl0_dn[t1, t2]
            add("PS", _quad_sum(gl0[0], gl0[-1], dir_of, nd, trg_loc, 1.0 / n))
        if trg_cc is not None:
            add("CCS", cc_step(T, g00, g0l, gl0, gll, dir_of, nd, trg_cc))
    return {k: (v * delta_tau, a * delta_tau) for k, (v, a) in out.items()}


def greens_sums(per_walker_blocks):
    """accumulate_greens over the walkers: sum G, sum G^2 (flat, block after block, column-major) and the occupations
    W - sum_w G_ii per block; each (value, abs_sum)"""
    W = len(per_walker_blocks)
    flat = np.array([np.concatenate([b.reshape(-1, order="F") for b in blocks]) for blocks in per_walker_blocks])
    diag = np.array([np.concatenate([np.diag(b) for b in blocks]) for blocks in per_walker_blocks])
    return {"G": (flat.sum(axis=0), np.abs(flat).sum(axis=0)),
            "G2": ((flat * flat).sum(axis=0), (flat * flat).sum(axis=0)),
            "occupation": (W - diag.sum(axis=0), W + np.abs(diag).sum(axis=0))}
