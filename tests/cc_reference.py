"""numpy restatement of cc_kernel (current_current_susceptibility, measurements.jl:268-317; attractive override
HubbardModelAttractive.jl:250-266) for the current-current tests: quad by quad on the 2N x 2N matrices, and summed
over EachLocalQuadBySyncedDistance with numpy (vectorised over all (src1, src2) pairs)."""
import numpy as np


def blockdiag(blocks, nb=2):
    """2N x 2N block diagonal from one (attractive: doubled) or two blocks"""
    n = blocks[0].shape[0]
    G = np.zeros((2 * n, 2 * n))
    G[:n, :n] = blocks[0]
    G[n:, n:] = blocks[1] if len(blocks) == 2 else blocks[0]
    return G


def cc_kernel(pg, T, N, src1, trg1, src2, trg2):
    """the generic 2N form, literally (0-based sites; pg = (G00, G0l, Gl0, Gll) and T are 2N x 2N)"""
    G00, G0l, Gl0, Gll = pg
    out = 0.0
    for sg1 in (0, N):
        for sg2 in (0, N):
            s1, t1, s2, t2 = src1 + sg1, trg1 + sg1, src2 + sg2, trg2 + sg2
            out += ((T[s1, t1] * Gll[t1, s1] - T[t1, s1] * Gll[s1, t1])
                    * (T[s2, t2] * G00[t2, s2] - T[t2, s2] * G00[s2, t2])
                    + T[t1, s1] * T[t2, s2] * (-G0l[s2, t1]) * Gl0[s1, t2]
                    - T[s1, t1] * T[t2, s2] * (-G0l[s2, s1]) * Gl0[t1, t2]
                    - T[t1, s1] * T[s2, t2] * (-G0l[t2, t1]) * Gl0[s1, s2]
                    + T[s1, t1] * T[s2, t2] * (-G0l[t2, s1]) * Gl0[t1, s2])
    return out


def cc_kernel_attractive(pg, T, src1, trg1, src2, trg2):
    """HubbardModelAttractive.jl:250-266 on the single N x N block"""
    G00, G0l, Gl0, Gll = pg
    s1, t1, s2, t2 = src1, trg1, src2, trg2
    return (4.0 * (T[s1, t1] * Gll[t1, s1] - T[t1, s1] * Gll[s1, t1])
            * (T[s2, t2] * G00[t2, s2] - T[t2, s2] * G00[s2, t2])
            + 2.0 * T[t1, s1] * T[t2, s2] * (-G0l[s2, t1]) * Gl0[s1, t2]
            - 2.0 * T[s1, t1] * T[t2, s2] * (-G0l[s2, s1]) * Gl0[t1, t2]
            - 2.0 * T[t1, s1] * T[s2, t2] * (-G0l[t2, t1]) * Gl0[s1, s2]
            + 2.0 * T[s1, t1] * T[s2, t2] * (-G0l[t2, s1]) * Gl0[t1, s2])


def _slice_sum(pg, T, dir_of, trg_of, nd, attractive):
    """sum over the synced quads of one slice: (nd, K), vectorised over the n^2 pairs (src1, src2)"""
    n, K = trg_of.shape
    S1, S2 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    S1, S2 = S1.ravel(), S2.ravel()
    D = dir_of[S1, S2]
    out = np.zeros((nd, K))
    shifts = [(0, 0)] if attractive else [(a, b) for a in (0, n) for b in (0, n)]
    G00, G0l, Gl0, Gll = pg
    for k in range(K):
        t1a, t2a = trg_of[S1, k], trg_of[S2, k]
        m = (t1a >= 0) & (t2a >= 0)
        src1, trg1, src2, trg2, d = S1[m], t1a[m], S2[m], t2a[m], D[m]
        v = np.zeros(len(d))
        for sg1, sg2 in shifts:
            s1, t1, s2, t2 = src1 + sg1, trg1 + sg1, src2 + sg2, trg2 + sg2
            a = T[s1, t1] * Gll[t1, s1] - T[t1, s1] * Gll[s1, t1]
            b = T[s2, t2] * G00[t2, s2] - T[t2, s2] * G00[s2, t2]
            x = (T[t1, s1] * T[t2, s2] * (-G0l[s2, t1]) * Gl0[s1, t2]
                 - T[s1, t1] * T[t2, s2] * (-G0l[s2, s1]) * Gl0[t1, t2]
                 - T[t1, s1] * T[s2, t2] * (-G0l[t2, t1]) * Gl0[s1, s2]
                 + T[s1, t1] * T[s2, t2] * (-G0l[t2, s1]) * Gl0[t1, s2])
            v += 4.0 * a * b + 2.0 * x if attractive else a * b + x
        out[:, k] = np.bincount(d, weights=v, minlength=nd)
    return out


def current_current_susceptibility(g00_blocks, steps, T_blocks, iterator, attractive, delta_tau):
    """what apply!(::CombinedGreensIterator) + finish! push for current_current_susceptibility: the sum over the
    steps (G0l, Gl0, Gll) (each a list of per-block matrices) of the synced quads, times delta_tau / N.
    `iterator` is an EachLocalQuadBySyncedDistance (its dir_of / trg_of tables are used)."""
    dir_of, trg_of = iterator.pairs_by_dir.dir_of, iterator.trg_of
    n, nd = trg_of.shape[0], iterator.pairs_by_dir.ndirections()
    if attractive:
        T = T_blocks[0]
        G00 = g00_blocks[0]
        mk = lambda g0l, gl0, gll: (G00, g0l[0], gl0[0], gll[0])
    else:
        T = blockdiag(T_blocks)
        G00 = blockdiag(g00_blocks)
        mk = lambda g0l, gl0, gll: (G00, blockdiag(g0l), blockdiag(gl0), blockdiag(gll))
    out = np.zeros((nd, iterator.K))
    for g0l, gl0, gll in steps:
        out += _slice_sum(mk(g0l, gl0, gll), T, dir_of, trg_of, nd, attractive)
    return out * delta_tau / n
