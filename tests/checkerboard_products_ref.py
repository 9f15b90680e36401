"""Extended-precision reference of the seven sparse checkerboard products (include/dqmc_hip.h, dqmc_set_checkerboard),
written from the header's description of the sequences, not from csrc/cb.hip:

  0 B X = P Mu eV X      1 B^-1 X = eV^-1 Mu^-1 P^-1 X      2 B' X = eV Mu P' X
  3 X B = X P Mu eV      4 X B^-1 = X eV^-1 Mu^-1 P^-1      5 X eT      6 eTinv X

P, eT and eTinv are the factor sequences of the tables (applied first to last), Mu = diag(mu[block]), eV = diag(exp(+lambda
s_i)) in block 0 and diag(exp(-lambda s_i)) in block 1 (the spin-down block of the repulsive model).  A left product mixes
the rows of X, a right product its columns, and a right product takes the rows of the stored (transposed) factors.

apply() takes the arrays the device got (tables() below packs them as DQMC.__init__ does) and works in np.longdouble with
ELL gathers only, so n = 1024 stays cheap.  It returns (value, bound_base): bound_base is the same chain evaluated with
absolute values, |post| |F_s| ... |F_1| |pre| |X| |qscale|, the quantity every rounding of the device is relative to.

Tolerance of the device tests (derived, not measured): |device - value| <= bound(...) = 2 (kmax seq_len + 6) eps
bound_base per element: kmax seq_len roundings of the factor applications (kmax products summed per factor), 6 for the two
scalings, their products with the conf-derived exponentials (whose last bit may differ between the two exp() in use) and
qscale, and the project's usual factor 2."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# which -> (side, pre, post); side 0: rows mixed (left product), 1: columns mixed; pre / post: (sign of lambda, vector) of
# the diagonal applied to the mixed index before / after the factors
SCALINGS = {
    0: (0, (+1, "mu"), None),
    1: (0, None, (-1, "mu_inv")),
    2: (0, None, (+1, "mu")),
    3: (1, None, (+1, "mu")),
    4: (1, (-1, "mu_inv"), None),
    5: (1, None, None),
    6: (0, None, None),
}
NAMES = ("B X", "B^-1 X", "B' X", "X B", "X B^-1", "X eT", "eTinv X")


def lambdas(U, delta_tau):
    """exp(+lambda), exp(-lambda), lambda = acosh(exp(U dtau / 2)) (HubbardModelAttractive.jl:103)"""
    lam = np.arccosh(np.exp(0.5 * U * delta_tau))
    return float(np.exp(lam)), float(np.exp(-lam))


def tables(pkg, model, delta_tau):
    """what DQMC.__init__ hands dqmc_set_checkerboard for `model`: ELL vals / cols of block 0, mu / mu_inv [nb][n], seqs"""
    tb = [pkg.checkerboard_tables(T, model.l, delta_tau) for T in model.hopping_matrix()]
    return dict(kmax=tb[0]["kmax"], vals=tb[0]["vals"], cols=tb[0]["cols"], seqs=[list(s) for s in tb[0]["seqs"]],
                mu=np.stack([t["mu"] for t in tb]), mu_inv=np.stack([t["mu_inv"] for t in tb]))


def padded(tabs, kmax):
    """the same factors in a wider ELL table: padding entries val 0, col = the row, as the header prescribes"""
    m, n, k0 = tabs["vals"].shape
    vals = np.zeros((m, n, kmax))
    cols = np.tile(np.arange(n, dtype=np.int32)[None, :, None], (m, 1, kmax))
    vals[:, :, :k0] = tabs["vals"]
    cols[:, :, :k0] = tabs["cols"]
    return dict(tabs, kmax=kmax, vals=vals, cols=np.ascontiguousarray(cols))


def _diagonal(spec, tabs, conf, epl, eml, nb, swap_block1):
    """[units][n]: the diagonal scaling of the mixed index, unit = walker * nb + block"""
    W, n = conf.shape
    s = np.ones((W, nb, n), dtype=LD)
    if spec is not None:
        sign, vec = spec
        for b in range(nb):
            sg = -sign if (b == 1 and swap_block1) else sign
            s[:, b, :] = np.where(conf * sg > 0, LD(epl), LD(eml)) * tabs[vec][b].astype(LD)[None, :]
    return s.reshape(W * nb, n)


def apply(which, X, tabs, conf, epl, eml, nb, qscale=None, Xabs=None, scalings=SCALINGS, swap_block1=True):
    """sequence `which` on X [units][n][n] (unit = walker * nb + block) with the HS slice conf [walkers][n] (+-1).
    Xabs: the bound_base of X when X is itself a computed product (compositions); default |X|.
    scalings / swap_block1 exist for the mutants of test_checkerboard_products_ref.py."""
    side, pre, post = scalings[which]
    Y = np.asarray(X).astype(LD)
    A = np.abs(np.asarray(X if Xabs is None else Xabs).astype(np.float64))  # (a bound's base needs no extended precision)
    if side == 1:  # mixed index first
        Y, A = np.ascontiguousarray(Y.transpose(0, 2, 1)), np.ascontiguousarray(A.transpose(0, 2, 1))
    spre = _diagonal(pre, tabs, conf, epl, eml, nb, swap_block1)
    spost = _diagonal(post, tabs, conf, epl, eml, nb, swap_block1)
    Y, A = Y * spre[:, :, None], A * np.abs(spre).astype(np.float64)[:, :, None]
    vals, cols = tabs["vals"], tabs["cols"]
    for m in tabs["seqs"][which]:
        Yn = An = None
        for j in range(vals.shape[2]):  # row k of the result gathers row cols[m, k, j]
            if not np.any(vals[m, :, j]):
                continue  # (a column of padding)
            t = np.take(Y, cols[m, :, j], axis=1)
            t *= vals[m, :, j].astype(LD)[None, :, None]
            a = np.take(A, cols[m, :, j], axis=1)
            a *= np.abs(vals[m, :, j])[None, :, None]
            Yn, An = (t, a) if Yn is None else (Yn + t, An + a)
        Y, A = Yn, An
    Y, A = Y * spost[:, :, None], A * np.abs(spost).astype(np.float64)[:, :, None]
    if qscale is not None:
        q = np.asarray(qscale, dtype=np.float64)
        Y, A = Y * q.astype(LD)[:, None, :], A * np.abs(q)[:, None, :]
    if side == 1:
        Y, A = Y.transpose(0, 2, 1), A.transpose(0, 2, 1)
    return Y, A


def roundings(tabs, which, kmax=None):
    """kmax seq_len + 6 (module docstring)"""
    return (tabs["kmax"] if kmax is None else kmax) * len(tabs["seqs"][which]) + 6


def bound(tabs, which, base, kmax=None):
    return 2.0 * roundings(tabs, which, kmax) * EPS * base


def apply_dense(which, X, factors, conf, epl, eml, nb):
    """the same seven products with the dense group matrices of checkerboard_exponentials(..., return_factors=True),
    factors = [per block: (H, Hinv, C, Cinv, mu, mu_inv, n_groups)], in np.longdouble, written out product by product
    (slice_matrices.jl:104-222, DQMC.jl:731-750)"""
    X = np.asarray(X).astype(LD)
    out = np.zeros_like(X)
    for u in range(X.shape[0]):
        w, b = divmod(u, nb)
        H, Hi, Cm, Ci, mu, mui, ng = factors[b]
        H, Hi = [h.astype(LD) for h in H], [h.astype(LD) for h in Hi]
        C1, Ci1 = Cm[0].astype(LD), Ci[0].astype(LD)
        sg = 1 if b == 0 else -1
        ev = np.where(conf[w] * sg > 0, LD(epl), LD(eml)) * mu.astype(LD)         # Mu eV
        evi = np.where(conf[w] * sg > 0, LD(eml), LD(epl)) * mui.astype(LD)       # eV^-1 Mu^-1
        M = X[u]

        def left(M, h, c, tr=False):
            t = (lambda a: a.T) if tr else (lambda a: a)
            for i in range(ng - 1, 0, -1):
                M = t(h[i]) @ M
            M = t(c) @ M
            for i in range(1, ng):
                M = t(h[i]) @ M
            return M

        def right(M, h, c):
            for i in range(ng - 1, 0, -1):
                M = M @ h[i]
            M = M @ c
            for i in range(1, ng):
                M = M @ h[i]
            return M

        if which == 0:
            M = left(ev[:, None] * M, H, C1)
        elif which == 1:
            M = evi[:, None] * left(M, Hi, Ci1)
        elif which == 2:
            M = ev[:, None] * left(M, H, C1, tr=True)
        elif which == 3:
            M = right(M, H, C1) * ev[None, :]
        elif which == 4:
            M = right(M * evi[None, :], Hi, Ci1)
        elif which == 5:
            for i in range(ng - 1, -1, -1):
                M = M @ H[i]
        else:
            for i in range(ng - 1, -1, -1):
                M = Hi[i] @ M
        out[u] = M
    return out
