"""The re-association that lets the first launch of a factored wrap apply a sweep's last chunk (kron.hip): the stand-alone
flush forms G + (C X Y) R0 with the block-triangular solves on the rows of C (sweep_lu.hip), the wrap forms
G + C (X Y R0) with the solves on the columns of R0, from the same LU image.  The elimination (PT_J, Q_J by rank-1
recurrences) and the literal sequence of accept_local! updates are tools/proto/lu_sweep_proto.py's (a script with one
fixed seed), restated here as functions of the seed; no GPU needed."""
import numpy as np
import pytest

KD = 64


def _blk(J):
    return slice(16 * J, 16 * J + 16)


def _eliminate(rng, n, site0):
    """phase A of the prototype: G0, the compact factor F (strict upper Uu, strict lower L), x, PT_J, Q_J, and the
    decisions (gamma, accepted) for the literal replay"""
    G0 = 0.5 * np.eye(n) + 0.1 * rng.standard_normal((n, n))
    gam = np.where(rng.random(KD) < 0.5, 0.88, -0.47)
    accept = rng.random(KD) < 0.8
    S = G0[site0:site0 + KD, site0:site0 + KD].copy()
    xs = np.zeros(KD)
    PT = [np.eye(16) for _ in range(4)]
    Q = [np.eye(16) for _ in range(4)]
    for s in range(KD):
        if not accept[s]:
            continue
        x = gam[s] / (1.0 + gam[s] * (1.0 - S[s, s]))
        xs[s] = x
        I0, cc = s // 16, s % 16
        v = S[s, :].copy(); v[: s + 1] = 0.0
        u = S[:, s].copy(); u[: s + 1] = 0.0
        S += np.outer(x * u, v)
        vb, ub = v[_blk(I0)], u[_blk(I0)]
        PT[I0] += np.outer(x * vb, PT[I0][cc, :])
        Q[I0] += np.outer(x * ub, Q[I0][cc, :])
    return G0, S, xs, PT, Q, gam, accept


def _sequential(G0, gam, accept, site0):
    """the literal sequence of rank-1 updates (accept_local!: G -= (e_i - G[:, i]) x G[i, :]), site by site"""
    G = G0.copy()
    for s in range(KD):
        if not accept[s]:
            continue
        i = site0 + s
        x = gam[s] / (1.0 + gam[s] * (1.0 - G[i, i]))
        IG = -G[:, i].copy()
        IG[i] += 1.0
        G -= np.outer(IG * x, G[i, :])
    return G


def _flush(G0, F, xs, PT, Q, site0):
    """sweep_flush_lu_kernel: T' = Y' X C' block by block, G + T R0"""
    n = G0.shape[0]
    X = np.diag(xs)
    C0T = G0[:, site0:site0 + KD].T.copy()
    C0T[np.arange(KD), site0 + np.arange(KD)] -= 1.0
    XZ = [None] * 4
    for J in range(4):
        acc = C0T[_blk(J), :].copy()
        for K in range(J):
            acc += F[_blk(K), _blk(J)].T @ XZ[K]
        XZ[J] = X[_blk(J), _blk(J)] @ (PT[J] @ acc)
    TT = [None] * 4
    for J in range(3, -1, -1):
        acc = np.zeros((16, n))
        for K in range(J + 1, 4):
            acc += F[_blk(K), _blk(J)].T @ TT[K]
        TT[J] = Q[J].T @ (XZ[J] + X[_blk(J), _blk(J)] @ acc)
    return G0 + np.vstack(TT).T @ G0[site0:site0 + KD, :]


def _wrap_fold(G0, F, xs, PT, Q, site0):
    """kr_apply_pending: R^ = X Y R0 on the columns (image tiles PT_J' = (I - X Uu_JJ)^-1 and Q_J as held), G + C R^"""
    X = np.diag(xs)
    R0 = G0[site0:site0 + KD, :]
    C = G0[:, site0:site0 + KD].copy()
    C[site0 + np.arange(KD), np.arange(KD)] -= 1.0
    XV = [None] * 4
    for J in range(4):
        acc = R0[_blk(J), :].copy()
        for K in range(J):
            acc += F[_blk(J), _blk(K)] @ XV[K]          # L_JK
        XV[J] = X[_blk(J), _blk(J)] @ (Q[J] @ acc)
    RH = [None] * 4
    for J in range(3, -1, -1):
        acc = np.zeros_like(XV[J])
        for K in range(J + 1, 4):
            acc += F[_blk(J), _blk(K)] @ RH[K]          # Uu_JK
        RH[J] = PT[J].T @ (XV[J] + X[_blk(J), _blk(J)] @ acc)
    return G0 + C @ np.vstack(RH)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("site0", [0, 192])
def test_fold_reassociation_matches_flush(seed, site0):
    rng = np.random.default_rng(seed)
    n = 256
    G0, F, xs, PT, Q, gam, accept = _eliminate(rng, n, site0)
    Gf = _flush(G0, F, xs, PT, Q, site0)
    Gw = _wrap_fold(G0, F, xs, PT, Q, site0)
    rel = np.abs(Gw - Gf).max() / np.abs(Gf).max()
    assert rel < 1e-14, rel
    # and both are the literal sequence of rank-1 updates (accept_local!) ...
    Gs = _sequential(G0, gam, accept, site0)
    assert np.abs(Gw - Gs).max() / np.abs(Gs).max() < 1e-12
    # ... and the closed form G + C X Y R0 with explicit inverses (independent of the block solves)
    X = np.diag(xs)
    Uu, L = np.triu(F, 1), np.tril(F, -1)
    Y = np.linalg.inv(np.eye(KD) - Uu @ X) @ np.linalg.inv(np.eye(KD) - L @ X)
    C = G0[:, site0:site0 + KD].copy()
    C[site0 + np.arange(KD), np.arange(KD)] -= 1.0
    Gd = G0 + C @ (X @ Y @ G0[site0:site0 + KD, :])
    assert np.abs(Gw - Gd).max() / np.abs(Gd).max() < 1e-12
