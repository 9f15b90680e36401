"""R^ of a pending chunk (kron.hip: kr_apply_pending) from explicit inverse triangles instead of the two block substitutions.
With the image of a chunk's elimination (tests/test_wrap_flush_algebra.py, tools/proto/lu_sweep_proto.py: F = [L \\ Uu], x,
PT_J' = (I - X_J Uu_JJ)^-1, Q_J = (I - L_JJ X_J)^-1) the substitution solves (I - L X) W = R0, XV = X W, (I - X Uu) R^ = XV.
The product form is R^ = Ainv (X (Binv R0)) with the blocks of Ainv = (I - X Uu)^-1 and Binv = (I - L X)^-1 from the
recurrences that leave only a multiply by the last diagonal inverse once a block row is decided:

    Ainv[I][J] = -(sum_{I<=K<J} Ainv[I][K] A[K][J]) Ainv[J][J],   A[K][J] = -X_K Uu_KJ      (I < J)
    Binv[I][J] = -Binv[I][I] (sum_{J<=K<I} B[I][K] Binv[K][J]),   B[I][K] = -L_IK X_K       (I > J)

(the sums need rows K < J of Uu and row I of L left of the diagonal, which are final before block J / I is decided).

Checked at random acceptance patterns, all-rejected (x = 0: identity triangles, R^ = 0) and all-accepted:
  * the recurrences reproduce numpy's inverses of both 64 x 64 triangles, within 64 eps cond (the forward error of an
    inverse is bounded by a modest multiple of eps cond; 64 = the order);
  * the product form's R^ against the substitution's.  Tolerance as measured, not chosen: the reference is the same
    substitution in np.longdouble on the same image, the float64 substitution's error against it (max-norm, relative,
    largest over all cases below) is the unit, and the product form may have 4 x that (two more roundings per entry and
    the explicit inverse).  Measured on these inputs (largest over the cases): substitution 4.1e-16, product form 3.7e-16;
  * G + C R^ against the flush's G + (C X Y) R0, within the 1e-14 tests/test_wrap_flush_algebra.py allows the substitution
    form for the same comparison."""
import numpy as np
import pytest

from test_wrap_flush_algebra import KD, _blk, _flush

CASES = [(seed, site0, p) for seed in range(4) for site0 in (0, 192) for p in (0.8, 0.3)] + \
        [(0, 0, 0.0), (1, 192, 0.0), (0, 0, 1.0), (1, 192, 1.0)]


def _eliminate(rng, n, site0, p_accept):
    """phase A of the prototype (as in tests/test_wrap_flush_algebra.py) with the acceptance probability as a parameter"""
    G0 = 0.5 * np.eye(n) + 0.1 * rng.standard_normal((n, n))
    gam = np.where(rng.random(KD) < 0.5, 0.88, -0.47)
    accept = rng.random(KD) < p_accept
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
    return G0, S, xs, PT, Q, accept


def _substitution(R0, F, xs, PT, Q, dtype):
    """kr_apply_pending as it is: the two block substitutions, in the given precision"""
    F, xs, R0 = F.astype(dtype), xs.astype(dtype), R0.astype(dtype)
    PT, Q = [p.astype(dtype) for p in PT], [q.astype(dtype) for q in Q]
    XV = [None] * 4
    for J in range(4):
        acc = R0[_blk(J), :].copy()
        for K in range(J):
            acc = acc + F[_blk(J), _blk(K)] @ XV[K]
        XV[J] = xs[_blk(J), None] * (Q[J] @ acc)
    RH = [None] * 4
    for J in range(3, -1, -1):
        acc = np.zeros_like(XV[J])
        for K in range(J + 1, 4):
            acc = acc + F[_blk(J), _blk(K)] @ RH[K]
        RH[J] = PT[J].T @ (XV[J] + xs[_blk(J), None] * acc)
    return np.vstack(RH)


def _inverse_blocks(F, xs, PT, Q):
    """the off-diagonal blocks of both inverse triangles by the recurrences of the module docstring"""
    Ai = {(J, J): PT[J].T for J in range(4)}
    Bi = {(J, J): Q[J] for J in range(4)}
    A = lambda K, J: -xs[_blk(K), None] * F[_blk(K), _blk(J)]
    B = lambda I, K: -F[_blk(I), _blk(K)] * xs[None, _blk(K)]
    for J in range(1, 4):
        for I in range(J):
            acc = np.zeros((16, 16))
            for K in range(I, J):
                acc += Ai[I, K] @ A(K, J)
            Ai[I, J] = -acc @ Ai[J, J]
    for I in range(1, 4):
        for J in range(I):
            acc = np.zeros((16, 16))
            for K in range(J, I):
                acc += B(I, K) @ Bi[K, J]
            Bi[I, J] = -Bi[I, I] @ acc
    return Ai, Bi


def _products(R0, xs, Ai, Bi):
    """R^ = Ainv (X (Binv R0)): block row w of each product is what wave w would form"""
    W = [sum(Bi[I, J] @ R0[_blk(J), :] for J in range(I + 1)) for I in range(4)]
    XV = [xs[_blk(I), None] * W[I] for I in range(4)]
    return np.vstack([sum(Ai[I, J] @ XV[J] for J in range(I, 4)) for I in range(4)])


def _case(seed, site0, p):
    rng = np.random.default_rng(1000 * seed + site0 + int(100 * p))
    G0, F, xs, PT, Q, accept = _eliminate(rng, 256, site0, p)
    return G0, F, xs, PT, Q, accept, G0[site0:site0 + KD, :]


def _relmax(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    d, m = np.abs(a - b).max(), np.abs(b).max()
    return 0.0 if d == 0 else float(d / m)


@pytest.fixture(scope="module")
def substitution_error():
    """the float64 substitution against the same substitution in extended precision: largest over all cases"""
    worst = 0.0
    for c in CASES:
        G0, F, xs, PT, Q, accept, R0 = _case(*c)
        worst = max(worst, _relmax(_substitution(R0, F, xs, PT, Q, np.float64), _substitution(R0, F, xs, PT, Q, np.longdouble)))
    return worst


@pytest.mark.parametrize("seed,site0,p", CASES)
def test_recurrence_gives_the_inverse_triangles(seed, site0, p):
    G0, F, xs, PT, Q, accept, R0 = _case(seed, site0, p)
    assert accept.all() if p == 1.0 else (not accept.any() if p == 0.0 else 0 < accept.sum() < KD)
    Ai, Bi = _inverse_blocks(F, xs, PT, Q)
    X = np.diag(xs)
    A = np.eye(KD) - X @ np.triu(F, 1)
    B = np.eye(KD) - np.tril(F, -1) @ X
    eps = np.finfo(np.float64).eps
    for name, M, blocks, upper in (("A", A, Ai, True), ("B", B, Bi, False)):
        full = np.zeros((KD, KD))
        for (I, J), t in blocks.items():
            full[_blk(I), _blk(J)] = t
        ref = np.linalg.inv(M)
        err = np.abs(full - ref).max() / np.abs(ref).max()
        bound = 64 * eps * np.linalg.cond(M)
        print("%s: |recurrence - inv| = %.3g (bound %.3g)" % (name, err, bound))
        assert err <= bound, (name, err, bound)
        if p == 0.0:
            assert np.array_equal(full, np.eye(KD))


@pytest.mark.parametrize("seed,site0,p", CASES)
def test_products_match_substitution_and_flush(seed, site0, p, substitution_error):
    G0, F, xs, PT, Q, accept, R0 = _case(seed, site0, p)
    Ai, Bi = _inverse_blocks(F, xs, PT, Q)
    Rp = _products(R0, xs, Ai, Bi)
    Rs = _substitution(R0, F, xs, PT, Q, np.float64)
    Rl = _substitution(R0, F, xs, PT, Q, np.longdouble)
    e_sub, e_prod = _relmax(Rs, Rl), _relmax(Rp, Rl)
    print("R^ against extended precision: substitution %.3g, products %.3g (allowed %.3g)" % (e_sub, e_prod, 4 * substitution_error))
    assert e_prod <= 4 * substitution_error, (e_prod, substitution_error)
    if p == 0.0:
        assert not Rp.any() and not Rs.any()
    C = G0[:, site0:site0 + KD].copy()
    C[site0 + np.arange(KD), np.arange(KD)] -= 1.0
    Gp, Gf = G0 + C @ Rp, _flush(G0, F, xs, PT, Q, site0)
    rel = np.abs(Gp - Gf).max() / np.abs(Gf).max()
    assert rel < 1e-14, rel
