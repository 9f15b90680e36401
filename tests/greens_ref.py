"""Chain-graded inputs and an extended-precision reference for calculate_greens_AVX! (stack.jl:337-393).

* graded_udt_inputs(n, g, seed, batch): (Ul, Dl, Tl, Ur, Dr, Tr) as a stack hands them over at low temperature - U random
  orthogonal, D = exp(linspace(+g, -g, n)) jittered by a seeded factor in [0.9, 1.1] and sorted descending (g = 20: more
  than 17 decades on each side of 1), T = (I + triu(0.3 randn, 1)) with a seeded column permutation, which is what
  D^-1 R P' of a pivoted UDT looks like: unit diagonal, bounded rows, well conditioned.  Unit u of a batch is the input
  of seed + u, whatever the batch, so that a stored expected value belongs to (n, g, seed + u).
* greens_mp(args, digits): G = [I + Ul Dl Tl (Ur Dr Tr)']^-1 by a direct product and an LU with partial pivoting in
  mpmath numbers (numpy object arrays of mpf: the arithmetic is mpmath's, the loops numpy's).  At g = 40 the product spans
  70 decades; 80 digits leave more than 40 for the inverse.
* probe(G, V): G V and G' V for a seeded V in {-1, +1}^(n x 4), in np.longdouble from a float64 G or in mpmath from an
  mp G.  Every entry of V is +-1, so an error in any single entry of G shows up undiminished in both probes.
* probe_err / diag_err: max |x - ref| / max |ref|, per probe (the larger of the two) and on diag(G): the measure of
  tests/golden/greens_graded.json / .npy (tools/make_greens_golden.py), test_greens_golden.py and test_gpu_greens_graded.py.
Plain Python, CPU only."""
import json
import os

import mpmath as mp
import numpy as np

DIGITS = 80
PROBE_COLUMNS = 4
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "greens_graded.json")
PRESORT_ALL_SITES = 7  # orc_set_udt_presort: every call site pre-sorted, as the device's default qrb_sites = 7


def load_golden():
    """the .json, with every case's "probe" (2 x n x 4) and "diag" (n) taken from the .npy at the case's offset"""
    with open(GOLDEN_PATH) as f:
        g = json.load(f)
    values = np.load(os.path.splitext(GOLDEN_PATH)[0] + ".npy")
    assert values.dtype == np.float64 and values.size == sum(9 * c["n"] for c in g["cases"])
    for c in g["cases"]:
        n, v = c["n"], values[c["offset"]:c["offset"] + 9 * c["n"]]
        c["probe"] = v[:8 * n].reshape(2, n, PROBE_COLUMNS)
        c["diag"] = v[8 * n:]
    return g


def graded_unit(n, g, seed):
    rng = np.random.Generator(np.random.Philox(key=seed))
    Ul, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Ur, _ = np.linalg.qr(rng.standard_normal((n, n)))
    D = []
    for _ in range(2):
        d = np.exp(np.linspace(g, -g, n)) * rng.uniform(0.9, 1.1, n)
        D.append(np.sort(d)[::-1].copy())
    T = []
    for _ in range(2):
        t = np.eye(n) + np.triu(0.3 * rng.standard_normal((n, n)), 1)
        T.append(np.ascontiguousarray(t[:, rng.permutation(n)]))
    return Ul, D[0], T[0], Ur, D[1], T[1]


def graded_udt_inputs(n, g, seed, batch):
    """-> (Ul, Dl, Tl, Ur, Dr, Tr), each stacked over the batch; g a number or one per unit"""
    gs = [g] * batch if np.isscalar(g) else list(g)
    units = [graded_unit(n, gs[u], seed + u) for u in range(batch)]
    return tuple(np.stack([a[k] for a in units]) for k in range(6))


def unit(args, u):
    return tuple(a[u] for a in args)


def _to_mp(a):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mp.mpf(float(a[idx]))
    return out


def _inverse_mp(A):
    """LU with partial pivoting, then both substitutions on all columns of the permuted identity at once"""
    n = A.shape[0]
    A = A.copy()
    B = _to_mp(np.eye(n))
    for k in range(n):
        p = k + max(range(n - k), key=lambda i: abs(A[k + i, k]))
        if p != k:
            A[[k, p]] = A[[p, k]]
            B[[k, p]] = B[[p, k]]
        if k + 1 < n:
            l = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] -= np.multiply.outer(l, A[k, k + 1:])
            B[k + 1:, :] -= np.multiply.outer(l, B[k, :])
    for k in range(n - 1, -1, -1):
        B[k, :] = B[k, :] / A[k, k]
        if k:
            B[:k, :] -= np.multiply.outer(A[:k, k], B[k, :])
    return B


def greens_mp(args, digits=DIGITS):
    """-> G as an n x n object array of mpf (use it under mp.workdps(digits))"""
    Ul, Dl, Tl, Ur, Dr, Tr = (_to_mp(a) for a in args)
    n = Ul.shape[0]
    with mp.workdps(digits):
        L = (Ul * Dl[None, :]).dot(Tl)
        R = (Ur * Dr[None, :]).dot(Tr)
        A = L.dot(R.T)
        for i in range(n):
            A[i, i] += 1
        return _inverse_mp(A)


def to_float(a):
    return np.array([float(x) for x in np.asarray(a).reshape(-1)]).reshape(np.shape(a))


def probe_matrix(n, seed):
    rng = np.random.Generator(np.random.Philox(key=[seed, 0x9e3779b9]))
    return (2.0 * rng.integers(0, 2, size=(n, PROBE_COLUMNS)) - 1.0)


def probe(G, V, digits=DIGITS):
    """-> (G V, G' V): np.longdouble arrays from a float64 G, object arrays of mpf from an mp G"""
    if np.asarray(G).dtype == object:
        with mp.workdps(digits):
            Vm = _to_mp(V)
            return G.dot(Vm), G.T.dot(Vm)
    Gl, Vl = np.asarray(G, dtype=np.longdouble), np.asarray(V, dtype=np.longdouble)
    return Gl @ Vl, Gl.T @ Vl


def rel(x, ref):
    x, ref = np.asarray(x, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def probe_err(G, V, ref_probes):
    """the larger of max |G V - ref| / max |ref| and the same for G' V; G float64, ref the stored float64 probes"""
    a, b = probe(G, V)
    return max(rel(a, ref_probes[0]), rel(b, ref_probes[1]))


def diag_err(G, ref_diag):
    return rel(np.diag(G), ref_diag)


def full_err(G, Gmp, digits=DIGITS):
    """relerr(G, G_mp) = max |G - G_mp| / max |G_mp| over every entry, the differences taken in mpmath"""
    with mp.workdps(digits):
        Gm = _to_mp(G)
        return float(max(abs(x) for x in (Gm - Gmp).reshape(-1)) / max(abs(x) for x in Gmp.reshape(-1)))


def oracle_greens(O, args, presort):
    """the float64 oracle's G under the reference's pivot rule (presort = 0) or the pre-sorted one (a site mask)"""
    O.lib().orc_set_udt_presort(presort)
    try:
        return np.array(O.calculate_greens(*args))
    finally:
        O.lib().orc_set_udt_presort(0)


def straddles_one(D):
    """at least a quarter of D below 1 and a quarter above: the scales a stack holds at low temperature"""
    n = len(D)
    return (np.asarray(D) < 1).sum() >= n / 4 and (np.asarray(D) > 1).sum() >= n / 4
