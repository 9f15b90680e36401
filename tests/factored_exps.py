"""Seeded hopping exponentials in factored form that no physical lattice gives: the inputs of test_factored_exps_host.py
and test_gpu_factored_generic.py.

The factored kernels (kron.hip, rect.hip, kron3.hip, bilayer.hip, tri.hip, ttp.hip) have only ever been given exp(-+dtau h)
of translation-invariant rings: symmetric, circulant, and equal in both spin blocks.  A factor set used in the place of
its transpose, an operand index reversed or rotated, or a block offset left out reads equal numbers from such input.
Here every factor is the exponential of its own one-dimensional generator

    H[i, i+1] = -a_i,  H[i+1, i] = -b_i  (indices mod m),  H[i, i] = d_i,   a, b in (0.6, 1.4), d in (-0.5, 0.5)

with a, b and d drawn independently (`symmetric=True`: b = a, the factors are symmetric and still not circulant), and the
four matrices are Kronecker products of the axis exponentials for s = -1/2, +1/2, -1, +1, each formed from its own
scipy.linalg.expm (eT2 is not eT squared):

    eT, eTinv, eT2, eTinv2 = kron(expm(s dtau H_z), expm(s dtau H_y), expm(s dtau H_x)),   site x + mx (y + my z)

The sign of the bonds is that of a hopping matrix, so the exponentials are positive like the physical ones.

tri.hip and ttp.hip apply (Fy (x) Fx) Ed [Ea] and need commuting parts, so their factors stay circulant; `generic=False`
makes them asymmetric instead: a ring with amplitude tR on the shift by +1 and tL != tR on the shift by -1, per axis and
per diagonal direction."""
import numpy as np
from scipy.linalg import expm

POWERS = (-0.5, 0.5, -1.0, 1.0)  # eT, eTinv, eT2, eTinv2


def ring_generator(m, rng, symmetric=False):
    """the generic generator above on a ring of m sites (m = 2: both bonds join the same two sites and add up)"""
    a = rng.uniform(0.6, 1.4, m)
    b = a if symmetric else rng.uniform(0.6, 1.4, m)
    H = np.diag(rng.uniform(-0.5, 0.5, m))
    for i in range(m):
        j = (i + 1) % m
        H[i, j] -= a[i]
        H[j, i] -= b[i]
    return H


def generators(dims, seed, symmetric=False):
    """one generator per axis, x first"""
    rng = np.random.default_rng(seed)
    return [ring_generator(m, rng, symmetric) for m in dims]


def axis_exponentials(gens, delta_tau):
    """[power][axis] -> expm(s dtau H_axis)"""
    return [[expm(s * delta_tau * H) for H in gens] for s in POWERS]


def factored_exps(dims, gens, delta_tau):
    """(eT, eTinv, eT2, eTinv2) of one block: each the Kronecker product of its own axis exponentials, the last axis
    outermost"""
    assert [H.shape for H in gens] == [(m, m) for m in dims]
    out = []
    for fs in axis_exponentials(gens, delta_tau):
        E = fs[0]
        for f in fs[1:]:
            E = np.kron(f, E)
        out.append(E)
    return tuple(out)


def blocks(dims, seeds, delta_tau, symmetric=False, generic=True, scales=None):
    """one four-tuple per seed (a different seed for each spin block gives blocks that differ), and the factor array of
    the commuting forms or None.  generic=True: Kronecker products over `dims` of the generic generators.  generic=False:
    the asymmetric circulant mode below, `dims` = (16, 16) and 3 or 4 commuting parts given by len(scales)"""
    if generic:
        return [factored_exps(dims, generators(dims, s, symmetric), delta_tau) for s in seeds], None
    assert tuple(dims) == (L, L) and not symmetric
    return commuting_blocks(len(scales), seeds, delta_tau, scales)


# ---- the commuting forms of tri.hip / ttp.hip: asymmetric circulant factors
L = 16


def _diagonal_operator(F, sign):
    """Ed (sign = -1): (Ed v)(x, y) = sum_y' F[y, y'] v(x - y + y', y'); Ea (sign = +1): v(x + y - y', y'); site x + 16 y"""
    E = np.zeros((L * L, L * L))
    for y in range(L):
        for y2 in range(L):
            for x in range(L):
                x2 = (x + sign * (y - y2)) % L
                E[x + L * y, x2 + L * y2] = F[y, y2]
    return E


def circulant_generators(n_parts, seed, scales=None):
    """n_parts ring generators H = -(tR S + tL S') with S the shift by +1, tR = scale (1.3 +- 0.2), tL = scale (0.7 +- 0.2);
    the first one carries a constant diagonal in (-0.5, 0.5) (the place of mu)"""
    rng = np.random.default_rng(seed)
    S = np.roll(np.eye(L), 1, axis=0)
    scales = scales or (1.0,) * n_parts
    gens = []
    for k in range(n_parts):
        tR, tL = scales[k] * rng.uniform(1.1, 1.5), scales[k] * rng.uniform(0.5, 0.9)
        gens.append(-(tR * S + tL * S.T))
    gens[0] = gens[0] + rng.uniform(-0.5, 0.5) * np.eye(L)
    return gens


def commuting_exps(gens, delta_tau):
    """gens = [Hx, Hy, Hd] (triangular) or [Hx, Hy, Hd, Ha] (t-t'): returns (eT, eTinv, eT2, eTinv2), each the dense
    product (Fy (x) Fx) Ed(Fd) [Ea(Fa)] of its own exponentials, and the factor array of one block in the layout of
    triangular_factors / square_tp_factors: [eT2: Fx Fy Fd (Fa)][eTinv2: Fx Fy Fd (Fa)], each 16 x 16 column-major"""
    dense, per_power = [], []
    for fs in axis_exponentials(gens, delta_tau):
        E = np.kron(fs[1], fs[0]) @ _diagonal_operator(fs[2], -1)
        if len(fs) == 4:
            E = E @ _diagonal_operator(fs[3], +1)
        dense.append(E)
        per_power.append(np.concatenate([f.reshape(-1, order="F") for f in fs]))
    return tuple(dense), np.concatenate([per_power[2], per_power[3]])


def commuting_blocks(n_parts, seeds, delta_tau, scales=None):
    """per seed (one per spin block) the four dense matrices, and the blocks' factor arrays concatenated"""
    res = [commuting_exps(circulant_generators(n_parts, s, scales), delta_tau) for s in seeds]
    return [r[0] for r in res], np.ascontiguousarray(np.concatenate([r[1] for r in res]))


# ---- the families the GPU tests run
DELTA_TAU = 0.1
FAMILIES = {
    "square16": (16, 16),
    "rect32x8": (32, 8),
    "cubic8": (8, 8, 8),
    "bilayer16": (16, 16, 2),
    "tri16": (16, 16),
    "ttp16": (16, 16),
}
KRONECKER = ("square16", "rect32x8", "cubic8", "bilayer16")
SCALES = {"tri16": (1.0, 1.0, 1.0), "ttp16": (1.0, 1.0, 0.3, 0.3)}  # (the diagonal hops of a t-t' model are the weaker ones)
# attractive: one block; repulsive: another seed per block; symmetric: b = a, one block (Kronecker families only).  The
# seeds are ones at which the two-layer form's 2 x 2 half-step factor, too, is 1e-2 away from circulant (three numbers
# decide that) and the half-step matrices of the two blocks of the commuting forms differ by 1e-2 (seven or nine numbers);
# the host test asserts both for every case
CASES = {"attractive": (12,), "repulsive": (16, 30), "symmetric": (28,)}
ALL_CASES = [(f, c) for f in FAMILIES for c in CASES if f in KRONECKER or c != "symmetric"]


def case_inputs(family, case):
    """(list of per-block four-tuples, factor array or None) of one GPU case, seeded by family and case"""
    seeds = [1000 * (1 + list(FAMILIES).index(family)) + s for s in CASES[case]]
    if family in KRONECKER:
        return blocks(FAMILIES[family], seeds, DELTA_TAU, symmetric=case == "symmetric")
    return blocks(FAMILIES[family], seeds, DELTA_TAU, generic=False, scales=SCALES[family])
