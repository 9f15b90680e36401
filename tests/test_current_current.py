"""current_current_susceptibility (measurements.jl:257-317) on the host side: EachLocalQuadBySyncedDistance against
a literal restatement of the reference's construction and iteration (lattice_iterators.jl:390-464), and the numpy
restatement of cc_kernel (tests/cc_reference.py) against exact diagonalisation at U = 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_reference as CC  # noqa: E402


def _reference_synced(pairs_by_dir, n, K):
    """EachLocalQuadBySyncedDistance{K}(lattice) and Base.iterate, statement by statement (1-based as in Julia)"""
    trg_from_src = [[] for _ in range(n)]
    for dir_ in range(1, K + 1):
        for src, trg in pairs_by_dir.pairs[dir_ - 1]:
            trg_from_src[src - 1].append((dir_, trg))
    npairs = len(pairs_by_dir.pairs)
    implied = {(a, b): [] for a in range(1, npairs + 1) for b in range(1, K + 1)}
    dir12, idx, i, j = 1, 1, 1, 1
    while True:
        if dir12 <= npairs:
            if idx <= len(pairs_by_dir.pairs[dir12 - 1]):
                src1, src2 = pairs_by_dir.pairs[dir12 - 1][idx - 1]
                if i <= len(trg_from_src[src1 - 1]):
                    dir1, trg1 = trg_from_src[src1 - 1][i - 1]
                    if j <= len(trg_from_src[src2 - 1]):
                        dir2, trg2 = trg_from_src[src2 - 1][j - 1]
                        j += 1
                        if dir1 != dir2:
                            continue
                        implied[(dir12, dir1)].append((src1, trg1, src2, trg2))
                    else:
                        i += 1
                        j = 1
                else:
                    idx += 1
                    i = j = 1
            else:
                dir12 += 1
                idx = i = j = 1
        else:
            break
    total = sum(len(x) for x in implied.values())
    # column-major linear order of the (npairs, K) array `implied`
    flat = [implied[(1 + (q % npairs), 1 + (q // npairs))] for q in range(npairs * K)]
    out = []
    state = (1, 1)
    while True:  # Base.iterate(iter, state)
        i, j = state
        if i <= len(flat):
            N = len(flat[i - 1])
            j = 1 if N == 0 else j
            done = False
            while N == 0:
                i += 1
                if i > len(flat):
                    done = True
                    break
                N = len(flat[i - 1])
            if done:
                break
            next_j = (j + 1 - 1) % N + 1  # mod1(j+1, N)
            next_i = i + j // N
            t = flat[i - 1][j - 1]
            out.append((i,) + tuple(t))
            state = (next_i, next_j)
        else:
            break
    return out, (npairs, K), total


@pytest.mark.parametrize("kind,size,K", [("square", 2, 1), ("square", 2, 4), ("square", 4, 1), ("square", 4, 5),
                                         ("chain", 6, 1), ("chain", 6, 3)])
def test_synced_iterator_against_reference(mc_amd, kind, size, K):
    lat = mc_amd.SquareLattice(size) if kind == "square" else mc_amd.Chain(size)
    it = mc_amd.EachLocalQuadBySyncedDistance(lat, K)
    ref, nd, total = _reference_synced(it.pairs_by_dir, len(lat), K)
    got = list(it)
    assert got == ref
    assert it.ndirections() == nd
    assert len(it) == total == len(ref)
    # the target table the device gets is the one the iterator uses
    for lin, s1, t1, s2, t2 in got:
        k = (lin - 1) // nd[0]
        assert it.trg_of[s1 - 1, k] == t1 - 1 and it.trg_of[s2 - 1, k] == t2 - 1


def test_synced_iterator_default_K_and_limits(mc_amd):
    assert mc_amd.EachLocalQuadBySyncedDistance(mc_amd.SquareLattice(4)).K == 5
    assert mc_amd.EachLocalQuadBySyncedDistance(mc_amd.Chain(6)).K == 3
    with pytest.raises(ValueError):
        mc_amd.EachLocalQuadBySyncedDistance(mc_amd.SquareLattice(2))  # default K = 5 > 4 directions
    with pytest.raises(ValueError):
        mc_amd.EachLocalQuadBySyncedDistance(mc_amd.Chain(6), 7)


def test_attractive_override_equals_generic_on_doubled_G():
    rng = np.random.default_rng(3)
    N = 5
    pg1 = tuple(rng.standard_normal((N, N)) for _ in range(4))
    T1 = rng.standard_normal((N, N))
    pg2 = tuple(CC.blockdiag([g]) for g in pg1)
    T2 = CC.blockdiag([T1])
    for s1, t1, s2, t2 in [(0, 1, 2, 3), (4, 4, 1, 0), (2, 3, 2, 3), (1, 0, 3, 2)]:
        a = CC.cc_kernel_attractive(pg1, T1, s1, t1, s2, t2)
        g = CC.cc_kernel(pg2, T2, N, s1, t1, s2, t2)
        assert abs(a - g) < 1e-12 * max(1.0, abs(g))


@pytest.mark.parametrize("attractive", [False, True])
def test_vectorised_sum_matches_quad_by_quad(mc_amd, attractive):
    rng = np.random.default_rng(7)
    it = mc_amd.EachLocalQuadBySyncedDistance(mc_amd.SquareLattice(4), 5)
    N, nb = 16, 1 if attractive else 2
    T = [rng.standard_normal((N, N)) for _ in range(nb)]
    g00 = [rng.standard_normal((N, N)) for _ in range(nb)]
    steps = [tuple([rng.standard_normal((N, N)) for _ in range(nb)] for _ in range(3)) for _ in range(2)]
    got = CC.current_current_susceptibility(g00, steps, T, it, attractive, 0.1)
    nd = it.ndirections()[0]
    flat = np.zeros(nd * 5)
    for g0l, gl0, gll in steps:
        for lin, s1, t1, s2, t2 in it:
            if attractive:
                v = CC.cc_kernel_attractive((g00[0], g0l[0], gl0[0], gll[0]), T[0], s1 - 1, t1 - 1, s2 - 1, t2 - 1)
            else:
                pg = tuple(CC.blockdiag(x) for x in (g00, g0l, gl0, gll))
                v = CC.cc_kernel(pg, CC.blockdiag(T), N, s1 - 1, t1 - 1, s2 - 1, t2 - 1)
            flat[lin - 1] += v
    ref = flat.reshape((nd, 5), order="F") * 0.1 / N
    assert np.abs(got - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


def test_cc_kernel_against_ed(mc_amd, O, R):
    """U = 0: Wick's theorem is exact, so <J1(tau) J2(0)> = tr(rho e^{tau H} J1 e^{-tau H} J2) from exact
    diagonalisation, J = sum_sigma (T[trg,src] c^dag_trg c_src - T[src,trg] c^dag_src c_trg) (test/ED/ED.jl:403-434),
    equals cc_kernel on the oracle's packed Green's functions for every synced quad (2x2 lattice, K = 4)."""
    from oracle import unequal_time_oracle as UT
    L, N, beta, dtau = 2, 4, 1.0, 0.1
    mc = O.OracleDQMC(L, "repulsive", beta=beta, delta_tau=dtau, safe_mult=5, U=0.0)
    mc.set_conf(O.random_conf(4, N, mc.slices)); mc.seed(4)
    mc.prepare()
    ut = [UT.UnequalTimeOracle(mc, b) for b in range(2)]
    neighs = O.square_neighs(L)
    rho, c, cd = R.ed_hubbard_greens(neighs, N, 0.0, 1.0, 0.0, beta, return_state=True)
    T1 = np.zeros((N, N))
    H = np.zeros_like(rho)
    for src in range(N):
        for trg in neighs[:, src] - 1:
            T1[trg, src] -= 1.0
            for s_ in range(2):
                H -= cd[N * s_ + trg] @ c[N * s_ + src]
    T = CC.blockdiag([T1, T1])
    w, V = np.linalg.eigh(H)

    def heis(A, tau):
        return (V * np.exp(tau * w)) @ V.T @ A @ (V * np.exp(-tau * w)) @ V.T

    def J(src, trg):
        out = np.zeros_like(rho)
        for s_ in range(2):
            a, b = N * s_ + src, N * s_ + trg
            out += T[b, a] * cd[b] @ c[a] - T[a, b] * cd[a] @ c[b]
        return out

    it = mc_amd.EachLocalQuadBySyncedDistance(mc_amd.SquareLattice(L), 4)
    quads = {(s1 - 1, t1 - 1, s2 - 1, t2 - 1) for _, s1, t1, s2, t2 in it}
    assert len(quads) == len(it)
    G00 = R.full_greens([ut[b].greens(0, 0) for b in range(2)])
    for l in (1, 3, 7, 10):
        tau = l * dtau
        pg = (G00,) + tuple(R.full_greens([ut[b].greens(*ix) for b in range(2)]) for ix in ((0, l), (l, 0), (l, l)))
        for s1, t1, s2, t2 in quads:
            ed = np.trace(rho @ heis(J(s1, t1), tau) @ J(s2, t2))
            assert abs(CC.cc_kernel(pg, T, N, s1, t1, s2, t2) - ed) < 1e-10, (l, s1, t1, s2, t2)
