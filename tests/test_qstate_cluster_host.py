"""The reflection cluster move of the q-state (Potts, clock) engine on the host, no GPU: the exact transition matrix of the
defined move leaves the Boltzmann weight invariant and satisfies detailed balance, the Potts case is the Wolff move, the
restatement's running E, Mx, My stay those of the configuration, sweeps with a move each reproduce the enumeration, and the
interface refuses what it should before any device is touched."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_cluster_ref as cref  # noqa: E402

GENERIC5 = [0.3, 1.0, -0.5, -0.5, 1.0]
CASES = {"chain4_potts3": (lambda g: g.Chain(4), 3, ref.potts_table(3), 0.9),
         "chain3_clock4": (lambda g: g.Chain(3), 4, ref.clock_table(4), 0.8),
         "chain3_generic5": (lambda g: g.Chain(3), 5, GENERIC5, 0.6),
         "chain2_q2": (lambda g: g.Chain(2), 2, ref.potts_table(2), 0.7)}  # both neighbours of a site are the other site


@pytest.mark.parametrize("case", list(CASES))
def test_the_move_leaves_the_boltzmann_weight_invariant_and_is_reversible(mc_amd, case):
    """pi P = pi and pi_a P_ab = pi_b P_ba for the exact matrix of one move, summed over the seed, the reflection and all
    subsets of the slots with non-zero probability p = fl(1 - w[a][b]), pi the Boltzmann weight of E_int 2^-30; both to
    1e-12 (the table entries carry a few ulp).  Every move changes the configuration: trace P == 0.  Observed residuals
    (max |pi P - pi|, max |pi_a P_ab - pi_b P_ba|): chain4_potts3 1.9e-16, 1.3e-18; chain3_clock4 2.8e-17, 4.3e-19;
    chain3_generic5 6.9e-18, 3.3e-19; chain2_q2 5.6e-17, 6.9e-18."""
    make, q, table, beta = CASES[case]
    l = make(mc_amd)
    e_q30 = ref.tables(q, table)[0]
    P, st = cref.cluster_matrix(l, q, e_q30, beta)
    assert np.allclose(P.sum(axis=1), 1.0, atol=1e-14) and P.min() >= 0.0
    E = ref.state_energies_q30(l, q, e_q30, st) / 2.0 ** 30
    pi = np.exp(-beta * (E - E.min()))
    pi /= pi.sum()
    resid = np.abs(pi @ P - pi).max()
    flow = pi[:, None] * P
    db = np.abs(flow - flow.T).max()
    print(case, "states", len(st), "max |pi P - pi| =", resid, "max |pi_a P_ab - pi_b P_ba| =", db)
    assert resid <= 1e-12
    assert db <= 1e-12
    assert np.trace(P) == 0.0
    # not vacuous: the same matrix does not preserve the weight of another temperature
    other = np.exp(-1.5 * beta * (E - E.min()))
    other /= other.sum()
    assert np.abs(other @ P - other).max() > 1e-4


def test_the_matrix_is_the_move_the_restatement_makes(mc_amd):
    """4000 walkers of ClusterWalkers from one state of Chain(4), q = 3, follow the matrix row (chi-square over its
    support, 5 sigma) and land nowhere else"""
    l, q, beta = mc_amd.Chain(4), 3, 0.9
    P, st = cref.cluster_matrix(l, q, ref.tables(q, ref.potts_table(q))[0], beta)
    W, start = 4000, 3  # (0, 1, 0, 0): sites 2, 3, 0 form a run of equal states on the ring
    wk = cref.ClusterWalkers(l, q, ref.potts_table(q), [beta] * W, range(2000, 2000 + W), rand=False)
    wk.c[:] = st[start]
    wk.observables()
    wk.cluster_move()
    counts = np.bincount((wk.c * 3 ** np.arange(4)).sum(axis=1), minlength=81)
    assert np.all(P[start][counts > 0] > 0)
    sup = P[start] > 0
    chi2 = ((counts[sup] - W * P[start][sup]) ** 2 / (W * P[start][sup])).sum()
    dof = sup.sum() - 1
    assert dof >= 3 and abs(chi2 - dof) <= 5.0 * math.sqrt(2.0 * dof), (chi2, dof)


def test_for_potts_models_it_is_the_wolff_move(mc_amd):
    """every cluster site had the seed's state, all of them end in one other state, the cluster is connected through
    bonds of equal states, and the one bond probability in use is fl(1 - exp(fl(-beta 1)))"""
    l, q, beta, W = mc_amd.SquareLattice(6), 3, 0.9, 16
    wk = cref.ClusterWalkers(l, q, ref.potts_table(q), [beta] * W, range(50, 50 + W))
    w = ref.weights(wk.e_q30, beta)
    p = 1.0 - math.exp(-beta * 1.0)
    assert all(1.0 - w[0, b] == p for b in range(1, q))                 # the slots that can be active
    assert all(wk.e_q30[a] <= wk.e_q30[b] for a in range(1, q) for b in range(q))  # no other slot ever is
    sizes = []
    for _ in range(10):
        wk.sweep()
        wk.cluster_move()
        for x in range(W):
            inC, before, after = wk.last["in_cluster"][x], wk.last["before"][x], wk.c[x]
            old, new = set(before[inC].tolist()), set(after[inC].tolist())
            assert len(old) == 1 and len(new) == 1 and old != new
            assert np.array_equal(before[~inC], after[~inC])
            sizes.append(int(inC.sum()))
    assert max(sizes) > 1 and min(sizes) >= 1
    assert wk.sum_cluster_size.sum() == sum(sizes) and np.all(wk.prop_global == 10) and np.all(wk.m == 10)


@pytest.mark.parametrize("shape", ["square5", "cubic3", "chain5", "honeycomb3"])
def test_running_sums_are_those_of_the_configuration(mc_amd, shape):
    """after 20 moves (a sweep between them) the running E_int, Mx, My equal observables() from scratch"""
    l = {"square5": lambda: mc_amd.SquareLattice(5), "cubic3": lambda: mc_amd.CubicLattice(3, 3),
         "chain5": lambda: mc_amd.Chain(5), "honeycomb3": lambda: mc_amd.HoneycombLattice(3)}[shape]()
    for q, table, beta in ((3, ref.potts_table(3), 0.9), (6, ref.clock_table(6), 1.1), (5, GENERIC5, 0.7)):
        wk = cref.ClusterWalkers(l, q, table, [0.6 * beta, beta, 1.5 * beta], [11, 12, 13])
        for _ in range(20):
            wk.cluster_move()
            wk.sweep()
        assert wk.sum_cluster_size.sum() > 3 * 20  # some clusters had more than one site
        E, Mx, My = wk.E.copy(), wk.Mx.copy(), wk.My.copy()
        wk.observables()
        assert np.array_equal(E, wk.E) and np.array_equal(Mx, wk.Mx) and np.array_equal(My, wk.My), (shape, q)


def test_on_the_triangular_lattice_e_is_the_start_plus_neighbour_differences(mc_amd):
    """TriangularLattice's bonds table also lists two-step bonds: the running E is the bonds energy of the start plus the
    moves' dE_int over the neighs table, as the header says for the local rule; Mx, My are those of the configuration"""
    l = mc_amd.TriangularLattice(4)
    wk = cref.ClusterWalkers(l, 6, ref.clock_table(6), [0.3, 0.5], [21, 22])
    want = wk.E.copy()
    for _ in range(20):
        wk.cluster_move()
        want += wk.last_dE
    assert np.array_equal(wk.E, want) and np.any(wk.last_dE != 0)
    Mx, My = wk.Mx.copy(), wk.My.copy()
    wk.observables()
    assert np.array_equal(Mx, wk.Mx) and np.array_equal(My, wk.My)
    # and dE_int is the change of the energy over the directed neighs table, halved (every bond from both ends)
    nb = np.asarray(l.neighs, dtype=np.int64) - 1

    def e_neighs(c):
        return -int(wk.e_q30[(c[None, :] - c[nb]) % 6].sum())
    before = [e_neighs(wk.c[x]) for x in range(2)]
    wk.cluster_move()
    assert [e_neighs(wk.c[x]) - before[x] for x in range(2)] == (2 * wk.last_dE).tolist()


def test_sweeps_with_a_move_each_against_enumeration(mc_amd):
    """the configuration of qstate_ref.stat_run (Potts q = 3 on SquareLattice(3) at beta = ln(1 + sqrt 3), 64 walkers,
    200 + 3000 sweeps, seed 4242) with cluster_rate = 1: <E> and <M2> within 5 cross-walker standard errors of the
    enumeration.  Observed z-scores: E +0.49, M2 -0.65 (mean cluster size 0.81 N)."""
    l = mc_amd.SquareLattice(ref.STAT_L)
    wk = cref.ClusterWalkers(l, ref.STAT_Q, ref.potts_table(ref.STAT_Q), [ref.STAT_BETA] * ref.STAT_W,
                             [ref.STAT_SEED + w for w in range(ref.STAT_W)])
    wk.run(1, ref.STAT_THERM + ref.STAT_SWEEPS, ref.STAT_THERM, 1, cluster_rate=1)
    assert wk.n_meas == ref.STAT_SWEEPS and np.all(wk.prop_global == ref.STAT_THERM + ref.STAT_SWEEPS)
    z = ref.stat_zscores(wk.sum_E, wk.sum_M2, wk.n_meas, l)
    print("z-scores", z, "mean cluster size / N", wk.sum_cluster_size.sum() / wk.prop_global.sum() / len(l))
    assert abs(z["E"]) <= 5.0 and abs(z["M2"]) <= 5.0, z
    E, Mx, My = wk.E.copy(), wk.Mx.copy(), wk.My.copy()
    wk.observables()
    assert np.array_equal(E, wk.E) and np.array_equal(Mx, wk.Mx) and np.array_equal(My, wk.My)
    assert 0 < wk.acc_global.sum() < wk.prop_global.sum()


def test_rate_zero_is_the_plain_run_and_the_rate_places_the_moves(mc_amd):
    l = mc_amd.SquareLattice(4)
    args = (l, 4, ref.potts_table(4), [0.8, 1.1], [5, 6])
    plain, off, on = ref.Walkers(*args), cref.ClusterWalkers(*args), cref.ClusterWalkers(*args)
    plain.run(1, 7, 1, 2)
    off.run(1, 7, 1, 2, cluster_rate=0)
    on.run(1, 7, 1, 2, cluster_rate=3)
    assert plain.stats(0) == off.stats(0) and np.array_equal(plain.c, off.c) and np.all(off.m == 0)
    assert np.all(on.m == 2) and np.all(on.prop_global == 2) and np.all(on.s == 7)  # behind sweeps 3 and 6
    split = cref.ClusterWalkers(*args)
    split.run(1, 3, 1, 2, cluster_rate=3)
    split.run(4, 4, 1, 2, cluster_rate=3)
    assert np.array_equal(split.c, on.c) and split.stats(1) == on.stats(1) and split.cluster_stats(1) == on.cluster_stats(1)
    on.seed(1, 99)
    assert on.cluster_stats(1)["moves_drawn"] == 0 and on.cluster_stats(0)["moves_drawn"] == 2


# ---- the interface, before any device is touched
def test_cluster_rate_is_validated_on_the_host(mc_amd):
    m = mc_amd.PottsModel(3, dims=2, L=4)
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="cluster_rate"):
            mc_amd.MC(m, beta=1.0, cluster_rate=bad)
    with pytest.raises(TypeError):
        mc_amd.MC(mc_amd.IsingModel(dims=2, L=4), beta=0.4, cluster_rate=1)  # an IsingModel has cluster_moves=True
    with pytest.raises(NotImplementedError, match="IsingModel only") as ei:
        mc_amd.MC(m, beta=1.0, cluster_moves=True)
    assert "cluster_rate" in str(ei.value)


def test_the_header_declares_the_abi_and_the_library_refuses_null_handles(mc_amd):
    import ctypes as C
    from montecarlo_jl_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dqmc_hip.h")).read()
    for name in ("dqmc_qs_set_cluster_rate", "dqmc_qs_cluster_move", "dqmc_qs_get_cluster_stats"):
        assert "int %s(dqmc_qs_handle *h, int32_t" % name in src and name in _lib.SIGNATURES
    assert "} dqmc_qs_cluster_stats;" in src
    assert [f[0] for f in _lib.QsClusterStats._fields_] == ["prop_global", "acc_global", "sum_cluster_size", "moves_drawn"]
    assert C.sizeof(_lib.QsClusterStats) == 32
    lib = _lib.lib()
    assert lib.dqmc_qs_set_cluster_rate(None, 1) == _lib.ERR_INVALID
    assert lib.dqmc_qs_cluster_move(None, -1) == _lib.ERR_INVALID
    assert lib.dqmc_qs_get_cluster_stats(None, 0, None) == _lib.ERR_INVALID
