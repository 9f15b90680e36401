"""The q-state engine's definition away from ferromagnetic Potts and clock tables at J = 1, on the host, no GPU:
antiferromagnetic coupling (e_q30[0] the smallest entry), a signed table that is not monotone in |d|, and the inclusive
table limit |e_q30| = 2^32.  The exact transition matrices of the defined sweep, cluster move and exchange try
(tests/qstate_ref.py, tests/qstate_cluster_ref.py, tests/qstate_tempering_ref.py) leave the Boltzmann weight invariant
under these tables too, the antiferromagnetic Potts cluster grows through bonds of unequal states, and the restatement
follows the enumeration.  tests/test_gpu_qstate_models.py compares the device with the same restatements."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_cluster_ref as cref  # noqa: E402
import qstate_tempering_ref as tref  # noqa: E402

GENERIC6 = [1.0, -0.5, 0.25, -1.0, 0.25, -0.5]  # signed, not monotone in |d|, symmetric

# name -> (q, table, J, beta); the cluster and exchange matrices use Chain(n_chain), the sweep also SquareLattice(2)
MODELS = {
    "afpotts3_Jm1": (3, ref.potts_table(3), -1.0, 0.9, 4),
    "clock4_Jm075": (4, ref.clock_table(4), -0.75, 0.8, 3),
    "generic6_J1": (6, GENERIC6, 1.0, 0.7, 3),
    "generic6_Jm2": (6, GENERIC6, -2.0, 0.45, 3),
    "clock5_J4": (5, ref.clock_table(5), 4.0, 0.2, 3),
}


def _boltzmann(l, q, e_q30, st, beta):
    E = ref.state_energies_q30(l, q, e_q30, st) / 2.0 ** 30
    pi = np.exp(-beta * (E - E.min()))
    return pi / pi.sum()


def test_the_tables_of_these_models(mc_amd):
    """antiferromagnetic coupling makes e_q30[0] the smallest entry, J = 4 puts it on the inclusive limit 2^32, and the
    signed table is monotone in neither direction; the package's tables are the restatement's"""
    for name, (q, table, J, beta, n) in MODELS.items():
        model = mc_amd.QStateModel(q, table, dims=1, L=4, J=J)
        e = ref.tables(q, table, J)[0]
        assert np.array_equal(model.e_q30, e), name
        assert all(e[d] == e[(q - d) % q] for d in range(q))
    assert ref.tables(5, ref.clock_table(5), 4.0)[0][0] == 2 ** 32
    assert ref.tables(7, ref.clock_table(7), 4.0)[0][0] == 2 ** 32
    af = ref.tables(3, ref.potts_table(3), -1.0)[0]
    assert af[0] == -2 ** 30 == af.min() and np.all(af[1:] == 0)
    g = ref.tables(6, GENERIC6, 1.0)[0][:4]
    assert not np.all(np.diff(g) <= 0) and not np.all(np.diff(g) >= 0) and g.min() < 0 < g.max()
    with pytest.raises(ValueError, match="at most 4"):
        mc_amd.ClockModel(5, dims=1, L=4, J=4.0000001)


@pytest.mark.parametrize("name,lattice", [(name, "chain") for name in MODELS] +
                         [("afpotts3_Jm1", "square2"), ("clock4_Jm075", "square2")])
def test_the_sweep_leaves_the_boltzmann_weight_invariant(mc_amd, name, lattice):
    """pi P = pi for the exact matrix of one sweep to 1e-12, the bound of test_qstate_host.py; SquareLattice(2) (every
    neighbour twice) for the tables with q <= 4, whose q^4 states the enumeration handles"""
    q, table, J, beta, n = MODELS[name]
    l =mc_amd.Chain(n) if lattice == "chain" else mc_amd.SquareLattice(2)
    e_q30 = ref.tables(q, table, J)[0]
    P, st = ref.sweep_matrix(l, q, e_q30, beta)
    assert np.allclose(P.sum(axis=1), 1.0, atol=1e-14) and P.min() >= 0.0
    pi = _boltzmann(l, q, e_q30, st, beta)
    resid = np.abs(pi @ P - pi).max()
    print(name, lattice, "states", len(st), "max |pi P - pi| =", resid)
    assert resid <= 1e-12
    other = _boltzmann(l, q, e_q30, st, 1.5 * beta)  # not vacuous: another temperature's weight is not preserved
    assert np.abs(other @ P - other).max() > 1e-4


@pytest.mark.parametrize("name", list(MODELS))
def test_the_cluster_move_leaves_the_boltzmann_weight_invariant_and_is_reversible(mc_amd, name):
    """pi P = pi and pi_a P_ab = pi_b P_ba for the exact matrix of one move, both to 1e-12, the bound of
    test_qstate_cluster_host.py; every move changes the configuration"""
    q, table, J, beta, n = MODELS[name]
    l = mc_amd.Chain(n)
    e_q30 = ref.tables(q, table, J)[0]
    P, st = cref.cluster_matrix(l, q, e_q30, beta)
    assert np.allclose(P.sum(axis=1), 1.0, atol=1e-14) and P.min() >= 0.0
    pi = _boltzmann(l, q, e_q30, st, beta)
    resid = np.abs(pi @ P - pi).max()
    flow = pi[:, None] * P
    db = np.abs(flow - flow.T).max()
    print(name, "states", len(st), "max |pi P - pi| =", resid, "max |pi_a P_ab - pi_b P_ba| =", db)
    assert resid <= 1e-12
    assert db <= 1e-12
    assert np.trace(P) == 0.0
    other = _boltzmann(l, q, e_q30, st, 1.5 * beta)
    assert np.abs(other @ P - other).max() > 1e-4


@pytest.mark.parametrize("name", list(MODELS))
def test_exchange_detailed_balance_to_the_stated_accuracy(mc_amd, name):
    """A(i, j) pi(i, j) = A(j, i) pi(j, i) for the restated acceptance of one try, to the header's (2 J + 4) 2^-53
    max(1, |db d|), as test_qstate_tempering_host.py asks of Potts and clock tables"""
    q, table, Jc, beta, n = MODELS[name]
    l = mc_amd.Chain(n)
    e_q30 = ref.tables(q, table, Jc)[0]
    E = ref.state_energies_q30(l, q, e_q30, ref.all_states(n, q))
    J = tref.exchange_bits(len(l.bonds), e_q30)
    decided = 0
    for beta_a, beta_b in ((beta, 1.4 * beta), (1.4 * beta, beta), (beta, beta * 1.0000001)):
        A = tref.exchange_matrix(E, beta_a, beta_b, J)
        db = beta_a - beta_b
        bound = (2 * J + 4) * 2.0 ** -53
        levels = np.unique(E)
        for Ei in levels:
            for Ej in levels:
                i, j = int(np.flatnonzero(E == Ei)[0]), int(np.flatnonzero(E == Ej)[0])
                x = db * (int(Ei) - int(Ej)) / 2.0 ** 30
                dev = abs(A[i, j] / (A[j, i] * math.exp(x)) - 1.0)
                decided += A[i, j] < 1.0
                assert dev <= bound * max(1.0, abs(x)), (name, beta_a, beta_b, Ei, Ej, dev)
        assert np.all(A <= 1.0) and np.all(A > 0.0)
    assert decided > 0


def test_for_antiferromagnetic_potts_models_the_cluster_grows_through_unequal_bonds(mc_amd):
    """the J < 0 mirror of test_for_potts_models_it_is_the_wolff_move: with e_q30 = (-2^30, 0, ..) a slot is active only
    where the states differ (a != 0) and the reflection would make them equal (b == 0), so every cluster is connected
    through bonds whose ends were unequal before the move, holds two states which the move exchanges, and the one bond
    probability in use is fl(1 - exp(fl(-beta 1)))"""
    l, q, beta, W = mc_amd.SquareLattice(6), 3, 0.9, 16
    wk = cref.ClusterWalkers(l, q, ref.potts_table(q), [beta] * W, range(50, 50 + W), J=-1.0)
    w = ref.weights(wk.e_q30, beta)
    p = 1.0 - math.exp(-beta * 1.0)
    assert all(1.0 - w[a, 0] == p for a in range(1, q))                  # the slots that can be active
    assert all(wk.e_q30[a] <= wk.e_q30[b] for a in range(q) for b in range(1, q))  # no other slot ever is
    assert all(wk.e_q30[0] <= wk.e_q30[b] for b in range(q))
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    sizes = []
    for _ in range(10):
        wk.sweep()
        wk.cluster_move()
        for x in range(W):
            inC, before, after = wk.last["in_cluster"][x], wk.last["before"][x], wk.c[x]
            r = int(wk.last["r"][x])
            assert np.array_equal(before[~inC], after[~inC])
            assert np.array_equal(after[inC], (r - before[inC]) % q)
            old = set(before[inC].tolist())
            assert len(old) <= 2 and {(r - s) % q for s in old} == set(after[inC].tolist())
            members = np.flatnonzero(inC)
            seen, todo = {int(members[0])}, [int(members[0])]
            while todo:  # the component of one member over bonds inside C with unequal ends
                i = todo.pop()
                for j in nb[:, i]:
                    j = int(j)
                    if inC[j] and j not in seen and before[i] != before[j]:
                        seen.add(j)
                        todo.append(j)
            assert seen == set(members.tolist()), (x, sorted(seen), members)
            if len(members) > 1:
                assert len(old) == 2 and sum(old) % q == r
            sizes.append(len(members))
    assert max(sizes) > 2 and min(sizes) >= 1
    assert wk.sum_cluster_size.sum() == sum(sizes) and np.all(wk.prop_global == 10) and np.all(wk.m == 10)
    E, Mx, My = wk.E.copy(), wk.Mx.copy(), wk.My.copy()
    wk.observables()
    assert np.array_equal(E, wk.E) and np.array_equal(Mx, wk.Mx) and np.array_equal(My, wk.My)


def test_the_bond_counts_behind_the_exchange_bits_at_the_limit(mc_amd):
    """tests/qs_exchange_check.cpp puts |e_q30| = 2^32 on 324 and 80 bonds: the bond counts of CubicLattice(4, 3) and
    BilayerSquareLattice(4); the restated J is 42 and 40 there (test_qs_exchange_host.py holds mc_tables.h to them)"""
    cubic, bilayer = mc_amd.CubicLattice(4, 3), mc_amd.BilayerSquareLattice(4)
    assert (len(cubic), len(cubic.bonds), np.asarray(cubic.neighs).shape[0]) == (81, 324, 8)
    assert (len(bilayer), len(bilayer.bonds), np.asarray(bilayer.neighs).shape[0]) == (32, 80, 5)
    assert tref.exchange_bits(len(cubic.bonds), ref.tables(7, ref.clock_table(7), 4.0)[0]) == 42
    assert tref.exchange_bits(len(bilayer.bonds), ref.tables(3, ref.potts_table(3), -4.0)[0]) == 40
    assert tref.exchange_bits(len(cubic.bonds), ref.tables(3, ref.potts_table(3), -4.0)[0]) == 42
    # the local rule's dE_int of one site reaches z (max - min) = 8 2^33 = 2^36 there, inside int64 by far
    assert 8 * (2 ** 32 - (-2 ** 32)) == 2 ** 36
