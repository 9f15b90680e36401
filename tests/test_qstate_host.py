"""The q-state (Potts, clock) models on the host, no GPU: the fixed-point tables, Potts q = 2 against the Ising model,
the invariance of the Boltzmann weight under the defined sweep (exact transition matrix), the restatement of
tests/qstate_ref.py against exact enumeration, and the errors that are raised before any device is touched."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402


# ---- tables
@pytest.mark.parametrize("q", [2, 3, 4, 5, 6, 8, 17, 64])
def test_tables(mc_amd, q):
    for model, table in ((mc_amd.PottsModel(q, dims=1, L=4), ref.potts_table(q)),
                         (mc_amd.ClockModel(q, dims=1, L=4, J=0.75), ref.clock_table(q))):
        e, c, s = model.e_q30, model.c_q30, model.s_q30
        assert e.dtype == np.int64 and c.dtype == np.int32 and s.dtype == np.int32
        assert all(e[d] == e[(q - d) % q] for d in range(q))
        want = ref.tables(q, table, model.J)
        assert np.array_equal(e, want[0]) and np.array_equal(c, want[1]) and np.array_equal(s, want[2])
        assert c[0] == 2 ** 30 and s[0] == 0 and np.all(np.abs(c) <= 2 ** 30) and np.all(np.abs(s) <= 2 ** 30)
        got = mc_amd.qstate_tables(q, table, model.J)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    potts = mc_amd.PottsModel(q, dims=1, L=4)
    assert potts.e_q30[0] == 2 ** 30 and np.all(potts.e_q30[1:] == 0)  # exactly {2^30, 0}
    if q == 2:
        assert list(potts.s_q30) == [0, 0] and list(potts.c_q30) == [2 ** 30, -2 ** 30]  # My = 0


# ---- Potts q = 2 is Ising
@pytest.mark.parametrize("L", [4, 3])
def test_potts_q2_is_ising(mc_amd, L):
    """E_potts = (E_ising - n_bonds) / 2 in units of J for every state of the L x L lattice (s = 0 <-> spin -1)"""
    l = mc_amd.SquareLattice(L)
    N, nb = len(l), len(l.bonds)
    potts, ising = mc_amd.PottsModel(2, l=l), mc_amd.IsingModel(l=l)
    st = ref.all_states(N, 2)
    b = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
    spins = 2 * st - 1
    E_ising = -(spins[:, b[:, 0]] * spins[:, b[:, 1]]).sum(axis=1)
    E_q30 = -potts.e_q30[(st[:, b[:, 0]] - st[:, b[:, 1]]) % 2].sum(axis=1)
    assert np.array_equal(2 * E_q30, (E_ising - nb) * 2 ** 30)  # all 2^N states, in the device's exact integers
    for a in range(0, len(st), 1 if L == 3 else 97):            # and through the models' own energy()
        assert ising.energy(spins[a]) == E_ising[a]
        assert potts.energy(st[a]) == (E_ising[a] - nb) / 2.0
        assert potts.energy_q30(st[a]) == E_q30[a]
    # propose_local is the energy difference of the single-site change, repeated neighbours included
    rng = np.random.default_rng(5)
    for _ in range(20):
        c = rng.integers(0, 2, N)
        i = int(rng.integers(1, N + 1))
        c2 = c.copy()
        c2[i - 1] ^= 1
        assert potts.propose_local(i, c2[i - 1], c) == potts.energy(c2) - potts.energy(c)


def test_propose_local_is_the_energy_difference(mc_amd):
    rng = np.random.default_rng(6)
    for model in (mc_amd.ClockModel(6, l=mc_amd.CubicLattice(3, 3)), mc_amd.PottsModel(3, l=mc_amd.SquareLattice(2)),
                  mc_amd.ClockModel(5, dims=1, L=5, J=1.5)):
        N, q = len(model), model.q
        for _ in range(20):
            c = rng.integers(0, q, N)
            i, t = int(rng.integers(1, N + 1)), int(rng.integers(0, q))
            c2 = c.copy()
            c2[i - 1] = t
            assert abs(model.propose_local(i, t, c) - (model.energy(c2) - model.energy(c))) < 1e-12
            # and the restatement's integer rule is the change of E_int exactly
            w = ref.weights(model.e_q30, 0.7)
            sj = c[np.asarray(model.l.neighs)[:, i - 1] - 1]
            dE, p = ref.local_rule(c[i - 1], t, sj, model.e_q30, w)
            assert dE == model.energy_q30(c2) - model.energy_q30(c)
            assert abs(p * math.exp(0.7 * dE / 2.0 ** 30) - 1.0) < 1e-14


# ---- the defined chain leaves the Boltzmann weight invariant
@pytest.mark.parametrize("case", ["chain4_q3", "square2_q2", "square2_clock4"])
def test_the_sweep_leaves_the_boltzmann_weight_invariant(mc_amd, case):
    """pi P = pi for the exact transition matrix of one sweep, built from the rule with the product p of table entries
    the device forms, to 1e-12.  Measured max |pi P - pi|: chain4_q3 (81 states, beta 0.9) 6.9e-17, square2_q2 (16 states,
    repeated neighbours, beta 0.6) 5.6e-17, square2_clock4 (256 states, beta 0.8) 3.9e-16: the few ulp of p that the
    header states, far below the bound."""
    l, q, table, beta = {"chain4_q3": (mc_amd.Chain(4), 3, ref.potts_table(3), 0.9),
                         "square2_q2": (mc_amd.SquareLattice(2), 2, ref.potts_table(2), 0.6),
                         "square2_clock4": (mc_amd.SquareLattice(2), 4, ref.clock_table(4), 0.8)}[case]
    e_q30 = ref.tables(q, table)[0]
    P, st = ref.sweep_matrix(l, q, e_q30, beta)
    assert np.allclose(P.sum(axis=1), 1.0, atol=1e-14) and P.min() >= 0.0
    E = ref.state_energies_q30(l, q, e_q30, st) / 2.0 ** 30
    pi = np.exp(-beta * (E - E.min()))
    pi /= pi.sum()
    resid = np.abs(pi @ P - pi).max()
    print(case, "states", len(st), "max |pi P - pi| =", resid)
    assert resid <= 1e-12
    # not vacuous: the same matrix does not preserve the weight of another temperature
    other = np.exp(-1.5 * beta * (E - E.min()))
    other /= other.sum()
    assert np.abs(other @ P - other).max() > 1e-4


def test_the_matrix_is_the_chain_the_restatement_runs(mc_amd):
    """one sweep of ref.Walkers from every state of Chain(4), q = 3, lands on a state the matrix gives weight to, and
    4000 walkers from one state follow the matrix row (chi-square over its support, 5 sigma)"""
    l, q, beta = mc_amd.Chain(4), 3, 0.9
    table = ref.potts_table(q)
    P, st = ref.sweep_matrix(l, q, ref.tables(q, table)[0], beta)
    W = 4000
    wk = ref.Walkers(l, q, table, [beta] * W, range(1000, 1000 + W), rand=False)
    start = 5
    wk.c[:] = st[start]
    wk.observables()
    wk.sweep()
    idx = (wk.c * 3 ** np.arange(4)).sum(axis=1)
    counts = np.bincount(idx, minlength=81)
    assert np.all(P[start][counts > 0] > 0)
    sup = P[start] > 0
    chi2 = ((counts[sup] - W * P[start][sup]) ** 2 / (W * P[start][sup])).sum()
    dof = sup.sum() - 1
    assert abs(chi2 - dof) <= 5.0 * math.sqrt(2.0 * dof), (chi2, dof)


# ---- the restatement against exact enumeration
def test_restatement_against_enumeration(mc_amd):
    """Potts q = 3 on SquareLattice(3) (19683 states) at beta = ln(1 + sqrt 3): 64 walkers, 200 + 3000 sweeps, seed 4242.
    <E> and <M2> within 5 cross-walker standard errors of the enumeration.  Observed z-scores: E +0.72, M2 -0.83."""
    l, wk = ref.stat_run()
    assert wk.n_meas == ref.STAT_SWEEPS
    z = ref.stat_zscores(wk.sum_E, wk.sum_M2, wk.n_meas, l)
    print("z-scores", z)
    assert abs(z["E"]) <= 5.0 and abs(z["M2"]) <= 5.0, z
    # the running E_int, Mx, My are those of the final configurations
    E, Mx, My = wk.E.copy(), wk.Mx.copy(), wk.My.copy()
    wk.observables()
    assert np.array_equal(E, wk.E) and np.array_equal(Mx, wk.Mx) and np.array_equal(My, wk.My)
    assert 0 < wk.acc_local.sum() < wk.prop_local.sum()


def test_exact_enumeration_limits(mc_amd):
    l = mc_amd.SquareLattice(2)
    hot = ref.qstate_exact(l, 3, ref.potts_table(3), 0.0)
    assert abs(hot["E"] + len(l.bonds) / 3.0) < 1e-12 and abs(hot["M2"] - len(l)) < 1e-7
    cold = ref.qstate_exact(l, 3, ref.potts_table(3), 40.0)
    assert abs(cold["E"] + len(l.bonds)) < 1e-9 and abs(cold["M2"] - len(l) ** 2) < 1e-5


# ---- errors, all before any device is touched
def test_model_errors(mc_amd):
    with pytest.raises(ValueError, match="symmetric"):
        mc_amd.QStateModel(3, [1.0, 0.5, 0.25], dims=1, L=4)
    for q in (1, 65, 0, 2.5):
        with pytest.raises(ValueError, match="q must be"):
            mc_amd.PottsModel(q, dims=1, L=4)
        with pytest.raises(ValueError, match="q must be"):
            mc_amd.ClockModel(q, dims=1, L=4)
    with pytest.raises(ValueError, match="q = 3"):
        mc_amd.QStateModel(3, [1.0, 0.0], dims=1, L=4)
    with pytest.raises(ValueError):
        mc_amd.PottsModel(3)  # no lattice
    m = mc_amd.QStateModel(4, [1.0, 0.25, -0.5, 0.25], dims=2, L=4, J=2.0)  # a general symmetric table is fine
    assert list(m.e_q30) == [2 ** 31, 2 ** 29, -2 ** 30, 2 ** 29]


def test_ising_only_options_are_refused(mc_amd):
    m = mc_amd.PottsModel(3, dims=2, L=4)
    for kw in ({"cluster_moves": True}, {"n_replicas": 2}, {"fss": True}, {"binning": True}, {"update": "sequential"},
               {"exchange_rate": 2}, {"global_moves": True}):
        with pytest.raises(NotImplementedError, match="IsingModel only"):
            mc_amd.MC(m, beta=1.0, **kw)
    with pytest.raises(ValueError):
        mc_amd.MC(m)  # neither beta nor T


def _params(mc_amd, l, q, colour, e=None, n_walkers=1):
    from montecarlo_jl_amd import _lib
    neighs = np.asfortranarray(np.asarray(l.neighs, dtype=np.int64))
    bonds = np.asfortranarray(np.asarray(l.bonds, dtype=np.int64)[:, :2])
    tabs = ref.tables(max(2, min(q, 64)), ref.potts_table(max(2, min(q, 64))))
    e_q30 = np.ascontiguousarray(tabs[0] if e is None else e, dtype=np.int64)
    c_q30, s_q30 = (np.ascontiguousarray(t, dtype=np.int32) for t in tabs[1:])
    colour = np.ascontiguousarray(colour, dtype=np.int32)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    p = _lib.QsParams(n_sites=len(l), z=neighs.shape[0], q=q, n_walkers=n_walkers, device_id=0, n_bonds=len(bonds),
                      series_capacity=0, n_colours=int(colour.max()) + 1, neighs=neighs.ctypes.data_as(i64),
                      bonds=bonds.ctypes.data_as(i64), e_q30=e_q30.ctypes.data_as(i64), c_q30=c_q30.ctypes.data_as(i32),
                      s_q30=s_q30.ctypes.data_as(i32), colour=colour.ctypes.data_as(i32))
    return p, (neighs, bonds, e_q30, c_q30, s_q30, colour)


def test_create_refuses_on_the_host_and_names_the_offender(mc_amd):
    """dqmc_qs_create validates everything before it looks for a device: DQMC_ERR_INVALID with or without a GPU"""
    from montecarlo_jl_amd import _lib
    lib = _lib.lib()
    l = mc_amd.SquareLattice(4)
    good = ref.greedy_colouring(l)

    def refused(p, text):
        h = C.c_void_p()
        rc = lib.dqmc_qs_create(C.byref(p[0]), C.byref(h))
        msg = lib.dqmc_qs_last_error(None).decode()
        assert rc == _lib.ERR_INVALID and not h.value, (rc, msg)
        assert text in msg, msg

    refused(_params(mc_amd, l, 1, good), "q = 1 is outside 2..64")
    refused(_params(mc_amd, l, 65, good), "q = 65 is outside 2..64")
    refused(_params(mc_amd, l, 3, good, e=[2 ** 30, 5, 7]), "e_q30[1] != e_q30[2]")
    refused(_params(mc_amd, l, 3, good, e=[2 ** 33, 0, 0]), "e_q30[0] exceeds 2^32")
    clash = good.copy()
    clash[1] = clash[0]
    refused(_params(mc_amd, l, 3, clash), "the neighbours 0 and 1 (0-based sites) share colour 0")
    far = good.copy()
    far[3] = 16
    refused(_params(mc_amd, l, 3, far), "n_colours must be in 1..16")
    big = mc_amd.RectangularLattice(256, 128)  # 32768 sites
    refused(_params(mc_amd, big, 3, ref.greedy_colouring(mc_amd.SquareLattice(2))), "n_sites = 32768 exceeds 16384")
    p = _params(mc_amd, l, 3, good)
    p[0].z = 9
    refused(p, "z = 9 is outside 1..8")
    p = _params(mc_amd, mc_amd.Chain(1), 3, [0])
    refused(p, "site 0 lists itself as a neighbour")
    # through the Python surface: the same refusal, as a DQMCError with the code
    with pytest.raises(mc_amd.DQMCError) as ei:
        mc_amd.MC(mc_amd.PottsModel(3, l=l), beta=1.0, colouring=clash)
    assert ei.value.code == _lib.ERR_INVALID and "share colour" in str(ei.value)
    for fn in (lib.dqmc_qs_destroy, lib.dqmc_qs_synchronize):
        assert fn(None) in (_lib.OK, _lib.ERR_INVALID)  # a null handle faults nothing
    assert lib.dqmc_qs_sweep(None, 1, 1, 0, 1) == _lib.ERR_INVALID


def test_ising_models_construct_what_they_did(mc_amd):
    """MC.__new__ hands q-state models to QStateMC and nothing else: an IsingModel still reaches MC.__init__ (which, with
    no device here or with one, is the same code as before), and the class of the result is MC"""
    assert not getattr(mc_amd.IsingModel(dims=2, L=4), "is_qstate", False)
    assert mc_amd.PottsModel(3, dims=2, L=4).is_qstate and mc_amd.ClockModel(5, dims=1, L=6).is_qstate
    with pytest.raises(ValueError, match="exactly one of beta and T"):
        mc_amd.MC(mc_amd.IsingModel(dims=2, L=4))  # raised by MC.__init__ itself
    if mc_amd.device_count() >= 1:
        mc = mc_amd.MC(mc_amd.IsingModel(dims=2, L=4), beta=0.4)
        assert type(mc) is mc_amd.MC
        mc.close()
