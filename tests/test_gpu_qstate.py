"""The q-state (Potts, clock) engine on the device (csrc/qstate.hip: one workgroup per walker, colour class by colour
class) against the numpy restatement of tests/qstate_ref.py, written from include/dqmc_hip.h.

Everything is compared with ==: the states, E_int, Mx, My, the counters, the cursors, the series and the fp64 sums (the
decisions are fp64 comparisons of a Philox uniform with a product of host table entries; the sums follow the header's
order of operations, compiled without contraction).  One exception, as the header says: sum_absM adds sqrt(m2), and the
device's fp64 sqrt need not be the correctly rounded one, so that sum is compared at 1e-13 relative."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (lattice, model kind, q, centre beta (acceptance near one half there), sweeps)
SHAPES = {
    "chain5_q2": (lambda g: g.Chain(5), "potts", 2, 0.9, 8),                       # z = 2, odd ring, 3 colours
    "square2_q3": (lambda g: g.SquareLattice(2), "potts", 3, 0.7, 8),              # repeated neighbours
    "square5_q5": (lambda g: g.SquareLattice(5), "potts", 5, 0.9, 8),              # N = 25 < a wave, 3 to 4 colours
    "square9_q64": (lambda g: g.SquareLattice(9), "clock", 64, 0.9, 6),            # the largest table
    "triangular6_clock6": (lambda g: g.TriangularLattice(6), "clock", 6, 0.4, 8),  # z = 6
    "cubic4_q4": (lambda g: g.CubicLattice(3, 4), "potts", 4, 0.55, 8),            # N = 64: exactly one wave
    "square18_clock8": (lambda g: g.SquareLattice(18), "clock", 8, 0.9, 8),        # N = 324: ragged last wave
}


def _table(kind, q):
    return ref.potts_table(q) if kind == "potts" else ref.clock_table(q)


def _model(g, kind, q, l, J=1.0):
    return g.PottsModel(q, l=l, J=J) if kind == "potts" else g.ClockModel(q, l=l, J=J)


def _check(mc, wk, label):
    for w in range(wk.W):
        want, want_absM = wk.stats(w)
        st = mc.stats(w)
        got = {k: getattr(st, k) for k in want}
        assert got == want, (label, w, got, want)
        assert abs(st.sum_absM - want_absM) <= 1e-13 * abs(want_absM), (label, w, st.sum_absM, want_absM)
        assert np.array_equal(mc.conf(w), wk.c[w]), (label, w)
        e, mx, my = mc.series(w)
        assert list(zip(e.tolist(), mx.tolist(), my.tolist())) == wk.ser[w], (label, w)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_on_the_shapes_where_the_kernel_can_go_wrong(gpu, shape):
    make, kind, q, beta, n = SHAPES[shape]
    l = make(gpu)
    W, seed, cap = 3, 700, 20
    betas = beta * np.array([0.8, 1.0, 1.25])
    mc = gpu.MC(_model(gpu, kind, q, l), beta=betas, n_walkers=W, seed=seed, series_capacity=cap)
    assert type(mc) is gpu.QStateMC
    wk = ref.Walkers(l, q, _table(kind, q), betas, [seed + w for w in range(W)], series_capacity=cap)
    _check(mc, wk, (shape, "initial"))  # the initial configuration and its E_int, Mx, My
    mc.sweep(n)
    wk.run(1, n, 0, 1)
    _check(mc, wk, shape)
    st = mc.stats(1)
    assert st.n_meas == n and st.n_colours == int(ref.greedy_colouring(l).max()) + 1
    rate = st.acc_local / st.prop_local
    print(shape, "acceptance at the centre beta", rate)
    assert 0.3 < rate < 0.7, (shape, rate)
    if q == 2:
        assert all(mc.stats(w).my_q30 == 0 for w in range(W))
    mc.close()


def test_a_coupling_other_than_one(gpu):
    """clock q = 6 on TriangularLattice(6) with J = 0.5: the table is llround(J e 2^30), and at twice the beta of the
    J = 1 shape the chain accepts as often"""
    l = gpu.TriangularLattice(6)
    W, seed, cap, n, J = 3, 700, 20, 8, 0.5
    betas = 0.8 * np.array([0.8, 1.0, 1.25])
    mc = gpu.MC(_model(gpu, "clock", 6, l, J=J), beta=betas, n_walkers=W, seed=seed, series_capacity=cap)
    wk = ref.Walkers(l, 6, _table("clock", 6), betas, [seed + w for w in range(W)], J=J, series_capacity=cap)
    assert wk.e_q30.tolist() == [2 ** 29, 2 ** 28, -2 ** 28, -2 ** 29, -2 ** 28, 2 ** 28]
    _check(mc, wk, "J = 0.5, initial")
    mc.sweep(n)
    wk.run(1, n, 0, 1)
    _check(mc, wk, "J = 0.5")
    st = mc.stats(1)
    assert st.n_meas == n and 0.3 < st.acc_local / st.prop_local < 0.7
    mc.close()


def test_the_site_ceiling(gpu):
    """N = 16384, the LDS limit: one walker, two sweeps"""
    l = gpu.SquareLattice(128)
    mc = gpu.MC(gpu.PottsModel(3, l=l), beta=1.0, n_walkers=1, seed=77, series_capacity=2)
    wk = ref.Walkers(l, 3, ref.potts_table(3), [1.0], [77], series_capacity=2)
    mc.sweep(2)
    wk.run(1, 2, 0, 1)
    _check(mc, wk, "square128")
    st = mc.stats(0)
    assert st.prop_local == 2 * 16384 and 0 < st.acc_local < st.prop_local and st.n_colours == 2
    mc.close()


@pytest.mark.parametrize("W", [1, 3, 65])
def test_walker_counts_with_a_beta_each(gpu, W):
    l = gpu.SquareLattice(5)
    betas = np.linspace(0.3, 1.6, W) if W > 1 else np.array([0.9])
    mc = gpu.MC(gpu.PottsModel(5, l=l), beta=betas, n_walkers=W, seed=31, first_walker=4, series_capacity=6)
    assert mc.seeds == [35 + w for w in range(W)]
    wk = ref.Walkers(l, 5, ref.potts_table(5), betas, mc.seeds, series_capacity=6)
    mc.sweep(6)
    wk.run(1, 6, 0, 1)
    _check(mc, wk, W)
    mc.close()


def test_beta_zero_accepts_every_proposal_and_beta_50_keeps_order(gpu):
    l = gpu.SquareLattice(6)
    N = len(l)
    mc = gpu.MC(gpu.ClockModel(6, l=l), beta=[0.0, 50.0], n_walkers=2, seed=9)
    wk = ref.Walkers(l, 6, ref.clock_table(6), [0.0, 50.0], [9, 10])
    ordered = np.full(N, 2, dtype=np.uint8)
    mc.set_conf(1, ordered)
    wk.set_conf(1, ordered)
    _check(mc, wk, "set")
    mc.sweep(5)
    wk.run(1, 5, 0, 1)
    _check(mc, wk, "beta 0 / 50")
    hot, cold = mc.stats(0), mc.stats(1)
    assert hot.acc_local == hot.prop_local == 5 * N
    assert cold.acc_local == 0 and np.array_equal(mc.conf(1), ordered)
    assert cold.energy_q30 == -len(l.bonds) * 2 ** 30 and mc.energy(1) == -float(len(l.bonds))
    mx, my = mc.order_parameter(1)
    assert abs(mx * mx + my * my - N * N) < 1e-6 * N * N
    mc.close()


def test_a_run_does_not_depend_on_how_it_is_split(gpu):
    """7 sweeps in one call equal 3 + 4 in two; measure_rate 3 with thermalization 2 measures sweeps 3 and 6"""
    l = gpu.SquareLattice(5)
    kw = dict(beta=[0.8, 1.0], n_walkers=2, seed=55, thermalization=2, measure_rate=3, series_capacity=8)
    one, two = gpu.MC(gpu.ClockModel(5, l=l), **kw), gpu.MC(gpu.ClockModel(5, l=l), **kw)
    one.sweep(7)
    two.sweep(3)
    two.sweep(4)
    wk = ref.Walkers(l, 5, ref.clock_table(5), [0.8, 1.0], [55, 56], series_capacity=8)
    wk.run(1, 7, 2, 3)
    assert wk.n_meas == 2
    _check(one, wk, "one call")
    _check(two, wk, "two calls")
    one.close()
    two.close()


def test_run_follows_thermalization_and_sweeps(gpu):
    l = gpu.Chain(6)
    mc = gpu.MC(gpu.PottsModel(3, l=l), beta=0.8, seed=3, thermalization=4, sweeps=9, measure_rate=2)
    assert mc.run() and mc.last_sweep == 13
    wk = ref.Walkers(l, 3, ref.potts_table(3), [0.8], [3])
    wk.run(1, 13, 4, 2)
    _check(mc, wk, "run")
    m, st = mc.measurements(0), mc.stats(0)
    n = st.n_meas
    assert n == 4 and m["n_meas"] == 4 and m["Energy"]["E"] == st.sum_E / n and m["Magn"]["M2"] == st.sum_M2 / n
    assert m["Magn"]["U4"] == 1.0 - (st.sum_M4 / n) / (2.0 * (st.sum_M2 / n) ** 2)
    assert m["Magn"]["m"] == (st.sum_absM / n) * (1.0 / 6) and m["Energy"]["e"] == (st.sum_E / n) * (1.0 / 6)
    a = mc.analysis(0)
    assert a["prop_local"] == 13 * 6 and a["acc_rate"] == st.acc_local / st.prop_local
    mc.close()


def test_set_conf_round_trip_and_reset(gpu):
    l = gpu.SquareLattice(7)
    model = gpu.ClockModel(7, l=l)
    mc = gpu.MC(model, beta=0.9, n_walkers=2, seed=12, series_capacity=3)
    conf = np.random.default_rng(1).integers(0, 7, len(l)).astype(np.uint8)
    mc.set_conf(1, conf)
    assert np.array_equal(mc.conf(1), conf)
    st = mc.stats(1)
    assert st.energy_q30 == model.energy_q30(conf) and (st.mx_q30, st.my_q30) == model.order_parameter_q30(conf)
    assert st.sweeps_drawn == 0 and st.confs_drawn == 1
    with pytest.raises(gpu.DQMCError) as ei:  # refused on the host: a state that is not below q
        mc.set_conf(0, np.full(len(l), 7))
    assert ei.value.code == -1
    wk = ref.Walkers(l, 7, ref.clock_table(7), [0.9, 0.9], [12, 13], series_capacity=3)
    wk.set_conf(1, conf)
    mc.sweep(5)
    wk.run(1, 5, 0, 1)
    _check(mc, wk, "before reset")  # the series stopped at its capacity of 3
    assert mc.stats(0).n_series == 3 and mc.stats(0).n_meas == 5
    mc.reset_accumulators()
    wk.reset_accumulators()
    st = mc.stats(0)
    assert (st.n_meas, st.n_series, st.sum_E, st.sum_M4) == (0, 0, 0.0, 0.0)
    assert st.prop_local == 5 * len(l) and st.acc_local == int(wk.acc_local[0]) and st.sweeps_drawn == 5  # these stay
    mc.sweep(2)
    wk.run(6, 2, 0, 1)
    _check(mc, wk, "after reset")
    mc.rand_conf(0)  # a second initial configuration comes from the next cursor value
    wk2 = ref.Walkers(l, 7, ref.clock_table(7), [0.9], [12], rand=False)
    wk2.r[:] = 1
    wk2.rand_conf()
    assert np.array_equal(mc.conf(0), wk2.c[0]) and mc.stats(0).confs_drawn == 2
    assert mc.stats(0).energy_q30 == int(wk2.E[0])
    mc.close()


def test_a_colouring_of_the_callers(gpu):
    """a 4-colouring of an even square lattice reproduces the restatement run with it; a clashing one is refused with
    DQMC_ERR_INVALID and the handle goes on as it was"""
    L = 6
    l = gpu.SquareLattice(L)
    i, j = np.arange(L * L) % L, np.arange(L * L) // L
    four = ((i % 2) + 2 * (j % 2)).astype(np.int32)
    assert ref.is_valid(l, four) and int(ref.greedy_colouring(l).max()) == 1
    mc = gpu.MC(gpu.PottsModel(4, l=l), beta=[0.9, 1.1], n_walkers=2, seed=8, colouring=four)
    wk = ref.Walkers(l, 4, ref.potts_table(4), [0.9, 1.1], [8, 9], colouring=four)
    mc.sweep(4)
    wk.run(1, 4, 0, 1)
    _check(mc, wk, "four colours")
    assert mc.stats(0).n_colours == 4
    two = gpu.MC(gpu.PottsModel(4, l=l), beta=[0.9, 1.1], n_walkers=2, seed=8)  # the greedy 2-colouring: another chain
    two.sweep(4)
    assert not np.array_equal(two.conf(0), mc.conf(0))
    two.close()
    clash = four.copy()
    clash[1] = clash[0]
    with pytest.raises(gpu.DQMCError) as ei:
        mc.set_colouring(clash)
    assert ei.value.code == -1 and "share colour" in str(ei.value)
    with pytest.raises(gpu.DQMCError) as ei:
        gpu.MC(gpu.PottsModel(4, l=l), beta=1.0, colouring=clash)
    assert ei.value.code == -1
    mc.sweep(3)  # still usable, still on the four colours
    wk.run(5, 3, 0, 1)
    _check(mc, wk, "after the refusal")
    mc.set_colouring(None)  # and a valid change takes effect between sweeps
    wk.set_colouring(ref.greedy_colouring(l))
    mc.sweep(2)
    wk.run(8, 2, 0, 1)
    _check(mc, wk, "greedy from now on")
    mc.close()


def test_the_device_run_against_enumeration(gpu):
    """the statistical check of test_qstate_host.py through the device (same seed and lengths): the device is bit-exact to
    the restatement, so it gives the same sums, and those lie within 5 standard errors of the enumeration"""
    l, wk = ref.stat_run()
    mc = gpu.MC(gpu.PottsModel(ref.STAT_Q, l=l), beta=ref.STAT_BETA, n_walkers=ref.STAT_W, seed=ref.STAT_SEED,
                thermalization=ref.STAT_THERM, sweeps=ref.STAT_SWEEPS)
    mc.run()
    sts = [mc.stats(w) for w in range(ref.STAT_W)]
    assert all(st.n_meas == ref.STAT_SWEEPS for st in sts)
    sum_E, sum_M2 = [st.sum_E for st in sts], [st.sum_M2 for st in sts]
    assert sum_E == wk.sum_E.tolist() and sum_M2 == wk.sum_M2.tolist()
    assert [st.acc_local for st in sts] == wk.acc_local.tolist()
    z = ref.stat_zscores(sum_E, sum_M2, ref.STAT_SWEEPS, l)
    print("z-scores", z)
    assert abs(z["E"]) <= 5.0 and abs(z["M2"]) <= 5.0, z
    mc.close()


def test_the_other_flavors_do_not_notice(gpu):
    """a DQMC handle and an Ising MC handle swept before and after a q-state run give what the same handles give in a
    stretch with no q-state run in between (compared in-process)"""
    def pair():
        d = gpu.DQMC(gpu.HubbardModelAttractive(4, 2), beta=1.0, n_walkers=2, seed=123)
        d.prepare()
        i = gpu.MC(gpu.IsingModel(dims=2, L=8), beta=[0.3, 0.5], n_walkers=2, seed=5, update="checkerboard")
        assert type(i) is gpu.MC
        return d, i

    def step(d, i):
        for _ in range(3):
            d.update()
        i.sweep(5)

    def state(d, i):
        return ([d.conf(w).copy() for w in range(2)] + [d.greens_eff(w)[0].copy() for w in range(2)] +
                [i.conf(w).copy() for w in range(2)] +
                [np.array([i.stats(w).energy, i.stats(w).sum_E, i.stats(w).acc_local]) for w in range(2)])

    d0, i0 = pair()
    step(d0, i0)
    step(d0, i0)
    want = state(d0, i0)
    d0.close()
    i0.close()
    d1, i1 = pair()
    step(d1, i1)
    l = gpu.SquareLattice(18)
    qs = gpu.MC(gpu.ClockModel(8, l=l), beta=0.9, n_walkers=3, seed=700)
    qs.sweep(4)
    step(d1, i1)
    qs.sweep(4)
    got = state(d1, i1)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    wk = ref.Walkers(l, 8, ref.clock_table(8), [0.9] * 3, [700, 701, 702])
    wk.run(1, 8, 0, 1)
    _check(qs, wk, "beside the others")
    for h in (d1, i1, qs):
        h.close()
