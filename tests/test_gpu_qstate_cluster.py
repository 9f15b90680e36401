"""The reflection cluster move of the q-state engine on the device (csrc/qstate.hip: inside the sweep kernel, on the sites
in LDS; a bitset, one append-only queue, level by level) against the numpy restatement of tests/qstate_cluster_ref.py,
written from include/dqmc_hip.h.

Everything is compared with ==: the states, E_int, Mx, My, the local and global counters, the three cursors, the series and
the fp64 sums; sum_absM at 1e-13 relative, as in test_gpu_qstate.py (the device's sqrt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_cluster_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (lattice, model kind, q, centre beta).  The centre lies at or above the ordering coupling of each model, so that
# clusters span several breadth-first levels; where N z > 64 some cluster then has more slots than one wave has lanes.
SHAPES = {
    "chain5_q2": (lambda g: g.Chain(5), "potts", 2, 1.2),                        # odd ring
    "square2_q3": (lambda g: g.SquareLattice(2), "potts", 3, 0.9),               # repeated neighbours
    "square5_q5": (lambda g: g.SquareLattice(5), "potts", 5, 1.3),               # N = 25: 64 threads
    "square9_q64": (lambda g: g.SquareLattice(9), "clock", 64, 1.2),             # the largest table
    "triangular6_clock6": (lambda g: g.TriangularLattice(6), "clock", 6, 0.6),   # z = 6, the E convention
    "honeycomb3_q3": (lambda g: g.HoneycombLattice(3), "potts", 3, 1.5),         # z = 3
    "cubic4_q4": (lambda g: g.CubicLattice(3, 4), "potts", 4, 0.7),              # N = 64
    "square18_clock8": (lambda g: g.SquareLattice(18), "clock", 8, 1.2),         # N = 324: ragged wave, many levels
}


def _table(kind, q):
    return ref.potts_table(q) if kind == "potts" else ref.clock_table(q)


def _model(g, kind, q, l):
    return g.PottsModel(q, l=l) if kind == "potts" else g.ClockModel(q, l=l)


def _fields(mc, w, n_series):
    st, cl = mc.stats(w), mc.cluster_stats(w)
    return ({k: getattr(st, k) for k, _ in st._fields_}, {k: getattr(cl, k) for k, _ in cl._fields_}, mc.conf(w).tolist(),
            [x.tolist() for x in mc.series(w)] if n_series else None)


def _check(mc, wk, label, walkers=None, at=None):
    """walker at[i] of the handle against walker walkers[i] of the restatement (default: all, in place)"""
    walkers = range(wk.W) if walkers is None else walkers
    for x, w in enumerate(walkers):
        d = w if at is None else at[x]
        want, want_absM = wk.stats(w)
        st = mc.stats(d)
        got = {k: getattr(st, k) for k in want}
        assert got == want, (label, w, got, want)
        assert abs(st.sum_absM - want_absM) <= 1e-13 * abs(want_absM), (label, w, st.sum_absM, want_absM)
        cl = mc.cluster_stats(d)
        want_cl = wk.cluster_stats(w)
        assert {k: getattr(cl, k) for k in want_cl} == want_cl, (label, w)
        assert np.array_equal(mc.conf(d), wk.c[w]), (label, w)
        e, mx, my = mc.series(d)
        assert list(zip(e.tolist(), mx.tolist(), my.tolist())) == wk.ser[w], (label, w)


@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_on_the_shapes_where_the_kernel_can_go_wrong(gpu, shape, rate):
    """8 sweeps, every second one measured: with rate 1 a move stands behind measured and unmeasured sweeps, with rate 3
    behind sweep 3 (unmeasured) and sweep 6 (measured)"""
    make, kind, q, beta = SHAPES[shape]
    l = make(gpu)
    W, seed, cap, n = 3, 900, 8, 8
    betas = beta * np.array([0.8, 1.0, 1.25])
    mc = gpu.MC(_model(gpu, kind, q, l), beta=betas, n_walkers=W, seed=seed, series_capacity=cap, measure_rate=2,
                cluster_rate=rate)
    assert type(mc) is gpu.QStateMC and mc.cluster_rate == rate
    wk = cref.ClusterWalkers(l, q, _table(kind, q), betas, [seed + w for w in range(W)], series_capacity=cap)
    mc.sweep(n)
    wk.run(1, n, 0, 2, cluster_rate=rate)
    _check(mc, wk, (shape, rate))
    cl = mc.cluster_stats(1)
    assert cl.prop_global == cl.moves_drawn == n // rate and mc.stats(1).n_meas == 4
    a = mc.analysis(1)
    assert (a["prop_global"], a["acc_global"]) == (cl.prop_global, cl.acc_global)
    N, z = len(l), np.asarray(l.neighs).shape[0]
    print(shape, "rate", rate, "mean cluster size / N at the centre beta", cl.sum_cluster_size / cl.prop_global / N,
          "its largest cluster", int(wk.max_cluster_size[1]), "of", N)
    if rate == 1 and N * z > 64:  # the device's sizes are the restatement's: the states agreed behind every launch
        assert int(wk.max_cluster_size[1]) * z > 64, (shape, wk.max_cluster_size)
    mc.close()


@pytest.mark.parametrize("case", ["potts3_ordered", "clock64"])
def test_the_ceilings(gpu, case):
    """N = 16384, one walker, two sweeps with a move each.  potts3_ordered: from an ordered start at beta = 1.2 the bond
    probability 1 - exp(-1.2) = 0.70 is far above the square lattice's bond-percolation threshold 1/2, so the cluster takes
    most of the lattice and the queue fills towards N.  clock64: q = 64, the largest LDS request (83 KiB, above the 64 KiB
    a kernel gets without the attribute)."""
    l = gpu.SquareLattice(128)
    N = len(l)
    if case == "potts3_ordered":
        kind, q, beta = "potts", 3, 1.2
    else:
        kind, q, beta = "clock", 64, 1.0
    mc = gpu.MC(_model(gpu, kind, q, l), beta=beta, n_walkers=1, seed=78, series_capacity=2, cluster_rate=1)
    wk = cref.ClusterWalkers(l, q, _table(kind, q), [beta], [78], series_capacity=2)
    if case == "potts3_ordered":
        ordered = np.full(N, 1, dtype=np.uint8)
        mc.set_conf(0, ordered)
        wk.set_conf(0, ordered)
    mc.sweep(2)
    wk.run(1, 2, 0, 1, cluster_rate=1)
    _check(mc, wk, case)
    cl = mc.cluster_stats(0)
    print(case, "cluster sizes sum", cl.sum_cluster_size, "of", 2 * N)
    assert cl.prop_global == 2 and 2 <= cl.sum_cluster_size <= 2 * N
    if case == "potts3_ordered":
        assert cl.sum_cluster_size > N  # more than half of the lattice per move
    mc.close()


def test_beta_50_reflects_the_whole_lattice_and_beta_0_single_sites(gpu):
    l = gpu.SquareLattice(6)
    N = len(l)
    mc = gpu.MC(gpu.PottsModel(4, l=l), beta=[50.0, 0.0], n_walkers=2, seed=19)
    wk = cref.ClusterWalkers(l, 4, ref.potts_table(4), [50.0, 0.0], [19, 20])
    ordered = np.full(N, 3, dtype=np.uint8)
    mc.set_conf(0, ordered)
    wk.set_conf(0, ordered)
    E0 = mc.stats(0).energy_q30
    assert E0 == -len(l.bonds) * 2 ** 30
    seen = []
    for k in range(5):
        mc.cluster_move()
        wk.cluster_move()
        conf = mc.conf(0)
        assert len(set(conf.tolist())) == 1  # every site in one state
        seen.append(int(conf[0]))
        assert mc.stats(0).energy_q30 == E0
    assert seen[0] != 3 and all(a != b for a, b in zip(seen, seen[1:]))  # a new state every time
    _check(mc, wk, "by hand")
    mc.set_cluster_rate(1)
    mc.sweep(4)
    wk.run(1, 4, 0, 1, cluster_rate=1)
    _check(mc, wk, "in the sweep")
    cold, hot = mc.cluster_stats(0), mc.cluster_stats(1)
    assert cold.prop_global == 9 and cold.acc_global == cold.prop_global and cold.sum_cluster_size == 9 * N
    assert mc.stats(0).energy_q30 == E0 and len(set(mc.conf(0).tolist())) == 1
    assert hot.prop_global == 9 and hot.acc_global == 0 and hot.sum_cluster_size == hot.moves_drawn == 9
    mc.close()


def test_a_run_does_not_depend_on_how_it_is_split(gpu):
    """7 sweeps in one call, as 3 + 4 and as seven calls of one; thermalization 2, measure_rate 3, a move behind sweeps 2,
    4 and 6"""
    l = gpu.SquareLattice(5)
    kw = dict(beta=[0.9, 1.2], n_walkers=2, seed=56, thermalization=2, measure_rate=3, series_capacity=8, cluster_rate=2)
    one, two, seven = (gpu.MC(gpu.ClockModel(5, l=l), **kw) for _ in range(3))
    one.sweep(7)
    two.sweep(3)
    two.sweep(4)
    for _ in range(7):
        seven.sweep(1)
    wk = cref.ClusterWalkers(l, 5, ref.clock_table(5), [0.9, 1.2], [56, 57], series_capacity=8)
    wk.run(1, 7, 2, 3, cluster_rate=2)
    assert wk.n_meas == 2 and np.all(wk.m == 3)
    for mc, label in ((one, "one call"), (two, "two calls"), (seven, "seven calls")):
        _check(mc, wk, label)
        mc.close()


def test_a_walker_does_not_depend_on_the_others(gpu):
    """the walker with key 640 alone in a handle and as walker 40 of 65"""
    l = gpu.SquareLattice(5)
    betas = np.linspace(0.6, 1.6, 65)
    many = gpu.MC(gpu.PottsModel(3, l=l), beta=betas, n_walkers=65, seed=600, series_capacity=6, cluster_rate=2)
    alone = gpu.MC(gpu.PottsModel(3, l=l), beta=betas[40], n_walkers=1, seed=600, first_walker=40, series_capacity=6,
                   cluster_rate=2)
    assert many.seeds[40] == alone.seeds[0] == 640
    many.sweep(6)
    alone.sweep(6)
    assert _fields(many, 40, 6) == _fields(alone, 0, 6)
    wk = cref.ClusterWalkers(l, 3, ref.potts_table(3), betas, many.seeds, series_capacity=6)
    wk.run(1, 6, 0, 1, cluster_rate=2)
    _check(many, wk, "65 walkers")
    _check(alone, wk, "alone", walkers=[40], at=[0])
    many.close()
    alone.close()


def test_a_thousand_sweeps_cross_the_launch_boundary(gpu):
    """SquareLattice(5): a launch runs at most 2^19 / (25 + 512) = 976 sweeps, so 1000 sweeps are two launches; rate 7
    puts moves on both sides (sweeps 973 and 980)"""
    l = gpu.SquareLattice(5)
    betas = [0.8, 1.0, 1.2]
    mc = gpu.MC(gpu.PottsModel(3, l=l), beta=betas, n_walkers=3, seed=77, measure_rate=10, series_capacity=100,
                cluster_rate=7)
    wk = cref.ClusterWalkers(l, 3, ref.potts_table(3), betas, [77, 78, 79], series_capacity=100)
    mc.sweep(1000)
    wk.run(1, 1000, 0, 10, cluster_rate=7)
    _check(mc, wk, "1000 sweeps")
    assert mc.cluster_stats(0).moves_drawn == 142 and mc.stats(0).n_meas == 100
    mc.close()


def test_moves_by_hand(gpu):
    """cluster_move(1) advances walker 1 alone, cluster_move() all of them, neither measures; seed() puts the move cursor
    back to 0, and the same key then repeats the same moves"""
    l = gpu.SquareLattice(7)
    betas = [0.9, 1.1, 1.3]
    mc = gpu.MC(gpu.ClockModel(7, l=l), beta=betas, n_walkers=3, seed=41, series_capacity=4)
    wk = cref.ClusterWalkers(l, 7, ref.clock_table(7), betas, [41, 42, 43], series_capacity=4)
    assert mc.cluster_rate == 0
    before = [_fields(mc, w, 4) for w in range(3)]
    mc.cluster_move(1)
    wk.cluster_move(1)
    assert [_fields(mc, w, 4) for w in (0, 2)] == [before[0], before[2]]
    assert [mc.cluster_stats(w).moves_drawn for w in range(3)] == [0, 1, 0]
    _check(mc, wk, "walker 1")
    mc.cluster_move()
    wk.cluster_move()
    assert [mc.cluster_stats(w).moves_drawn for w in range(3)] == [1, 2, 1]
    _check(mc, wk, "all walkers")
    assert all(mc.stats(w).n_meas == 0 and mc.stats(w).n_series == 0 and mc.stats(w).sweeps_drawn == 0 for w in range(3))
    mc.sweep(3)  # rate 0: sweeps make no move
    wk.run(1, 3, 0, 1)
    _check(mc, wk, "sweeps at rate 0")
    mc.reset_accumulators()  # leaves the global counters alone
    wk.reset_accumulators()
    _check(mc, wk, "after reset")
    assert mc.cluster_stats(1).prop_global == 2
    mc.seed(1, 42)
    wk.seed(1, 42)
    assert mc.cluster_stats(1).moves_drawn == 0 and mc.cluster_stats(1).prop_global == 2
    mc.cluster_move(1)
    wk.cluster_move(1)
    _check(mc, wk, "after seed")
    with pytest.raises(gpu.DQMCError) as ei:
        mc.cluster_move(3)
    assert ei.value.code == -1
    with pytest.raises(ValueError):
        mc.set_cluster_rate(-2)
    mc.close()


def test_rate_zero_after_a_rate_is_a_handle_that_never_had_one(gpu):
    l = gpu.SquareLattice(18)
    kw = dict(beta=[0.9, 1.1], n_walkers=2, seed=33, series_capacity=6, measure_rate=2)
    a, b = gpu.MC(gpu.ClockModel(8, l=l), **kw), gpu.MC(gpu.ClockModel(8, l=l), **kw)
    a.set_cluster_rate(3)
    a.set_cluster_rate(0)
    a.sweep(6)
    b.sweep(6)
    for w in range(2):
        assert _fields(a, w, 6) == _fields(b, w, 6)
        assert a.cluster_stats(w).moves_drawn == 0 and a.cluster_stats(w).prop_global == 0
    wk = ref.Walkers(l, 8, ref.clock_table(8), [0.9, 1.1], [33, 34], series_capacity=6)  # and both are the plain engine
    wk.run(1, 6, 0, 2)
    for w in range(2):
        want, _ = wk.stats(w)
        assert {k: getattr(a.stats(w), k) for k in want} == want and np.array_equal(a.conf(w), wk.c[w])
    a.close()
    b.close()
