"""The checkerboard sweep on the device (csrc/ising_cb.inl: one workgroup per walker, colour class by colour class)
against the numpy restatement of tests/ising_checkerboard_ref.py, written from include/dqmc_hip.h (dqmc_mc_set_update).

Everything is compared with ==: the decisions are fp64 comparisons of a Philox uniform with the host's exp table, E and
M are integers, and the sums add integers held in fp64 in the order of the measurements.  Two exceptions, under the
rules of test_gpu_ising_fss.py: sum_S at rtol 1e-13 and the binner's FSS section at rtol 1e-12 (S_k is three or four
roundings depending on contraction)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ising_checkerboard_ref as ref  # noqa: E402
import ising_fss_ref as fss_ref  # noqa: E402
import ising_wolff_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("energy", "magnetization", "sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "prop_local", "acc_local",
               "uniforms_used")
SHAPES = {
    "square2": lambda g: g.SquareLattice(2),          # repeated neighbours
    "square4": lambda g: g.SquareLattice(4),          # N < the lanes of a wave: idle lanes
    "square8": lambda g: g.SquareLattice(8),
    "square5": lambda g: g.SquareLattice(5),          # 4 uneven classes
    "chain10": lambda g: g.Chain(10),
    "chain7": lambda g: g.Chain(7),                   # a class of one site
    "cubic4": lambda g: g.CubicLattice(3, 4),         # z = 6
    "triangular4": lambda g: g.TriangularLattice(4),  # 4 colours
    "triangular6": lambda g: g.TriangularLattice(6),
    "square24": lambda g: g.SquareLattice(24),        # N = 576: strided class loop, 288 sites per class, shared words
}


def _stats(mc, w):
    st = mc.stats(w)
    return {f: getattr(st, f) for f in STAT_FIELDS}


def _gstats(mc, w):
    g = mc.global_stats(w)
    return {f: getattr(g, f) for f in ("prop_global", "acc_global", "sum_cluster_size", "moves_drawn")}


def _xstats(mc, w):
    x = mc.exchange_stats(w)
    return {f: getattr(x, f) for f in ("prop_exchange", "acc_exchange", "replica", "rounds")}


def _check_slot(mc, lad, w, label):
    want = lad.stats(w)
    got = _stats(mc, w)
    assert {k: got[k] for k in want} == want, (label, w, got, want)
    assert np.array_equal(mc.conf(w), lad.c[w]), (label, w)
    e, m = mc.series(w)
    assert list(e) == lad.serE[w] and list(m) == lad.serM[w], (label, w)
    u = mc.update_stats(w)
    assert (u.kind, u.sweeps_drawn) == (1 if lad.update == "checkerboard" else 0, int(lad.s[w])), (label, w)


@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_on_the_small_lattices(gpu, shape, rate):
    l = SHAPES[shape](gpu)
    W, seed, therm, cap = 8, 900, 2, 50
    betas = np.linspace(0.2, 0.6, W)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=W, seed=seed, thermalization=therm, measure_rate=rate,
                series_capacity=cap, update="checkerboard")
    for n in (13, 1, 27):
        mc.sweep(n)
    lad = ref.Ladders(l, betas, [seed + w for w in range(W)], series_capacity=cap)
    lad.run(1, 41, therm, rate)
    n_colours = int(ref.greedy_colouring(l).max()) + 1
    for w in range(W):
        _check_slot(mc, lad, w, (shape, rate))
        assert mc.update_stats(w).n_colours == n_colours
        assert mc.uniforms_used(w) == len(l) and mc.stats(w).prop_local == 41 * len(l)
        assert mc.global_stats(w).moves_drawn == 0 and mc.exchange_stats(w).rounds == 0
    assert sum(mc.stats(w).acc_local for w in range(W)) > 0
    mc.close()


def test_the_site_ceiling(gpu):
    """N = 16384: two sweeps from set_conf states, near T_c from a random state and frozen (beta = 50 from all-up:
    nothing flips, the counts are exact)"""
    l = gpu.SquareLattice(128)
    N = len(l)
    betas, keys = [0.44, 50.0], [31, 32]
    confs = [np.random.default_rng(3).choice([-1, 1], N).astype(np.int8), np.ones(N, dtype=np.int8)]
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=2, seed=0, update="checkerboard")
    for w in range(2):
        mc.set_conf(w, confs[w])
        mc.seed(w, keys[w])
    mc.sweep(2)
    for w in range(2):
        one = ref.Walker(l, betas[w], keys[w], conf=confs[w])
        one.run(1, 2, 0, 1, 0)
        want = one.stats()
        got = _stats(mc, w)
        assert {k: got[k] for k in want} == want, (w, got, want)
        assert np.array_equal(mc.conf(w), one.c), w
        assert mc.update_stats(w).sweeps_drawn == 2 and mc.update_stats(w).n_colours == 2
    st = mc.stats(1)
    assert (st.acc_local, st.prop_local, st.energy, st.magnetization) == (0, 2 * N, -2 * N, N)
    assert 0 < mc.stats(0).acc_local < 2 * N
    mc.close()


def test_with_the_rest_of_the_flavor_on(gpu):
    """8x8 with cluster moves every third sweep, ladders of 4 with a round every second, the binner and FSS"""
    from montecarlo_jl_amd import lattices
    l = gpu.SquareLattice(8)
    W, Rr, seed, therm, n, cap = 8, 4, 55, 3, 32, 100
    ladder = np.linspace(0.35, 0.5, Rr)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=ladder, n_walkers=W, seed=seed, thermalization=therm, cluster_moves=True,
                global_rate=3, n_replicas=Rr, exchange_rate=2, binning=True, binning_capacity=cap, fss=True,
                series_capacity=40, update="checkerboard")
    assert not mc.exchange_fused()  # rounds run as their launch in this mode
    for k in (5, 20, 7):
        mc.sweep(k)
    tables = fss_ref.q30(lattices._positions(l), mc.k_vectors)
    lad = ref.Ladders(l, np.tile(ladder, W // Rr), [seed + w for w in range(W)], n_replicas=Rr, series_capacity=40,
                      binning_capacity=cap, fss_tables=tables)
    lad.run(1, n, therm, 1, global_rate=3, exchange_rate=2)
    L, T = mc.binner_size()
    assert T == n - therm == lad.n_meas
    for w in range(W):
        _check_slot(mc, lad, w, "all")
        assert _gstats(mc, w) == lad.gs[w], w
        assert _xstats(mc, w) == lad.exchange_stats(w), w
        for lv in range(L):
            xs, x2, xy, cnt = mc.binner_level(w, lv)
            rs, r2, rxy, rc = lad.binner.sums(w, lv)
            assert cnt == rc, (w, lv)
            assert np.array_equal(xs, rs) and np.array_equal(x2, r2) and np.array_equal(xy, rxy), (w, lv)
        f = mc.fss_sums(w)
        assert (f.n_meas, f.n_k) == (lad.fss_n, 2), w
        assert f.sum_M4 == lad.fss_sums[w, 1], w
        np.testing.assert_allclose(np.array(f.sum_S[:2]), lad.fss_sums[w, 2:], rtol=1e-13, atol=0, err_msg=str(w))
        b = lad.fss_binners[w]
        for lv in range(L):
            xs, x2, xy, cnt = mc.fss_binner_level(w, lv)
            assert cnt == b.count[lv], (w, lv)
            np.testing.assert_allclose(xs, b.x_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
            np.testing.assert_allclose(x2, b.x2_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
            np.testing.assert_allclose(xy, b.xy_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
    assert mc.replicas().tolist() == lad.replica.tolist()
    assert sum(mc.exchange_stats(w).acc_exchange for w in range(W)) > 0
    assert sum(mc.global_stats(w).acc_global for w in range(W)) > 0
    mc.close()


def test_batch_and_split_independence(gpu):
    model = gpu.IsingModel(dims=2, L=8)
    kw = dict(beta=0.44, seed=300, thermalization=4, measure_rate=2, series_capacity=20, update="checkerboard")
    five = gpu.MC(model, n_walkers=5, **kw)
    one = gpu.MC(model, n_walkers=1, first_walker=3, **kw)
    five.sweep(30)
    for n in (7, 23):
        one.sweep(n)
    assert _stats(five, 3) == _stats(one, 0)
    assert np.array_equal(five.conf(3), one.conf(0))
    assert [list(x) for x in five.series(3)] == [list(x) for x in one.series(0)]
    assert five.update_stats(3).sweeps_drawn == one.update_stats(0).sweeps_drawn == 30
    five.close()
    one.close()


def test_switching_modes_between_sweeps(gpu):
    """10 sequential sweeps, 10 checkerboard, 10 sequential: the restatement switches where the handle does, so every
    leg starts from the previous leg's configuration, sums and cursors"""
    l = gpu.SquareLattice(8)
    W, seed = 4, 71
    betas = np.linspace(0.3, 0.5, W)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=W, seed=seed, thermalization=1, series_capacity=40)
    lad = ref.Ladders(l, betas, [seed + w for w in range(W)], series_capacity=40, update="sequential")
    first = 1
    for leg, kind in enumerate(("sequential", "checkerboard", "sequential")):
        if leg:
            mc.set_update(kind)
            lad.update = kind
        mc.sweep(10)
        lad.run(first, first + 9, 1, 1)
        first += 10
        for w in range(W):
            _check_slot(mc, lad, w, kind)
    for w in range(W):
        assert mc.update_stats(w).sweeps_drawn == 10 and mc.uniforms_used(w) > len(l)
    mc.close()


def test_the_default_is_unchanged(gpu):
    model = gpu.IsingModel(dims=2, L=8)
    kw = dict(beta=[0.3, 0.44, 0.6], n_walkers=3, seed=9, thermalization=5, measure_rate=2)
    named = gpu.MC(model, update="sequential", **kw)
    plain = gpu.MC(model, **kw)
    named.sweep(50)
    plain.sweep(50)
    for w in range(3):
        assert _stats(named, w) == _stats(plain, w)
        assert np.array_equal(named.conf(w), plain.conf(w))
        u = named.update_stats(w)
        assert (u.kind, u.n_colours, u.sweeps_drawn) == (0, 0, 0)
        one = R.Walker(gpu.SquareLattice(8), kw["beta"][w], 9 + w)  # the sequential chain of the reference
        one.run(1, 50, 5, 2, 0)
        want = one.stats()
        assert {k: _stats(plain, w)[k] for k in want} == want, w
        assert np.array_equal(plain.conf(w), one.c)
    named.close()
    plain.close()


def test_errors(gpu):
    l = gpu.SquareLattice(4)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=0.4, n_walkers=2, seed=1)
    bad = ref.greedy_colouring(l).copy()
    bad[5] = bad[4]  # sites 4 and 5 are neighbours
    with pytest.raises(gpu.DQMCError) as e:
        mc.set_update("checkerboard", bad)
    assert e.value.code == -1 and " 5 " in str(e.value) and "share colour" in str(e.value)  # (a pair with site 5)
    with pytest.raises(gpu.DQMCError) as e:  # 17 colours (a valid colouring otherwise)
        mc.set_update("checkerboard", np.arange(16) + 1)
    assert e.value.code == -1
    with pytest.raises(gpu.DQMCError) as e:
        gpu.MC(gpu.IsingModel(l=gpu.Chain(1)), beta=0.4, update="checkerboard", colouring=[0])
    assert e.value.code == -1
    assert mc.update_stats(0).kind == 0 and mc.update == "sequential"
    mc.sweep(3)  # the handle stays usable, in the mode it had
    assert mc.stats(0).prop_local == 48 and mc.update_stats(0).sweeps_drawn == 0
    mc.set_update("checkerboard", np.arange(16))  # 16 colours: the most there may be
    mc.sweep(3)
    u = mc.update_stats(1)
    assert (u.kind, u.n_colours, u.sweeps_drawn) == (1, 16, 3) and mc.stats(1).prop_local == 96
    lad = ref.Ladders(l, [0.4, 0.4], [1, 2], update="sequential")
    lad.run(1, 3, 0, 1)
    lad.update, lad.classes = "checkerboard", ref.classes(np.arange(16))
    lad.run(4, 6, 0, 1)
    for w in range(2):
        assert np.array_equal(mc.conf(w), lad.c[w]) and mc.stats(w).energy == lad.E[w]
    mc.close()


def test_4x4_exact_enumeration_on_the_device(gpu):
    """the run of test_ising_checkerboard.py on the device: the per-walker sums are the restatement's, so the 4.5 sigma
    check against the enumeration is a consequence"""
    l, lad = ref.enum_run()
    W = 3 * ref.ENUM_WB
    mc = gpu.MC(gpu.IsingModel(dims=2, L=4), beta=np.repeat(ref.ENUM_BETAS, ref.ENUM_WB), n_walkers=W,
                seed=ref.ENUM_SEED, thermalization=ref.ENUM_THERM, sweeps=ref.ENUM_SWEEPS, update="checkerboard")
    mc.run()
    sums = np.zeros((W, 4))
    for w in range(W):
        st = mc.stats(w)
        assert st.n_meas == ref.ENUM_SWEEPS
        sums[w] = (st.sum_E, st.sum_E2, st.sum_absM, st.sum_M2)
    assert np.array_equal(sums, lad.sums)
    ref.check_enum(sums, ref.ENUM_SWEEPS, l)
    mc.close()
