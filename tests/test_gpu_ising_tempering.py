"""The Ising flavor's replica exchange on the MI355X (the round fused into ising_sweep_kernel / ising_sweep_binned_kernel
where 64 % R == 0, ising_exchange_kernel otherwise, behind a cluster move and by hand): bit-exact against the
restatement (ising_tempering_ref.py) for every slot, the two forms against each other, independence of the split, the
order with cluster moves, the binner, off is off, set_beta, the refusals, and 4x4 ladders against exact enumeration."""
import numpy as np
import pytest

import ising_tempering_ref as T
from ising_binner_ref import from_series
from test_gpu_ising import _exact_4x4

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "acc_local", "prop_local", "uniforms_used",
               "energy", "magnetization")
GLOBAL_FIELDS = ("prop_global", "acc_global", "sum_cluster_size", "moves_drawn")
EXCHANGE_FIELDS = ("prop_exchange", "acc_exchange", "replica", "rounds")
SEED = 4321

LATTICES = {
    "square4": lambda g: g.SquareLattice(4),     # N = 16, one word
    "square8": lambda g: g.SquareLattice(8),     # two words: multi-word swap
    "chain33": lambda g: g.Chain(33),            # partial last word
    "cubic3": lambda g: g.CubicLattice(3, 3),    # z = 6
}
# (R, walkers, fused): two waves; last wave partly empty; whole wave; a ladder across the wave boundary; R > 64
LADDERS = {"R4": (4, 128, True), "R8": (8, 72, True), "R64": (64, 64, True), "R3": (3, 66, False),
           "R128": (128, 128, False)}


def ladder_betas(R):
    """R betas in 0.30 .. 0.60: steps of 0.04 for R <= 4, a fixed permutation of an even grid above (neighbouring slots
    then differ by a few hundredths at least; the rule does not ask for monotone betas).  Chosen so that draws decide
    both ways in both parities within twenty sweeps from random configurations, which each test asserts on the
    restatement."""
    if R <= 4:
        return [0.30 + 0.04 * i for i in range(R)]
    return [0.30 + 0.30 * ((37 * i) % R) / (R - 1) for i in range(R)]


def _state(mc, w):
    st, x, g = mc.stats(w), mc.exchange_stats(w), mc.global_stats(w)
    return ({f: getattr(st, f) for f in STAT_FIELDS}, {f: getattr(x, f) for f in EXCHANGE_FIELDS},
            {f: getattr(g, f) for f in GLOBAL_FIELDS}, mc.conf(w).tolist())


def _ref_state(lad, w):
    return lad.stats(w), lad.exchange_stats(w), lad.gs[w], lad.c[w].tolist()


def _assert_equals_ref(label, mc, lad):
    assert np.array_equal(mc.replicas(), lad.replica), label
    for w in range(lad.W):
        assert _state(mc, w) == _ref_state(lad, w), (label, w)
        e, m = mc.series(w)
        assert list(e) == lad.serE[w] and list(m) == lad.serM[w], (label, w)


def _assert_same(label, a, b):
    for w in range(a.n_walkers):
        assert _state(a, w) == _state(b, w), (label, w)


_refs = {}


def reference(g, lattice, R, W, rate, sweeps=20, therm=0, measure_rate=2, global_rate=0, cap=10):
    """the restatement's run of one case, computed once and shared (read-only)"""
    key = (lattice, R, W, rate, sweeps, therm, measure_rate, global_rate, cap)
    if key not in _refs:
        lad = T.Ladders(LATTICES[lattice](g), ladder_betas(R) * (W // R), [SEED + w for w in range(W)], n_replicas=R,
                        series_capacity=cap)
        lad.run(1, sweeps, therm, measure_rate, global_rate, rate)
        _refs[key] = lad
    return _refs[key]


def _mc(g, lattice, R, W, rate, therm=0, measure_rate=2, cap=10, **kw):
    return g.MC(g.IsingModel(l=LATTICES[lattice](g)), beta=ladder_betas(R), n_walkers=W, seed=SEED, thermalization=therm,
                measure_rate=measure_rate, series_capacity=cap, n_replicas=R, exchange_rate=rate, **kw)


PARITY_CASES = [("square8", k) for k in LADDERS] + [(l, k) for l in ("square4", "chain33", "cubic3") for k in ("R4", "R3")]


@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("lattice,ladder", PARITY_CASES)
def test_twenty_sweeps_match_the_restatement_bit_exactly(gpu, lattice, ladder, rate):
    R, W, fused = LADDERS[ladder]
    lad = reference(gpu, lattice, R, W, rate)
    for parity in (0, 1):  # the case decides something: draws that accept and draws that refuse, in both parities
        assert lad.drawn[parity][0] >= 1 and lad.drawn[parity][1] >= 1, (lattice, ladder, rate, lad.drawn)
    assert lad.rounds == 20 // rate and lad.n_meas == 10
    mc = _mc(gpu, lattice, R, W, rate)
    assert mc.exchange_fused() == fused
    mc.sweep(20)
    _assert_equals_ref((lattice, ladder, rate), mc, lad)
    a = mc.analysis(0)
    x = mc.exchange_stats(0)
    assert (a["prop_exchange"], a["acc_exchange"]) == (x.prop_exchange, x.acc_exchange)
    assert a["acc_rate_exchange"] == x.acc_exchange / x.prop_exchange
    for w in range(R - 1, W, R):  # the last slot of a ladder has no pair of its own
        assert mc.exchange_stats(w).prop_exchange == 0
    for w in (0, W - 1):          # E and M moved with the spins
        c, st = mc.conf(w), mc.stats(w)
        assert st.energy == mc.model.energy(c) and st.magnetization == int(c.sum())
    mc.close()


def test_the_fused_round_equals_the_round_by_hand(gpu):
    """R = 4: sweeps with exchange_rate = 1 (the round inside the sweep kernel) against sweep(1) without exchange
    followed by exchange(), twenty times (no measurements: by hand the round would follow the sweep's measurement)"""
    a = _mc(gpu, "square8", 4, 128, 1, therm=10 ** 6)
    b = _mc(gpu, "square8", 4, 128, 0, therm=10 ** 6)
    assert a.exchange_fused() and not b.exchange_fused()
    a.sweep(20)
    for _ in range(20):
        b.sweep(1)
        b.exchange()
    assert a.exchange_stats(0).rounds == 20 and sum(a.exchange_stats(w).acc_exchange for w in range(128)) > 0
    _assert_same("fused / by hand", a, b)
    assert np.array_equal(a.replicas(), b.replicas()) and len(set(a.replicas()[:4])) == 4
    a.close()
    b.close()


@pytest.mark.parametrize("ladder", ["R4", "R3"])
def test_results_do_not_depend_on_the_split(gpu, ladder):
    R, W, fused = LADDERS[ladder]
    whole, parts = _mc(gpu, "square8", R, W, 3), _mc(gpu, "square8", R, W, 3)
    assert whole.exchange_fused() == fused
    whole.sweep(20)
    parts.sweep(7)
    parts.sweep(13)
    _assert_same(ladder, whole, parts)
    _assert_equals_ref(ladder, parts, reference(gpu, "square8", R, W, 3))
    whole.close()
    parts.close()


@pytest.mark.parametrize("rate", [2, 3])
@pytest.mark.parametrize("R,W", [(4, 24), (3, 24)])
def test_with_cluster_moves_the_order_is_local_wolff_exchange_measure(gpu, R, W, rate):
    lad = reference(gpu, "square8", R, W, rate, global_rate=2)
    assert sum(g["acc_global"] for g in lad.gs) > 0 and lad.acc_x.sum() > 0
    mc = _mc(gpu, "square8", R, W, rate, cluster_moves=True, global_rate=2)
    mc.sweep(9)
    mc.sweep(11)
    _assert_equals_ref((R, rate), mc, lad)
    assert mc.global_stats(0).prop_global == 10 and mc.exchange_stats(0).rounds == 20 // rate
    mc.close()


@pytest.mark.parametrize("R,W,rate,global_rate", [(4, 72, 1, 0), (3, 66, 1, 0), (4, 24, 2, 2)])
def test_with_binning_every_level_of_every_slot(gpu, R, W, rate, global_rate):
    """the fused round in ising_sweep_binned_kernel, the measurement ising_exchange_kernel takes, and a round behind a
    cluster move: each slot's binner holds the restated binner of that slot's series"""
    lad = reference(gpu, "square8", R, W, rate, global_rate=global_rate)
    ref = from_series(np.array(lad.serE).T, np.array(lad.serM).T, 12)
    mc = _mc(gpu, "square8", R, W, rate, binning=True, binning_capacity=12, cluster_moves=global_rate > 0,
             global_rate=global_rate or 5)
    mc.sweep(6)
    mc.sweep(14)
    _assert_equals_ref((R, rate), mc, lad)
    L, n = mc.binner_size()
    assert (L, n) == (ref.L, 10)
    for w in range(W):
        for lv in range(L):
            xs, x2, xy, cnt = mc.binner_level(w, lv)
            rs, r2, rxy, rc = ref.sums(w, lv)
            assert cnt == rc, (w, lv)
            assert np.array_equal(xs, rs) and np.array_equal(x2, r2) and np.array_equal(xy, rxy), (w, lv)
    mc.close()


def test_off_is_off(gpu):
    kw = dict(beta=ladder_betas(4) * 16, n_walkers=64, seed=SEED, measure_rate=2, series_capacity=10)
    model = gpu.IsingModel(l=gpu.SquareLattice(8))
    plain = gpu.MC(model, **kw)
    plain.sweep(20)
    for R, rate in ((4, 0), (0, 3), (1, 3)):
        mc = gpu.MC(model, **kw)
        mc.set_exchange(4, 1)
        mc.set_exchange(R, rate)
        assert not mc.exchange_fused()
        mc.sweep(20)
        for w in range(64):
            assert _state(mc, w)[0] == _state(plain, w)[0] and _state(mc, w)[3] == _state(plain, w)[3], (R, rate, w)
            x = mc.exchange_stats(w)
            assert (x.prop_exchange, x.acc_exchange, x.rounds) == (0, 0, 0)
        mc.close()
    plain.close()


@pytest.mark.parametrize("ladder", ["R4", "R3"])
def test_set_beta_after_set_exchange_rebuilds_the_pair_tables(gpu, ladder):
    R, W, _ = LADDERS[ladder]
    l = LATTICES["square8"](gpu)
    lad = T.Ladders(l, ladder_betas(R) * (W // R), [SEED + w for w in range(W)], n_replicas=R, series_capacity=10)
    mc = _mc(gpu, "square8", R, W, 1)
    for w, beta in ((0, 0.52), (R - 1, 0.33), (R + 1, 0.41), (W - 1, 0.47), (W - 2, 0.47)):
        mc.set_beta(w, beta)
        lad.set_beta(w, beta)
    mc.sweep(20)
    lad.run(1, 20, 0, 2, 0, 1)
    assert min(lad.drawn[0] + lad.drawn[1]) >= 1
    _assert_equals_ref(ladder, mc, lad)
    mc.close()


def test_refusals(gpu):
    model = gpu.IsingModel(l=gpu.SquareLattice(4))
    with pytest.raises(gpu.DQMCError, match="multiple of n_replicas"):
        gpu.MC(model, beta=0.4, n_walkers=10, n_replicas=4, exchange_rate=1)
    with pytest.raises(gpu.DQMCError, match="must be >= 0"):
        gpu.MC(model, beta=0.4, n_walkers=8, n_replicas=4, exchange_rate=-1)
    mc = gpu.MC(model, beta=0.4, n_walkers=8)
    with pytest.raises(gpu.DQMCError, match="dqmc_mc_exchange: no ladders") as e:
        mc.exchange()
    assert e.value.code == -4
    with pytest.raises(gpu.DQMCError, match="out of range"):
        mc.exchange_stats(8)
    mc.set_exchange(4, 0)
    mc.exchange()  # ladders without a rate: by hand only
    assert mc.exchange_stats(0).rounds == 1 and mc.exchange_stats(0).prop_exchange == 1
    mc.close()


def test_4x4_ladders_against_exact_enumeration(gpu):
    """SquareLattice(4), R = 8, betas 0.25 .. 0.60, 64 ladders, 200 + 2000 sweeps with a round after each: per
    temperature the means of E and |M| over the 64 independent ladders against the 2^16 states, |z| < 5 with the
    cross-ladder standard error (the restatement, which the device follows bit for bit, gives max |z| = 1.61 with this
    seed)"""
    R, W = 8, 512
    betas = np.linspace(0.25, 0.60, R)
    mc = gpu.MC(gpu.IsingModel(dims=2, L=4), beta=betas, n_walkers=W, seed=2024, thermalization=200, sweeps=2000,
                n_replicas=R, exchange_rate=1)
    assert mc.exchange_fused()
    mc.run()
    stats = [mc.stats(w) for w in range(W)]
    assert all(st.n_meas == 2000 for st in stats) and mc.exchange_stats(0).rounds == 2200
    for i in range(R):
        assert mc.betas[i] == betas[i]
        ex = _exact_4x4(betas[i])
        for name, field in (("E", "sum_E"), ("M", "sum_absM")):
            v = np.array([getattr(stats[w], field) / 2000 for w in range(i, W, R)])
            se = v.std(ddof=1) / np.sqrt(len(v))
            z = (v.mean() - ex[name]) / se
            print("beta %.2f %s mean %.5f exact %.5f se %.5f z %+.2f" % (betas[i], name, v.mean(), ex[name], se, z))
            assert abs(z) < 5, (i, name, v.mean(), ex[name], se)
    labels = mc.replicas().reshape(-1, R)
    assert all(sorted(row) == list(range(R)) for row in labels)  # a permutation within every ladder
    mc.close()
