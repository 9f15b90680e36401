"""The Ising flavor's replica exchange without a device: the restatement (ising_tempering_ref.py) against the
single-walker restatement it is built on, the product rule against exp, exact stationarity of the exchange step as
defined on all joint states of two Chain(4) replicas, and the ABI surface."""
import ctypes as C
import decimal
import math

import numpy as np
import pytest

import ising_tempering_ref as T
import ising_wolff_ref as R


def test_per_key_philox_and_the_vectorised_sweep_equal_the_single_walker_restatement(mc_amd):
    keys = np.array([0, 5, 2 ** 32 + 7, 0xDEADBEEFCAFEF00D], dtype=np.uint64)
    idx = np.array([0, 4095, 2 ** 32, 2 ** 40 + 3], dtype=np.uint64)
    assert np.array_equal(T.philox_keys(keys, idx), [float(R.local_uniform(int(k), int(i))) for k, i in zip(keys, idx)])
    l = mc_amd.SquareLattice(4)
    betas = [0.2, 0.44, 0.7]
    lad = T.Ladders(l, betas, [91, 92, 93], series_capacity=4)
    lad.run(1, 12, 2, 3, global_rate=4)
    for w, b in enumerate(betas):
        ref = R.Walker(l, b, 91 + w, series_capacity=4)
        ref.run(1, 12, 2, 3, 4)
        assert lad.stats(w) == ref.stats(), w
        assert lad.gs[w] == ref.gs and np.array_equal(lad.c[w], ref.c)
        assert lad.serE[w] == ref.serE and lad.serM[w] == ref.serM


def test_rounds_pairs_labels_and_what_stays_with_the_slot(mc_amd):
    """R = 5, two ladders: even rounds try (0,1), (2,3), odd rounds (1,2), (3,4); no pair crosses a ladder; beta = const
    makes every try a swap, so the labels follow the odd-even transposition sort's permutation; keys, cursors and sums
    stay with the slot"""
    l = mc_amd.Chain(6)
    lad = T.Ladders(l, [0.4] * 10, range(10), n_replicas=5)
    conf0, E0, draw0 = lad.c.copy(), lad.E.copy(), lad.draw.copy()
    lad.exchange_round()
    assert list(lad.prop_x) == [1, 0, 1, 0, 0] * 2 and list(lad.acc_x) == [1, 0, 1, 0, 0] * 2
    assert list(lad.replica) == [1, 0, 3, 2, 4] * 2
    assert np.array_equal(lad.c[[1, 0, 3, 2, 4, 6, 5, 8, 7, 9]], conf0) and np.array_equal(lad.E[[1, 0, 3, 2, 4]], E0[:5])
    lad.exchange_round()
    assert list(lad.prop_x) == [1, 1, 1, 1, 0] * 2
    assert list(lad.replica) == [1, 3, 0, 4, 2] * 2
    assert lad.rounds == 2 and np.array_equal(lad.draw, draw0) and lad.drawn == [[0, 0], [0, 0]]
    assert all(g["moves_drawn"] == 0 for g in lad.gs)


def test_the_product_rule_is_exp_within_its_rounding():
    """p = prod q[j] over the bits of |d| against exp(-2 |db| |d|) in 50 digits: 17 factors, each an exp of an exact
    argument within 1 ulp, and 16 products within half an ulp each: 25 ulp at the most, 2^-52 each"""
    decimal.getcontext().prec = 50
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(300):
        db = float(rng.uniform(1e-4, 0.4)) * (1 if rng.random() < 0.5 else -1)
        sgn, q = T.pair_table(0.3 + db, 0.3, 65536)
        db = (0.3 + db) - 0.3
        assert len(q) == 17 and sgn == (1 if db > 0 else -1)
        d = int(rng.integers(1, 1 << int(rng.integers(1, 17))))
        p = T.product_rule(q, d)
        exact = (decimal.Decimal(-2) * abs(decimal.Decimal(db)) * d).exp()
        if exact > decimal.Decimal("1e-290"):
            worst = max(worst, abs(float((decimal.Decimal(p) - exact) / exact)))
    assert 0.0 < worst <= 25 * 2.0 ** -52, worst
    assert T.pair_table(0.4, 0.4, 16) == (0, [1.0] * 5)
    assert len(T.pair_table(0.4, 0.5, 15)[1]) == 4 and len(T.pair_table(0.4, 0.5, 16)[1]) == 5  # 2^J > n_bonds


@pytest.mark.parametrize("ba,bb", [(0.3, 0.6), (0.6, 0.3), (0.44, 0.44), (0.0, 1.5), (2.0, 0.1)])
def test_the_exchange_step_leaves_the_product_distribution_stationary(mc_amd, ba, bb):
    """Chain(4), two replicas, all 16 x 16 joint states (s in slot a, t in slot b): the step moves (s, t) to (t, s) with
    the rule's probability (1, or the product-rule p) and stays otherwise; pi_ba (x) pi_bb is stationary to 1e-12, and
    the flows between (s, t) and (t, s) balance"""
    l = mc_amd.Chain(4)
    bonds0 = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
    n = 16
    E = np.array([R.energy(np.array([1 if (s >> i) & 1 else -1 for i in range(4)]), bonds0) for s in range(n)])
    assert set(E % 2) == {len(bonds0) % 2}
    sgn, q = T.pair_table(ba, bb, len(bonds0))
    P = np.zeros((n * n, n * n))
    for s in range(n):
        for t in range(n):
            d = int(E[s] - E[t]) // 2
            p = 1.0 if (sgn == 0 or d == 0 or (d > 0) == (sgn > 0)) else T.product_rule(q, d)
            P[s * n + t, t * n + s] += p
            P[s * n + t, s * n + t] += 1.0 - p
    pa, pb = np.exp(-ba * (E - E.min())), np.exp(-bb * (E - E.min()))
    pi = np.outer(pa / pa.sum(), pb / pb.sum()).reshape(-1)
    assert np.allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.max(np.abs(pi @ P - pi)) <= 1e-12
    flow = pi[:, None] * P
    assert np.max(np.abs(flow - flow.T)) <= 1e-12
    if ba != bb:
        assert np.count_nonzero((P > 0) & (P < 1)) > 0  # some pairs are decided by a draw


def test_abi_surface(mc_amd):
    """the four entry points are exported by the library and declared in the header, and the struct mirrors it"""
    from montecarlo_jl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    src = open(_lib.HEADER_PATH).read()
    for name in ("dqmc_mc_set_exchange", "dqmc_mc_exchange", "dqmc_mc_get_exchange_stats", "dqmc_mc_exchange_fused"):
        assert hasattr(L, name), name
        assert ("int %s(dqmc_mc_handle *h" % name) in src, name
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.McExchangeStats) == 32
    assert [f for f, _ in _lib.McExchangeStats._fields_] == ["prop_exchange", "acc_exchange", "replica", "rounds"]
    assert "int64_t prop_exchange, acc_exchange;" in src and "int64_t replica;" in src and "uint64_t rounds;" in src
    assert "dqmc_mc_exchange_stats;" in src


def test_argument_checks_without_a_device(mc_amd):
    from montecarlo_jl_amd import _lib
    L = _lib.lib()
    st = _lib.McExchangeStats()
    f = C.c_int32()
    assert L.dqmc_mc_set_exchange(None, 2, 1) == _lib.ERR_INVALID
    assert b"dqmc_mc_set_exchange: null handle" in L.dqmc_mc_last_error(None)
    assert L.dqmc_mc_exchange(None) == _lib.ERR_INVALID
    assert b"dqmc_mc_exchange: null handle" in L.dqmc_mc_last_error(None)
    assert L.dqmc_mc_get_exchange_stats(None, 0, C.byref(st)) == _lib.ERR_INVALID
    assert L.dqmc_mc_exchange_fused(None, C.byref(f)) == _lib.ERR_INVALID
    model = mc_amd.IsingModel(dims=2, L=4)
    with pytest.raises(ValueError, match="n_replicas and exchange_rate"):
        mc_amd.MC(model, beta=0.4, n_walkers=4, n_replicas=2.5, exchange_rate=1)
    with pytest.raises(ValueError, match="n_replicas and exchange_rate"):
        mc_amd.MC(model, beta=0.4, n_walkers=4, n_replicas=2, exchange_rate=0.5)
    assert math.isfinite(T.exchange_uniform(7, 2 ** 40 + 1))
