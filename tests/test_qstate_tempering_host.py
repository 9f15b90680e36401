"""Replica exchange and the binner of the q-state engine on the host, no GPU: detailed balance of the restated exchange
rule by enumeration, the rule's cases, split invariance of the restatement, the restated binner against the plain
LogBinnerRef, and the interface (header, exports, null handles, struct sizes, keyword validation)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_binner_ref as bref  # noqa: E402
import qstate_tempering_ref as tref  # noqa: E402
from logbinner_ref import LogBinnerRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- detailed balance
@pytest.mark.parametrize("case", ["ring3_potts3", "ring4_potts3", "ring3_clock5", "ring4_clock5"])
def test_the_exchange_satisfies_detailed_balance(mc_amd, case):
    """Every pair of configurations (i at beta_a, j at beta_b) of a small ring: pi(i, j) A(i, j) = pi(j, i) A(j, i) with
    pi = exp(-beta_a E_i - beta_b E_j) and A the restated acceptance (1, or the product p).  One of the two directions
    accepts with 1, the other with p, so the relative deviation is |p exp(-db d) - 1|: the header bounds it by the
    rounding of J factors and J products plus the error of exp itself, 2 J ulp to first order; the test allows
    (2 J + 4) 2^-53 max(1, |db d|), the 4 ulp for the exp calls of this test.  Largest deviation seen: ring3_potts3
    (J = 33) 4.4e-16, ring4_potts3 (J = 34) 4.4e-16, ring3_clock5 (J = 33) 6.7e-16, ring4_clock5 (J = 34) 1.6e-15, against
    bounds of 7.8e-15 and 8.0e-15."""
    N = 3 if "ring3" in case else 4
    q, table = (3, ref.potts_table(3)) if "potts3" in case else (5, ref.clock_table(5))
    l = mc_amd.Chain(N)
    e_q30 = ref.tables(q, table)[0]
    E = ref.state_energies_q30(l, q, e_q30, ref.all_states(N, q))
    J = tref.exchange_bits(len(l.bonds), e_q30)
    worst, decided = 0.0, 0
    for beta_a, beta_b in ((0.7, 1.1), (1.1, 0.7), (0.4, 0.4000001), (2.5, 0.1)):
        A = tref.exchange_matrix(E, beta_a, beta_b, J)
        db = beta_a - beta_b
        bound = (2 * J + 4) * 2.0 ** -53
        for Ei in np.unique(E):      # the acceptance depends on the energies alone
            for Ej in np.unique(E):
                i, j = int(np.flatnonzero(E == Ei)[0]), int(np.flatnonzero(E == Ej)[0])
                x = db * (int(Ei) - int(Ej)) / 2.0 ** 30   # log of pi(j, i) / pi(i, j)
                lhs, rhs = A[i, j], A[j, i] * math.exp(x)
                dev = abs(lhs / rhs - 1.0)
                worst = max(worst, dev)
                decided += A[i, j] < 1.0
                assert dev <= bound * max(1.0, abs(x)), (case, beta_a, beta_b, Ei, Ej, dev)
        assert np.all(A <= 1.0) and np.all(A > 0.0)
    print(case, "J", J, "largest deviation from detailed balance", worst)
    assert decided > 0


# ---- the rule's cases
def _walkers(mc_amd, betas, R, k, L=3, q=3, seed=50, binner=None, cap=0, table=None):
    l = mc_amd.SquareLattice(L)
    wk = tref.TemperingWalkers(l, q, ref.potts_table(q) if table is None else table, betas,
                               [seed + w for w in range(len(betas))], series_capacity=cap, binner=binner)
    wk.set_exchange(R, k)
    return wk


def test_pair_selection(mc_amd):
    assert tref.tried_pairs(0, 2, 2) == [0] and tref.tried_pairs(1, 2, 2) == []
    assert tref.tried_pairs(0, 3, 3) == [0] and tref.tried_pairs(1, 3, 3) == [1]  # R odd: the unpaired slot alternates
    assert tref.tried_pairs(0, 4, 8) == [0, 2, 4, 6] and tref.tried_pairs(1, 4, 8) == [1, 5]
    assert tref.tried_pairs(6, 5, 10) == [0, 2, 5, 7] and tref.tried_pairs(7, 5, 10) == [1, 3, 6, 8]
    assert tref.tried_pairs(0, 0, 4) == [] and tref.tried_pairs(3, 1, 4) == []


def test_the_rules_cases(mc_amd):
    """db == 0 and d == 0 swap without a draw, and so do equal signs; opposite signs decide by the product"""
    assert tref.rule(0.0, 5) == "swap" and tref.rule(0.3, 0) == "swap"
    assert tref.rule(0.3, 7) == "swap" and tref.rule(-0.3, -7) == "swap"
    assert tref.rule(0.3, -7) == "decide" and tref.rule(-0.3, 7) == "decide"
    # equal betas: every try swaps, and the labels walk through the ladder
    wk = _walkers(mc_amd, [0.8] * 3, 3, 1)
    before = wk.c.copy()
    wk.exchange()
    assert np.array_equal(wk.c[0], before[1]) and np.array_equal(wk.c[1], before[0]) and np.array_equal(wk.c[2], before[2])
    assert list(wk.replica) == [1, 0, 2] and wk.x == 1
    wk.exchange()
    assert list(wk.replica) == [1, 2, 0] and list(wk.prop_exchange) == [1, 1, 0] and list(wk.acc_exchange) == [1, 1, 0]
    E = wk.E.copy()
    wk.observables()
    assert np.array_equal(E, wk.E)  # E travelled with the configuration
    # non-monotone betas, R = W and several ladders: both outcomes of the product rule occur
    for betas, R in (([0.9, 1.1, 0.8, 1.0], 4), ([0.9, 1.1, 0.8, 1.0] * 3, 4), ([1.0, 0.9] * 4, 2)):
        wk = _walkers(mc_amd, betas, R, 1)
        wk.run(1, 40, 0, 1)
        assert wk.decided["acc"] > 0 and wk.decided["rej"] > 0 and wk.decided["free"] > 0, (betas, wk.decided)
        for lad in range(len(betas) // R):
            assert sorted(wk.replica[lad * R:(lad + 1) * R]) == list(range(R))
            assert wk.prop_exchange[lad * R + R - 1] == 0
        E = wk.E.copy()
        wk.observables()
        assert np.array_equal(E, wk.E)
        assert wk.x == 40 and np.all(wk.s == 40)


def test_split_invariance(mc_amd):
    """one call or any split of it: cluster_rate 2 and measure_rate 3 do not divide k = 5, thermalization 4"""
    betas = [0.9, 1.0, 1.1, 0.95] * 2

    def run(splits):
        wk = _walkers(mc_amd, betas, 4, 5, binner=20, cap=6)
        first = 1
        for n in splits:
            wk.run(first, n, 4, 3, cluster_rate=2)
            first += n
        return wk

    one = run([23])
    assert one.x == 4 and one.n_meas == 6 and one.bin.T == 6
    for splits in ([5, 5, 13], [1] * 23, [4, 1, 10, 8], [22, 1]):
        two = run(splits)
        for w in range(len(betas)):
            assert two.stats(w) == one.stats(w) and two.exchange_stats(w) == one.exchange_stats(w)
            assert two.cluster_stats(w) == one.cluster_stats(w) and two.ser[w] == one.ser[w]
        assert np.array_equal(two.c, one.c)
        for a, b in ((two.bin.x_sum, one.bin.x_sum), (two.bin.x2_sum, one.bin.x2_sum), (two.bin.xy_sum, one.bin.xy_sum)):
            assert np.array_equal(a, b)


def test_the_order_inside_a_sweep(mc_amd):
    """a round stands behind the cluster move and before the measurement: with equal betas the measurement of slot 0
    after sweep 1 is taken on the configuration slot 1 had after its sweep and move"""
    wk = _walkers(mc_amd, [0.9, 0.9], 2, 1, cap=4)
    plain = _walkers(mc_amd, [0.9, 0.9], 0, 0, cap=4)
    wk.run(1, 1, 0, 1, cluster_rate=1)
    plain.run(1, 1, 0, 1, cluster_rate=1)
    assert wk.ser[0] == plain.ser[1] and wk.ser[1] == plain.ser[0]
    assert np.array_equal(wk.c[0], plain.c[1]) and np.all(wk.m == 1) and np.all(plain.m == 1)


# ---- the binner
def test_the_restated_binner_is_the_plain_one_with_cross_sums(mc_amd):
    rng = np.random.default_rng(3)
    W, cap = 3, 21
    b = bref.QsBinnerRef(W, cap)
    plain = LogBinnerRef(6 * W, cap)
    samples = []
    for _ in range(cap):
        E, Mx, My = (rng.integers(-2 ** 34, 2 ** 34, W) for _ in range(3))
        x = bref.sample(E, Mx, My)
        samples.append(x)
        b.push_measurement(E, Mx, My)
        plain.push(x.reshape(-1))
    assert np.array_equal(b.x_sum, plain.x_sum) and np.array_equal(b.x2_sum, plain.x2_sum) and b.T == cap
    assert list(b.count) == [cap >> l for l in range(b.L)] and b.L == 5
    with pytest.raises(OverflowError):
        b.push_measurement(E, Mx, My)
    # level 1 holds the averages of consecutive pairs: its cross sums are the sums of their products
    s = np.array(samples)                                   # [T][6][W]
    lvl1 = 0.5 * (s[0:cap - 1:2] + s[1:cap:2])
    want = (lvl1[:, 0::2] * lvl1[:, 1::2]).sum(axis=0)
    assert np.allclose(b.xy_sum[1].reshape(3, W), want, rtol=1e-14)
    assert np.array_equal(b.x_sum[0].reshape(6, W)[3], b.x_sum[0].reshape(6, W)[4])  # M2 twice
    f = b.finish(1, 1)
    assert f["count"] == cap >> 1 and np.isfinite(f["covN"]).all() and np.isfinite(f["tau"]).all()
    n = float(cap >> 1)
    assert abs(f["covN"][2] - np.cov(lvl1[:, 4, 1], lvl1[:, 5, 1])[0, 1] / n) <= 1e-10 * abs(f["covN"][2])
    assert b.finish(0)["level"] == 0  # no level with 32 values


# ---- the interface
NEW = ["dqmc_qs_set_exchange", "dqmc_qs_exchange", "dqmc_qs_get_exchange_stats", "dqmc_qs_binner_enable",
       "dqmc_qs_binner_size", "dqmc_qs_binner_reliable_level", "dqmc_qs_binner_get_level", "dqmc_qs_binner_finish"]


def test_the_header_declares_and_the_library_exports_the_abi(mc_amd):
    from montecarlo_jl_amd import _lib
    src = open(os.path.join(ROOT, "include", "dqmc_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"^int %s\(dqmc_qs_handle \*h" % name, src, re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for text in ("Replica exchange (dqmc_qs_set_exchange", "Order inside a sweep", "Binner (dqmc_qs_binner_enable",
                 "P(key_a; 0, low32(x), 7, high32(x))", "2 J ulp"):
        assert text in src, text
    # null handles are refused, with the message where dqmc_qs_last_error(NULL) finds it
    calls = {"dqmc_qs_set_exchange": (2, 1), "dqmc_qs_exchange": (), "dqmc_qs_get_exchange_stats": (0, None),
             "dqmc_qs_binner_enable": (8,), "dqmc_qs_binner_size": (None, None), "dqmc_qs_binner_reliable_level": (None,),
             "dqmc_qs_binner_get_level": (0, 0, None, None, None, None), "dqmc_qs_binner_finish": (0, -1, None)}
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == _lib.ERR_INVALID, name
        assert lib.dqmc_qs_last_error(None).decode() == name + ": null handle"
    # the structs mirror the header
    assert C.sizeof(_lib.QsExchangeStats) == 32 and C.sizeof(_lib.QsBinned) == (4 * 6 + 3) * 8 + 16
    assert [f for f, _ in _lib.QsExchangeStats._fields_] == ["prop_exchange", "acc_exchange", "replica", "rounds"]
    assert [f for f, _ in _lib.QsBinned._fields_] == ["mean", "varN", "varN0", "tau", "covN", "count", "level"]
    for struct, fields in (("dqmc_qs_exchange_stats", "int64_t prop_exchange, acc_exchange;"),
                           ("dqmc_qs_binned", "double covN[3];")):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, src).group(1)
        assert fields in body, struct


def test_keywords_are_validated_before_any_device_is_touched(mc_amd):
    m = mc_amd.PottsModel(3, dims=2, L=4)
    for bad in ((2,), 3, (2, -1), (-2, 1), (2.5, 1), (True, 1), "ab"):
        with pytest.raises(ValueError, match="tempering"):
            mc_amd.MC(m, beta=1.0, n_walkers=4, tempering=bad)
    with pytest.raises(ValueError, match="not a multiple"):
        mc_amd.MC(m, beta=1.0, n_walkers=5, tempering=(2, 1))
    for bad in (0, -3, 2.5, "x"):
        with pytest.raises(ValueError, match="binner"):
            mc_amd.MC(m, beta=1.0, binner=bad)
    # the Ising keywords are still refused, and the message names the new ones
    for kw in ({"n_replicas": 2}, {"exchange_rate": 2}, {"binning": True}, {"fss": True}):
        with pytest.raises(NotImplementedError, match="IsingModel only") as ei:
            mc_amd.MC(m, beta=1.0, **kw)
        assert "tempering=(R, k)" in str(ei.value) and "binner=True | capacity" in str(ei.value)
    for name in ("set_exchange", "exchange", "exchange_stats", "replicas", "enable_binning", "binner_size",
                 "binner_reliable_level", "binner_level", "binner_finish", "binned"):
        assert callable(getattr(mc_amd.QStateMC, name)), name
