"""Replica exchange of the q-state engine on the device (csrc/qstate.hip: qs_exchange_kernel, the DEFER forms of the sweep
kernel) against the numpy restatement of tests/qstate_tempering_ref.py, written from include/dqmc_hip.h.

Compared with ==: the states, E_int, Mx, My, the labels, all counters and cursors, sum_E, sum_E2, sum_M2, sum_M4, the series
and the binner sums of the elements without a square root; at 1e-13 relative: sum_absM, the |M| elements of the binner and
its (|M|, M2) cross sum (the rule of test_gpu_qstate.py for the device's sqrt)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_binner_ref as bref  # noqa: E402
import qstate_tempering_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu


def _table(kind, q):
    return ref.potts_table(q) if kind == "potts" else ref.clock_table(q)


def _model(g, kind, q, l):
    return g.PottsModel(q, l=l) if kind == "potts" else g.ClockModel(q, l=l)


def _close(a, b):
    return abs(a - b) <= 1e-13 * abs(b)


def check_binner(mc, wk, label):
    L, T = mc.binner_size()
    assert (L, T) == (wk.bin.L, wk.bin.T), label
    assert mc.binner_reliable_level() == wk.bin.reliable_level(), label
    for w in range(wk.W):
        for l in range(L):
            xs, x2, xy, n = mc.binner_level(w, l)
            rxs, rx2, rxy, rn = wk.bin.level(w, l)
            assert n == rn, (label, w, l)
            for k in range(bref.N_ELEM):
                if k in bref.SQRT_ELEMENTS:
                    assert _close(xs[k], rxs[k]) and _close(x2[k], rx2[k]), (label, w, l, k)
                else:
                    assert xs[k] == rxs[k] and x2[k] == rx2[k], (label, w, l, k, xs[k], rxs[k])
            for p in range(bref.N_PAIRS):
                assert _close(xy[p], rxy[p]) if p in bref.SQRT_PAIRS else xy[p] == rxy[p], (label, w, l, p)


def check(mc, wk, label):
    for w in range(wk.W):
        want, want_absM = wk.stats(w)
        st = mc.stats(w)
        got = {k: getattr(st, k) for k in want}
        assert got == want, (label, w, got, want)
        assert abs(st.sum_absM - want_absM) <= 1e-13 * abs(want_absM), (label, w, st.sum_absM, want_absM)
        cl, want_cl = mc.cluster_stats(w), wk.cluster_stats(w)
        assert {k: getattr(cl, k) for k in want_cl} == want_cl, (label, w)
        x, want_x = mc.exchange_stats(w), wk.exchange_stats(w)
        assert {k: getattr(x, k) for k in want_x} == want_x, (label, w, want_x)
        assert np.array_equal(mc.conf(w), wk.c[w]), (label, w)
        e, mx, my = mc.series(w)
        assert list(zip(e.tolist(), mx.tolist(), my.tolist())) == wk.ser[w], (label, w)
    assert np.array_equal(mc.replicas(), wk.replica), label
    if wk.bin is not None:
        check_binner(mc, wk, label)


def pair(g, l, kind, q, betas, R, k, seed=300, cap=8, binner=None, cluster_rate=0, **kw):
    """a handle and its restatement"""
    W = len(betas)
    mc = g.MC(_model(g, kind, q, l), beta=betas, n_walkers=W, seed=seed, series_capacity=cap, cluster_rate=cluster_rate,
              tempering=(R, k) if R or k else None, binner=binner if binner else False, **kw)
    assert type(mc) is g.QStateMC and (mc.n_replicas, mc.exchange_rate) == (R, k)
    wk = tref.TemperingWalkers(l, q, _table(kind, q), betas, [seed + w for w in range(W)], series_capacity=cap,
                               binner=binner)
    wk.set_exchange(R, k)
    return mc, wk


# name -> (lattice, kind, q, one ladder's betas, ladders, sweeps)
CASES = {
    "square3_potts2_R2": (lambda g: g.SquareLattice(3), "potts", 2, [0.40, 0.47], 1, 16),             # My = 0, W = R
    "square3_potts3_R3_desc": (lambda g: g.SquareLattice(3), "potts", 3, [1.10, 1.00, 0.90], 4, 12),  # W = 4 R, R odd
    "square4_clock5_R4_mixed": (lambda g: g.SquareLattice(4), "clock", 5, [0.9, 1.1, 0.8, 1.0], 1, 12),  # full product
    "triangular4_potts3_R4_equal": (lambda g: g.TriangularLattice(4), "potts", 3, [0.55, 0.63, 0.63, 0.70], 4, 12),
    "square4_clock64_R2": (lambda g: g.SquareLattice(4), "clock", 64, [1.0, 1.3], 2, 16),             # the largest table
    "square36_potts3_R2": (lambda g: g.SquareLattice(36), "potts", 3, [1.000, 1.015], 4, 6),         # Nw = 324 > 256
    "square36_clock5_R3": (lambda g: g.SquareLattice(36), "clock", 5, [1.100, 1.115, 1.130], 3, 6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_parity_on_the_shapes_where_the_kernels_can_go_wrong(gpu, name):
    """a round behind every sweep, a cluster move behind every second, every second sweep measured; the betas are close
    enough that the product rule both accepts and rejects (asserted on the restatement, which the device then equals)"""
    make, kind, q, ladder, n_ladders, n = CASES[name]
    l = make(gpu)
    R = len(ladder)
    mc, wk = pair(gpu, l, kind, q, ladder * n_ladders, R, 1, cluster_rate=2, measure_rate=2)
    mc.sweep(n)
    wk.run(1, n, 0, 2, cluster_rate=2)
    print(name, "decisions", wk.decided, "Nw", (len(l) + 3) // 4)
    assert wk.decided["acc"] > 0 and wk.decided["rej"] > 0, (name, wk.decided)
    check(mc, wk, name)
    assert mc.exchange_stats(0).rounds == n and mc.stats(0).n_meas == n // 2
    mc.close()


@pytest.mark.parametrize("binner", [None, 64])
@pytest.mark.parametrize("k,cluster_rate,measure_rate,therm", [(2, 2, 2, 0), (3, 0, 2, 0), (1, 2, 5, 3), (2, 0, 1, 3),
                                                               (3, 2, 1, 0)])
def test_order_and_deferral(gpu, k, cluster_rate, measure_rate, therm, binner):
    """(2, 2, 2, 0): move, round and measurement on one sweep; (3, 0, 2, 0): a round's sweep unmeasured (3), measured (6),
    a measured sweep without a round (2, 4); (1, 2, 5, 3): every sweep has a round, few are measured; (2, 0, 1, 3) and
    (3, 2, 1, 0): every sweep past the thermalization measured, by both kernels in turn"""
    l = gpu.SquareLattice(4)
    betas = [0.9, 1.0, 1.1] * 2
    mc, wk = pair(gpu, l, "clock", 5, betas, 3, k, cluster_rate=cluster_rate, measure_rate=measure_rate,
                  thermalization=therm, binner=binner)
    mc.sweep(13)
    wk.run(1, 13, therm, measure_rate, cluster_rate=cluster_rate)
    assert wk.decided["acc"] + wk.decided["rej"] > 0 and wk.n_meas > 0
    check(mc, wk, (k, cluster_rate, measure_rate, therm, binner))
    mc.close()


def test_a_run_does_not_depend_on_how_it_is_split(gpu):
    l = gpu.TriangularLattice(4)
    betas = [0.5, 0.6, 0.7, 0.65]
    kw = dict(cluster_rate=2, measure_rate=3, thermalization=4, binner=32)
    one, wk = pair(gpu, l, "potts", 3, betas, 4, 5, **kw)
    two, _ = pair(gpu, l, "potts", 3, betas, 4, 5, **kw)
    one.sweep(23)
    for n in (4, 1, 10, 8):
        two.sweep(n)
    wk.run(1, 23, 4, 3, cluster_rate=2)
    assert wk.x == 4 and wk.n_meas == 6
    check(one, wk, "one call")
    check(two, wk, "four calls")
    one.close()
    two.close()


def test_rounds_by_hand_and_set_beta(gpu):
    """exchange() between sweeps takes no measurement; set_beta after set_exchange rebuilds the tables of the slot's pairs;
    a ladder the handle's walkers do not fill is refused"""
    l = gpu.SquareLattice(3)
    betas = [0.7, 1.0, 1.3, 1.6]
    mc, wk = pair(gpu, l, "potts", 3, betas, 4, 0)
    for step in range(6):
        mc.sweep(2)
        wk.run(1 + 2 * step, 2, 0, 1)
        mc.exchange()
        wk.exchange()
        if step == 2:  # the middle slot of three moves: both of its pairs get new tables
            mc.set_beta(1, 1.15)
            wk.set_beta(1, 1.15)
            mc.set_beta(3, 0.95)
            wk.set_beta(3, 0.95)
    assert wk.decided["acc"] > 0 and wk.decided["rej"] > 0, wk.decided
    check(mc, wk, "by hand")
    assert mc.stats(0).n_meas == 12 and mc.exchange_stats(0).rounds == 6
    with pytest.raises(gpu.DQMCError) as ei:
        mc.set_exchange(3, 1)
    assert ei.value.code == -1 and "multiple of n_replicas" in str(ei.value)
    check(mc, wk, "after the refusal")
    mc.set_exchange(2, 0)  # resets the cursor, the labels and the counters
    wk.set_exchange(2, 0)
    check(mc, wk, "after set_exchange")
    mc.set_exchange(0, 0)
    with pytest.raises(gpu.DQMCError, match="no ladders"):
        mc.exchange()
    mc.close()


def test_exchange_off_is_a_handle_that_never_had_it(gpu):
    l = gpu.SquareLattice(4)
    betas = [0.9, 1.0, 1.1, 1.2]
    plain, wk = pair(gpu, l, "clock", 5, betas, 0, 0, cluster_rate=2, measure_rate=2)
    off, _ = pair(gpu, l, "clock", 5, betas, 0, 0, cluster_rate=2, measure_rate=2)
    rate0, _ = pair(gpu, l, "clock", 5, betas, 0, 0, cluster_rate=2, measure_rate=2)
    off.set_exchange(2, 1)
    off.set_exchange(0, 0)
    rate0.set_exchange(4, 0)
    for mc in (plain, off, rate0):
        mc.sweep(9)
    wk.run(1, 9, 0, 2, cluster_rate=2)
    check(plain, wk, "never")
    check(off, wk, "set_exchange(0, 0)")
    wk.R = 4  # (labels 0..3, no rounds)
    wk.replica = np.arange(4)
    check(rate0, wk, "rate 0")
    for mc in (plain, off, rate0):
        mc.close()


def test_tempering_at_the_potts_transition_against_enumeration(gpu):
    """3 x 3 Potts q = 3 (19683 states), R = 4 betas around beta_c = ln(1 + sqrt 3), 64 ladders, a round every second
    sweep, no cluster moves, binner on, seeds 7100 + w, 2000 sweeps after 200.  Per beta the pooled <e> lies within 5 pooled
    binned standard errors of the enumeration, and every pair's swap rate is strictly between 0 and 1.  The run is bit
    reproducible: the restatement with these seeds gives z = -1.16, -0.25, -1.12, -0.21 and swap rates between 0.76 and
    0.92, so a correct device cannot fail it."""
    l = gpu.SquareLattice(tref.PHYS_L)
    R, n_lad = tref.PHYS_R, tref.PHYS_LADDERS
    W = R * n_lad
    mc = gpu.MC(gpu.PottsModel(tref.PHYS_Q, l=l), beta=tref.PHYS_BETAS, n_walkers=W, seed=tref.PHYS_SEED,
                thermalization=tref.PHYS_THERM, sweeps=tref.PHYS_SWEEPS, tempering=(R, tref.PHYS_K), binner=tref.PHYS_SWEEPS)
    assert list(mc.betas[:R]) == tref.PHYS_BETAS and list(mc.betas[R:2 * R]) == tref.PHYS_BETAS  # tiled over the ladders
    mc.run()
    assert mc.binner_size()[1] == tref.PHYS_SWEEPS
    for i, beta in enumerate(tref.PHYS_BETAS):
        b = mc.binned(walkers=range(i, W, R))
        exact = tref.exact_energy_per_site(l, tref.PHYS_Q, beta)
        e = b["Energy"]["e"]
        z = (e["mean"] - exact) / e["std_error"]
        print("beta", beta, "e", e["mean"], "+-", e["std_error"], "exact", exact, "z", z, "tau", e["tau"])
        assert e["std_error"] > 0 and abs(z) <= 5.0, (beta, z)
        assert math.isfinite(b["Energy"]["C"]["std_error"]) and math.isfinite(b["Magn"]["U4"]["std_error"])
    for w in range(W):
        x = mc.exchange_stats(w)
        if w % R == R - 1:
            assert x.prop_exchange == 0
        else:
            assert 0 < x.acc_exchange < x.prop_exchange, (w, x.acc_exchange, x.prop_exchange)
    assert sorted(mc.replicas()[:R]) == list(range(R))
    mc.close()
