"""The q-state engine on the device (csrc/qstate.hip, csrc/qs_sweep.inl) where its other device tests do not go: odd
coordination (z = 3, 5), the full neighbour row (z = 8, CubicLattice(4, L)), BilayerSquareLattice, antiferromagnetic
coupling, a signed table that is not monotone in |d|, the inclusive table limit |e_q30| = 2^32 and the edge of the beta
domain of the acceptance product, with cluster moves, replica exchange and the binner on together.  The reference is the
numpy restatement of tests/qstate_tempering_ref.py (on qstate_ref.py, qstate_cluster_ref.py, qstate_binner_ref.py), written
from include/dqmc_hip.h.

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
import qstate_tempering_ref as tref  # noqa: E402
from test_gpu_qstate_tempering import check  # noqa: E402

pytestmark = pytest.mark.gpu

GENERIC6 = [1.0, -0.5, 0.25, -1.0, 0.25, -0.5]  # signed, not monotone in |d|


def table(kind, q):
    return {"potts": ref.potts_table, "clock": ref.clock_table}[kind](q) if kind != "generic6" else np.array(GENERIC6)


def model(g, kind, q, J, l):
    if kind == "potts":
        return g.PottsModel(q, l=l, J=J)
    if kind == "clock":
        return g.ClockModel(q, l=l, J=J)
    return g.QStateModel(q, table(kind, q), l=l, J=J)


def restatement(l, kind, q, J, betas, R, k, seed, cap=8, binner=None):
    wk = tref.TemperingWalkers(l, q, table(kind, q), betas, [seed + w for w in range(len(betas))], J=J,
                               series_capacity=cap, binner=binner)
    wk.set_exchange(R, k)
    return wk


def pair(g, l, kind, q, J, betas, R, k, seed=300, cap=8, binner=None, cluster_rate=0, **kw):
    """a handle of a model with its J and table, and its restatement"""
    W = len(betas)
    mc = g.MC(model(g, kind, q, J, l), beta=betas, n_walkers=W, seed=seed, series_capacity=cap, cluster_rate=cluster_rate,
              tempering=(R, k) if R or k else None, binner=binner if binner else False, **kw)
    assert type(mc) is g.QStateMC and (mc.n_replicas, mc.exchange_rate) == (R, k)
    return mc, restatement(l, kind, q, J, betas, R, k, seed, cap, binner)


# name -> (lattice, (N, z, colours), kind, q, J, one ladder's betas, ladders, sweeps, seed)
CASES = {
    # odd z in the sweep, the first int4 of a row partly used
    "honeycomb3_generic6": (lambda g: g.HoneycombLattice(3), (18, 3, 2), "generic6", 6, 1.0, [1.0, 1.2, 1.4], 2, 12, 300),
    # z = 5, repeated neighbours, N below a wave
    "bilayer2_afpotts3": (lambda g: g.BilayerSquareLattice(2), (8, 5, 2), "potts", 3, -1.0, [0.6, 0.8, 1.0], 2, 12, 300),
    # odd L (more than 2 colours), N no multiple of 4 (2 pad bytes), 2.5 N bonds
    "bilayer5_clock5_Jm075": (lambda g: g.BilayerSquareLattice(5), (50, 5, None), "clock", 5, -0.75, [0.9, 1.0, 1.1], 2,
                              12, 300),
    # the full row, every neighbour twice
    "cubic4d2_potts4": (lambda g: g.CubicLattice(4, 2), (16, 8, 2), "potts", 4, 1.0, [0.30, 0.36, 0.42], 2, 12, 300),
    # the full row, a ragged second wave, up to 9 colours, 3 pad bytes
    "cubic4d3_generic6_Jm2": (lambda g: g.CubicLattice(4, 3), (81, 8, None), "generic6", 6, -2.0, [0.10, 0.11, 0.12], 2,
                              12, 300),
    # the table limit e_q30[0] = 2^32, a larger exchange J, dE_int past 2^32
    "cubic4d3_clock7_J4": (lambda g: g.CubicLattice(4, 3), (81, 8, None), "clock", 7, 4.0, [0.050, 0.055, 0.060], 2, 12,
                           300),
    # My = 0 with q = 2, odd x odd, antiferromagnetic frustration
    "rect7x3_afpotts2": (lambda g: g.RectangularLattice(7, 3), (21, 4, None), "potts", 2, -1.0, [0.5, 0.9, 1.3], 2, 12,
                         300),
}


def run_case(l, name):
    """the restatement of one case, run, with the conditions that keep the case from passing while it exercises nothing"""
    _, (N, z, colours), kind, q, J, ladder, n_ladders, n, seed = CASES[name]
    assert (len(l), np.asarray(l.neighs).shape[0]) == (N, z), name
    R = len(ladder)
    wk = restatement(l, kind, q, J, ladder * n_ladders, R, 1, seed, binner=32)
    wk.run(1, n, 0, 2, cluster_rate=2)
    rate = wk.acc_local[1] / wk.prop_local[1]
    print(name, "decisions", wk.decided, "partial clusters", wk.n_partial.tolist(), "acceptance of walker 1", rate,
          "largest accepted |dE_int| / 2^32", wk.max_acc_dE.max() / 2.0 ** 32, "colours", len(wk.classes), "J", wk.J)
    assert wk.decided["acc"] > 0 and wk.decided["rej"] > 0, (name, wk.decided)
    assert wk.n_partial.sum() > 0, name
    assert 0.1 < rate < 0.9, (name, rate)
    if colours is not None:
        assert len(wk.classes) == colours, name
    return wk


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_every_feature_on(gpu, name):
    """three walkers per ladder, a round behind every sweep, a cluster move behind every second, every second sweep
    measured into the sums, the series and a binner of capacity 32.  The betas are chosen on the restatement so that the
    exchange rule both accepts and rejects, some cluster is neither a site nor the lattice and the middle walker accepts
    between 0.1 and 0.9 of its local proposals; all of it is asserted on the restatement before the device is compared."""
    make, _, kind, q, J, ladder, n_ladders, n, seed = CASES[name]
    l = make(gpu)
    wk = run_case(l, name)
    if name == "cubic4d3_clock7_J4":
        assert wk.e_q30[0] == 2 ** 32 and wk.max_acc_dE.max() > 2 ** 32, wk.max_acc_dE
        assert wk.J == tref.exchange_bits(324, wk.e_q30) == 42
    if name == "bilayer5_clock5_Jm075":
        assert len(wk.classes) > 2 and len(l.bonds) == 125
    if name == "cubic4d3_generic6_Jm2":
        assert len(wk.classes) > 2
    if name == "rect7x3_afpotts2":
        assert np.all(wk.My == 0) and len(wk.classes) > 2
    R = len(ladder)
    mc, _ = pair(gpu, l, kind, q, J, ladder * n_ladders, R, 1, seed=seed, binner=32, cluster_rate=2, measure_rate=2)
    mc.sweep(n)
    check(mc, wk, name)
    assert mc.stats(0).n_colours == len(wk.classes) == int(ref.greedy_colouring(l).max()) + 1
    assert mc.exchange_stats(0).rounds == n and mc.stats(0).n_meas == n // 2
    mc.close()


def test_the_full_row_at_scale(gpu):
    """CubicLattice(4, 11): N = 14641, z = 8, clock q = 64, the largest LDS layout that has z = 8.  One walker, two sweeps
    (the second measured), then a cluster move by hand.  The restatement takes about a second on one core."""
    l = gpu.CubicLattice(4, 11)
    assert (len(l), np.asarray(l.neighs).shape[0]) == (14641, 8)
    beta = 0.25
    mc, wk = pair(gpu, l, "clock", 64, 1.0, [beta], 0, 0, seed=81, cap=2, measure_rate=2)
    mc.sweep(2)
    wk.run(1, 2, 0, 2)
    check(mc, wk, "two sweeps")
    mc.cluster_move()
    wk.cluster_move()
    check(mc, wk, "and a move")
    st, cl = mc.stats(0), mc.cluster_stats(0)
    print("acceptance", st.acc_local / st.prop_local, "cluster", cl.sum_cluster_size, "colours", st.n_colours)
    assert st.n_meas == 1 and st.prop_local == 2 * 14641 and 0.1 < st.acc_local / st.prop_local < 0.9
    assert cl.prop_global == 1 and 1 < wk.max_cluster_size[0] < len(l)
    assert st.n_colours == len(wk.classes) > 2
    mc.close()


def test_a_walker_does_not_depend_on_the_others(gpu):
    """the z = 8 signed-table case with one walker and with 65: walker 0 of the 65 has the single walker's key and beta,
    no tempering, a cluster move behind every second sweep, the binner on; both against the restatement"""
    l = gpu.CubicLattice(4, 3)
    betas = [0.11] + list(np.linspace(0.05, 0.2, 64))
    kw = dict(seed=640, binner=32, cluster_rate=2, measure_rate=2)
    many, wk = pair(gpu, l, "generic6", 6, -2.0, betas, 0, 0, **kw)
    alone, wk1 = pair(gpu, l, "generic6", 6, -2.0, betas[:1], 0, 0, **kw)
    assert many.seeds[0] == alone.seeds[0] == 640
    for h in (many, alone):
        h.sweep(8)
    for w in (wk, wk1):
        w.run(1, 8, 0, 2, cluster_rate=2)
    assert wk.n_partial[0] > 0 and 0.1 < wk.acc_local[0] / wk.prop_local[0] < 0.9
    check(many, wk, "65 walkers")
    check(alone, wk1, "alone")
    assert np.array_equal(many.conf(0), alone.conf(0))
    a, b = many.stats(0), alone.stats(0)
    assert all(getattr(a, k) == getattr(b, k) for k, _ in a._fields_)
    assert all(np.array_equal(x, y) for x, y in zip(many.binner_level(0, 1)[:3], alone.binner_level(0, 1)[:3]))
    many.close()
    alone.close()


def test_the_beta_domain_guard(gpu):
    """CubicLattice(4, 2), clock q = 7, J = 4 (z = 8, range 4 (1 - cos(6 pi / 7)) = 7.6): set_beta at the largest beta with
    fl(fl(beta z) range) <= 700 succeeds, math.exp does not raise for its table and three sweeps match; the next double
    is refused with DQMC_ERR_INVALID, the handle is as it was and goes on matching; a handle created out there is
    refused too"""
    l = gpu.CubicLattice(4, 2)
    mc, wk = pair(gpu, l, "clock", 7, 4.0, [0.05, 0.06], 0, 0, seed=44, cluster_rate=2)
    assert wk.e_q30[0] == 2 ** 32 and wk.z == 8
    inside, outside = ref.domain_edge(wk.z, wk.e_q30)
    assert ref.beta_in_domain(inside, 8, wk.e_q30) and not ref.beta_in_domain(outside, 8, wk.e_q30)
    assert 11.0 < inside < 12.0 and outside == math.nextafter(inside, math.inf)
    mc.sweep(2)
    wk.run(1, 2, 0, 1, cluster_rate=2)
    mc.set_beta(1, inside)
    wk.set_beta(1, inside)  # (math.exp raises on overflow: not here)
    assert np.all(np.isfinite(wk.w[1])) and np.all(wk.w[1] > 0.0)
    mc.sweep(3)
    wk.run(3, 3, 0, 1, cluster_rate=2)
    check(mc, wk, "at the edge")
    for w, beta in ((1, outside), (0, outside), (0, 1.0e6)):
        with pytest.raises(gpu.DQMCError) as ei:
            mc.set_beta(w, beta)
        msg = str(ei.value)
        assert ei.value.code == -1, msg  # DQMC_ERR_INVALID
        assert all(word in msg for word in ("dqmc_qs_set_beta", "beta = ", "z = 8", "range", "700")), msg
    assert list(mc.betas) == [0.05, inside]
    check(mc, wk, "after the refusals")
    mc.sweep(3)
    wk.run(6, 3, 0, 1, cluster_rate=2)
    check(mc, wk, "three more sweeps")
    assert 0 < wk.acc_local[0] < wk.prop_local[0]
    with pytest.raises(gpu.DQMCError) as ei:
        gpu.MC(model(gpu, "clock", 7, 4.0, l), beta=[0.05, outside], n_walkers=2, seed=44)
    assert ei.value.code == -1 and "dqmc_qs_set_beta" in str(ei.value)
    mc.close()


# ---- the physics check: the frustrated 3 x 3 antiferromagnetic Potts model against enumeration
PHYS_BETAS = [0.6, 0.85, 1.1, 1.4]
PHYS_LADDERS, PHYS_K, PHYS_CLUSTER, PHYS_SEED = 64, 2, 2, 9300


def phys_pooled(finish, W, N):
    """per slot of the ladder the pooled <e> and its pooled binned standard error, as QStateMC.binned(walkers=) forms them
    from the per-walker (mean, varN) of element 0"""
    R = len(PHYS_BETAS)
    out = []
    for i in range(R):
        ws = range(i, W, R)
        mean = sum(finish(w)[0] for w in ws) / len(ws) / N
        err = math.sqrt(sum(finish(w)[1] for w in ws)) / len(ws) / N
        out.append((mean, err))
    return out


def test_tempering_the_frustrated_antiferromagnet_against_enumeration(gpu):
    """SquareLattice(3), Potts q = 3, J = -1 (19683 states; the odd rings are frustrated), R = 4 betas 0.6, 0.85, 1.1,
    1.4, 64 ladders, a round and a cluster move behind every second sweep, binner on, seeds 9300 + w, 2000 sweeps after
    200.  Per beta the pooled <e> lies within 5 pooled binned standard errors of the enumeration, and every tried pair's
    swap rate is strictly between 0 and 1.  The run is bit reproducible: the restatement with these seeds gives
    z = -1.37, -1.90, +0.22, +0.78 and swap rates between 0.73 and 0.84 (phys_pooled restates the pooling of
    QStateMC.binned from the restatement's binner), so a correct device cannot fail it."""
    l = gpu.SquareLattice(3)
    R, n_lad = len(PHYS_BETAS), PHYS_LADDERS
    W = R * n_lad
    therm, sweeps = tref.PHYS_THERM, tref.PHYS_SWEEPS
    mc = gpu.MC(gpu.PottsModel(3, l=l, J=-1.0), beta=PHYS_BETAS, n_walkers=W, seed=PHYS_SEED, thermalization=therm,
                sweeps=sweeps, tempering=(R, PHYS_K), cluster_rate=PHYS_CLUSTER, binner=sweeps)
    assert list(mc.betas[:R]) == PHYS_BETAS and list(mc.betas[R:2 * R]) == PHYS_BETAS
    mc.run()
    assert mc.binner_size()[1] == sweeps
    for i, beta in enumerate(PHYS_BETAS):
        b = mc.binned(walkers=range(i, W, R))
        exact = ref.qstate_exact(l, 3, ref.potts_table(3), beta, J=-1.0)["E"] / len(l)
        e = b["Energy"]["e"]
        z = (e["mean"] - exact) / e["std_error"]
        print("beta", beta, "e", e["mean"], "+-", e["std_error"], "exact", exact, "z", z, "tau", e["tau"])
        assert e["std_error"] > 0 and abs(z) <= 5.0, (beta, z)
    for w in range(W):
        x = mc.exchange_stats(w)
        if w % R == R - 1:
            assert x.prop_exchange == 0
        else:
            assert 0 < x.acc_exchange < x.prop_exchange, (w, x.acc_exchange, x.prop_exchange)
    assert sorted(mc.replicas()[:R]) == list(range(R))
    cl = mc.cluster_stats(0)
    assert cl.prop_global == (therm + sweeps) // PHYS_CLUSTER and 0 < cl.acc_global
    mc.close()
