"""The q-state engine's scaling measurement on the device (csrc/qs_scaling.inl: qs_scaling_kernel behind every measured
sweep; include/dqmc_hip.h, "Scaling" of the q-state section) against the numpy restatement of tests/qstate_scaling_ref.py.

The method: measure_rate = 1, sweep(1) over and over, mc.conf(w) after each call, S_k on the host from that
configuration, summed in the order of the measurements.  n_meas and sum_S are compared with ==: the per-state sums are
exact integers and the fp64 part is defined operation by operation.  A twin handle with the same seeds does the same
sweeps in one sweep(n).  The binner's scaling section is compared level by level with the restatement's binner fed the
host values, with == as well (no element has a square root)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref  # noqa: E402
import qstate_scaling_ref as ref  # noqa: E402
from test_qstate_scaling_host import hot_binners  # noqa: E402

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("energy_q30", "mx_q30", "my_q30", "sum_E", "sum_E2", "sum_absM", "sum_M2", "sum_M4", "n_meas",
               "prop_local", "acc_local", "sweeps_drawn", "confs_drawn", "n_series", "n_colours")
SIGNED5 = [1.0, -0.5, 0.25, 0.25, -0.5]  # a signed table, e[d] == e[5 - d]

# name: (lattice, model kind, q, n_k, walkers)
CASES = {
    "chain32_q2": (lambda g: g.Chain(32), "potts", 2, 1, 3),                  # one full set of words, My = 0
    "cubic3_q3": (lambda g: g.CubicLattice(3, 3), "potts", 3, 3, 3),          # N = 27: zero bytes pad the last word
    "square6_q8": (lambda g: g.SquareLattice(6), "clock", 8, 8, 3),
    "square20_q64": (lambda g: g.SquareLattice(20), "clock", 64, 1, 3),       # more sites than lanes in a workgroup
    "triangular5_q5": (lambda g: g.TriangularLattice(5), "signed", 5, 2, 70),  # more walkers than a wave has lanes
    "square6_q9": (lambda g: g.SquareLattice(6), "clock", 9, 2, 3),           # the first q with 16 copies of a bin
}


def _model(g, kind, q, l):
    if kind == "potts":
        return g.PottsModel(q, l=l)
    if kind == "clock":
        return g.ClockModel(q, l=l)
    return g.QStateModel(q, SIGNED5, l=l)


def _k_vectors(g, l, n_k):
    """n_k distinct wave vectors: integer combinations of the reciprocal vectors, the smallest first"""
    import itertools
    b = g.reciprocal_vectors(l)
    d = len(b)
    combos = [(j,) for j in range(1, 9)] if d == 1 else [c for c in itertools.product(range(3), repeat=d) if any(c)]
    ks = [np.array(c, dtype=float) @ b for c in combos[:n_k]]
    assert len(ks) == n_k
    return ks


def _tables(l, ks):
    from montecarlo_jl_amd import lattices
    return ref.q30(lattices._positions(l), ks)


class _Host:
    """the host's sums of the walkers `ws`, fed one configuration per measurement"""

    def __init__(self, q, tables, ws, n_k):
        self.cq, self.sq = tables
        self.c, self.s = ref.state_tables(q)
        self.ws, self.n_k, self.n = list(ws), n_k, 0
        self.sum_S = {w: np.zeros(n_k) for w in self.ws}
        self.series = {w: [] for w in self.ws}

    def take(self, mc):
        self.n += 1
        for w in self.ws:
            v = ref.values(mc.conf(w), self.c, self.s, self.cq, self.sq)
            self.sum_S[w] = self.sum_S[w] + v[1:]
            self.series[w].append(v)

    def check(self, mc, label):
        for w in self.ws:
            f = mc.scaling_sums(w)
            assert (f.n_meas, f.n_k) == (self.n, self.n_k), (label, w, f.n_meas, self.n)
            got = np.array(f.sum_S[:self.n_k])
            print(label, w, "sum_S", got, self.sum_S[w])
            assert np.array_equal(got, self.sum_S[w]), (label, w, got, self.sum_S[w])
            assert not any(f.sum_S[self.n_k:])


def _stepwise(mc, host, n):
    """n x sweep(1); the host measures where the engine's rule does"""
    for _ in range(n):
        mc.sweep(1)
        g = mc.last_sweep
        if g > mc.thermalization and g % mc.measure_rate == 0:
            host.take(mc)


def _levels(mc, w):
    return [tuple(x.tolist() if hasattr(x, "tolist") else x for x in mc.binner_level(w, l))
            for l in range(mc.binner_size()[0])]


def _scaling_levels(mc, w):
    return [tuple(x.tolist() if hasattr(x, "tolist") else x for x in mc.scaling_binner_level(w, l))
            for l in range(mc.binner_size()[0])]


def _chain_state(mc, w, binner):
    """everything of walker w that a handle without the measurement has, in a form that compares with =="""
    st, cl, x = mc.stats(w), mc.cluster_stats(w), mc.exchange_stats(w)
    out = [[getattr(st, f) for f in STAT_FIELDS], [a.tolist() for a in mc.series(w)], mc.conf(w).tolist(),
           [cl.prop_global, cl.acc_global, cl.sum_cluster_size, cl.moves_drawn],
           [x.prop_exchange, x.acc_exchange, x.replica, x.rounds]]
    if binner:
        out.append(_levels(mc, w))
    return out


def _scaling_state(mc, w, binner):
    f = mc.scaling_sums(w)
    return [f.n_meas, f.n_k, list(f.sum_S)] + ([_scaling_levels(mc, w)] if binner else [])


def _picked(W):
    return sorted({0, W // 2, 63 % W, 64 % W, W - 1})


@pytest.mark.parametrize("name", list(CASES))
def test_sums_against_the_host_and_a_one_call_twin(gpu, name):
    make, kind, q, n_k, W = CASES[name]
    l = make(gpu)
    ks = _k_vectors(gpu, l, n_k)
    betas = np.linspace(0.3, 1.2, W)
    betas[0] = 3.0  # walker 0 starts from all-zero states and stays near them
    kw = dict(beta=betas, n_walkers=W, seed=77, scaling=ks, series_capacity=4)
    mc, twin = gpu.MC(_model(gpu, kind, q, l), **kw), gpu.MC(_model(gpu, kind, q, l), **kw)
    assert type(mc) is gpu.QStateMC and len(mc.k_vectors) == n_k
    for h in (mc, twin):
        h.set_conf(0, np.zeros(len(l), dtype=np.uint8))
    ws = _picked(W)
    host = _Host(q, _tables(l, ks), ws, n_k)
    n = 20
    _stepwise(mc, host, n)
    twin.sweep(n)
    assert host.n == n
    host.check(mc, name)
    for w in ws:
        assert _scaling_state(mc, w, False) == _scaling_state(twin, w, False), (name, w)
        assert _chain_state(mc, w, False) == _chain_state(twin, w, False), (name, w)
    if q == 2:
        assert all(mc.stats(w).my_q30 == 0 for w in ws)
    # the first measurement of walker 0 is near the ordered state: S_k far below S(0) there
    out = mc.scaling(0)
    assert out["S"].shape == (n_k,) and out["xi"].shape == (n_k,) and out["n_meas"] == n and out["k"].shape[0] == n_k
    assert out["M2"] == mc.stats(0).sum_M2 / n and np.array_equal(out["S"], np.array(mc.scaling_sums(0).sum_S[:n_k]) / n)
    mc.close()
    twin.close()


def test_splitting_with_rate_and_thermalization(gpu):
    """stepwise against one call, measure_rate 3 and thermalization 4, with cluster moves, rounds and a binner: every
    sum, the series and all levels of both binner sections bit for bit; the stepwise handle against the host"""
    l = gpu.SquareLattice(6)
    q, W, n = 8, 6, 64
    ks = _k_vectors(gpu, l, 2)
    kw = dict(beta=np.linspace(0.6, 1.1, 3), n_walkers=W, seed=4242, scaling=ks, thermalization=4, measure_rate=3,
              cluster_rate=2, tempering=(3, 2), binner=30, series_capacity=8)
    mc, once = gpu.MC(gpu.ClockModel(q, l=l), **kw), gpu.MC(gpu.ClockModel(q, l=l), **kw)
    ws = list(range(W))
    host = _Host(q, _tables(l, ks), ws, 2)
    _stepwise(mc, host, n)
    once.sweep(n)
    assert host.n == 20 == mc.binner_size()[1] == once.binner_size()[1]
    host.check(mc, "splitting")
    for w in ws:
        assert _scaling_state(mc, w, True) == _scaling_state(once, w, True), w
        assert _chain_state(mc, w, True) == _chain_state(once, w, True), w
    # sweeps in odd pieces on a third handle
    parts = gpu.MC(gpu.ClockModel(q, l=l), **kw)
    for m in (5, 1, 7, 30, 21):
        parts.sweep(m)
    for w in ws:
        assert _scaling_state(parts, w, True) == _scaling_state(once, w, True), w
        assert _chain_state(parts, w, True) == _chain_state(once, w, True), w
    for h in (mc, once, parts):
        h.close()


def test_scaling_leaves_the_chain_unchanged(gpu):
    """a handle with the measurement against one that never had it: same seeds, cluster moves, ladders and a binner"""
    l = gpu.SquareLattice(8)
    W = 72
    kw = dict(beta=np.linspace(0.7, 1.1, 4), n_walkers=W, seed=5, thermalization=2, measure_rate=2, cluster_rate=2,
              tempering=(4, 3), binner=64, series_capacity=16)
    on = gpu.MC(gpu.PottsModel(3, l=l), scaling=True, **kw)
    off = gpu.MC(gpu.PottsModel(3, l=l), **kw)
    for n in (7, 1, 15):
        on.sweep(n)
        off.sweep(n)
    assert on.scaling_sums(0).n_meas == 10 == off.stats(0).n_meas and off.scaling_sums(0).n_k == 0
    assert on.binner_size() == off.binner_size() == (7, 10)
    for w in range(W):
        assert _chain_state(on, w, True) == _chain_state(off, w, True), w  # (|M| too: the device runs the same code)
    assert on.replicas().tolist() == off.replicas().tolist()
    assert sum(on.exchange_stats(w).acc_exchange for w in range(W)) > 0
    with pytest.raises(gpu.DQMCError) as e:
        off.scaling()
    assert e.value.code == -4
    with pytest.raises(gpu.DQMCError) as e:  # no scaling section on the other handle
        off.scaling_binner_level(0, 0)
    assert e.value.code == -4
    on.close()
    off.close()


def test_with_an_exchange_round_behind_every_sweep(gpu):
    """tempering=(4, 1): every measurement is the exchange kernel's, and mc.conf(w), read after the call and so after the
    swap, is the configuration the slot's S_k belongs to"""
    l = gpu.SquareLattice(6)
    q, W = 5, 8
    ks = _k_vectors(gpu, l, 2)
    kw = dict(beta=np.linspace(0.5, 0.9, 4), n_walkers=W, seed=31, scaling=ks, tempering=(4, 1))
    mc, once = gpu.MC(gpu.ClockModel(q, l=l), **kw), gpu.MC(gpu.ClockModel(q, l=l), **kw)
    ws = list(range(W))
    host = _Host(q, _tables(l, ks), ws, 2)
    _stepwise(mc, host, 24)
    once.sweep(24)
    host.check(mc, "exchange")
    assert sum(mc.exchange_stats(w).acc_exchange for w in ws) > 0  # (configurations did change slots)
    for w in ws:
        assert _scaling_state(mc, w, False) == _scaling_state(once, w, False), w
        assert mc.stats(w).n_meas == 24
    mc.close()
    once.close()


@pytest.mark.parametrize("n, capacity", [(37, 40), (7, 7)])
def test_binner_section_against_the_restatement(gpu, n, capacity):
    """37 pushes at capacity 40 pass several compressor levels; 7 at capacity 7 fill the top level"""
    l = gpu.SquareLattice(6)
    q, W, n_k = 3, 66, 3
    ks = _k_vectors(gpu, l, n_k)
    kw = dict(beta=np.linspace(0.7, 1.1, W), n_walkers=W, seed=99, cluster_rate=4, binner=capacity)
    mc = gpu.MC(gpu.PottsModel(q, l=l), scaling=ks, **kw)
    plain = gpu.MC(gpu.PottsModel(q, l=l), **kw)
    ws = [1, 65]
    host = _Host(q, _tables(l, ks), ws, n_k)
    _stepwise(mc, host, n)
    plain.sweep(n)
    L, T = mc.binner_size()
    assert (L, T) == (math.ceil(math.log2(capacity + 1)), n) == plain.binner_size()
    for w in ws:
        b = ref.ScalingBinnerRef(n_k, capacity=capacity)
        for v in host.series[w]:
            b.push(v)
        for lv in range(L):
            xs, x2, xy, cnt = mc.scaling_binner_level(w, lv)
            assert cnt == b.count[lv] == T >> lv, (w, lv)
            print(w, lv, xs, b.x_sum[lv])
            assert np.array_equal(xs, b.x_sum[lv]), (w, lv, xs, b.x_sum[lv])
            assert np.array_equal(x2, b.x2_sum[lv]), (w, lv, x2, b.x2_sum[lv])
            assert np.array_equal(xy, b.xy_sum[lv]), (w, lv, xy, b.xy_sum[lv])
            # M2 is the value the first section gets (its elements 3 and 4)
            assert xs[0] == mc.binner_level(w, lv)[0][3] and x2[0] == mc.binner_level(w, lv)[1][3]
        assert _levels(mc, w) == _levels(plain, w)  # the six-element section is the one of a handle without scaling
        lv = b.reliable_level()
        f = mc.scaling_binner_finish(w)
        assert (f.level, f.count, f.n_k) == (lv, b.count[lv], n_k)
        np.testing.assert_allclose(f.mean[:1 + n_k], b.mean(), rtol=1e-12)
        np.testing.assert_allclose(f.varN[:1 + n_k], b.varN(lv), rtol=1e-12)
        np.testing.assert_allclose(f.covN[:n_k], b.covN(lv), rtol=1e-12)
        got = mc.binned_scaling(w)
        M2, v = b.mean()[0], b.varN(lv)
        for k in range(n_k):
            Sk, kn = b.mean()[1 + k], float(np.linalg.norm(ks[k]))
            assert got["S"][k]["mean"] == pytest.approx(Sk, rel=1e-12)
            assert got["S"][k]["std_error"] == pytest.approx(math.sqrt(max(v[1 + k], 0.0)), rel=1e-12)
            assert got["S"][k]["tau"] == pytest.approx(b.tau(lv)[1 + k], rel=1e-12, nan_ok=True)
            want_xi = ref.xi(M2, Sk, len(l), kn)
            assert got["xi"][k]["mean"] == pytest.approx(want_xi, rel=1e-12, nan_ok=True)
            if want_xi == want_xi:
                fd = ref.fd_variance(lambda a, s: ref.xi(a, s, len(l), kn), M2, Sk, v[0], v[1 + k], b.covN(lv)[k])
                assert got["xi"][k]["std_error"] ** 2 == pytest.approx(max(fd, 0.0), rel=1e-4, abs=1e-12 * want_xi ** 2)
            assert "tau" not in got["xi"][k] and got["xi_over_L"][k]["mean"] == pytest.approx(
                got["xi"][k]["mean"] / 6.0, nan_ok=True)
        assert (got["count"], got["level"]) == (b.count[lv], lv)
    # beyond the capacity: refused before anything runs, every sum as it was
    if n < capacity:
        mc.sweep(capacity - n)
    before = [(_scaling_state(mc, w, True), _chain_state(mc, w, True)) for w in ws], mc.last_sweep
    with pytest.raises(gpu.DQMCError) as e:
        mc.sweep(1)
    assert e.value.code == -4
    assert ([(_scaling_state(mc, w, True), _chain_state(mc, w, True)) for w in ws], mc.last_sweep) == before
    pooled = mc.binned_scaling(walkers=[1, 1])
    assert pooled["n_walkers"] == 2 and pooled["S"][0]["mean"] == pytest.approx(mc.binned_scaling(1)["S"][0]["mean"])
    mc.close()
    plain.close()


def test_switching_and_errors(gpu):
    l = gpu.CubicLattice(3, 3)
    N = len(l)
    mc = gpu.MC(gpu.PottsModel(3, l=l), beta=0.4, n_walkers=3, seed=8, binner=10)
    mc.sweep(4)
    assert mc.scaling_sums(1).n_k == 0 and mc.binner_size() == (4, 4) and mc.k_vectors is None
    mc.set_scaling(True)  # mid-run: the binner restarts with every section empty, the capacity kept
    assert mc.binner_size() == (4, 0) and mc.scaling_sums(1).n_meas == 0 and mc.scaling_sums(1).n_k == 3
    mc.sweep(3)
    f = mc.scaling_sums(1)
    assert f.n_meas == 3 and f.sum_S[0] > 0 and mc.stats(1).n_meas == 7 and mc.scaling_binner_level(1, 0)[3] == 3
    with pytest.raises(gpu.DQMCError) as e:  # 7 M2 measurements but 3 of S
        mc.scaling(1)
    assert e.value.code == -4
    mc.set_scaling(_k_vectors(gpu, l, 1))  # again: the sums start anew
    f = mc.scaling_sums(1)
    assert (f.n_meas, f.n_k, f.sum_S[0]) == (0, 1, 0.0) and mc.binner_size() == (4, 0)
    with pytest.raises(gpu.DQMCError) as e:  # nothing measured yet
        mc.reset_accumulators()
        mc.scaling(1)
    assert e.value.code == -1
    mc.sweep(5)
    assert mc.scaling_sums(1).n_meas == 5 and mc.scaling(1)["n_meas"] == 5
    mc.reset_accumulators()
    f = mc.scaling_sums(1)
    assert (f.n_meas, f.sum_S[0]) == (0, 0.0) and mc.stats(1).n_meas == 0
    xs, x2, xy, cnt = mc.scaling_binner_level(1, 0)
    assert cnt == 0 and not xs.any() and not x2.any() and not xy.any()
    mc.sweep(2)
    # refused tables leave the handle as it was
    from montecarlo_jl_amd import _lib
    before = _scaling_state(mc, 1, True)
    big = (C.c_int32 * (9 * N))(*([2 ** 30 + 1] * (9 * N)))
    ok = (C.c_int32 * (9 * N))(*([2 ** 30] * (9 * N)))
    assert _lib.lib().dqmc_qs_set_scaling(mc._h, 9, ok, ok) == -1 and _lib.lib().dqmc_qs_set_scaling(mc._h, -1, ok, ok) == -1
    assert _lib.lib().dqmc_qs_set_scaling(mc._h, 1, None, ok) == -1 and _lib.lib().dqmc_qs_set_scaling(mc._h, 1, big, ok) == -1
    assert _lib.lib().dqmc_qs_set_scaling(mc._h, 1, ok, big) == -1
    assert _scaling_state(mc, 1, True) == before and mc.binner_size() == (4, 2)
    mc.sweep(1)
    assert mc.scaling_sums(1).n_meas == 3
    # off again: present behaviour, beside a handle that never had the measurement
    plain = gpu.MC(gpu.PottsModel(3, l=l), beta=0.4, n_walkers=3, seed=8)
    plain.sweep(mc.last_sweep)
    plain.enable_binning(10)
    mc.set_scaling(None)
    assert mc.scaling_sums(1).n_k == 0 and mc.binner_size() == (4, 0) and mc.k_vectors is None
    mc.sweep(6)
    plain.sweep(6)
    for w in range(3):
        assert mc.conf(w).tolist() == plain.conf(w).tolist() and _levels(mc, w) == _levels(plain, w)
        assert [getattr(mc.stats(w), f) for f in STAT_FIELDS[:3]] == [getattr(plain.stats(w), f) for f in STAT_FIELDS[:3]]
    with pytest.raises(gpu.DQMCError) as e:
        mc.scaling_binner_finish(1)
    assert e.value.code == -4
    mc.close()
    plain.close()


def test_physics_at_beta_zero(gpu):
    """PottsModel(3, dims=2, L=8), 64 walkers, 200 measurements at beta = 0: <S_k> = 1 for k != 0 within 5 pooled
    standard errors from binned_scaling.  The restatement alone, same seeds (test_qstate_scaling_host.py): 1.004594 +-
    0.007274 and 1.007452 +- 0.007533.  The device's sums are the restatement's, bit for bit."""
    W = ref.HOT_W
    mc = gpu.MC(gpu.PottsModel(ref.HOT_Q, dims=2, L=ref.HOT_L), beta=0.0, n_walkers=W, seed=ref.HOT_SEED,
                sweeps=ref.HOT_MEAS, scaling=True, binner=ref.HOT_MEAS)
    mc.run()
    got = mc.binned_scaling(walkers=range(W))
    assert got["count"] == ref.HOT_MEAS >> got["level"] and got["level"] == 2 and got["n_walkers"] == W
    for k in range(2):
        o = got["S"][k]
        print("S_%d" % k, o, (o["mean"] - 1.0) / o["std_error"])
        assert o["std_error"] > 0 and abs(o["mean"] - 1.0) <= 5.0 * o["std_error"], (k, o)
    # the restatement's chain, measured by the restatement: the same sums
    l = mc.model.l
    wk = qstate_ref.Walkers(l, ref.HOT_Q, qstate_ref.potts_table(ref.HOT_Q), [0.0] * W, [ref.HOT_SEED + w for w in range(W)])

    def confs_of(m):
        wk.sweep()
        return wk.c

    bins = hot_binners(l, confs_of)
    for w in (0, 63):
        assert np.array_equal(mc.conf(w), wk.c[w])
        assert np.array_equal(np.array(mc.scaling_sums(w).sum_S[:2]), bins[w].x_sum[0][1:])
    for e in (1, 2):
        mean, err = ref.pooled(bins, e)
        assert got["S"][e - 1]["mean"] == pytest.approx(mean, rel=1e-12)
        assert got["S"][e - 1]["std_error"] == pytest.approx(err, rel=1e-9)
    mc.close()
