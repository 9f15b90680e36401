"""The finite-size-scaling measurement on the device (ising_fss.inl: ising_fss_kernel behind every measured sweep;
include/dqmc_hip.h "finite-size-scaling observables") against the numpy restatement of tests/ising_fss_ref.py.

The method: measure_rate = 1, sweep(1) over and over, mc.conf(w) after each call, M4 and S_k on the host from that
configuration, summed in the order of the measurements.  n_meas and sum_M4 are compared with ==: M4 is one rounding of
an exact product and the running sum adds the same values in the same order.  sum_S is compared at rtol 1e-13: a term
is three or four roundings depending on contraction, a few ulp (2.2e-16 each) per term, summed over at most ~50
measurements of non-negative terms.  A twin handle with the same seeds does the same sweeps in one sweep(n).

The binner's FSS section is compared level by level with the restatement's binner fed the host values, at rtol 1e-12
(the cascade adds an fma-or-not per level to the few ulp of each value); counts are exact."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ising_fss_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("energy", "magnetization", "sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "prop_local", "acc_local",
               "uniforms_used", "n_series")
SHAPES = {"chain32": lambda g: g.Chain(32),             # exactly one word
          "square6": lambda g: g.SquareLattice(6),      # N = 36: a partial second word
          "square8": lambda g: g.SquareLattice(8),
          "cubic3": lambda g: g.CubicLattice(3, 3)}     # N = 27, z = 6


def _k_vectors(gpu, l, n_k):
    """n_k distinct wave vectors: integer combinations of the reciprocal vectors, the smallest ones first"""
    b = gpu.reciprocal_vectors(l)
    d = len(b)
    combos = [(j,) for j in range(1, 9)] if d == 1 else \
        [c for c in itertools.product(range(3), repeat=d) if any(c)]
    ks = [np.array(c, dtype=float) @ b for c in combos[:n_k]]
    assert len(ks) == n_k and len({tuple(np.round(k, 9)) for k in ks}) == n_k
    return ks


def _tables(gpu, l, ks):
    from montecarlo_jl_amd import lattices
    return ref.q30(lattices._positions(l), ks) if len(ks) else (np.zeros((0, len(l)), np.int64),) * 2


class _Host:
    """the host's sums of the walkers `ws`, fed one configuration per measurement"""

    def __init__(self, tables, ws, n_k):
        self.cq, self.sq = tables
        self.ws, self.n_k = list(ws), n_k
        self.n = 0
        self.sum_M4 = {w: np.float64(0.0) for w in self.ws}
        self.sum_S = {w: np.zeros(n_k) for w in self.ws}
        self.series = {w: [] for w in self.ws}

    def take(self, mc):
        self.n += 1
        for w in self.ws:
            v = ref.values(mc.conf(w), self.cq, self.sq)
            self.sum_M4[w] = self.sum_M4[w] + v[1]
            self.sum_S[w] = self.sum_S[w] + v[2:]
            self.series[w].append(v)

    def check(self, mc, label):
        for w in self.ws:
            f = mc.fss_sums(w)
            assert (f.n_meas, f.n_k) == (self.n, self.n_k), (label, w, f.n_meas, self.n)
            assert f.sum_M4 == self.sum_M4[w], (label, w, f.sum_M4, self.sum_M4[w])
            got = np.array(f.sum_S[:self.n_k])
            print(label, w, "sum_S", got, self.sum_S[w])
            np.testing.assert_allclose(got, self.sum_S[w], rtol=1e-13, atol=0, err_msg=str((label, w)))
            assert not any(f.sum_S[self.n_k:])


def _stepwise(mc, host, n):
    """n x sweep(1); the host measures where run!'s rule does"""
    for _ in range(n):
        mc.sweep(1)
        g = mc.last_sweep
        if g > mc.thermalization and g % mc.measure_rate == 0:
            host.take(mc)


def _same_fss(a, b, ws, label):
    for w in ws:
        fa, fb = a.fss_sums(w), b.fss_sums(w)
        assert (fa.n_meas, fa.n_k) == (fb.n_meas, fb.n_k), (label, w)
        assert fa.sum_M4 == fb.sum_M4, (label, w)
        np.testing.assert_allclose(np.array(fa.sum_S[:]), np.array(fb.sum_S[:]), rtol=1e-13, atol=0, err_msg=str((label, w)))


def _picked(W):
    return sorted({0, W // 2, max(W - 2, 0), W - 1})


@pytest.mark.parametrize("n_k", [0, 1, 8])
@pytest.mark.parametrize("W", [1, 64, 65, 130])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sums_against_the_host_and_a_one_call_twin(gpu, shape, W, n_k):
    l = SHAPES[shape](gpu)
    ks = _k_vectors(gpu, l, n_k)
    kw = dict(beta=np.linspace(0.2, 0.6, W), n_walkers=W, seed=77, fss=ks)
    mc, twin = gpu.MC(gpu.IsingModel(l=l), **kw), gpu.MC(gpu.IsingModel(l=l), **kw)
    ws = _picked(W)
    host = _Host(_tables(gpu, l, ks), ws, n_k)
    _stepwise(mc, host, 20)
    twin.sweep(20)
    host.check(mc, shape)
    _same_fss(mc, twin, ws, shape)
    for w in ws:
        assert np.array_equal(mc.conf(w), twin.conf(w))
    mc.close()
    twin.close()


COMBINATIONS = {
    "thermalization": dict(n_walkers=5, thermalization=3),
    "measure_rate": dict(n_walkers=5, thermalization=2, measure_rate=3),
    "cluster": dict(n_walkers=5, cluster_moves=True, global_rate=2),           # deferred measurements
    "exchange_fused": dict(n_walkers=8, n_replicas=4, exchange_rate=1),
    "exchange_launched": dict(n_walkers=6, n_replicas=3, exchange_rate=2),
    "exchange_behind_cluster": dict(n_walkers=8, n_replicas=4, exchange_rate=1, cluster_moves=True, global_rate=2),
    "exchange_launched_behind_cluster": dict(n_walkers=6, n_replicas=3, exchange_rate=1, cluster_moves=True,
                                             global_rate=3, measure_rate=2),
}


@pytest.mark.parametrize("name", list(COMBINATIONS))
def test_every_place_a_measurement_is_taken(gpu, name):
    """the per-sweep handle against the host, and one sweep(n) against the per-sweep twin"""
    l = gpu.SquareLattice(6)
    kw = dict(COMBINATIONS[name])
    W = kw["n_walkers"]
    R = kw.get("n_replicas", 0)
    kw["beta"] = np.linspace(0.35, 0.5, R) if R else np.linspace(0.3, 0.5, W)
    ks = _k_vectors(gpu, l, 2)
    mc = gpu.MC(gpu.IsingModel(l=l), seed=4242, fss=ks, **kw)
    once = gpu.MC(gpu.IsingModel(l=l), seed=4242, fss=ks, **kw)
    if R:
        assert mc.exchange_fused() == (R == 4)
    ws = list(range(W))
    host = _Host(_tables(gpu, l, ks), ws, 2)
    n = 21
    _stepwise(mc, host, n)
    once.sweep(n)
    assert host.n >= 6
    host.check(mc, name)
    _same_fss(mc, once, ws, name)
    for w in ws:
        assert mc.stats(w).n_meas == host.n
        assert [getattr(mc.stats(w), f) for f in STAT_FIELDS] == [getattr(once.stats(w), f) for f in STAT_FIELDS]
    if R:
        assert sum(mc.exchange_stats(w).acc_exchange for w in ws) > 0  # (configurations did change slots)
    mc.close()
    once.close()


def _levels(mc, w):
    return [mc.binner_level(w, l) for l in range(mc.binner_size()[0])]


def test_binner_section_against_the_restatement(gpu):
    l = gpu.SquareLattice(6)
    W, n, therm = 66, 37, 2
    ks = _k_vectors(gpu, l, 3)
    kw = dict(beta=np.linspace(0.3, 0.5, W), n_walkers=W, seed=99, thermalization=therm, cluster_moves=True,
              global_rate=4, binning=True, binning_capacity=100)
    mc = gpu.MC(gpu.IsingModel(l=l), fss=ks, **kw)
    plain = gpu.MC(gpu.IsingModel(l=l), **kw)
    ws = [1, 65]
    host = _Host(_tables(gpu, l, ks), ws, 3)
    _stepwise(mc, host, n)
    plain.sweep(n)
    L, T = mc.binner_size()
    assert (L, T) == (7, n - therm) == plain.binner_size()
    for w in ws:
        b = ref.FssBinnerRef(3, capacity=100)
        for v in host.series[w]:
            b.push(v)
        for lv in range(L):
            xs, x2, xy, cnt = mc.fss_binner_level(w, lv)
            assert cnt == b.count[lv] == T >> lv, (w, lv)
            print(w, lv, xs, b.x_sum[lv])
            np.testing.assert_allclose(xs, b.x_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
            np.testing.assert_allclose(x2, b.x2_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
            np.testing.assert_allclose(xy, b.xy_sum[lv], rtol=1e-12, atol=0, err_msg=str((w, lv)))
        # the four-element section is the one of a handle without FSS
        for p, q in zip(_levels(mc, w), _levels(plain, w)):
            assert all(np.array_equal(p[i], q[i]) for i in range(3)) and p[3] == q[3]
        # finish and binned_fss on those sums
        lv = b.reliable_level()
        f = mc.fss_binner_finish(w)
        assert (f.level, f.count, f.n_k) == (lv, b.count[lv], 3)
        np.testing.assert_allclose(f.mean[:5], b.mean(), rtol=1e-12)
        np.testing.assert_allclose(f.varN[:5], b.varN(lv), rtol=1e-9)
        np.testing.assert_allclose(f.covN[:4], b.covN(lv), rtol=1e-9, atol=1e-9 * np.abs(b.covN(lv)).max())
        got = mc.binned_fss(w)
        M2, M4 = b.mean()[0], b.mean()[1]
        assert got["U4"]["mean"] == pytest.approx(ref.binder(M2, M4), rel=1e-12)
        assert got["U4"]["std_error"] ** 2 == pytest.approx(
            max(ref.fd_variance(ref.binder, M2, M4, b.varN(lv)[0], b.varN(lv)[1], b.covN(lv)[0]), 0.0), rel=1e-5)
        assert got["M4"]["std_error"] == pytest.approx(math.sqrt(b.varN(lv)[1]), rel=1e-9) and "tau" in got["M4"]
        assert len(got["S"]) == len(got["xi"]) == len(got["xi_over_L"]) == 3 and "tau" not in got["U4"]
    with pytest.raises(gpu.DQMCError) as e:  # no FSS section on the other handle
        plain.fss_binner_level(0, 0)
    assert e.value.code == -4
    mc.close()
    plain.close()


def test_fss_leaves_the_chain_unchanged(gpu):
    l = gpu.SquareLattice(8)
    W = 72
    kw = dict(beta=np.linspace(0.3, 0.55, 4), n_walkers=W, seed=5, thermalization=2, measure_rate=2, cluster_moves=True,
              global_rate=3, n_replicas=4, exchange_rate=2, series_capacity=16)
    on = gpu.MC(gpu.IsingModel(l=l), fss=True, **kw)
    off = gpu.MC(gpu.IsingModel(l=l), **kw)
    for n in (7, 1, 15):
        on.sweep(n)
        off.sweep(n)
    assert on.fss_sums(0).n_meas == 10 == off.stats(0).n_meas and off.fss_sums(0).n_k == -1
    for w in range(W):
        assert np.array_equal(on.conf(w), off.conf(w)), w
        a, b = on.stats(w), off.stats(w)
        assert [getattr(a, f) for f in STAT_FIELDS] == [getattr(b, f) for f in STAT_FIELDS], w
        assert on.uniforms_used(w) == off.uniforms_used(w)
    assert on.replicas().tolist() == off.replicas().tolist()
    with pytest.raises(gpu.DQMCError):
        off.fss()
    on.close()
    off.close()


def test_state_handling(gpu):
    l = gpu.SquareLattice(6)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=0.4, n_walkers=3, seed=8, binning=True, binning_capacity=10)
    mc.sweep(4)
    assert mc.fss_sums(1).n_k == -1 and mc.binner_size() == (4, 4)
    mc.set_fss(True)  # mid-run: the binner restarts with every section empty, the capacity kept
    assert mc.binner_size() == (4, 0) and mc.fss_sums(1).n_meas == 0 and mc.fss_sums(1).n_k == 2
    mc.sweep(3)
    f = mc.fss_sums(1)
    assert f.n_meas == 3 and f.sum_M4 > 0 and mc.stats(1).n_meas == 7 and mc.fss_binner_level(1, 0)[3] == 3
    with pytest.raises(gpu.DQMCError) as e:  # 7 M2 measurements but 3 of M4
        mc.fss(1)
    assert e.value.code == -4
    mc.set_fss(_k_vectors(gpu, l, 1))  # again: the sums start anew
    f = mc.fss_sums(1)
    assert (f.n_meas, f.n_k, f.sum_M4, f.sum_S[0]) == (0, 1, 0.0, 0.0) and mc.binner_size() == (4, 0)
    mc.sweep(5)
    assert mc.fss_sums(1).n_meas == 5
    mc.reset_accumulators()
    f = mc.fss_sums(1)
    assert (f.n_meas, f.sum_M4, f.sum_S[0]) == (0, 0.0, 0.0) and mc.stats(1).n_meas == 0
    xs, x2, xy, cnt = mc.fss_binner_level(1, 0)
    assert cnt == 0 and not xs.any() and not x2.any() and not xy.any()
    mc.sweep(8)
    before = (mc.fss_sums(1).n_meas, mc.fss_sums(1).sum_M4, mc.conf(1).tolist(), mc.last_sweep)
    with pytest.raises(gpu.DQMCError) as e:  # 8 + 3 > 10: refused before anything runs
        mc.sweep(3)
    assert e.value.code == -4
    assert (mc.fss_sums(1).n_meas, mc.fss_sums(1).sum_M4, mc.conf(1).tolist(), mc.last_sweep) == before
    mc.sweep(2)
    out = mc.fss(1)
    assert out["n_meas"] == 10 and out["S"].shape == (1,) and out["xi_over_L"].shape == (1,)
    assert out["M4"] == mc.fss_sums(1).sum_M4 / 10 and out["U4"] == pytest.approx(1.0 - out["M4"] / (3.0 * out["M2"] ** 2), rel=1e-14)
    mc.set_fss(None)
    assert mc.fss_sums(1).n_k == -1 and mc.binner_size() == (4, 0)
    mc.sweep(2)  # as a handle that never had it
    assert mc.stats(1).n_meas == 12
    from montecarlo_jl_amd import _lib
    import ctypes as C
    tab = (C.c_int32 * 72)(*([2 ** 30 + 1] * 72))
    assert _lib.lib().dqmc_mc_set_fss(mc._h, 9, tab, tab) == -1 and _lib.lib().dqmc_mc_set_fss(mc._h, 1, None, tab) == -1
    assert _lib.lib().dqmc_mc_set_fss(mc._h, 1, tab, tab) == -1  # an entry above 2^30
    mc.close()


def _exact_4x4_fss(beta, kvec):
    """<M2>, <M4>, <S(k)> and U4 of the 4x4 periodic Ising model by enumeration of its 2^16 states"""
    from montecarlo_jl_amd import lattices
    l = lattices.SquareLattice(4)
    bits = (np.arange(1 << 16)[:, None] >> np.arange(16)) & 1
    s = (2 * bits - 1).astype(np.float64)
    b = np.asarray(l.bonds)[:, :2] - 1
    E = -(s[:, b[:, 0]] * s[:, b[:, 1]]).sum(axis=1)
    wgt = np.exp(-beta * (E - E.min()))
    wgt /= wgt.sum()
    M = s.sum(axis=1)
    ph = np.array(lattices._positions(l)) @ np.asarray(kvec)
    Sk = ((s @ np.cos(ph)) ** 2 + (s @ np.sin(ph)) ** 2) / 16.0
    M2, M4 = float(wgt @ M ** 2), float(wgt @ M ** 4)
    return {"M2": M2, "M4": M4, "S": float(wgt @ Sk), "U4": 1.0 - M4 / (3.0 * M2 * M2)}


def test_physics_4x4_at_tc(gpu):
    """256 chains at T_c with cluster moves against the exact enumeration: <M4>, S at k = (2 pi / 4, 0) and U4 within 6
    pooled standard errors.  The chain is reproducible bit for bit, so the outcome is fixed."""
    W = 256
    mc = gpu.MC(gpu.IsingModel(dims=2, L=4), T=gpu.IsingTc, n_walkers=W, seed=2024, thermalization=200, sweeps=2000,
                cluster_moves=True, binning=True, fss=True)
    mc.run()
    assert np.allclose(mc.k_vectors[0], [2 * math.pi / 4, 0.0], rtol=0, atol=1e-15)
    ex = _exact_4x4_fss(1.0 / gpu.IsingTc, mc.k_vectors[0])
    got = mc.binned_fss(walkers=range(W))
    assert got["count"] == 2000 >> got["level"] and got["n_walkers"] == W
    for name, o in (("M4", got["M4"]), ("S", got["S"][0]), ("U4", got["U4"])):
        print(name, o, ex[name], (o["mean"] - ex[name]) / o["std_error"])
        assert o["std_error"] > 0 and abs(o["mean"] - ex[name]) <= 6.0 * o["std_error"], (name, o, ex[name])
    plain = mc.fss(0)
    assert plain["n_meas"] == 2000 and 0.0 < plain["U4"] < 2.0 / 3.0 and plain["xi_over_L"].shape == (2,)
    mc.close()
