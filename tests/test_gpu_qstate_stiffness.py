"""The q-state engine's stiffness measurement on the device (csrc/qs_stiffness.inl: qs_stiffness_kernel behind every
measured sweep; include/dqmc_hip.h, "Stiffness" of the q-state section) against the numpy restatement of
tests/qstate_stiffness_ref.py.

The method: measure_rate = 1, sweep(1) over and over, mc.conf(w) after each call, the class sums and T, J, J2 on the host
from that configuration, summed in the order of the measurements.  n_meas, the sums, the last sample's I_c and K_c and
every level of the binner's stiffness section are compared with ==: the class sums are exact integers and the fp64 part
is defined operation by operation (no element has a square root).  Twin handles with the same seeds do the same sweeps
in one call, or without the measurement."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_stiffness_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("energy_q30", "mx_q30", "my_q30", "sum_E", "sum_E2", "sum_absM", "sum_M2", "sum_M4", "n_meas",
               "prop_local", "acc_local", "sweeps_drawn", "confs_drawn", "n_series", "n_colours")
S3 = 0.8660254037844386
SIGNED5 = [1.0, -0.5, 0.25, 0.25, -0.5]  # a signed, non-monotone table, e[d] == e[5 - d]
# twist tables at the magnitude bound with J = -2: |J d| = 4 for the entries 2.0
TWIST5 = ([0.0, 2.0, -0.3, 0.3, -2.0], [-2.0, 0.7, 2.0, 2.0, 0.7])

# name: (lattice, directions, walkers, sweeps)
SHAPES = {
    "chain7": (lambda g: g.Chain(7), True, 3, 8),                       # N % 4 != 0, N < one wave, one class
    "square3": (lambda g: g.SquareLattice(3), True, 3, 8),
    "square17": (lambda g: g.SquareLattice(17), True, 3, 8),            # N = 289 > THREADS: strided loop, padding
    "triangular6": (lambda g: g.TriangularLattice(6), [[0.5, S3], [1.0, 0.0]], 3, 8),  # z = 6, three classes, x not integer
    "honeycomb3": (lambda g: g.HoneycombLattice(3), True, 3, 8),        # the class depends on the sublattice
    "bilayer3": (lambda g: g.BilayerSquareLattice(3), True, 3, 8),      # z = 5, a class of zero projection
    "cubic4x3": (lambda g: g.CubicLattice(4, 3), True, 3, 8),           # z = 8, four classes, n_dir = 4
    "square128": (lambda g: g.SquareLattice(128), True, 1, 2),          # N = 16384: the LDS limit
}


def _model(g, kind, q, l):
    if kind == "clock":
        return g.ClockModel(q, l=l), ref.clock_twist(q), 1.0
    return g.QStateModel(q, SIGNED5, l=l, J=-2.0, twist=TWIST5), TWIST5, -2.0


def _host(g, l, q, twist, J, directions, ws, capacity=None):
    cls, vec, x = g.bond_classes(l, directions)
    return ref.Measurer(l, q, twist, x, cls, ws, J=J, capacity=capacity)


def _stepwise(mc, host, n):
    """n x sweep(1); the host measures where the engine's rule does"""
    for _ in range(n):
        mc.sweep(1)
        s = mc.last_sweep
        if s > mc.thermalization and s % mc.measure_rate == 0:
            host.take(mc.conf)


def _levels(mc, w, getter):
    return [tuple(x.tolist() if hasattr(x, "tolist") else x for x in getter(w, l)) for l in range(mc.binner_size()[0])]


def _stiff_state(mc, w, binner):
    f = mc.stiffness_sums(w)
    I, K = mc.stiffness_sample(w)
    return [f.n_meas, f.n_dir, list(f.sum_T), list(f.sum_J), list(f.sum_J2), I.tolist(), K.tolist()] + (
        [_levels(mc, w, mc.stiffness_binner_level)] if binner else [])


def _chain_state(mc, w, binner):
    """everything of walker w that a handle without the measurement has, in a form that compares with =="""
    st, cl, x = mc.stats(w), mc.cluster_stats(w), mc.exchange_stats(w)
    out = [[getattr(st, f) for f in STAT_FIELDS], [a.tolist() for a in mc.series(w)], mc.conf(w).tolist(),
           [cl.prop_global, cl.acc_global, cl.sum_cluster_size, cl.moves_drawn],
           [x.prop_exchange, x.acc_exchange, x.replica, x.rounds]]
    if binner:
        out.append(_levels(mc, w, mc.binner_level))
    return out


def _check(mc, host, label):
    """sums, the last sample and, where the host bins, every level of the stiffness section: bit for bit"""
    nd = host.n_dir
    for w in host.ws:
        f = mc.stiffness_sums(w)
        assert (f.n_meas, f.n_dir) == (host.n, nd), (label, w, f.n_meas, host.n)
        for name, got, want in (("T", f.sum_T, host.sum_T[w]), ("J", f.sum_J, host.sum_J[w]), ("J2", f.sum_J2, host.sum_J2[w])):
            print(label, w, "sum_" + name, list(got[:nd]), want)
            assert np.array_equal(np.array(got[:nd]), want), (label, w, name, list(got), want)
            assert not any(got[nd:])
        I, K = mc.stiffness_sample(w)
        assert np.array_equal(I, host.sample[w][0]) and np.array_equal(K, host.sample[w][1]), (label, w, I, K, host.sample[w])
        if host.bins:
            b = host.bins[w]
            L, T = mc.binner_size()
            assert L == b.L and T == host.n
            for lv in range(L):
                xs, x2, xy, cnt = mc.stiffness_binner_level(w, lv)
                assert cnt == b.count[lv] == T >> lv, (label, w, lv)
                assert np.array_equal(xs, b.x_sum[lv]), (label, w, lv, xs, b.x_sum[lv])
                assert np.array_equal(x2, b.x2_sum[lv]), (label, w, lv, x2, b.x2_sum[lv])
                assert np.array_equal(xy, b.xy_sum[lv]), (label, w, lv, xy, b.xy_sum[lv])


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_host(gpu, name):
    make, directions, W, n = SHAPES[name]
    l = make(gpu)
    q = 6
    model, twist, J = _model(gpu, "clock", q, l)
    betas = np.linspace(0.4, 1.6, W) if W > 1 else 0.9
    mc = gpu.MC(model, beta=betas, n_walkers=W, seed=41, stiffness=directions, binner=12)
    assert type(mc) is gpu.QStateMC
    host = _host(gpu, l, q, twist, J, directions, range(W), capacity=12)
    assert len(mc.stiffness_directions) == host.n_dir and len(mc.bond_vectors) == host.n_c
    _stepwise(mc, host, n)
    assert host.n == n
    _check(mc, host, name)
    if name == "bilayer3":  # the interlayer class projects to zero on both directions and still has its sums
        assert not host.x[:, 2].any() and (host.cls == 2).sum() == 9 and host.sample[0][1][2] % 2 ** 29 == 0
    out = mc.stiffness(0)
    beta0 = float(np.atleast_1d(betas)[0])
    assert out["n_meas"] == n and out["Upsilon"].shape == (host.n_dir,) and out["directions"].shape[0] == host.n_dir
    want = (host.sum_T[0] / n - beta0 * (host.sum_J2[0] / n)) / len(l)
    assert np.array_equal(out["Upsilon"], want) and np.array_equal(out["J"], host.sum_J[0] / n)
    mc.close()


@pytest.mark.parametrize("kind, q", [("clock", 2), ("clock", 5), ("clock", 64), ("signed", 5)])
def test_states_and_tables(gpu, kind, q):
    """q = 2: d1 = 0, so J is +0.0 at every measurement; q = 64: the largest tables; the signed model: pair energies and
    twist tables of both signs at the magnitude bound |J d| = 4 (2^32 in the integer tables), J < 0"""
    l = gpu.SquareLattice(6)
    model, twist, J = _model(gpu, kind, q, l)
    W = 3
    betas = [0.2, 0.5, 0.8] if kind == "signed" else [0.5, 1.0, 2.0]
    mc = gpu.MC(model, beta=betas, n_walkers=W, seed=7, stiffness=True, binner=20)
    if kind == "signed":
        assert np.abs(model.twist_q30[0]).max() == 2 ** 32 == np.abs(model.twist_q30[1]).max()
    host = _host(gpu, l, q, twist, J, True, range(W), capacity=20)
    assert np.array_equal(host.d1, model.twist_q30[0]) and np.array_equal(host.d2, model.twist_q30[1])
    _stepwise(mc, host, 10)
    _check(mc, host, "%s%d" % (kind, q))
    for w in range(W):
        f = mc.stiffness_sums(w)
        if q == 2:
            assert not any(f.sum_J) and not any(f.sum_J2) and not mc.stiffness_sample(w)[0].any()
        else:
            assert any(f.sum_J2[:2]) and any(f.sum_T[:2])
    mc.close()


def test_with_cluster_moves(gpu):
    l = gpu.SquareLattice(6)
    q, W = 6, 3
    model, twist, J = _model(gpu, "clock", q, l)
    kw = dict(beta=[0.8, 1.1, 1.4], n_walkers=W, seed=19, cluster_rate=1, stiffness=True)
    mc, once = gpu.MC(model, **kw), gpu.MC(model, **kw)
    host = _host(gpu, l, q, twist, J, True, range(W))
    _stepwise(mc, host, 10)
    once.sweep(10)
    _check(mc, host, "cluster")
    assert sum(mc.cluster_stats(w).acc_global for w in range(W)) > 0
    for w in range(W):
        assert _stiff_state(mc, w, False) == _stiff_state(once, w, False) and _chain_state(mc, w, False) == _chain_state(once, w, False)
    mc.close()
    once.close()


def test_with_an_exchange_round_behind_every_sweep(gpu):
    """tempering=(4, 1): every E, M measurement is the exchange kernel's; the stiffness kernel runs behind it, on the
    configuration the slot holds after the swap, which is what mc.conf(w) reads after the call"""
    l = gpu.SquareLattice(6)
    q, W = 5, 8
    model, twist, J = _model(gpu, "clock", q, l)
    kw = dict(beta=np.linspace(0.5, 0.9, 4), n_walkers=W, seed=31, stiffness=True, tempering=(4, 1), binner=16)
    mc, once = gpu.MC(model, **kw), gpu.MC(model, **kw)
    host = _host(gpu, l, q, twist, J, True, range(W), capacity=16)
    _stepwise(mc, host, 12)
    once.sweep(12)
    _check(mc, host, "exchange")
    assert sum(mc.exchange_stats(w).acc_exchange for w in range(W)) > 0  # (configurations did change slots)
    for w in range(W):
        assert _stiff_state(mc, w, True) == _stiff_state(once, w, True), w
        assert mc.stats(w).n_meas == 12
    mc.close()
    once.close()


def test_beside_the_scaling_measurement(gpu):
    """both measurements on: one cut, two kernels; the stiffness section against the host, the scaling sums and its
    binner section bit for bit those of a handle without stiffness"""
    l = gpu.SquareLattice(6)
    q, W = 6, 3
    model, twist, J = _model(gpu, "clock", q, l)
    kw = dict(beta=[0.7, 1.0, 1.3], n_walkers=W, seed=23, scaling=True, binner=16, cluster_rate=2, thermalization=2,
              measure_rate=2)
    both, plain = gpu.MC(model, stiffness=True, **kw), gpu.MC(model, **kw)
    host = _host(gpu, l, q, twist, J, True, range(W), capacity=16)
    _stepwise(both, host, 12)
    plain.sweep(12)
    assert host.n == 5
    _check(both, host, "both")
    for w in range(W):
        a, b = both.scaling_sums(w), plain.scaling_sums(w)
        assert (a.n_meas, a.n_k, list(a.sum_S)) == (b.n_meas, b.n_k, list(b.sum_S)) and a.n_meas == 5
        assert _levels(both, w, both.scaling_binner_level) == _levels(plain, w, plain.scaling_binner_level)
        assert _chain_state(both, w, True) == _chain_state(plain, w, True)
    assert plain.stiffness_sums(0).n_dir == 0
    both.close()
    plain.close()


def test_switching_mid_run(gpu):
    l = gpu.SquareLattice(6)
    q, W = 6, 3
    model, twist, J = _model(gpu, "clock", q, l)
    kw = dict(beta=[0.7, 1.0, 1.3], n_walkers=W, seed=29, binner=16)
    mc, plain = gpu.MC(model, **kw), gpu.MC(model, **kw)
    mc.sweep(4)
    plain.sweep(4)
    assert mc.stiffness_sums(1).n_dir == 0 and mc.stiffness_directions is None and mc.binner_size() == (5, 4)
    with pytest.raises(gpu.DQMCError) as e:
        mc.stiffness(1)
    assert e.value.code == -4
    with pytest.raises(gpu.DQMCError) as e:  # no stiffness section yet
        mc.stiffness_binner_level(1, 0)
    assert e.value.code == -4
    mc.set_stiffness(True)  # mid-run: the binner restarts with every section empty, the capacity kept
    assert mc.binner_size() == (5, 0) and mc.stiffness_sums(1).n_meas == 0 and mc.stiffness_sums(1).n_dir == 2
    with pytest.raises(gpu.DQMCError) as e:  # nothing measured yet
        mc.stiffness(1)
    assert e.value.code == -1
    host = _host(gpu, l, q, twist, J, True, range(W), capacity=16)
    _stepwise(mc, host, 5)
    _check(mc, host, "mid-run")
    assert mc.stiffness_sums(1).n_meas == 5 and mc.stats(1).n_meas == 9  # an n_meas of its own
    mc.reset_accumulators()
    assert _stiff_state(mc, 1, True)[0] == 0 and not any(mc.stiffness_sums(1).sum_T) and not mc.stiffness_sample(1)[1].any()
    xs, x2, xy, cnt = mc.stiffness_binner_level(1, 0)
    assert cnt == 0 and not xs.any() and not x2.any() and not xy.any()
    mc.set_stiffness([[0.0, 1.0]])  # another set of directions: the sums start anew
    assert mc.stiffness_sums(1).n_dir == 1 and mc.stiffness_binner_level(1, 0)[0].shape == (2,)
    mc.sweep(2)
    assert mc.stiffness_sums(1).n_meas == 2
    # off again: a handle that never had the measurement
    mc.set_stiffness(None)
    assert mc.stiffness_sums(1).n_dir == 0 and mc.stiffness_directions is None and mc.binner_size() == (5, 0)
    plain.sweep(7)
    plain.enable_binning(16)
    mc.sweep(6)
    plain.sweep(6)
    for w in range(W):
        assert mc.conf(w).tolist() == plain.conf(w).tolist()
        assert _levels(mc, w, mc.binner_level) == _levels(plain, w, plain.binner_level)
        assert [getattr(mc.stats(w), f) for f in STAT_FIELDS[:3]] == [getattr(plain.stats(w), f) for f in STAT_FIELDS[:3]]
    with pytest.raises(gpu.DQMCError) as e:
        mc.stiffness_binner_finish(1)
    assert e.value.code == -4
    mc.close()
    plain.close()


def test_invariance(gpu):
    """1 + 5 sweeps against 6 in one call; walker w of three against a handle of one walker with w's key; and the chain
    (conf, stats, series, the first binner section) against a handle without the measurement"""
    l = gpu.SquareLattice(17)
    q, W = 6, 3
    betas = [0.6, 1.0, 1.4]
    kw = dict(n_walkers=W, seed=53, binner=10, series_capacity=8, cluster_rate=3)
    model = gpu.ClockModel(q, l=l)
    split, once = gpu.MC(model, beta=betas, stiffness=True, **kw), gpu.MC(model, beta=betas, stiffness=True, **kw)
    off = gpu.MC(model, beta=betas, **kw)
    split.sweep(1)
    split.sweep(5)
    once.sweep(6)
    off.sweep(6)
    for w in range(W):
        assert _stiff_state(split, w, True) == _stiff_state(once, w, True), w
        assert _chain_state(split, w, True) == _chain_state(once, w, True) == _chain_state(off, w, True), w
        single = gpu.MC(model, beta=betas[w], n_walkers=1, seed=53, first_walker=w, stiffness=True, binner=10,
                        series_capacity=8, cluster_rate=3)
        single.sweep(6)
        assert _stiff_state(single, 0, True) == _stiff_state(once, w, True), w
        single.close()
    assert once.stiffness_sums(0).n_meas == 6 and any(once.stiffness_sums(0).sum_J2[:2])
    for h in (split, once, off):
        h.close()


@pytest.mark.parametrize("n, capacity", [(37, 40), (7, 7)])
def test_binner_section(gpu, n, capacity):
    """37 pushes at capacity 40 pass several compressor levels; 7 at capacity 7 fill the top level.  binned_stiffness
    against the restatement's delta-method value at 1e-12, the margin of the binned_scaling tests: host fp64 formulas of
    identical inputs"""
    l = gpu.SquareLattice(6)
    q, W = 6, 66
    model, twist, J = _model(gpu, "clock", q, l)
    betas = np.linspace(0.7, 1.4, W)
    mc = gpu.MC(model, beta=betas, n_walkers=W, seed=99, cluster_rate=4, binner=capacity, stiffness=True)
    ws = [1, 65]
    host = _host(gpu, l, q, twist, J, True, ws, capacity=capacity)
    _stepwise(mc, host, n)
    assert mc.binner_size() == (math.ceil(math.log2(capacity + 1)), n)
    _check(mc, host, "binner%d" % n)
    N = len(l)
    for w in ws:
        b = host.bins[w]
        lv = b.reliable_level()
        f = mc.stiffness_binner_finish(w)
        assert (f.level, f.count, f.n_dir) == (lv, b.count[lv], 2)
        np.testing.assert_allclose(f.mean[:4], b.mean(), rtol=1e-12)
        np.testing.assert_allclose(f.varN[:4], b.varN(lv), rtol=1e-12)
        np.testing.assert_allclose(f.covN[:2], b.covN(lv), rtol=1e-12)
        assert not any(f.mean[4:]) and not any(f.covN[2:])
        got = mc.binned_stiffness(w)
        assert (got["count"], got["level"]) == (b.count[lv], lv)
        for mu in range(2):
            U, var = ref.binned_upsilon(b, mu, float(betas[w]), N)
            print(w, mu, got["Upsilon"][mu], U, math.sqrt(var))
            assert got["Upsilon"][mu]["mean"] == pytest.approx(U, rel=1e-12)
            assert got["Upsilon"][mu]["std_error"] == pytest.approx(math.sqrt(var), rel=1e-12)
            assert "tau" not in got["Upsilon"][mu]
            for key, e in (("T", 2 * mu), ("J2", 2 * mu + 1)):
                assert got[key][mu]["mean"] == pytest.approx(b.mean()[e], rel=1e-12)
                assert got[key][mu]["std_error"] == pytest.approx(math.sqrt(max(b.varN(lv)[e], 0.0)), rel=1e-12)
                assert got[key][mu]["tau"] == pytest.approx(b.tau(lv)[e], rel=1e-12, nan_ok=True)
    pooled = mc.binned_stiffness(walkers=[1, 1])
    assert pooled["n_walkers"] == 2 and pooled["Upsilon"][0]["mean"] == pytest.approx(mc.binned_stiffness(1)["Upsilon"][0]["mean"])
    with pytest.raises(ValueError, match="share one beta"):
        mc.binned_stiffness(walkers=[1, 2])
    mc.close()


def test_capacity_is_checked_before_anything_runs(gpu):
    l = gpu.SquareLattice(6)
    mc = gpu.MC(gpu.ClockModel(6, l=l), beta=[0.8, 1.2], n_walkers=2, seed=3, binner=7, stiffness=True)
    before = [(_stiff_state(mc, w, True), _chain_state(mc, w, True)) for w in range(2)], mc.last_sweep
    with pytest.raises(gpu.DQMCError) as e:
        mc.sweep(13)
    assert e.value.code == -4
    assert ([(_stiff_state(mc, w, True), _chain_state(mc, w, True)) for w in range(2)], mc.last_sweep) == before
    mc.sweep(7)
    assert mc.stiffness_sums(1).n_meas == 7 and mc.stiffness_binner_level(1, 0)[3] == 7
    with pytest.raises(gpu.DQMCError) as e:
        mc.sweep(1)
    assert e.value.code == -4 and mc.stiffness_sums(1).n_meas == 7
    mc.close()


def test_refused_arguments_leave_the_handle_as_it_was(gpu):
    """every DQMC_ERR_INVALID branch of dqmc_qs_set_stiffness, each from an accepted argument set with one thing wrong"""
    from montecarlo_jl_amd import _lib
    l = gpu.SquareLattice(6)
    q, N, z = 5, 36, 4
    model = gpu.ClockModel(q, l=l)
    mc = gpu.MC(model, beta=[0.8, 1.2], n_walkers=2, seed=3, binner=20, stiffness=True)
    mc.sweep(3)
    before = [_stiff_state(mc, w, True) for w in range(2)], mc.binner_size()
    cls, vec, x = gpu.bond_classes(l, True)
    d1, d2 = (np.array(t) for t in model.twist_q30)
    f = _lib.lib().dqmc_qs_set_stiffness

    def call(n_dir=2, n_c=2, c=cls, a=d1, b=d2, xx=x):
        cc = None if c is None else np.asfortranarray(c, dtype=np.int8)
        aa = None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.int64)
        xc = None if xx is None else np.ascontiguousarray(xx, dtype=np.float64)
        p = lambda v, t: None if v is None else v.ctypes.data_as(C.POINTER(t))  # noqa: E731
        return f(mc._h, n_dir, n_c, p(cc, C.c_int8), p(aa, C.c_int64), p(bb, C.c_int64), p(xc, C.c_double))

    def changed(arr, at, v):
        out = np.array(arr).copy()
        out[at] = v
        return out

    bad = [dict(n_dir=5), dict(n_dir=-1), dict(n_c=0), dict(n_c=9), dict(c=None), dict(a=None), dict(b=None), dict(xx=None),
           dict(c=changed(cls, (z - 1, N - 1), 2)), dict(c=changed(cls, (0, 0), -2)),
           dict(a=changed(d1, 1, d1[1] + 1)), dict(a=changed(d1, 0, 1)), dict(b=changed(d2, 4, d2[4] - 1)),
           dict(a=changed(changed(d1, 1, 2 ** 32 + 1), 4, -2 ** 32 - 1)), dict(b=changed(d2, 0, -2 ** 32 - 1)),
           dict(xx=changed(x, (1, 1), np.inf)), dict(xx=changed(x, (0, 0), np.nan))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert ([_stiff_state(mc, w, True) for w in range(2)], mc.binner_size()) == before, kw
    mc.sweep(1)  # still on, still counting
    assert mc.stiffness_sums(1).n_meas == 4 and mc.binner_size() == (5, 4)
    assert call() == 0  # the accepted set: the sums and the binner start anew
    assert mc.stiffness_sums(1).n_meas == 0 and mc.binner_size() == (5, 0)
    mc.close()


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_physics(gpu, beta):
    """Clock q = 6 on SquareLattice(8), 64 walkers, cluster_rate = 1, 500 sweeps unmeasured and 2000 measured.  The pooled
    Upsilon_x and Upsilon_y agree within 4 standard errors of their difference (the two pooled errors in quadrature), at
    beta = 0.5 (disordered: Upsilon near 0) and at beta = 2.0 (ordered).  At beta = 2.0 each also lies within 4 standard
    errors (the device's and the reference's in quadrature: two independent estimates) of the value the restatement alone
    gets from the same number of sweeps of 8 walkers with local updates only (qstate_stiffness_ref.physics_reference):
    Upsilon_x = 0.945995 +- 0.000862, Upsilon_y = 0.946128 +- 0.000896.  The device's values are in the README."""
    W, N = 64, ref.PHYS_L ** 2
    mc = gpu.MC(gpu.ClockModel(ref.PHYS_Q, dims=2, L=ref.PHYS_L), beta=beta, n_walkers=W, seed=ref.PHYS_SEED,
                thermalization=ref.PHYS_THERM, cluster_rate=1, stiffness=True, binner=ref.PHYS_SWEEPS)
    mc.sweep(ref.PHYS_THERM + ref.PHYS_SWEEPS)
    got = mc.binned_stiffness(walkers=range(W))
    assert got["n_walkers"] == W and got["count"] == ref.PHYS_SWEEPS >> got["level"]
    ux, uy = got["Upsilon"]
    print("beta", beta, "Upsilon_x", ux, "Upsilon_y", uy)
    assert ux["std_error"] > 0 and uy["std_error"] > 0
    assert abs(ux["mean"] - uy["mean"]) <= 4.0 * math.hypot(ux["std_error"], uy["std_error"]), (ux, uy)
    plain = mc.stiffness(0)
    assert plain["n_meas"] == ref.PHYS_SWEEPS and plain["Upsilon"][0] == pytest.approx(
        mc.binned_stiffness(0)["Upsilon"][0]["mean"], rel=1e-12)
    if beta == 2.0:
        rx, ex, ry, ey = ref.physics_reference(beta)
        print("reference", rx, ex, ry, ey)
        for o, r, e in ((ux, rx, ex), (uy, ry, ey)):
            assert abs(o["mean"] - r) <= 4.0 * math.hypot(o["std_error"], e), (o, r, e)
    else:
        assert abs(ux["mean"]) < 0.2  # (far above the transitions the modulus vanishes up to finite-size terms)
    mc.close()
