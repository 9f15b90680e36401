"""The Ising flavor's device binner (ising.hip: ising_bin_push inside ising_sweep_binned_kernel<Z> and
ising_bin_push_kernel; include/dqmc_hip.h "error bars of the MC flavor") against the numpy restatement of
tests/ising_binner_ref.py, fed with the measurement series the same handle recorded (mc.series()).

Level sums are compared with np.array_equal.  Why equality is fair: E, |M| and their squares are integers, a level-l
value is the mean of 2^l of them and has at most l fractional bits, and at the sizes used here (8x8: |E| <= 128,
E^2 <= 2^14, M^2 <= 2^12, T <= 1024) every sum needs at most 28 + 2l + (10 - l) <= 48 bits: each is an exact dyadic
rational below 2^53 whatever the order of the additions and whether or not a product is fused into the sum.  The other
lattices of this file are smaller or run fewer measurements (cubic 4^3 and the z = 8 table of 40 sites: |E| <= 320,
E^4 < 2^34 and T = 40, 34 + 2l + (6 - l) <= 45 bits; 2x2: E^2 <= 2^6 and T < 2^13, 25 + l bits).

The statistics (finish, binned) are compared with the restatement's formulas on those bit-identical sums.  Their only
difference is a handful of roundings and a possible fused multiply-add in varN = (a - b)/n with a = x2_sum/(n - 1) and
b = x_sum^2/(n (n - 1)) (covN alike): |d varN| <= 64 eps (|a| + |b|)/n.  tau, the errors of C and chi and the pooled
results follow from varN and covN by first-order propagation of those bounds plus 8 eps of the terms of each formula."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ising_binner_ref import PAIRS, delta_variance, from_series, pool  # noqa: E402
from test_gpu_ising import STAT_FIELDS, _exact_4x4  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
GLOBAL_FIELDS = ("prop_global", "acc_global", "sum_cluster_size", "moves_drawn")


def _series(mc, walkers=None):
    ws = range(mc.n_walkers) if walkers is None else walkers
    per = [mc.series(w) for w in ws]
    return np.stack([p[0] for p in per], axis=1), np.stack([p[1] for p in per], axis=1)


def _restate(mc, capacity=None, walkers=None):
    E, M = _series(mc, walkers)
    return from_series(E, M) if capacity is None else from_series(E, M, capacity)


def _levels(mc, w):
    L, T = mc.binner_size()
    return [mc.binner_level(w, l) for l in range(L)]


def _same_levels(a, b):
    return len(a) == len(b) and all(np.array_equal(p[k], q[k]) for p, q in zip(a, b) for k in range(3)) and \
        all(p[3] == q[3] for p, q in zip(a, b))


def _assert_levels(label, mc, ref, walkers=None):
    L, T = mc.binner_size()
    assert (L, T) == (ref.L, int(ref.count[0])), (label, L, T, ref.L, ref.count[0])
    for i, w in enumerate(range(mc.n_walkers) if walkers is None else walkers):
        for l in range(L):
            xs, x2, xy, cnt = mc.binner_level(w, l)
            rs, r2, rxy, rc = ref.sums(i, l)
            assert cnt == rc == T >> l, (label, w, l, cnt, rc)
            assert np.array_equal(xs, rs), (label, "x_sum", w, l, xs, rs)
            assert np.array_equal(x2, r2), (label, "x2_sum", w, l, x2, r2)
            assert np.array_equal(xy, rxy), (label, "xy_sum", w, l, xy, rxy)


def _state(mc, w):
    st, g = mc.stats(w), mc.global_stats(w)
    e, m = mc.series(w)
    return ([getattr(st, f) for f in STAT_FIELDS] + [st.n_series] + [getattr(g, f) for f in GLOBAL_FIELDS],
            e.tolist(), m.tolist(), mc.conf(w).tolist())


@pytest.mark.parametrize("T,capacity", [(1000, None), (1023, 1023), (1024, 1024)])
def test_level_sums_bit_for_bit_and_the_chain_untouched(gpu, T, capacity):
    W, therm, rate = 100, 3, 2
    total = rate * T + 2  # measured sweeps 4, 6, ..., 2 T + 2
    kw = dict(beta=np.linspace(0.2, 0.6, W), n_walkers=W, seed=515, thermalization=therm, measure_rate=rate,
              series_capacity=T)
    model = gpu.IsingModel(dims=2, L=8)
    mc = gpu.MC(model, binning=True, binning_capacity=capacity, **kw)
    plain = gpu.MC(model, **kw)
    for n in (37, total - 37 - 611, 611):
        mc.sweep(n)
        plain.sweep(n)
    assert mc.binner_size() == (17 if capacity is None else 10 if capacity == 1023 else 11, T)
    assert mc.stats(0).n_meas == T == mc.stats(0).n_series
    _assert_levels("8x8", mc, _restate(mc, capacity))
    for w in range(W):
        assert _state(mc, w) == _state(plain, w), w
    with pytest.raises(gpu.DQMCError) as e:   # no binner on the other handle
        plain.binner_size()
    assert e.value.code == -4
    mc.close()
    plain.close()


class _Table:
    """N sites with the neighbours i + 1, ..., i + z (mod N), 1-based as the project's lattices, and the bonds that
    table lists; not symmetric - the device is only compared with the restatement of its own series"""

    def __init__(self, N, z):
        i = np.arange(N)
        self.sites = N
        self.neighs = np.vstack([(i + k) % N for k in range(1, z + 1)]).astype(np.int64) + 1
        self.bonds = np.array([(a, (a + k) % N) for k in range(1, z + 1) for a in i], dtype=np.int64) + 1

    def __len__(self):
        return self.sites


@pytest.mark.parametrize("global_rate", [1, 3])
@pytest.mark.parametrize("name,make", [
    ("chain10_z2", lambda g: g.Chain(10)),
    ("cubic4_z6", lambda g: g.CubicLattice(3, 4)),
    ("triangular4_z6", lambda g: g.TriangularLattice(4)),
    ("table_z1", lambda g: _Table(40, 1)),
    ("table_z3", lambda g: _Table(40, 3)),
    ("table_z4", lambda g: _Table(40, 4)),
    ("table_z5", lambda g: _Table(40, 5)),
    ("table_z7", lambda g: _Table(40, 7)),
    ("table_z8", lambda g: _Table(40, 8)),
])
def test_every_z_form_and_the_move_path(gpu, name, make, global_rate):
    """with cluster moves a measurement that follows a move is pushed by ising_bin_push_kernel, the others by the
    binned sweep form: global_rate 1 takes every one through the former, 3 one in three"""
    l = make(gpu)
    W, therm, sweeps = 70, 2, 40
    kw = dict(beta=np.linspace(0.1, 0.5, W), n_walkers=W, seed=99, thermalization=therm, series_capacity=sweeps,
              cluster_moves=True, global_rate=global_rate)
    mc = gpu.MC(gpu.IsingModel(l=l), binning=True, **kw)
    plain = gpu.MC(gpu.IsingModel(l=l), **kw)
    for n in (5, 17, therm + sweeps - 22):
        mc.sweep(n)
        plain.sweep(n)
    assert mc.binner_size()[1] == sweeps and mc.global_stats(0).prop_global == (therm + sweeps) // global_rate
    _assert_levels(name, mc, _restate(mc))
    for w in (0, 1, 63, 64, 69):
        assert _state(mc, w) == _state(plain, w), (name, w)
    mc.close()
    plain.close()


def test_batch_and_split_independence(gpu):
    model = gpu.IsingModel(dims=2, L=8)
    seed, therm, sweeps = 2718, 5, 150
    kw = dict(beta=0.44, seed=seed, thermalization=therm, binning=True, cluster_moves=True, global_rate=4)
    big = gpu.MC(model, n_walkers=100, **kw)
    big.sweep(therm + sweeps)
    rng = np.random.default_rng(3)
    mid = gpu.MC(model, n_walkers=100, **kw)
    while mid.last_sweep < therm + sweeps:
        mid.sweep(int(min(rng.integers(1, 17), therm + sweeps - mid.last_sweep)))
    for k in (0, 63, 64, 99):
        one = gpu.MC(model, n_walkers=1, first_walker=k, **kw)
        one.sweep(therm + sweeps)
        assert _same_levels(_levels(one, 0), _levels(big, k)), k
        assert _same_levels(_levels(mid, k), _levels(big, k)), k
        one.close()
    big.close()
    mid.close()
    # across a launch boundary: 2x2, the launch budget 2^28 / (4 * 16384) = 4096 sweeps
    small = gpu.IsingModel(dims=2, L=2)
    n = 4100
    kw = dict(beta=[0.2, 0.3, 0.4], n_walkers=3, seed=7, thermalization=1, binning=True, series_capacity=n)
    a = gpu.MC(small, **kw)
    a.sweep(n)
    b = gpu.MC(small, **kw)
    for part in (1000, 3000, 100):
        b.sweep(part)
    assert a.binner_size() == (17, n - 1)
    _assert_levels("2x2", a, _restate(a))
    for w in range(3):
        assert _same_levels(_levels(a, w), _levels(b, w)), w
    a.close()
    b.close()


def test_capacity_reset_and_reenable(gpu):
    model = gpu.IsingModel(dims=2, L=8)
    W = 70
    mc = gpu.MC(model, beta=np.linspace(0.3, 0.5, W), n_walkers=W, seed=31, series_capacity=16, cluster_moves=True,
                global_rate=2, binning=True, binning_capacity=10)
    mc.sweep(7)

    def everything():
        return [(_state(mc, w), [tuple(np.concatenate(lv[:3]).tolist()) + (lv[3],) for lv in _levels(mc, w)])
                for w in (0, 63, 64, 69)] + [mc.binner_size(), mc.binner_reliable_level(), mc.last_sweep]

    before = everything()
    with pytest.raises(gpu.DQMCError) as e:
        mc.sweep(4)  # 7 + 4 measurements > 10: refused before anything runs
    assert e.value.code == -4
    assert everything() == before
    mc.global_move()  # no measurement: the chain moves, the binner does not
    assert [s[1] for s in everything()[:4]] == [s[1] for s in before[:4]] and mc.binner_size() == (4, 7)
    assert mc.global_stats(0).prop_global == 3 + 1
    mc.sweep(3)
    assert mc.binner_size() == (4, 10)
    _assert_levels("full", mc, _restate(mc, 10))
    mc.reset_accumulators()
    assert mc.binner_size() == (4, 0) and mc.stats(0).n_meas == 0
    for w in (0, 69):
        for xs, x2, xy, cnt in _levels(mc, w):
            assert cnt == 0 and not xs.any() and not x2.any() and not xy.any()
    mc.sweep(5)  # (the compressors were cleared too)
    _assert_levels("after reset", mc, _restate(mc, 10))
    mc.enable_binning(100)
    assert mc.binner_size() == (7, 0)
    for xs, x2, xy, cnt in _levels(mc, 69):
        assert cnt == 0 and not xs.any() and not x2.any() and not xy.any()
    mc.sweep(11)
    E, M = _series(mc)
    _assert_levels("re-enabled", mc, from_series(E[5:], M[5:], 100))
    mc.close()


# ---- statistics
def _varN_bound(a_sum, b_sum, q_sum, n):
    """64 eps (|a| + |b|)/n for (q/(n - 1) - a b/(n (n - 1)))/n"""
    return 64.0 * EPS * (abs(q_sum) / (n - 1.0) + abs(a_sum * b_sum) / (n * (n - 1.0))) / n


def _close(label, got, want, bound):
    if math.isnan(want):
        assert math.isnan(got), (label, got, want)
    else:
        assert abs(got - want) <= bound, (label, got, want, abs(got - want), bound)


def _sqrt_bound(var, d):
    """bound on sqrt(max(var, 0)) from the bound d on var (unused where var is NaN)"""
    if var != var:
        return 0.0
    return (min(d / math.sqrt(var), math.sqrt(d)) if var > 0 else math.sqrt(d)) + 4.0 * EPS * math.sqrt(max(var, 0.0))


def _walker_reference(ref, i, level, beta, N):
    """{name: dict(mean, dmean, var, dvar, v0, dv0, tau, dtau)} of walker i of the restatement (var = the variance of
    the mean at `level`, v0 at level 0, d* = the bounds of the module docstring; C and chi have no v0 and no tau), and
    covN with its bounds"""
    mean, vl, v0, cov = ref.mean_w(i), ref.varN_w(i, level), ref.varN_w(i, 0), ref.covN_w(i, level)
    xs, x2, xy, n = ref.sums(i, level)
    xs0, x20, _, n0 = ref.sums(i, 0)
    dvl = [_varN_bound(xs[k], xs[k], x2[k], n) if n >= 2 else math.nan for k in range(4)]
    dv0 = [_varN_bound(xs0[k], xs0[k], x20[k], n0) if n0 >= 2 else math.nan for k in range(4)]
    dcov = [_varN_bound(xs[a], xs[b], xy[q], n) if n >= 2 else math.nan for q, (a, b) in enumerate(PAIRS)]
    out, invN = {}, 1.0 / N
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, name in enumerate(("E", "E2", "M", "M2")):
            ratio = vl[k] / v0[k]
            out[name] = dict(mean=mean[k], dmean=0.0, var=vl[k], dvar=dvl[k], v0=v0[k], dv0=dv0[k],
                             tau=0.5 * (ratio - 1.0), dtau=_ratio_bound(vl[k], dvl[k], v0[k], dv0[k]))
        for name, src in (("e", "E"), ("m", "M")):
            o, s2 = out[src], invN * invN
            out[name] = dict(mean=o["mean"] * invN, dmean=0.0, var=o["var"] * s2,
                             dvar=(o["dvar"] + 4.0 * EPS * abs(o["var"])) * s2, v0=o["v0"] * s2,
                             dv0=(o["dv0"] + 4.0 * EPS * abs(o["v0"])) * s2, tau=o["tau"], dtau=2.0 * o["dtau"])
        for name, pair, scale in (("C", 0, beta * beta * invN), ("chi", 1, beta * invN)):
            a, b = PAIRS[pair]
            x = mean[a]
            terms = abs(vl[b]) + 4.0 * abs(x * cov[pair]) + 4.0 * x * x * abs(vl[a])
            out[name] = dict(mean=scale * (mean[b] - x * x), dmean=8.0 * EPS * scale * (abs(mean[b]) + x * x),
                             var=float(delta_variance(scale, x, vl[a], vl[b], cov[pair])),
                             dvar=scale * scale * (dvl[b] + 4.0 * abs(x) * dcov[pair] + 4.0 * x * x * dvl[a] +
                                                   8.0 * EPS * terms), v0=None, dv0=None, tau=None, dtau=None)
    return out, cov, dcov


def _ratio_bound(vl, dvl, v0, dv0):
    """bound on tau = (vl / v0 - 1)/2 from those on vl and v0"""
    return 0.5 * (dvl / abs(v0) + abs(vl) * dv0 / (v0 * v0)) + 8.0 * EPS * (abs(vl / v0) + 1.0)


def _std_error(var):
    return math.sqrt(max(var, 0.0)) if var == var else var


GROUPS = (("Energy", ("E", "E2", "e", "C")), ("Magn", ("M", "M2", "m", "chi")))


@pytest.fixture(scope="module")
def finished(gpu):
    """one run shared by the statistics tests: 8x8, 70 walkers of one beta, 300 measurements"""
    W, T = 70, 300
    mc = gpu.MC(gpu.IsingModel(dims=2, L=8), beta=0.4, n_walkers=W, seed=808, thermalization=10, series_capacity=T,
                binning=True)
    mc.sweep(10 + T)
    ref = _restate(mc)
    yield mc, ref
    mc.close()


@pytest.mark.parametrize("level", [None, 0, 5, 8, 16])
def test_finish_against_the_restatement(gpu, finished, level):
    """level None: the reliable one (3 at T = 300); 8: one sample, NaN errors; 16: no sample"""
    mc, ref = finished
    lv = ref.reliable_level() if level is None else level
    assert mc.binner_reliable_level() == ref.reliable_level() == 3
    for w in (0, 63, 64, 69):
        want, cov, dcov = _walker_reference(ref, w, lv, 0.4, 64)
        b = mc.binner_finish(w, level)
        assert (b.level, b.count) == (lv, ref.count[lv])
        for k, name in enumerate(("E", "E2", "M", "M2")):
            r = want[name]
            assert b.mean[k] == r["mean"], (w, name)
            _close((w, name, "varN"), b.varN[k], r["var"], r["dvar"])
            _close((w, name, "varN0"), b.varN0[k], r["v0"], r["dv0"])
            _close((w, name, "tau"), b.tau[k], r["tau"], r["dtau"])
        for q in range(2):
            _close((w, "covN", q), b.covN[q], cov[q], dcov[q])
        got = mc.binned(w, level)
        assert (got["level"], got["count"]) == (lv, ref.count[lv])
        for group, names in GROUPS:
            for name in names:
                o, r = got[group][name], want[name]
                _close((w, name, "mean"), o["mean"], r["mean"], r["dmean"])
                _close((w, name, "std_error"), o["std_error"], _std_error(r["var"]), _sqrt_bound(r["var"], r["dvar"]))
                assert ("tau" in o) == (r["tau"] is not None) and "std_error_walkers" not in o, name
                if r["tau"] is not None:
                    _close((w, name, "tau"), o["tau"], r["tau"], r["dtau"])


def test_pooled_results_against_the_restatement(gpu, finished):
    mc, ref = finished
    ws = list(range(70))
    lv, W = ref.reliable_level(), 70.0
    per = [_walker_reference(ref, w, lv, 0.4, 64)[0] for w in ws]
    got = mc.binned(walkers=ws)
    assert got["n_walkers"] == 70 and got["level"] == lv and got["count"] == ref.count[lv]
    for group, names in GROUPS:
        for name in names:
            o, rs = got[group][name], [p[name] for p in per]
            mean, se, sew = pool([r["mean"] for r in rs], [r["var"] for r in rs])
            dmean = sum(r["dmean"] for r in rs) / W + W * EPS * max(abs(r["mean"]) for r in rs)
            vsum = sum(r["var"] for r in rs)
            dv = sum(r["dvar"] for r in rs) + W * EPS * sum(abs(r["var"]) for r in rs)
            _close((name, "mean"), o["mean"], mean, dmean)
            _close((name, "std_error"), o["std_error"], se, _sqrt_bound(vsum, dv) / W)
            _close((name, "std_error_walkers"), o["std_error_walkers"], sew,
                   2.0 * (max(r["dmean"] for r in rs) + dmean) / math.sqrt(W - 1.0) + 8.0 * EPS * sew)
            assert ("tau" in o) == (rs[0]["tau"] is not None), name
            if rs[0]["tau"] is not None:
                v0 = sum(r["v0"] for r in rs)
                dv0 = sum(r["dv0"] for r in rs) + W * EPS * sum(abs(r["v0"]) for r in rs)
                _close((name, "tau"), o["tau"], 0.5 * (vsum / v0 - 1.0), _ratio_bound(vsum, dv, v0, dv0))
    two = gpu.MC(gpu.IsingModel(dims=2, L=4), beta=[0.3, 0.4], n_walkers=2, binning=True)
    with pytest.raises(ValueError):
        two.binned(walkers=[0, 1])
    two.close()


def test_physics_4x4_at_beta_044(gpu):
    """256 chains with a cluster move per sweep against the exact enumeration of the 2^16 states.  E and |M| within 5
    pooled std_error; C and chi within 5 delta-method errors plus the bias of a variance estimated from T correlated
    samples, value (2 tau + 1)/T with the device's tau of E and |M|; and the binned error against the error from the
    scatter of the walkers' means: the ratio of the two estimates has sigma^2 = 1/(2 (W - 1)) + 2/((n_l - 1) W), n_l
    the count at the reliable level (0.24 for 5 sigma at W = 256, n_l = 32)."""
    W, beta, T = 256, 0.44, 4096
    mc = gpu.MC(gpu.IsingModel(dims=2, L=4), beta=beta, n_walkers=W, seed=1234, thermalization=200, sweeps=T,
                cluster_moves=True, global_rate=1, binning=True)
    mc.run()
    ex = _exact_4x4(beta)
    got = mc.binned(walkers=range(W))
    assert mc.binner_size() == (17, T) and got["level"] == 7 and got["count"] == 32
    E, M = got["Energy"]["E"], got["Magn"]["M"]
    for o, k in ((E, "E"), (got["Energy"]["E2"], "E2"), (M, "M"), (got["Magn"]["M2"], "M2")):
        print(k, o, ex[k])
        assert abs(o["mean"] - ex[k]) <= 5.0 * o["std_error"], (k, o, ex[k])
    for o, exact, tau in ((got["Energy"]["C"], beta * beta / 16 * (ex["E2"] - ex["E"] ** 2), E["tau"]),
                          (got["Magn"]["chi"], beta / 16 * (ex["M2"] - ex["M"] ** 2), M["tau"])):
        print(o, exact, tau)
        assert "tau" not in o
        assert abs(o["mean"] - exact) <= 5.0 * o["std_error"] + exact * (2.0 * max(tau, 0.0) + 1.0) / T, (o, exact, tau)
    sigma = math.sqrt(1.0 / (2.0 * (W - 1.0)) + 2.0 / ((got["count"] - 1.0) * W))
    for o in (E, M):
        assert abs(o["std_error"] / o["std_error_walkers"] - 1.0) <= 5.0 * sigma, (o, sigma)
    mc.close()
