"""The device-side LogBinners (csrc/binner.hip, include/dqmc_hip.h "error bars") against the numpy reference of
tests/logbinner_ref.py.

Bounds.  eps = 2^-52.  A sum of T terms accumulated in order carries a rounding error of at most T eps times the sum of
the absolute values of its terms; the device contracts x2_sum += x*x into a fused multiply-add and the reference does
not, and the carried pair averages of the upper levels add a rounding per level: delta = 4 T eps, relative to the
sum of the absolute values of the terms.  A value of level l is the average of 2^l samples and may cancel, so its
rounding is relative to the size of the samples, not to itself: with S1 = sum |x| <= sqrt(T x2_sum(0)) (Cauchy-Schwarz)
and S2 = x2_sum(0) over the level-0 samples, the level-l sums run over values v with sum |v| <= S1 / 2^l and
sum v^2 <= S2 / 2^l (Jensen), and

    |d x_sum(l)| <= delta sqrt(T x2_sum(0)) / 2^l            |d x2_sum(l)| <= delta x2_sum(0) / 2^l

(This is "4 T eps relative" read as summation rounding is: relative to the sum of the absolute values of what went
into a sum, which for a sum that does not cancel is the sum itself.  For the mean = standard deviation series of
item 1 the Cauchy-Schwarz step makes it sqrt(2) looser than a bound relative to x_sum(0) itself; the form is chosen
because the sums of real sections (an Mz, an off-diagonal G element) do cancel.)

The statistics are compared with the host formulas applied to the REFERENCE's sums, and inherit delta through the
cancellation of the variance formula.  With n = count[l], varN = x2_sum/(n(n-1)) - x_sum^2/(n^2 (n-1)); both terms are
at most x2_sum(l)/(n(n-1)) <= x2_sum(0)/(2^l n(n-1)) and each is known to delta of that, so

    |d varN_w(l)| <= 2 delta x2_sum_w(0) / (2^l n (n-1)),      A_l = sum_w of that over the walkers

which relative to varN is 2 delta (mean^2 + var)/var - the bound of the level sums times the cancellation factor.  Then
    std_error = sqrt(V_l)/W, V_l = sum_w varN_w(l):   |d| <= min(A_l / sqrt(V_l), sqrt(A_l)) / W
    2 tau + 1 = V_l / V_0:                             |d tau| <= (A_l + (V_l/V_0) A_0) / (2 (V_0 - A_0))
    mean:                                              |d| <= delta sum_w sqrt(x2_sum_w(0)/n) / W =: m
    std_error_walkers (l2 norm of mean_w - mean):      |d| <= 2 max_w m_w / sqrt(W - 1)
(tau is bounded through the ratio it is made of: at level 0 it is exactly 0, where no relative bound exists.)"""
import os
import sys

import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from logbinner_ref import LogBinnerRef, combine_walkers  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _delta(T):
    return 4.0 * T * EPS


def _check_level_sums(label, mc, which, refs, delta, levels=None, pick=None):
    """x_sum, x2_sum and count of every level and walker against the reference binners"""
    E, L, T = mc.binner_size(which)
    assert L == refs[0].L and T == refs[0].count[0], (label, L, T)
    worst = 0.0
    for w, ref in enumerate(refs):
        for l in (range(L) if levels is None else levels):
            xs, x2, cnt = mc.binner_level(which, w, l)
            if pick is not None:
                xs, x2 = xs[pick], x2[pick]
            assert cnt == ref.count[l] == T >> l, (label, w, l, cnt)
            scale = np.sqrt(float(T) * ref.x2_sum[0]) / 2.0 ** l
            for name, dev, r in (("x_sum", xs, ref.x_sum[l]), ("x2_sum", x2, ref.x2_sum[l])):
                err = np.abs(dev - r)
                bound = delta * (scale if name == "x_sum" else ref.x2_sum[0] / 2.0 ** l)
                ratio = float(np.max(err / np.where(bound > 0, bound, 1.0)))
                worst = max(worst, ratio)
                assert np.all(err <= bound), (label, name, "walker", w, "level", l, "error / bound", ratio)
    print("%s: level sums, worst error / bound = %.3g" % (label, worst))


def _check_statistics(label, got, refs, level, delta):
    """mean, std_error, std_error_walkers and tau (flat arrays) against combine_walkers on the reference's sums, under
    the bounds derived in the module docstring"""
    W = len(refs)
    ref = combine_walkers(refs, level)
    lv = ref["level"]
    n0, nl = float(refs[0].count[0]), float(refs[0].count[lv])
    m_w = np.stack([delta * np.sqrt(r.x2_sum[0] / n0) for r in refs])
    report = {}

    def cmp(name, dev, r, bound):
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(dev), nan), (label, name, "NaN pattern")
        err = np.abs(dev - r)[~nan]
        b = bound[~nan]
        report[name] = float(np.max(err / np.where(b > 0, b, 1.0))) if err.size else 0.0
        assert np.all(err <= b), (label, name, "level", lv, "error / bound", report[name],
                                  "max abs error", float(err.max()))

    cmp("mean", got["mean"], ref["mean"], m_w.sum(axis=0) / W)
    if W >= 2:
        cmp("std_error_walkers", got["std_error_walkers"], ref["std_error_walkers"],
            2.0 * m_w.max(axis=0) / np.sqrt(W - 1.0))
    else:
        assert np.all(np.isnan(got["std_error_walkers"]))
    if nl >= 2:
        A_l = np.sum([2.0 * delta * r.x2_sum[0] / (2.0 ** lv * nl * (nl - 1.0)) for r in refs], axis=0)
        A_0 = np.sum([2.0 * delta * r.x2_sum[0] / (n0 * (n0 - 1.0)) for r in refs], axis=0)
        V_l, V_0 = ref["sum_varN_level"], ref["sum_varN_0"]
        with np.errstate(invalid="ignore", divide="ignore"):
            se_bound = np.minimum(A_l / np.sqrt(np.maximum(V_l, 0.0)), np.sqrt(A_l)) / W
            se_bound = np.where(np.isnan(se_bound), np.sqrt(A_l) / W, se_bound)
            cmp("std_error", got["std_error"], ref["std_error"], se_bound)
            ok = V_0 - A_0 > 0                      # elsewhere the ratio is undetermined within the rounding
            tau_bound = (A_l + np.abs(V_l / V_0) * A_0) / (2.0 * (V_0 - A_0))
            if lv == 0:
                assert np.all(got["tau"][ok] == 0.0), (label, "tau at level 0")
            else:
                cmp("tau", got["tau"][ok], ref["tau"][ok], tau_bound[ok])
    else:
        assert np.all(np.isnan(got["std_error"])) and np.all(np.isnan(got["tau"]))
    print("%s level %d: error / bound %s" % (label, lv, {k: "%.3g" % v for k, v in report.items()}))
    return ref


# ---- 1. the user binner against the numpy reference -------------------------------------------------------------
@pytest.mark.parametrize("T,capacity", [(1000, None), (1023, 1023), (1024, 1024)])
def test_user_binner_matches_the_numpy_reference(gpu, T, capacity):
    """A seeded series (mean 1, standard deviation 1, so the variance formula loses few digits) pushed from a torch
    device tensor.  T = 1000 is no power of two (default capacity, 17 levels); T = 1023 with capacity 1023 runs the
    cascade into the top level, which has no compressor; T = 1024 with capacity 1024 ends on the longest cascade (push
    index 1023: ten completed pairs) and fills the binner exactly."""
    W, E = 4, 1000
    mc = gpu.DQMC(gpu.HubbardModelAttractive(2, 2), beta=1.0, n_walkers=W, seed=5)
    rng = np.random.default_rng(77 + T)
    data = 1.0 + rng.standard_normal((T, W, E))
    dev = torch.from_numpy(data).to("cuda:0")
    mc.user_binner(E, capacity)
    refs = [LogBinnerRef(E, capacity or 100000) for _ in range(W)]
    assert mc.binner_size("user") == (E, refs[0].L, 0)
    for t in range(T):
        mc.user_push(dev[t])
        for w in range(W):
            refs[w].push(data[t, w])
    delta = _delta(T)
    _check_level_sums("user T=%d" % T, mc, "user", refs, delta)
    assert mc.binner_reliable_level("user") == refs[0].reliable_level() == {1000: 4, 1023: 4, 1024: 5}[T]
    for level in (None, 0, 1, refs[0].L - 1, int(np.log2(T)) - 1):
        got = mc.binned_raw("user", level)
        assert got["count"] == T and got["reliable_level"] == refs[0].reliable_level()
        _check_statistics("user T=%d" % T, got, refs, level, delta)
    b = mc.binned("user")
    assert b["x"].shape == (E,) and b["x_std_error"].shape == (E,) and b["count"] == T
    # the binning error of an uncorrelated series is its naive error, within the scatter of a variance from 62 / 32 bins
    r = b["x_std_error"] / mc.binned_raw("user", 0)["std_error"]
    assert 0.9 < np.median(r) < 1.1
    if capacity is not None:  # full: the next push is refused
        with pytest.raises(gpu.DQMCError) as e:
            mc.user_push(dev[0])
        assert e.value.code == -4
    with pytest.raises(gpu.DQMCError):
        mc.binned_raw("user", refs[0].L)
    mc.close()


# ---- 2. the measurement sections against a host recomputation ------------------------------------------------------
def _section_flat(mc, which):
    """the raw accumulator of a section without its sample count (the G.^2 block of the Green's section dropped too)"""
    import ctypes as C
    from montecarlo_jl_amd._lib import dptr, lib
    L = lib()
    size_fn, get_fn = {"greens": (L.dqmc_accumulator_size, L.dqmc_get_accumulators),
                       "correlations": (L.dqmc_correlations_size, L.dqmc_get_correlations),
                       "pairing": (L.dqmc_pairing_size, L.dqmc_get_pairing),
                       "susceptibilities": (L.dqmc_susceptibilities_size, L.dqmc_get_susceptibilities)}[which]
    n = C.c_size_t()
    mc._c(size_fn(mc._h, C.byref(n)))
    out = np.zeros(n.value)
    mc._c(get_fn(mc._h, dptr(out)))
    if which == "greens":
        n2 = mc.nb * mc.N * mc.N
        return np.concatenate([out[:n2], out[2 * n2:-1]])
    return out[:-1]


SECTIONS = ("greens", "correlations", "pairing", "susceptibilities")


def _make(gpu, kind, W, first=0, seed=61, sweeps=60):
    if kind == "attractive":
        model = gpu.HubbardModelAttractive(4, 2)
    else:
        model = gpu.HubbardModelRepulsive(2, 2)
    mc = gpu.DQMC(model, beta=1.0, n_walkers=W, seed=seed, first_walker=first, thermalization=10, sweeps=sweeps,
                  measure_rate=5)
    K = 5 if kind == "attractive" else 3
    mc.set_local_targets(gpu.EachLocalQuadByDistance(model.l, K))
    if kind == "attractive":
        mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(model.l))
    return mc


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_sections_match_a_host_recomputation(gpu, kind):
    """4 x 4 attractive (with the current-current section configured) and 2 x 2 repulsive, W = 4, 12 measurements.
    Green's section: every walker's greens(w) read in on_measure and pushed into the reference.  The other sections:
    a W = 1 handle seeded as walker w (first_walker = w) runs the same trajectory, and its raw accumulator grows by
    exactly that walker's sample per measurement: the difference of successive reads is pushed (the subtraction's
    own rounding, at most count eps relative to the accumulated sum, is inside delta).  The accumulators of the
    binned run equal those of a run without binning bit for bit."""
    W = 4
    mc = _make(gpu, kind, W)
    n, nb = mc.N, mc.nb
    sizes = {}
    refs = {}

    def push_greens(m, i):
        if "greens" not in refs:
            refs["greens"] = [LogBinnerRef(nb * n * n + nb * n) for _ in range(W)]
        for w in range(W):
            G = m.greens(w)
            x = np.concatenate([g.reshape(-1, order="F") for g in G] + [1.0 - np.diag(g) for g in G])
            refs["greens"][w].push(x)

    assert mc.run(measurements=SECTIONS, binning=True, on_measure=push_greens)
    plain = _make(gpu, kind, W)
    assert plain.run(measurements=SECTIONS)
    for which in SECTIONS:
        assert np.array_equal(_section_flat(mc, which), _section_flat(plain, which)), which
        with pytest.raises(gpu.DQMCError):
            plain.binned_raw(which)
    assert np.array_equal(mc.accumulators(), plain.accumulators())
    plain.close()
    T = mc.binner_size("greens")[2]
    assert T == 12
    for which in SECTIONS[1:]:
        sizes[which] = mc.binner_size(which)[0]
        assert mc.binner_size(which)[1:] == (17, T)
        refs[which] = [LogBinnerRef(sizes[which]) for _ in range(W)]
    nd = mc._ndirs
    assert sizes["correlations"] == 4 * nd + 3 * n and sizes["pairing"] == nd * mc._K ** 2
    assert sizes["susceptibilities"] == 4 * nd + nd * mc._K ** 2 + nd * getattr(mc, "_Kcc", 0)
    for w in range(W):
        one = _make(gpu, kind, 1, first=w)
        prev = {}

        def push_diff(m, i):
            for which in SECTIONS[1:]:
                cur = _section_flat(m, which)
                refs[which][w].push(cur - prev.get(which, 0.0))
                prev[which] = cur

        assert one.run(measurements=SECTIONS, on_measure=push_diff)
        assert np.array_equal(one.conf(0), mc.conf(w))
        one.close()
    delta = _delta(T)
    for which in SECTIONS:
        _check_level_sums("%s %s" % (kind, which), mc, which, refs[which], delta, levels=range(4))
        for level in (None, 1, 2):
            got = mc.binned_raw(which, level)
            _check_statistics("%s %s" % (kind, which), got, refs[which], level, delta)
            assert got["reliable_level"] == 0 and got["count"] == T
    # shapes of binned() follow the existing getters
    b = mc.binned("greens")
    assert len(b["G"]) == nb and b["G"][0].shape == (n, n) and b["occupation_std_error"][0].shape == (n,)
    assert np.allclose(b["G"][0], mc.unpack_accumulators(mc.accumulators())["G"][0], rtol=0, atol=1e-13)
    c = mc.binned("correlations")
    assert c["CDC"].shape == (nd,) and c["Mz_tau"].shape == (n,) and np.all(c["Mx"] == 0.0)
    assert np.allclose(c["CDC"], mc.correlations()["CDC"], rtol=0, atol=1e-12)
    p = mc.binned("pairing")
    assert p["PC"].shape == p["PC_std_error_walkers"].shape == (nd, mc._K, mc._K)
    assert np.allclose(p["PC"], mc.pairing()[0], rtol=0, atol=1e-12)
    s = mc.binned("susceptibilities")
    sus = mc.susceptibilities()
    for k in ("CDS", "SDSz", "PS") + (("CCS",) if kind == "attractive" else ()):
        assert s[k].shape == sus[k].shape and np.allclose(s[k], sus[k], rtol=0, atol=1e-12), k
    mc.close()


# ---- 3. additivity over handles -----------------------------------------------------------------------------------
def test_moments_add_over_handles(gpu):
    """walkers 0..3 and 4..7 on two handles against one handle with 0..7.  A walker's trajectory and samples do not
    depend on the sharding (item 2 holds a W = 1 handle to the W = 4 one within the bounds of item 1), so the
    per-walker terms of the moments are the same numbers and only the order of the sum over 8 walkers differs:
    delta = 4 T eps (item 1, for the terms) + 8 eps (the order of summation), in the bounds of the module docstring."""
    T_meas = 8
    delta = _delta(T_meas) + 8.0 * EPS
    model = lambda: gpu.HubbardModelRepulsive(4, 2)
    hs = []
    for first, W in ((0, 4), (4, 4), (0, 8)):
        mc = gpu.DQMC(model(), beta=2.0, n_walkers=W, seed=123, first_walker=first, thermalization=4, sweeps=16,
                      measure_rate=2)
        mc.set_pair_directions(gpu.EachSitePairByDistance(mc.model.l))
        assert mc.run(measurements=("greens", "correlations"), binning=True)
        hs.append(mc)
    a, b, big = hs
    for which in ("greens", "correlations"):
        E, _, T = big.binner_size(which)
        assert T == 8
        for level in (None, 1):
            ma, mb, mbig = (m.binner_moments(which, level).cpu().numpy() for m in hs)
            assert ma[-1] == 4 and mb[-1] == 4 and mbig[-1] == 8 and ma.size == 4 * E + 1
            tot = ma + mb
            n0, nl = 8.0, 8.0 if level is None else 4.0
            # per-walker sums of the big handle give the scales of the bounds
            x2_0 = np.stack([big.binner_level(which, w, 0)[1] for w in range(8)])
            x2_l = x2_0 / (1.0 if level is None else 2.0 ** level)
            m_w = delta * np.sqrt(x2_0 / n0)
            bounds = [m_w.sum(0),                                                 # sum mean_w
                      (2.0 * np.sqrt(x2_0 / n0) * m_w).sum(0) + 1e-300,           # sum mean_w^2
                      (2.0 * delta * x2_l / (nl * (nl - 1.0))).sum(0),            # sum varN_w(level)
                      (2.0 * delta * x2_0 / (n0 * (n0 - 1.0))).sum(0)]            # sum varN_w(0)
            for q, name in enumerate(("sum mean", "sum mean^2", "sum varN(l)", "sum varN(0)")):
                err = np.abs(tot[q * E:(q + 1) * E] - mbig[q * E:(q + 1) * E])
                ratio = float(np.max(err / np.where(bounds[q] > 0, bounds[q], 1.0)))
                print("additivity %s level %s %s: error / bound %.3g" % (which, level, name, ratio))
                assert np.all(err <= bounds[q]), (which, name, ratio)
            fin = gpu.finish_moments(tot)
            ref = big.binned_raw(which, level)
            assert fin["n_walkers"] == 8
            A_l, A_0, V_l, V_0 = bounds[2], bounds[3], mbig[2 * E:3 * E], mbig[3 * E:4 * E]
            assert np.all(np.abs(fin["mean"] - ref["mean"]) <= bounds[0] / 8.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                se_b = np.where(V_l > 0, np.minimum(A_l / np.sqrt(np.abs(V_l)), np.sqrt(A_l)), np.sqrt(A_l)) / 8.0
                assert np.all(np.abs(fin["std_error"] - ref["std_error"]) <= se_b)
                ok = V_0 - A_0 > 0
                tau_b = (A_l + np.abs(V_l / V_0) * A_0) / (2.0 * (V_0 - A_0))
                assert np.all(np.abs(fin["tau"] - ref["tau"])[ok] <= tau_b[ok])
                # the cross-walker error from the moments cancels sum mean^2 against (sum mean)^2 / W: its square is
                # known to the bound of sum mean^2 plus that of (sum mean)^2 / W
                v_b = (bounds[1] + 2.0 * np.abs(mbig[:E]) * bounds[0] / 8.0) / (8.0 * 7.0)
                assert np.all(np.abs(fin["std_error_walkers"] ** 2 - ref["std_error_walkers"] ** 2) <= v_b + 1e-300)
            shaped = big.finish_moments(tot, which)
            key = "G" if which == "greens" else "CDC"
            assert np.shape(shaped[key + "_std_error"]) == np.shape(big.binned(which, level)[key + "_std_error"])
    for m in hs:
        m.close()


# ---- 4. capacity --------------------------------------------------------------------------------------------------
def test_capacity_and_reset(gpu):
    W, E, cap = 3, 70, 5
    mc = gpu.DQMC(gpu.HubbardModelAttractive(2, 2), beta=1.0, n_walkers=W, seed=5)
    mc.user_binner(E, cap)
    assert mc.binner_size("user") == (E, 3, 0)
    rng = np.random.default_rng(3)
    data = torch.from_numpy(rng.standard_normal((cap + 1, W, E))).to("cuda:0")
    for t in range(cap):
        mc.user_push(data[t])                                    # the capacity-th push succeeds
    assert mc.binner_size("user")[2] == cap
    before = [mc.binner_level("user", w, l) for w in range(W) for l in range(3)]
    with pytest.raises(gpu.DQMCError) as e:
        mc.user_push(data[cap])
    assert e.value.code == -4                                    # DQMC_ERR_STATE
    after = [mc.binner_level("user", w, l) for w in range(W) for l in range(3)]
    for x, y in zip(before, after):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    assert mc.binner_size("user")[2] == cap and np.any(before[0][0] != 0.0)
    mc.reset_accumulators()
    assert mc.binner_size("user")[2] == 0
    for w in range(W):
        for l in range(3):
            xs, x2, cnt = mc.binner_level("user", w, l)
            assert cnt == 0 and not xs.any() and not x2.any()
    mc.user_push(data[0])                                        # usable again, and from a clean state
    xs, x2, cnt = mc.binner_level("user", 1, 0)
    assert cnt == 1 and np.array_equal(xs, data[0, 1].cpu().numpy())
    # a full section binner refuses the measurement before anything is accumulated
    mc.prepare()
    mc.enable_binning(("greens",), capacity=2)
    mc.reset_accumulators()
    mc.accumulate_greens()
    mc.accumulate_greens()
    acc = mc.accumulators()
    with pytest.raises(gpu.DQMCError) as e:
        mc.accumulate_greens()
    assert e.value.code == -4 and np.array_equal(mc.accumulators(), acc) and acc[-1] == 2 * W
    with pytest.raises(gpu.DQMCError):
        mc.enable_binning(("pairing",))                          # its measurement is not configured
    mc.close()


# ---- 5. the benchmark's shape ---------------------------------------------------------------------------------------
def test_greens_binner_at_the_benchmark_shape(gpu):
    """n = 256, W = 32 (the shape of the benchmark configuration, default capacity: 0.84 GB of level state), six
    measurements: the Green's section against the reference on a seeded sample of 4096 of its 65792 elements"""
    W, n = 32, 256
    mc = gpu.DQMC(gpu.HubbardModelAttractive(16, 2), beta=1.0, n_walkers=W, seed=11, thermalization=1, sweeps=6,
                  measure_rate=1)
    E = n * n + n
    pick = np.sort(np.random.default_rng(256).choice(E, size=4096, replace=False))
    assert pick[-1] >= n * n                                     # (the occupation block is sampled too)
    refs = [LogBinnerRef(4096) for _ in range(W)]

    def push(m, i):
        for w in range(W):
            G = m.greens(w)[0]
            refs[w].push(np.concatenate([G.reshape(-1, order="F"), 1.0 - np.diag(G)])[pick])

    assert mc.run(measurements=("greens",), binning=True, on_measure=push)
    assert mc.binner_size("greens") == (E, 17, 6)
    delta = _delta(6)
    _check_level_sums("n=256 greens", mc, "greens", refs, delta, levels=range(4), pick=pick)
    for level in (None, 1):
        got = mc.binned_raw("greens", level)
        _check_statistics("n=256 greens", {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in got.items()},
                          refs, level, delta)
    mc.close()


# ---- 6. golden sanity, not parity ------------------------------------------------------------------------------------
# ratio of a single run's median std_error to the pooled one over seeds of the CPU oracle: (low, high) = the extremes
# measured over 32 seeds, see the docstring of the test
GOLDEN_BAND = {"G": (0.902, 1.057), "CDC": (0.829, 1.183)}
GOLDEN_MARGIN = 1.25


def test_binned_errors_against_the_published_ones(gpu):
    """The attractive 4 x 4 golden run shape (beta = 1, 10 + 1000 sweeps, measure_rate = 10: 100 measurements per
    walker, reliable level 1 with 50 entries) on 32 walkers.  The reference publishes the std_error of ONE such chain
    (tests/golden/integration_attractive_4x4.json), itself an estimate from 100 correlated samples.  Ours, for one
    chain, is sqrt(mean_w varN_w(1)) = sqrt(W) * the binned std_error of the handle: the pooled estimate of 32 chains.
    Compared is  r = median over the elements of published / ours_one_chain  for the diagonal of G and for the CDC.
    The admissible band comes from the reference side: the CPU oracle run at the same shape over 32 seeds (walker
    seeds 7000..7031, numpy LogBinner of tests/logbinner_ref.py at its reliable level 1), r_s = median over the
    elements of se_s / sqrt(mean_s se_s^2).  Measured on the CPU:
      diagonal G: mean 0.995, standard deviation 0.031, extremes 0.902 and 1.057 (pooled std_error 0.0171 .. 0.0180)
      CDC:        mean 0.996, standard deviation 0.098, extremes 0.829 and 1.183 (pooled std_error 0.0152 .. 0.0156)
    (tools/binner_golden_band.py 32 prints these; the CDC entries of a run rise and fall together, so its median
    scatters three times as much as that of the diagonal of G.)
    A single published run is one more draw of r_s, and the pooled estimate of 32 device walkers scatters by about
    sd / sqrt(32) itself, so the band is the measured extremes widened by the factor GOLDEN_MARGIN = 1.25 on both
    sides."""
    import golden_stats as gs
    W = 32
    model = gpu.HubbardModelAttractive(4, 2)
    mc = gpu.DQMC(model, beta=1.0, n_walkers=W, seed=4242, thermalization=10, sweeps=1000, measure_rate=10)
    mc.set_pair_directions(gpu.EachSitePairByDistance(model.l))
    assert mc.run(measurements=("greens", "correlations"), binning=True)
    A = gs.load("integration_attractive_4x4.json")["all"]
    bg, bc = mc.binned("greens"), mc.binned("correlations")
    assert bg["count"] == 100 and bg["reliable_level"] == 1 and bc["reliable_level"] == 1
    _, se_G = gs.golden_arrays(A["G"], (16, 16))
    _, se_C = gs.golden_arrays(A["CDC"])
    ours = {"G": np.sqrt(W) * np.diag(bg["G_std_error"][0]), "CDC": np.sqrt(W) * bc["CDC_std_error"]}
    pub = {"G": np.diag(se_G), "CDC": se_C}
    for k in ("G", "CDC"):
        r = float(np.median(pub[k] / ours[k]))
        lo, hi = GOLDEN_BAND[k][0] / GOLDEN_MARGIN, GOLDEN_BAND[k][1] * GOLDEN_MARGIN
        tau = (bg["G_tau"][0].diagonal() if k == "G" else bc["CDC_tau"])
        print("golden sanity %s: published / ours = %.4f (band %.3f .. %.3f); tau median %.3f; "
              "binning / cross-walker error median %.3f"
              % (k, r, lo, hi, float(np.median(tau)),
                 float(np.median((np.diag(bg["G_std_error"][0]) / np.diag(bg["G_std_error_walkers"][0])) if k == "G"
                                 else bc["CDC_std_error"] / bc["CDC_std_error_walkers"]))))
        assert lo <= r <= hi, (k, r, lo, hi)
    mc.close()
