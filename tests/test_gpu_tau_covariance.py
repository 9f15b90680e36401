"""The tau-tau' covariance accumulators on the MI355X (csrc/taucov.hip, taucov.inl) against the numpy restatement
(tau_covariance_ref.py): the kernel on chosen data through user_covariance, the accumulator wired into
accumulate_susceptibilities against samples recovered from the momentum binner, that nothing else moves, the errors, and a
small continuation with the full covariance end to end.

The series lengths R of the kernel tests.  Asked for: 1, 2, 33, 64, 65, 130.  Added for the kernel as written (256 lanes
per workgroup; four series per workgroup, one wave each, for R <= 16; S2 streamed as a flat run in 16-byte pairs with a
misaligned head and a left-over tail done apart):
  3         R^2 = 9: pairs, head and tail inside one wave of a shared workgroup, with n_series = 5 leaving three idle teams
  16, 17    either side of the switch from four series per workgroup to one
  22, 23    R^2 / 2 = 242 and 264 pairs: either side of one step of the 256-lane pair loop
  256, 257  either side of one step of the 256-lane gather loop; 257^2 is odd, so odd series start misaligned
(33, 65 and 257 are odd: every other series starts on an odd double and takes the head element; 2, 16, 64, 130 and 256
never do.)"""
import numpy as np
import pytest
import torch  # (before the package: the process then has one HIP runtime, torch's)

import tau_covariance_ref as T

pytestmark = pytest.mark.gpu

W, NS, PUSHES = 3, 5, 7
RS = [1, 2, 3, 16, 17, 22, 23, 33, 64, 65, 130, 256, 257]


def new_mc(g, n_walkers, seed=77, **kw):
    l = g.SquareLattice(4)
    return g.DQMC(g.HubbardModelAttractive(l=l), beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=n_walkers, seed=seed, **kw), l


@pytest.fixture(scope="module")
def pair(gpu):
    a, b = new_mc(gpu, W)[0], new_mc(gpu, W)[0]
    yield a, b
    a.close()
    b.close()


def chosen(R, seed=11):
    rng = np.random.RandomState(seed + R)
    z = rng.standard_normal((PUSHES, W, NS, R))
    return 0.4 + 0.2 * (z + 0.6 * np.roll(z, 1, axis=3))


def feed(mc, x, bin_size):
    mc.user_covariance(x.shape[2], x.shape[3], bin_size)
    for s in x:
        mc.user_covariance_push(torch.from_numpy(np.ascontiguousarray(s)).cuda())
    return mc.user_covariance_result()


def restated(x, bin_size):
    acc = T.Accumulator(x.shape[1], x.shape[2], x.shape[3], bin_size)
    for s in x:
        acc.push(s)
    return acc


@pytest.mark.parametrize("bin_size", [1, 3])
@pytest.mark.parametrize("R", RS)
def test_kernel_matches_the_restatement(pair, R, bin_size):
    """7 pushes: 7 closed bins, or 2 and one sample left open.  nb and shift exactly; S1 and S2 element by element within
    4 (n_closed + 2) eps sum |terms| (tau_covariance_ref.Accumulator.bounds); S2 bitwise symmetric; a second handle
    gives the same bits"""
    x = chosen(R)
    out, ref = feed(pair[0], x, bin_size), restated(x, bin_size)
    n = PUSHES // bin_size
    assert list(out["nb"]) == [n] * W and ref.nb == n
    assert pair[0].user_covariance_result()["bin_size"] == bin_size
    assert np.array_equal(out["shift"], ref.c)
    b1, b2 = ref.bounds()
    e1, e2 = np.abs(out["S1"] - ref.S1), np.abs(out["S2"] - ref.S2)
    print("R", R, "bin", bin_size, "max S1 err / bound", (e1 / np.maximum(b1, 1e-300)).max(),
          "max S2 err / bound", (e2 / np.maximum(b2, 1e-300)).max())
    assert np.all(e1 <= b1) and np.all(e2 <= b2)
    assert np.array_equal(out["S2"], np.swapaxes(out["S2"], 2, 3))
    if n > 1:
        assert np.abs(out["S2"]).min() > 0.0  # every element was written
    again = feed(pair[1], x, bin_size)
    for k in ("nb", "shift", "S1", "S2"):
        assert np.array_equal(out[k], again[k]), k


@pytest.mark.parametrize("bin_size", [1, 3])
def test_kernel_keeps_the_digits_of_series_near_one(gpu, pair, bin_size):
    """mean 1, fluctuations 1e-8 (the data of the host test): the pooled device moments give the np.longdouble
    covariance within tau_covariance_ref.near_one_tolerance.  An un-shifted kernel misses by the factor the host test
    shows"""
    R = 6
    x = T.near_one_samples(12, W, NS, R)
    out = gpu.tau_covariance_from_moments(feed(pair[0], x, bin_size))
    b = T.bin_means(x, bin_size)
    mean, ref = T.covariance_of_mean(b.reshape((-1,) + b.shape[2:]).astype(np.longdouble))
    tol = T.near_one_tolerance(x, bin_size)
    err = np.abs(out["cov"] - ref).astype(np.float64)
    print("bin", bin_size, "max err / tol", (err / tol).max())
    assert out["n_bins"] == W * (12 // bin_size)
    assert np.all(err <= tol)
    assert np.abs(out["mean"] - mean).max() <= 4 * T.EPS


def test_reset_clears_everything_and_off_frees(gpu, pair):
    from montecarlo_jl_amd import _lib
    mc = pair[0]
    x = chosen(17)
    feed(mc, x[:5], 3)  # one closed bin, two samples open
    mc.reset_accumulators()
    out = mc.user_covariance_result()
    assert list(out["nb"]) == [0] * W
    assert not out["shift"].any() and not out["S1"].any() and not out["S2"].any()
    for s in x[:3]:  # the open bin was cleared too: these three alone make the first bin, and the shift
        mc.user_covariance_push(torch.from_numpy(np.ascontiguousarray(s)).cuda())
    out, ref = mc.user_covariance_result(), restated(x[:3], 3)
    assert list(out["nb"]) == [1] * W and np.array_equal(out["shift"], ref.c)
    mc.user_covariance(0, 0, 0)
    with pytest.raises(gpu.DQMCError) as e:
        mc.user_covariance_push(0)
    assert e.value.code == _lib.ERR_STATE
    for bad in ((0, 3, 1), (2, 0, 1), (2, 3, -1), (2, 2049, 1)):
        with pytest.raises(gpu.DQMCError) as e:
            mc.user_covariance(*bad)
        assert e.value.code == _lib.ERR_INVALID


# ---- wired into DQMC ---------------------------------------------------------------------------------------------------
QS = {"all": "all", "three": [(0, 0), (2, 2), (1, 3)]}
WHAT = {"greens": ("greens",), "density": ("density",), "both": ("greens", "density")}


def configured(g, every, qs, seed=77, td_what=("greens", "density"), n_walkers=4):
    mc, l = new_mc(g, n_walkers, seed=seed)
    mc.set_pair_directions(g.EachSitePairByDistance(l))
    mc.set_momenta(QS[qs] if isinstance(qs, str) else qs)
    mc.set_time_displaced(every, td_what)
    mc.prepare()
    return mc


def series_of(sample, nb, R, nq, td_what, what):
    """one walker's momentum time-displaced sample -> [S, R] in the order of include/dqmc_hip.h"""
    out, off = [], 0
    if "greens" in td_what:
        if "greens" in what:
            out.append(np.moveaxis(sample[:nb * R * nq].reshape(nb, R, nq), 1, 2).reshape(nb * nq, R))
        off = 4 * nb * R * nq
    if "density" in what:
        out.append(np.moveaxis(sample[off:off + 4 * R * nq].reshape(4, R, nq), 1, 2).reshape(4 * nq, R))
    return np.concatenate(out)


def passes(mc, n, record=None):
    for _ in range(n):
        mc.update_until_measure()
        mc.accumulate_susceptibilities(recalculate=5)
        if record is not None:
            record.append(np.stack([mc.binner_level("momentum_time_displaced", w, 0)[0] for w in range(mc.n_walkers)]))


@pytest.mark.parametrize("what", sorted(WHAT))
@pytest.mark.parametrize("qs", sorted(QS))
@pytest.mark.parametrize("every", [1, 5])
def test_wired_accumulator_matches_samples_recovered_from_the_binner(gpu, every, qs, what):
    """bin_size 2, 7 passes: 3 closed bins.  A walker's samples are the increments of level 0 of its momentum binner,
    x^_k = T_k - T_(k-1): T_k carries the rounding of its own addition, eps |T_k|, and the difference that of the
    subtraction, eps |x^_k|, so |x^_k - x_k| <= eps (|T_k| + |x^_k|) =: dx_k.  The restatement is fed x^ and carries dx
    through (tau_covariance_ref.Accumulator: e_shift, e1, e2), and those widen the bounds of the kernel test"""
    mc = configured(gpu, every, qs)
    try:
        mc.enable_binning(("momentum_time_displaced",), capacity=8)
        mc.set_tau_covariance(2, WHAT[what])
        nq, R = mc.momenta().shape[0], 1 + 10 // every
        S = (("greens" in WHAT[what]) * mc.nb + ("density" in WHAT[what]) * 4) * nq
        plan = mc.tau_covariance_plan()
        assert (plan["bin_size"], plan["series"], plan["rows"], plan["n_bins"]) == (2, S, R, 0)
        assert plan["bytes"] >= 4 * S * (R * R + 3 * R) * 8
        sums = []
        passes(mc, 7, sums)
        assert mc.tau_covariance_plan()["n_bins"] == 3
        out = mc.tau_covariance_moments()
        ref = T.Accumulator(4, S, R, 2)
        prev = np.zeros_like(sums[0])
        for Tk in sums:
            xh = Tk - prev
            dx = T.EPS * (np.abs(Tk) + np.abs(xh))
            ser = lambda v: np.stack([series_of(v[w], mc.nb, R, nq, ("greens", "density"), WHAT[what]) for w in range(4)])
            ref.push(ser(xh), ser(dx))
            prev = Tk
        assert list(out["nb"]) == [3] * 4 and out["shift"].shape == (4, S, R)
        b1, b2 = ref.bounds()
        es = np.abs(out["shift"] - ref.c)
        e1, e2 = np.abs(out["S1"] - ref.S1), np.abs(out["S2"] - ref.S2)
        bs = ref.e_shift + 3 * T.EPS * np.abs(ref.c)
        print(every, qs, what, "shift err / bound", (es / bs).max(), "S1", (e1 / (b1 + ref.e1)).max(), "S2",
              (e2 / (b2 + ref.e2)).max())
        assert np.all(es <= bs)
        assert np.all(e1 <= b1 + ref.e1) and np.all(e2 <= b2 + ref.e2)
        assert np.array_equal(out["S2"], np.swapaxes(out["S2"], 2, 3))
        assert np.abs(out["S1"]).max() > 0.0 and np.abs(out["S2"]).max() > 0.0
    finally:
        mc.close()


@pytest.mark.parametrize("td_what", [("greens", "density"), ("density",)])
def test_series_order_against_momentum_time_displaced(gpu, td_what):
    """bin_size 1 and no binner (the accumulator transforms into its own sample): the pooled mean of every series is the
    mean of all samples, which momentum_time_displaced() forms on the host from the accumulated sums.  Both are sums of 16
    directions x 12 samples of O(1) terms in different orders: they agree to 1e-12, and a series taken from another row,
    block or channel differs in the second digit"""
    mc = configured(gpu, 5, "three", td_what=td_what)
    try:
        mc.set_tau_covariance(1, td_what)
        passes(mc, 3)
        tc, m = mc.tau_covariance(), mc.momentum_time_displaced()
        assert tc["n_bins"] == 12 and tc["bin_size"] == 1 and np.array_equal(tc["tau"], m["tau"])
        names = (["Gk_l0"] if "greens" in td_what else []) + ["CDCk", "SDCxk", "SDCyk", "SDCzk"]
        means = [np.asarray(m[k]).real for k in names]
        for i, k in enumerate(names):
            assert tc[k + "_mean"].shape == means[i].shape
            assert tc[k + "_cov"].shape == means[i].shape[:-2] + (3, 3, 3)
            assert np.abs(tc[k + "_mean"] - means[i]).max() <= 1e-12, k
        # the check can tell the channels, the rows and the momenta apart (SDCx, SDCy and SDCz are one function on the
        # attractive model, sample by sample: the order among those three is the sample's, checked in the wired test)
        assert np.abs(m["CDCk"] - m["SDCzk"]).max() > 1e-3
        assert np.abs(m["SDCzk"][0] - m["SDCzk"][1]).max() > 1e-3 and np.abs(m["SDCzk"][:, 0] - m["SDCzk"][:, 1]).max() > 1e-3
        assert "Gk_l0_cov" in tc or "greens" not in td_what
    finally:
        mc.close()


def snapshot(mc):
    return {"td": mc.time_displaced_raw(), "sus": mc._section("susceptibilities"),
            "bins": [mc.binner_level("momentum_time_displaced", w, l) for w in range(mc.n_walkers) for l in range(2)],
            "conf": [mc.conf(w) for w in range(mc.n_walkers)], "G": [mc.greens_eff(w) for w in range(mc.n_walkers)]}


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_nothing_else_moves(gpu):
    """the same seeds with the accumulator on and never enabled: accumulators, binner levels, HS fields and G after the
    passes are bit-identical; off, the plan is zeros and the launch plan that of the other handle"""
    on, off = configured(gpu, 1, "three"), configured(gpu, 1, "three")
    try:
        for mc in (on, off):
            mc.enable_binning(("momentum_time_displaced",), capacity=8)
        on.set_tau_covariance(2)
        assert set(off.tau_covariance_plan().values()) == {0}
        assert on.launch_plan() == off.launch_plan()
        passes(on, 4)
        passes(off, 4)
        a, b = snapshot(on), snapshot(off)
        for k in a:
            assert same(a[k], b[k]), k
        on.set_tau_covariance(0)
        assert set(on.tau_covariance_plan().values()) == {0}
        passes(on, 1)
        passes(off, 1)
        assert same(snapshot(on)["td"], snapshot(off)["td"])
    finally:
        on.close()
        off.close()


def test_errors_and_what_drops_it(gpu, tmp_path):
    from montecarlo_jl_amd import _lib

    def refused(code, f, *a, **kw):
        with pytest.raises(gpu.DQMCError) as e:
            f(*a, **kw)
        assert e.value.code == code, e.value

    mc, l = new_mc(gpu, 4)
    try:
        mc.set_pair_directions(gpu.EachSitePairByDistance(l))
        refused(_lib.ERR_STATE, mc.set_tau_covariance, 2)          # no momenta
        mc.set_momenta("all")
        refused(_lib.ERR_STATE, mc.set_tau_covariance, 2)          # no time-displaced recording
        mc.set_time_displaced(5, ("density",))
        refused(_lib.ERR_STATE, mc.set_tau_covariance, 2, ("greens",))  # rows that are not recorded
        mc.set_time_displaced(5)
        refused(_lib.ERR_INVALID, mc.set_tau_covariance, -1)
        refused(_lib.ERR_INVALID, mc.set_tau_covariance, 2, 0)
        refused(_lib.ERR_INVALID, mc.set_tau_covariance, 2, 4)
        assert set(mc.tau_covariance_plan().values()) == {0}
        mc.set_sign_weighting(True)
        refused(_lib.ERR_STATE, mc.set_tau_covariance, 2)
        mc.set_sign_weighting(False)
        mc.set_tau_covariance(2)
        assert mc.tau_covariance_plan()["bin_size"] == 2
        mc.set_sign_weighting(True)                                # switching it on drops the accumulator
        assert set(mc.tau_covariance_plan().values()) == {0}
        mc.set_sign_weighting(False)
        for drop in (lambda: mc.set_momenta([(0, 0), (1, 1)]), lambda: mc.set_time_displaced(2),
                     lambda: mc.set_pair_directions(gpu.EachSitePairByDistance(l))):
            if mc.momenta() is None:
                mc.set_momenta("all")
            if not mc.time_displaced_plan()["every"]:
                mc.set_time_displaced(5)
            mc.set_tau_covariance(2)
            assert mc.tau_covariance_plan()["series"] > 0
            drop()
            assert set(mc.tau_covariance_plan().values()) == {0}
            refused(_lib.ERR_STATE, mc.tau_covariance)
        mc.set_momenta("all")
        mc.set_time_displaced(5)
        mc.prepare()
        mc.update_until_measure()
        mc.save(str(tmp_path / "plain.ckpt"))                      # off: as before
        mc.set_tau_covariance(2)
        with pytest.raises(gpu.DQMCError, match=r"set_tau_covariance\(0\)") as e:
            mc.save(str(tmp_path / "on.ckpt"))
        assert e.value.code == _lib.ERR_STATE
        mc.accumulate_susceptibilities(recalculate=5)              # 4 walkers, one sample: no closed bin
        refused(_lib.ERR_STATE, mc.spectral_function, np.linspace(-6.0, 6.0, 21), covariance=True)
        mc.set_tau_covariance(1)
        mc.accumulate_susceptibilities(recalculate=5)              # 4 bins for R = 3: enough; 3 would not be
        mc.set_tau_covariance(0)
        mc.save(str(tmp_path / "off.ckpt"))
    finally:
        mc.close()


def test_continuation_with_the_covariance_end_to_end(gpu):
    """R = 3, 4 walkers x 3 passes of bin_size 1: 12 bins.  Finite spectra whose weights sum to the norm handed to SAC (1
    for A(k, omega), C(q, 0) for the structure factor) to the precision of the grid sum, chi2 per problem; and the
    default spectral_function is still the diagonal path, bit for bit what its inputs give when handed to SAC as the
    function did before it had the keyword"""
    mc = configured(gpu, 5, "all", seed=53)
    try:
        mc.enable_binning(("momentum_time_displaced",), capacity=8)
        mc.set_tau_covariance(1)
        passes(mc, 3)
        omega = np.linspace(-6.0, 6.0, 41)
        kw = dict(n_deltas=32, thetas=[2.0, 1.0, 0.5], seed=9001, run=dict(thermalization=40, sweeps=80))
        out = mc.spectral_function(omega, covariance=True, **kw)
        out["sac"].close()
        assert out["n_bins"] == 12 and out["A"].shape == out["weight"].shape == (1, 16, 41)
        assert out["chi2"].shape == out["theta"].shape == (1, 16) and np.all(np.isfinite(out["chi2"]))
        assert np.all(np.isfinite(out["A"])) and np.all(out["A"] >= 0.0)
        assert np.all(np.abs(out["weight"].sum(axis=2) - 1.0) <= 2 * 41 * 2.0 ** -53)

        wpos = np.linspace(0.0, 8.0, 33)
        sq = mc.dynamical_structure_factor(wpos, "SDCz", **kw)
        sq["sac"].close()
        nk = sq["momenta"].shape[0]
        assert nk >= 1 and nk + sq["left_out"].size == 16
        assert sq["B"].shape == sq["S"].shape == sq["weight"].shape == (nk, 33)
        assert sq["chi2"].shape == sq["theta"].shape == (nk,) and np.all(np.isfinite(sq["chi2"]))
        assert np.all(np.isfinite(sq["S"])) and np.all(sq["S"] >= 0.0) and np.all(sq["S"] <= sq["B"])
        norm = sq["sac"].norm
        keep = [k for k in range(16) if k not in set(sq["left_out"].tolist())]
        assert np.array_equal(norm, mc.tau_covariance()["SDCzk_mean"][0, keep]) and np.all(norm > 0.0)
        assert np.all(np.abs(sq["weight"].sum(axis=1) - norm) <= 2 * 33 * 2.0 ** -53 * norm)
        assert sq["sac"].g.shape[1] <= 2  # tau = 0 and 0.5 = beta / 2 only

        plain = mc.spectral_function(omega, **kw)
        plain["sac"].close()
        b, m = mc.binned("momentum_time_displaced"), mc.momentum_time_displaced()
        flat = lambda v: np.ascontiguousarray(np.moveaxis(v, 1, 2).reshape(16, 3))
        s = gpu.SAC(np.asarray(b["tau"], dtype=np.float64), flat(m["Gk_l0"].real),
                    error=np.maximum(flat(np.asarray(b["Gk_l0_std_error_re"])), 1e-6), kernel=gpu.fermion_kernel,
                    omega=omega, beta=1.0, n_deltas=32, thetas=[2.0, 1.0, 0.5], seed=9001)
        try:
            s.run(thermalization=40, sweeps=80)
            sp = s.spectrum()
        finally:
            s.close()
        assert np.array_equal(plain["A"].reshape(16, 41), sp["A"]) and np.array_equal(plain["chi2"].reshape(16), sp["chi2"])
    finally:
        mc.close()
