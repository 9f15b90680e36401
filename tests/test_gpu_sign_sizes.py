"""The signed measurement sums (csrc/sign.hip, binner_push_signed_kernel, the signed branches of thermo_reduce_kernel and of
the momentum launch, sign_begin in global_move.inl) at the sizes where their grids, caps and walker loops take another
trip, with mixed signs and with walkers that are left out (a sign of 0).

Real fields give a negative sign only where a seed search found one and never a sign of 0, so group A imposes the per-unit
signs with the diagnostic dqmc_impose_unit_signs (DQMC.impose_unit_signs); group B uses the chain's own signs on the golden
fields of tests/golden/logdet_sizes.json at walker counts other than 4; group C shows that a left-out walker's sample is
never read (its G is NaN); group D takes non-zero sign_failures through a checkpoint.

Reference: a pair of handles with the same model, seeds and fields.  The twin has weighting off and every binner on: after
one pass level 0 of its binner of a section is walker w's bare sample x_w in the section's element order.  The signed
handle has sign_weighting=True and the same binners.  Precondition per case: greens(w) of the two is bit-identical.

* binners, exactly: level-0 x_sum = s_w x_w (a product with +-1 is exact; 0.0 for a left-out walker; compared by value, so
  that -0.0 == 0.0), x2_sum = (s_w x_w)^2, count 1, the section's sign binner holds s_w; the momentum and thermodynamics
  samples end with s_w itself (negation commutes with rounding, so the transform of s_w x is s_w times the twin's).
* sums: |acc[e] - sum_w s_w x_w[e]| <= (W + 2) 2^-53 sum_w |x_w[e]| over the walkers kept, the host adding in walker order
  in float64: W - 1 roundings of a re-associated sum plus the one factor * s product of the susceptibility reduce.  Green's
  section: the second block is sum s g^2 with the bound on sum g^2, the diagonal block sum s - sum s g_ii with the bound on
  sum |g_ii|.  Every section prints its largest err / bound (DESIGN.md 6 records them).
* counts: a section's count = walkers kept, its sum of signs = sum s_w exactly, sign_failures grows by one per signed
  accumulate call for exactly the walkers with s_w = 0.
* non-vacuity, per section and case: max_e |sum s x - sum x| > 10^6 max_e bound, so a kernel that dropped the sign, or took
  the neighbour's, fails.

Group A: HubbardModelRepulsive(U = 4), beta = 1, delta_tau = 0.1, safe_mult = 5 after prepare() and update_until_measure().
The caps a case is there for are asserted from the launch arithmetic (2 n^2 against 512 * 256, E against ceil(2048 / W) * 256,
W against 256), so that a changed cap shows up as a failed precondition."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_move_ref as ref  # noqa: E402
import lattice_tables as LT  # noqa: E402
import logbinner_ref as LB  # noqa: E402
import sign_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
STD = S.SECTIONS  # the sections with an entry in DQMC_RED_SIGN, in its order
ALL = ("greens", "correlations", "pairing", "susceptibilities", "thermodynamics")
ALL_MOM = ("momentum_correlations", "momentum_susceptibilities", "momentum_time_displaced")
NE = 10  # DQMC_THERMO_ELEMENTS
CAPACITY = 7  # three levels

_tables = {}


def tables(l):
    """(pair directions, local quads, synced quads) of a lattice from tests/lattice_tables.py, built once"""
    key = (type(l).__name__, l.sites)
    if key not in _tables:
        pairs = LT.fast_pairs(l)
        _tables[key] = (pairs, LT.fast_quads(l, pairs=pairs), LT.fast_quads(l, pairs=pairs, synced=True))
    return _tables[key]


def binned(secs, mom):
    return tuple(secs) + (("time_displaced",) if "susceptibilities" in secs else ()) + tuple(mom)


def handle(gpu, l, W, secs, mom=(), signed=False, seed=60, model=None, beta=1.0, safe_mult=5, fields=None):
    """a handle at its measurement point with the sections of `secs`, the momentum binners of `mom` and every binner on.
    fields: the seeded HS fields of the walkers (then no update runs: prepare, replay_greens(0))"""
    model = gpu.HubbardModelRepulsive(l=l, U=4.0) if model is None else model
    mc = gpu.DQMC(model, n_walkers=W, beta=beta, delta_tau=0.1, safe_mult=safe_mult, seed=seed, sign_weighting=signed)
    try:
        pairs, local, synced = tables(l)
        mc.set_pair_directions(pairs)
        if "pairing" in secs:
            mc.set_local_targets(local)
        if "susceptibilities" in secs:
            mc.set_current_targets(synced)
            mc.set_time_displaced(5, ("greens", "density"))
        if mom:
            mc.set_momenta("all")
        if "thermodynamics" in secs:
            mc.set_thermodynamics()
        if fields is not None:
            for w, f in enumerate(fields):
                mc.set_conf(w, f)
        mc.prepare()
        if fields is None:
            mc.update_until_measure()
        else:
            mc.replay_greens(0)
        mc.enable_binning(binned(secs, mom), capacity=CAPACITY)
    except BaseException:
        mc.close()
        raise
    return mc


def one_pass(mc, secs):
    """one measurement pass over `secs`; -> the number of accumulate calls"""
    calls = {"greens": mc.accumulate_greens, "correlations": mc.accumulate_correlations, "pairing": mc.accumulate_pairing,
             "susceptibilities": lambda: mc.accumulate_susceptibilities(recalculate=mc.p.safe_mult),  # and the recorded rows
             "thermodynamics": mc.accumulate_thermodynamics}
    for sec in secs:
        calls[sec]()
    return len(secs)


def sign_level(gpu, mc, sec, w, level=0):
    """(x_sum, x2_sum, count) of one level of the sign binner that goes with a section's pushes"""
    x, x2, cnt = np.zeros(1), np.zeros(1), C.c_int64()
    mc._c(gpu.lib().dqmc_binner_get_level(mc._h, gpu._lib.BIN_SIGN + STD.index(sec), w, level, gpu._lib.dptr(x),
                                          gpu._lib.dptr(x2), C.byref(cnt)))
    return x[0], x2[0], cnt.value


def samples(twin, which):
    """level 0 of the twin's binner after one push -> (x [W, E], x^2 [W, E])"""
    lv = [twin.binner_level(which, w, 0) for w in range(twin.n_walkers)]
    assert all(v[2] == 1 for v in lv), which
    return np.stack([v[0] for v in lv]), np.stack([v[1] for v in lv])


def weighted(X, s):
    """sum_w s_w X[w] in walker order in float64 and sum_w |X[w]|, both over the walkers kept: a left-out one is not read"""
    acc, mag = np.zeros(X.shape[1]), np.zeros(X.shape[1])
    for w in range(len(s)):
        if s[w] != 0:
            acc += float(s[w]) * X[w]
            mag += np.abs(X[w])
    return acc, mag


def check_sum(label, got, X, s, skip=(), minus_from=None):
    """got against sum_w s_w X[w] (minus_from = S: against S - that sum) within (W + 2) 2^-53 sum_w |X[w]|, and the
    non-vacuity gate against the unsigned sum over the walkers whose sample can be read (all but `skip`)"""
    W = len(s)
    want, mag = weighted(X, s)
    plain = sum(X[w] for w in range(W) if w not in skip)
    if minus_from is not None:
        want, plain = minus_from - want, float(W - len(skip)) - plain
    bound = (W + 2) * U53 * mag
    assert np.isfinite(got).all(), label
    err = np.abs(got - want)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print("signed sums %s: %d elements, max |device - host| = %.3e, worst err / bound = %.3f, sign matters by %.3e x bound"
          % (label, got.size, float(err.max()), worst, float(np.abs(want - plain).max() / bound.max())))
    assert (err <= bound).all(), label
    assert np.abs(want - plain).max() > 1e6 * bound.max(), label  # the sum without the signs lies far outside


def check_binner(gpu, label, twin_lv0, mc, which, s, tail):
    """level 0 of the signed handle's binner `which` after one push against s_w x_w of the twin, walker by walker"""
    X, X2 = twin_lv0
    E = X.shape[1]
    assert mc.binner_size(which)[0] == E + tail and mc.binner_size(which)[2] == 1, (label, which)
    for w in range(len(s)):
        xs, x2, cnt = mc.binner_level(which, w, 0)
        where = (label, which, w)
        assert cnt == 1, where
        if s[w] == 0:
            assert not xs.any() and not x2.any(), where  # all 0.0, the trailing s_w too
            continue
        assert np.array_equal(xs[:E], float(s[w]) * X[w]), where
        assert np.array_equal(x2[:E], X2[w]), where
        if tail:
            assert xs[E] == s[w] and x2[E] == 1.0, where


def check_pass(gpu, label, twin, mc, secs, mom, s, passes, fail0, skip=()):
    """everything the module docstring lists, after one pass of both handles"""
    W, n, nb = mc.n_walkers, mc.N, mc.nb
    kept, Ssum = int((s != 0).sum()), float(s.sum())
    lv0 = {k: samples(twin, k) for k in binned(secs, mom)}
    for w in skip:  # the poison was really there: the twin read it
        assert all(np.isnan(lv0[k][0][w]).any() for k in lv0), label
    # ---- binners
    for k in binned(secs, mom):
        check_binner(gpu, label, lv0[k], mc, k, s, tail=1 if (k in ALL_MOM or k == "thermodynamics") else 0)
        if k in STD:
            for w in range(W):
                assert sign_level(gpu, mc, k, w) == (float(s[w]), float(s[w] * s[w]), 1), (label, k, w)
    # ---- sums and counts
    sums = mc._section("sign")
    fed = [k for k in STD if k in binned(secs, mom)]
    assert sums.tolist() == [Ssum if k in fed else 0.0 for k in STD], label
    for sec in fed:
        raw, X = mc._section(sec), lv0[sec][0]
        assert raw[-1] == kept and twin._section(sec)[-1] == W, (label, sec)
        if sec != "greens":
            assert raw.size == X.shape[1] + 1
            check_sum("%s %s" % (label, sec), raw[:-1], X, s, skip)
            continue
        per = nb * n * n
        assert raw.size == 2 * per + nb * n + 1 and X.shape[1] == per + nb * n
        G = X[:, :per]
        diag = np.concatenate([b * n * n + np.arange(n) * (n + 1) for b in range(nb)])
        check_sum("%s greens G" % label, raw[:per], G, s, skip)
        check_sum("%s greens G^2" % label, raw[per:2 * per], G * G, s, skip)
        check_sum("%s greens occupation" % label, raw[2 * per:-1], G[:, diag], s, skip, minus_from=Ssum)
    if "thermodynamics" in secs:
        raw = mc._section("thermodynamics")
        assert raw.size == NE + 2 and (raw[-2], raw[-1]) == (Ssum, kept), label
        check_sum("%s thermodynamics" % label, raw[:NE], lv0["thermodynamics"][0], s, skip)
    assert np.array_equal(mc.sign_failures() - fail0, passes * (s == 0)), label
    assert not twin.sign_failures().any()


@contextlib.contextmanager
def pair(gpu, label, l, W, secs, mom=(), unit_signs=None, real_signs=None, poison=None, check=True, **kw):
    """the twin and the signed handle of a case after one pass, checked; both are closed on the way out"""
    twin = mc = None
    try:
        twin = handle(gpu, l, W, secs, mom, signed=False, **kw)
        mc = handle(gpu, l, W, secs, mom, signed=True, **kw)
        skip = () if poison is None else (poison,)
        for w in skip:
            nan = [np.full((mc.N, mc.N), np.nan)] * mc.nb
            twin.set_greens_eff(w, nan)
            mc.set_greens_eff(w, nan)
        for w in range(W):
            if w not in skip:
                assert np.stack(twin.greens(w)).tobytes() == np.stack(mc.greens(w)).tobytes(), (label, w)
        if unit_signs is not None:
            mc.impose_unit_signs(unit_signs)
            s = np.asarray(unit_signs).prod(axis=1)
        else:
            s = np.asarray(real_signs)
        assert np.array_equal(mc.sign(), s), label
        fail0 = mc.sign_failures()
        assert not fail0.any()
        assert one_pass(twin, secs) == len(secs)
        passes = one_pass(mc, secs)
        if check:
            check_pass(gpu, label, twin, mc, secs, mom, s, passes, fail0, skip)
        yield twin, mc, s
    finally:
        for m in (twin, mc):
            if m is not None:
                m.close()


# ---- group A: imposed signs -----------------------------------------------------------------------------------------
A1_SIGNS = np.array([[-1, -1], [-1, 1], [0, -1], [1, -1], [1, 1]])  # + - 0 - +: the block product, a zero in one block only


def a1(gpu):
    return dict(l=gpu.SquareLattice(10), W=5, secs=ALL, mom=ALL_MOM, seed=61)


def test_a1_off_the_tile_grid_every_section(gpu):
    assert A1_SIGNS.prod(axis=1).tolist() == [1, -1, 0, -1, 1]
    with pair(gpu, "A1", unit_signs=A1_SIGNS, **a1(gpu)) as (_, mc, _s):
        assert mc.N == 100 and mc.N % 64 != 0


def test_a2_second_trip_of_the_signed_sum_and_of_the_signed_push(gpu):
    l, W = gpu.SquareLattice(18), 3
    signs = np.array([[-1, 1], [-1, 0], [1, 1]])  # - 0 +
    with pair(gpu, "A2", l, W, ("greens", "correlations", "thermodynamics"), ("momentum_correlations",), unit_signs=signs,
              seed=62) as (_, mc, _s):
        n, E = mc.N, mc.binner_size("greens")[0]
        assert n == 324 and E == 210600
        assert 2 * n * n > 512 * 256                   # accumulate_signed_kernel: a second grid-stride trip
        assert E > ((2048 + W - 1) // W) * 256         # binner_push_signed_kernel<GREENS>: a second trip per walker


def test_a3_the_cap_exactly_and_two_groups_of_units(gpu):
    l, W = gpu.SquareLattice(16), 5
    signs = np.array([[-1, 1], [1, 1], [1, 0], [1, -1], [-1, 1]])  # - + 0 - -
    with pair(gpu, "A3", l, W, ("greens", "correlations", "pairing", "thermodynamics"), unit_signs=signs,
              seed=63) as (_, mc, _s):
        n = mc.N
        assert 2 * n * n == 512 * 256                  # the cap with no second trip
        assert 8 < W * mc.nb < 16                      # one whole group of eight units and a partial one


def a4_signs():
    signs = np.random.default_rng(7).integers(-1, 2, size=(257, 2))
    signs[255] = (0, 1)
    signs[256] = (1, -1)
    return signs


def test_a4_more_walkers_than_one_stride_of_the_walker_loop(gpu):
    signs, W = a4_signs(), 257
    s = signs.prod(axis=1)
    assert (s[255], s[256]) == (0, -1) and {-1, 0, 1} == set(s[:255].tolist())
    assert W > 256                                     # sign_prepare_kernel: a second trip over the walkers
    assert (2048 + W - 1) // W == 8                    # launch_binner_push: the cap per walker
    with pair(gpu, "A4", gpu.SquareLattice(4), W, ALL, ALL_MOM, unit_signs=signs, seed=64) as (_, mc, _s):
        assert mc.N == 16


def test_two_passes_with_different_signs_and_no_update_between(gpu):
    """s then s' = -s for walkers 0 and 1: level 0 holds (s + s') x, an exact 0 where they cancel, level 1 their average"""
    cfg = a1(gpu)
    secs, mom, W = cfg["secs"], cfg["mom"], cfg["W"]
    second = A1_SIGNS.copy()
    second[0] = (1, -1)
    second[1] = (1, 1)
    with pair(gpu, "two passes", unit_signs=A1_SIGNS, check=False, **cfg) as (twin, mc, s):
        s2 = second.prod(axis=1)
        assert s2.tolist() == [-1, 1, 0, -1, 1] and s.tolist() == [1, -1, 0, -1, 1]
        mc.impose_unit_signs(second)
        assert np.array_equal(mc.sign(), s2)
        passes = one_pass(mc, secs)
        assert np.array_equal(mc.sign_failures(), 2 * passes * (s == 0))
        for k in binned(secs, mom):
            X, X2 = samples(twin, k)
            tail = k in ALL_MOM or k == "thermodynamics"
            E, L, T = mc.binner_size(k)
            assert (E, L, T) == (X.shape[1] + tail, 3, 2), k
            for w in range(W):
                b = LB.LogBinnerRef(E, CAPACITY)
                for sg in (s[w], s2[w]):
                    x = float(sg) * X[w] if sg != 0 else np.zeros(E - tail)
                    b.push(np.concatenate([x, [float(sg)]]) if tail else x)
                for lv in (0, 1):
                    xs, x2, cnt = mc.binner_level(k, w, lv)
                    assert np.array_equal(xs, b.x_sum[lv]) and np.array_equal(x2, b.x2_sum[lv]) and cnt == b.count[lv], (k, w, lv)
                xs, x2, _ = mc.binner_level(k, w, 0)
                assert np.array_equal(xs[:E - tail], float(s[w] + s2[w]) * X[w]), (k, w)
                if w < 2:
                    assert not xs.any(), (k, w)  # the signs cancel: 0.0, no rounding residue
                if s[w] != 0:
                    assert np.array_equal(x2[:E - tail], 2.0 * X2[w]), (k, w)
                xs, _, cnt = mc.binner_level(k, w, 1)
                assert cnt == 1 and np.array_equal(xs[:E - tail], 0.5 * float(s[w] + s2[w]) * X[w]), (k, w)
        assert mc._section("sign").tolist() == [float(s.sum() + s2.sum())] * 5


# Where an observable is the same for every field (the density of the half-filled model is 1) the jackknife error is the
# rounding noise of the leave-one-out ratios r_w, and two ways of forming them agree only to that noise: each r_w carries
# at most three roundings (sum, difference, quotient), 3 2^-53 |r|, the deviations r_w - mean twice that, and
# sqrt((W - 1) / W sum_w (.)^2) of W = 5 such deviations at most sqrt(W - 1) 6 2^-53 |r| = 12 2^-53 |r|: a floor of 16 2^-53 |r|
# next to the relative 1e-12.
JK_FLOOR = 16 * U53


def test_signed_ratio_and_its_jackknife_with_a_walker_left_out(gpu):
    """signs + - 0 + +: the sum of signs (2) and every sum with one walker left out (1, 3, 2, 1, 1) is away from 0"""
    signs = np.array([[1, 1], [-1, 1], [0, -1], [-1, -1], [1, 1]])
    with pair(gpu, "ratio", gpu.SquareLattice(10), 5, ("greens", "thermodynamics"), unit_signs=signs, seed=61) as (twin, mc, s):
        assert s.tolist() == [1, -1, 0, 1, 1]
        W, n, nb, Ssum, kept = 5, mc.N, mc.nb, 2.0, 4
        per = nb * n * n
        # greens
        X = samples(twin, "greens")[0]
        diag = np.concatenate([b * n * n + np.arange(n) * (n + 1) for b in range(nb)])
        want, mag = weighted(X[:, :per], s)
        occ, occ_mag = weighted(X[:, diag], s)
        want, mag = np.concatenate([want, Ssum - occ]), np.concatenate([mag, occ_mag])  # occupation = sum s - sum s g_ii
        sx, sw = mc.signed_walker_sums("greens")
        assert sw.tolist() == s.tolist() and not sx[2].any()  # the left-out walker enters as (0, 0)
        ratio, err = S.jackknife_ratio(sx, sw)
        res = mc.signed("greens")
        assert (res["count"], res["sign_sum"], res["mean_sign"]) == (kept, Ssum, Ssum / kept)
        assert mc.mean_sign("greens") == Ssum / kept
        got = np.concatenate([g.reshape(-1, order="F") for g in res["G"]] + list(res["occupation"]))
        bound = ((W + 2) * U53 * mag + U53 * np.abs(want)) / Ssum  # the sums' bound and the one division
        assert (np.abs(got - want / Ssum) <= bound).all()
        got_err = np.concatenate([g.reshape(-1, order="F") for g in res["G_std_error"]] + list(res["occupation_std_error"]))
        assert (err > 0).any() and (np.abs(got_err - err) <= 1e-12 * err + JK_FLOOR * np.abs(ratio)).all()
        # thermodynamics
        X = samples(twin, "thermodynamics")[0]
        want, mag = weighted(X, s)
        sx, sw = mc.signed_walker_sums("thermodynamics")
        assert sw.tolist() == s.tolist() and not sx[2].any()
        ratio, err = S.jackknife_ratio(sx, sw)
        res = mc.signed("thermodynamics")
        assert (res["count"], res["sign_sum"], res["mean_sign"]) == (kept, Ssum, Ssum / kept)
        assert mc.mean_sign("thermodynamics") == Ssum / kept
        for e, name in enumerate(gpu._lib.THERMO_FIELDS):
            assert abs(res[name] - want[e] / Ssum) <= ((W + 2) * U53 * mag[e] + U53 * abs(want[e])) / Ssum, name
            assert abs(res[name + "_std_error"] - err[e]) <= 1e-12 * err[e] + JK_FLOOR * abs(ratio[e]), name
        assert (err > 0).any()


def test_the_override_ends_with_the_cache_and_the_refusals(gpu):
    l = gpu.SquareLattice(10)
    mc = fresh = att = None
    try:
        mc = handle(gpu, l, 5, ("greens",), signed=True, seed=61)
        lib, ERR = gpu.lib(), gpu._lib
        true = mc.sign()
        assert true.tolist() == [1] * 5  # a square lattice at half filling
        imposed = np.tile([-1, 1], (5, 1))

        def impose():
            mc.impose_unit_signs(imposed)
            assert mc.sign().tolist() == [-1] * 5

        impose()
        _, sg = mc.logdet()  # recomputes from scratch
        assert np.array_equal(sg.prod(axis=1), true) and np.array_equal(mc.sign(), true)
        impose()
        mc.sweep(1)
        assert (mc.current_slice, mc.direction) == (1, 1) and mc.sign().tolist() == [1] * 5
        impose()
        mc.set_conf(0, mc.conf(0))
        assert mc.sign().tolist() == [1] * 5
        # refusals; a refused call leaves the signs in force as they were
        impose()
        assert lib.dqmc_impose_unit_signs(mc._h, None) == ERR.ERR_INVALID
        for bad in (2, -2):
            sg = imposed.copy()
            sg[4, 1] = bad
            with pytest.raises(gpu.DQMCError) as e:
                mc.impose_unit_signs(sg)
            assert e.value.code == ERR.ERR_INVALID
        with pytest.raises(ValueError):
            mc.impose_unit_signs(imposed[:4])
        assert mc.sign().tolist() == [-1] * 5
        fresh = gpu.DQMC(gpu.HubbardModelRepulsive(l=gpu.SquareLattice(4), U=4.0), n_walkers=2, beta=1.0, safe_mult=5)
        with pytest.raises(gpu.DQMCError) as e:  # before dqmc_prepare
            fresh.impose_unit_signs(np.ones((2, 2), dtype=int))
        assert e.value.code == ERR.ERR_STATE
        att = gpu.DQMC(gpu.HubbardModelAttractive(l=gpu.SquareLattice(4), U=4.0), n_walkers=2, beta=1.0, safe_mult=5)
        att.prepare()
        with pytest.raises(gpu.DQMCError) as e:  # +1 by construction, no array behind it
            att.impose_unit_signs(np.ones((2, 1), dtype=int))
        assert e.value.code == ERR.ERR_STATE and att.sign().tolist() == [1, 1]
    finally:
        for m in (mc, fresh, att):
            if m is not None:
                m.close()


# ---- group B: the chain's own signs, W != 4 -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def golden_pair(gpu, golden, name, seeds, secs, label):
    case = golden["logdet"][name]
    by_seed = dict(zip(case["seeds"], S.sign_products(case).tolist()))
    signs = np.array([by_seed[sd] for sd in seeds])
    fields = [ref.field(sd, case["n"], case["slices"]) for sd in seeds]
    model = ref.golden_model(gpu, case)
    return pair(gpu, label, model.l, len(seeds), secs, real_signs=signs, model=model, beta=case["beta"],
                safe_mult=golden["safe_mult"], fields=fields), signs


def test_b1_real_signs_of_nine_walkers(gpu, golden):
    seeds = [(0, 2, 3, 4)[w % 4] for w in range(9)]
    cm, signs = golden_pair(gpu, golden, "triangular10", seeds, ("greens", "correlations", "pairing"), "B1")
    assert signs.tolist() == [1, -1, 1, -1, 1, -1, 1, -1, 1]
    with cm as (_, mc, _s):
        assert (mc.N, mc.p.slices, mc.n_walkers) == (100, 40, 9)


def test_b2_real_signs_of_five_walkers_at_n_256(gpu, golden):
    cm, signs = golden_pair(gpu, golden, "triangular16", [0, 64, 71, 73, 64], ("greens", "correlations", "thermodynamics"),
                            "B2")
    assert signs.tolist() == [1, -1, -1, -1, -1]
    with cm as (_, mc, _s):
        assert (mc.N, mc.p.slices, mc.n_walkers) == (256, 20, 5) and mc.kron_hopping()  # the three-factor hopping


# ---- group C: a left-out walker's sample is never read --------------------------------------------------------------
def test_c_a_left_out_walkers_nan_reaches_nothing(gpu):
    """G of walker 1 is NaN on both handles; only the equal-time passes run (products and pair sums: no factorisation
    sees the NaN).  check_pass asserts the twin's NaN, finite sums equal to the two-walker expectation, walker 1's binners
    all 0.0."""
    signs = np.array([[-1, 1], [0, -1], [1, 1]])
    secs = ("greens", "correlations", "pairing", "thermodynamics")
    with pair(gpu, "C", gpu.SquareLattice(6), 3, secs, ("momentum_correlations",), unit_signs=signs, poison=1,
              seed=65) as (twin, mc, s):
        assert s.tolist() == [-1, 0, 1]
        for k in binned(secs, ("momentum_correlations",)):
            for w in (0, 2):
                for lv in range(mc.binner_size(k)[1]):
                    xs, x2, _ = mc.binner_level(k, w, lv)
                    assert np.isfinite(xs).all() and np.isfinite(x2).all(), (k, w, lv)
            for lv in range(mc.binner_size(k)[1]):
                xs, x2, _ = mc.binner_level(k, 1, lv)
                assert not xs.any() and not x2.any(), (k, lv)
        assert np.isnan(twin._section("greens")[:-1]).any() and np.isfinite(mc._section("greens")).all()
        assert mc.sign_failures().tolist() == [0, len(secs), 0]


# ---- group D: checkpoint --------------------------------------------------------------------------------------------
def test_d_sign_failures_and_sign_sums_through_a_checkpoint(gpu):
    cfg = a1(gpu)
    with pair(gpu, "D", unit_signs=A1_SIGNS, check=False, **cfg) as (_, mc, s):
        fresh = handle(gpu, signed=True, **cfg)
        try:
            want = mc.sign_failures()
            assert want.tolist() == [0, 0, len(cfg["secs"]), 0, 0] and not fresh.sign_failures().any()
            fresh.set_state(mc.state())
            assert np.array_equal(fresh.sign_failures(), want)
            assert fresh._section("sign").tobytes() == mc._section("sign").tobytes()
            assert mc._section("sign").tolist() == [float(s.sum())] * 5
            for sec in STD + ("thermodynamics",):
                a, b = mc._section(sec), fresh._section(sec)
                assert a.tobytes() == b.tobytes() and a[-1] == 4, sec
            th = fresh._section("thermodynamics")
            assert (th[-2], th[-1]) == (float(s.sum()), 4.0)
        finally:
            fresh.close()
