"""Global moves of the DQMC flavor on the device (include/dqmc_hip.h "global moves"; csrc/logdet.hip,
csrc/global_move.inl) against tests/global_move_ref.py.

LOGDET_TOL, the absolute tolerance on logabsdet.  The float64 restatement of the reference's algorithm
(global_move_ref.oracle_logdet: the CPU oracle's udt_AVX_pivot! and rdivp!, sum log D2) was compared with the 60-digit
mpmath value on the very inputs of test_logdet_against_mpmath; the largest differences were 8.7e-15 (attractive square,
beta = 2), 7.6e-13 (repulsive square, beta = 2) and 6.2e-12 (repulsive triangular, beta = 4, seed 59290).  The device
reorders the sums, so it is allowed ten times the largest: 6.2e-11.  At n = 256 (attractive 16 x 16, beta = 1, seeds 200
and 201) the same oracle differs from a 100-digit evaluation (400-bit fixed-point slice chain, LU in mpmath) by 9.4e-14
and 1.45e-13; ten times the larger: LOGDET_TOL_256 = 1.45e-12.

The triangular case.  Negative determinants are rare among random fields at U = 8, beta = 4 on TriangularLattice(4): the
stabilised float64 oracle finds 162 among the fields of seeds 0 .. 59999 (a plain float64 product of the slices gives
about one half, which is rounding noise, not physics).  Seeds 58187 (signs -1, +1) and 59290 (+1, -1) are two of them,
confirmed with mpmath; seeds 100 and 101 have both signs +1.  The test asserts that mix so that it cannot pass vacuously.

Away from 4 x 4 (sections 9 to 11) the expected log-determinants of the current and the proposed fields come from
tests/golden/logdet_sizes.json (tools/make_logdet_golden.py, checked on the CPU by test_logdet_golden.py).  The
tolerance on logabsdet is ten times the oracle's largest distance from them on these very fields: TriangularLattice(8),
beta = 4: 4.7e-10 -> LOGDET_TOL_T8 = 4.7e-9; 4 x 4 attractive with 300 slices of dtau = 0.01: 1.5e-14 -> LOGDET_TOL_300 =
1.5e-13.  A weight ratio carries four log-determinant errors (two blocks, or one block squared, before and after), and
the rounding of exp's argument: |p / p_ref - 1| <= expm1(4 tol) + 2^-52 (|log|p_ref|| + 1).  FLIP_ALL of the repulsive
model at mu = 0 exchanges the two blocks' matrices, so p = 1 up to rounding on every lattice: negative weights are found
among the FLIP_SITE proposals only (17 of walker 0's 64 sites; the golden sites give p < 0 for three of the four walkers)."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

import global_move_ref as ref
from conftest import relerr

pytestmark = pytest.mark.gpu

LOGDET_TOL = 6.2e-11
LOGDET_TOL_256 = 1.45e-12
LOGDET_TOL_T8 = 4.7e-9
LOGDET_TOL_300 = 1.5e-13
TOL_G = 1e-10  # the project's bound on Green's functions


def field(seed, n, M):
    rng = np.random.Generator(np.random.Philox(key=seed))
    return np.asfortranarray((2 * rng.integers(0, 2, size=(n, M)) - 1).astype(np.int8))


def make(gpu, case, n_walkers, **kw):
    if case == "attractive":
        model = gpu.HubbardModelAttractive(4, 2, U=4.0, mu=0.5)
    elif case == "repulsive":
        model = gpu.HubbardModelRepulsive(4, 2, U=8.0)
    else:
        model = gpu.HubbardModelRepulsive(l=gpu.TriangularLattice(4), U=8.0)
    kw.setdefault("beta", 1.0)
    return gpu.DQMC(model, n_walkers=n_walkers, delta_tau=0.1, **kw)


def confs(mc):
    return [mc.conf(w) for w in range(mc.n_walkers)]


# ---- 1. logdet against the reference -------------------------------------------------------------------------------
LOGDET_CASES = {"attractive": (2.0, (100, 101, 102, 103)), "repulsive": (2.0, (100, 101, 102, 103)),
                "triangular": (4.0, (100, 101, 58187, 59290))}


@pytest.mark.parametrize("case", sorted(LOGDET_CASES))
def test_logdet_against_mpmath(gpu, case):
    """attractive 4 x 4 (U = 4, mu = 0.5, beta = 2), repulsive 4 x 4 (U = 8, beta = 2), repulsive TriangularLattice(4)
    (U = 8, beta = 4); dtau = 0.1, four seeded random fields each: |logabsdet - mpmath| <= LOGDET_TOL (module docstring),
    signs equal.  Triangular: both signs occur and one walker's product of signs is negative."""
    beta, seeds = LOGDET_CASES[case]
    mc = make(gpu, case, len(seeds), beta=beta)
    try:
        fields = [field(s, 16, mc.p.slices) for s in seeds]
        for w, c in enumerate(fields):
            mc.set_conf(w, c)
        lad, sg = mc.logdet()
        worst = 0.0
        for w, c in enumerate(fields):
            l0, s0 = ref.slogdet_mp(mc.model, 0.1, c)
            assert list(sg[w]) == s0, (case, seeds[w], sg[w], s0)
            worst = max(worst, max(abs(float(lad[w, b] - l0[b])) for b in range(mc.nb)))
        print("logdet %s: max |device - mpmath| = %.3e" % (case, worst))
        assert worst <= LOGDET_TOL
        if case == "triangular":
            assert set(sg.reshape(-1)) == {-1, 1}
            assert any(sg[w, 0] * sg[w, 1] < 0 for w in range(len(seeds)))
        # from scratch every time, and nothing of the sweep state is touched
        lad2, sg2 = mc.logdet()
        assert np.array_equal(lad, lad2) and np.array_equal(sg, sg2)
    finally:
        mc.close()


# ---- 2. one size off the small path --------------------------------------------------------------------------------
def test_logdet_at_256_against_the_float64_oracle(gpu, O):
    """attractive 16 x 16, beta = 1, 2 walkers: the size of the one-launch UDT and the slab kernels, and of the LU that
    runs in memory instead of LDS; against the float64 oracle's sum log D2 and sign det A2"""
    model = gpu.HubbardModelAttractive(16, 2, U=4.0, mu=0.5)
    mc = gpu.DQMC(model, n_walkers=2, beta=1.0, delta_tau=0.1)
    try:
        assert mc.udt_one_launch_sites() != 0
        fields = [field(s, 256, 10) for s in (200, 201)]
        for w, c in enumerate(fields):
            mc.set_conf(w, c)
        lad, sg = mc.logdet()
        for w, c in enumerate(fields):
            l0, s0, _ = ref.oracle_logdet(O, model, 0.1, 10, c)
            print("logdet 256 walker %d: |device - oracle| = %.3e" % (w, abs(lad[w, 0] - l0[0])))
            assert sg[w, 0] == s0[0]
            assert abs(lad[w, 0] - l0[0]) <= LOGDET_TOL_256
    finally:
        mc.close()


# ---- 3. decision parity ----------------------------------------------------------------------------------------------
PARITY_SEEDS = tuple(range(304, 312))


@pytest.fixture(scope="module")
def parity_ref(gpu):
    """reference weight ratios of both kinds for the eight fields (attractive 4 x 4, U = 4, mu = 0.5, beta = 1)"""
    model = gpu.HubbardModelAttractive(4, 2, U=4.0, mu=0.5)
    out = {}
    for s in PARITY_SEEDS:
        c = field(s, 16, 10)
        site = (5 * s + 3) % 16
        out[s] = dict(conf=c, site=site,
                      p={"all": float(ref.weight_ratio(model, 0.1, c, ref.apply_flip(c, ref.FLIP_ALL))),
                         "site": float(ref.weight_ratio(model, 0.1, c, ref.apply_flip(c, ref.FLIP_SITE, site)))})
    return out


@pytest.mark.parametrize("kind", ["all", "site"])
def test_decisions_match_the_reference(gpu, parity_ref, kind):
    """host-supplied streams: [site uniform (FLIP_SITE only)][acceptance uniform][filler].  Walkers with p <= 1 alternate
    between u = p / 2 (accepted) and u = (1 + p) / 2 (rejected), so every p is a factor two away from its uniform (cap on
    walkers skipped for a margin below 1e-8: 0 of 8).  The accepted / rejected pattern, the fields (bit for bit), the
    counters and the number of uniforms consumed - the second only when p <= 1 - equal the reference's."""
    mc = make(gpu, "attractive", len(PARITY_SEEDS))
    try:
        expect, streams, cats, toggle, skipped = [], [], set(), 0, 0
        for w, s in enumerate(PARITY_SEEDS):
            r = parity_ref[s]
            p = r["p"][kind]
            mc.set_conf(w, r["conf"])
            stream = [(r["site"] + 0.5) / 16] if kind == "site" else []
            u = 0.25
            if p <= 1:
                u = p / 2 if toggle % 2 == 0 else (1 + p) / 2
                toggle += 1
                if abs(u - p) <= 1e-8 * p:
                    skipped += 1
            it = iter([u])
            acc, drawn = ref.decide(p, lambda: next(it))
            cats.add("p>1" if p > 1 else ("u<p" if acc else "rejected"))
            new = ref.apply_flip(r["conf"], ref.FLIP_ALL if kind == "all" else ref.FLIP_SITE, r["site"])
            expect.append(dict(acc=acc, used=len(stream) + int(drawn), conf=new if acc else r["conf"]))
            mc.set_uniforms(w, np.array(stream + [u, 0.5, 0.5]))
        assert skipped == 0
        assert cats == {"p>1", "u<p", "rejected"}, cats
        mc.prepare()
        mc.global_move(kind)
        for w, e in enumerate(expect):
            st = mc.global_stats(w)
            assert (st["prop_global"], st["acc_global"], st["moves_drawn"]) == (1, int(e["acc"]), 1), (w, st, e["acc"])
            assert np.array_equal(mc.conf(w), e["conf"]), w
            assert mc.uniforms_used(w) == e["used"], (w, mc.uniforms_used(w), e["used"])
            a = mc.analysis(w)
            assert (a.prop_global, a.acc_global) == (1, int(e["acc"]))
    finally:
        mc.close()


# ---- 4. state after a move -------------------------------------------------------------------------------------------
def _state_after_a_move(mc, fresh, kind):
    W = mc.n_walkers
    try:
        before = confs(mc)
        mc.prepare()
        mc.global_move(kind)
        M = mc.p.slices
        assert (mc.current_slice, mc.direction) == (M, -1)
        after = confs(mc)
        acc = [mc.global_stats(w)["acc_global"] for w in range(W)]
        for w in range(W):
            assert np.array_equal(after[w], before[w]) == (acc[w] == 0)
            assert mc.uniforms_used(w) == 0
            fresh.set_conf(w, after[w])
        fresh.prepare()
        for w in range(W):
            g = mc.greens_eff(w)
            for b in range(mc.nb):
                assert relerr(g[b], mc.calculate_greens(M - 1, w)[b]) < TOL_G
                assert relerr(g[b], fresh.greens_eff(w)[b]) < TOL_G
        mc.sweep(1)
        fresh.sweep(1)
        for w in range(W):
            assert np.array_equal(mc.conf(w), fresh.conf(w))
            assert mc.uniforms_used(w) == fresh.uniforms_used(w) > 0
            for b in range(mc.nb):
                assert relerr(mc.greens_eff(w)[b], fresh.greens_eff(w)[b]) < TOL_G
        return acc
    finally:
        mc.close()
        fresh.close()


@pytest.mark.parametrize("kind", ["all", "site"])
def test_state_after_a_move_is_the_prepared_state(gpu, kind):
    """after a move the handle stands where dqmc_prepare leaves it: (current_slice, direction) = (slices, -1), and
    mc.s.greens is the from-scratch Green's function of the resulting field there.  In the reference's convention the
    down pass at current_slice = l holds G wrapped to l - 1 (propagate wraps once after the turn, stack.jl:571-580), i.e.
    calculate_greens(mc, slices - 1), which is what prepare() gives as well; both are asserted, within the project's
    1e-10.  A following sweep(1) equals that of a fresh handle given the fields by set_conf + prepare, with the same
    local stream (the move does not draw from it)."""
    _state_after_a_move(make(gpu, "repulsive", 4, seed=77), make(gpu, "repulsive", 4, seed=77), kind)


# ---- 5. independence -------------------------------------------------------------------------------------------------
def test_a_walker_does_not_depend_on_its_batch(gpu):
    """walker w of a 4-walker handle makes the moves of a 1-walker handle with first_walker = w: same sites, same
    decisions, same fields after three moves of each kind; and a move of one walker leaves the others' fields alone"""
    big = make(gpu, "repulsive", 4, seed=31)
    try:
        big.prepare()
        for kind in ("site", "site", "all", "site"):
            big.global_move(kind)
        for w in range(4):
            one = make(gpu, "repulsive", 1, seed=31, first_walker=w)
            try:
                one.prepare()
                for kind in ("site", "site", "all", "site"):
                    one.global_move(kind)
                assert np.array_equal(one.conf(0), big.conf(w)), w
                assert one.global_stats(0) == big.global_stats(w)
                assert np.abs(one.logdet()[0][0] - big.logdet()[0][w]).max() <= LOGDET_TOL
            finally:
                one.close()
        before, st = confs(big), [big.global_stats(w) for w in range(4)]
        big.global_move("all", walker=2)  # (exactly p = 1 at half filling up to rounding: accepted)
        for w in (0, 1, 3):
            assert np.array_equal(big.conf(w), before[w]) and big.global_stats(w) == st[w]
        assert big.global_stats(2)["prop_global"] == st[2]["prop_global"] + 1
    finally:
        big.close()


@pytest.fixture(scope="module")
def rate_runs(gpu):
    """rate = 2 over 4 sweeps in one call, and the same by hand: in the last update of sweeps 2 and 4 a global_move
    between propagate and sweep_spatial (the reference's hook, DQMC.jl:526-532)"""
    auto = make(gpu, "attractive", 3, seed=55, global_moves=True, global_rate=2, global_kind="site")
    hand = make(gpu, "attractive", 3, seed=55)
    auto.prepare()
    auto.sweep(4)
    hand.prepare()
    accepted = [0, 0, 0]
    M = hand.p.slices
    for i in range(1, 5):
        for _ in range(2 * M - 1):
            hand.update()
        hand.propagate()
        if i % 2 == 0:
            assert (hand.current_slice, hand.direction) == (M, -1)
            before = confs(hand)
            hand.global_move("site")
            for w in range(3):
                accepted[w] += int(not np.array_equal(hand.conf(w), before[w]))
        hand.sweep_spatial()
    yield auto, hand, accepted
    auto.close()
    hand.close()


def test_rate_equals_interleaving_by_hand(rate_runs):
    auto, hand, _ = rate_runs
    assert (auto.current_slice, auto.direction) == (hand.current_slice, hand.direction)
    for w in range(3):
        assert np.array_equal(auto.conf(w), hand.conf(w))
        assert relerr(auto.greens_eff(w)[0], hand.greens_eff(w)[0]) < TOL_G
        assert auto.uniforms_used(w) == hand.uniforms_used(w)


# ---- 6. rate and counters --------------------------------------------------------------------------------------------
def test_rate_counters(rate_runs):
    """prop_global = sweeps // rate; acc_global = the moves that changed the field in the run by hand"""
    auto, hand, accepted = rate_runs
    for w in range(3):
        st = auto.global_stats(w)
        assert st["prop_global"] == 4 // 2 and st["moves_drawn"] == 2
        assert st["acc_global"] == accepted[w] == hand.global_stats(w)["acc_global"]
        assert auto.analysis(w).prop_global == 2


def test_rate_zero_changes_nothing(gpu):
    """three seeded sweeps with the rate set to 0, and with update_until_measure: conf and mc.s.greens bit for bit those of
    a handle that was never told about global moves"""
    plain = make(gpu, "repulsive", 2, seed=9)
    off = make(gpu, "repulsive", 2, seed=9)
    try:
        off.set_global_rate(0, "all")
        for mc in (plain, off):
            mc.prepare()
            mc.sweep(3)
            mc.update_until_measure()
        for w in range(2):
            assert np.array_equal(plain.conf(w), off.conf(w))
            for b in range(2):
                assert np.array_equal(plain.greens_eff(w)[b], off.greens_eff(w)[b])
            assert off.global_stats(w) == dict(prop_global=0, acc_global=0, moves_drawn=0)
    finally:
        plain.close()
        off.close()


# ---- 7. exact known answer -------------------------------------------------------------------------------------------
def test_flip_all_is_always_accepted_at_half_filling(gpu):
    """repulsive 4 x 4 square lattice: det_up(-s) = det_dn(s), so p = 1 up to rounding for every field; the sums of
    logabsdet over the blocks before and after agree within LOGDET_TOL and the blocks' values are exchanged"""
    mc = make(gpu, "repulsive", 4, seed=13, beta=2.0)
    try:
        before = confs(mc)
        lad0, sg0 = mc.logdet()
        mc.prepare()
        for rep in (1, 2):
            mc.global_move("all")
            for w in range(4):
                assert mc.global_stats(w)["acc_global"] == rep
                assert np.array_equal(mc.conf(w), before[w] if rep == 2 else -before[w])
        mc.global_move("all")
        lad1, sg1 = mc.logdet()
        assert np.abs(lad0.sum(axis=1) - lad1.sum(axis=1)).max() <= LOGDET_TOL
        assert np.abs(lad0 - lad1[:, ::-1]).max() <= LOGDET_TOL and np.array_equal(sg0, sg1[:, ::-1])
    finally:
        mc.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from montecarlo_jl_amd import _lib
    mc = make(gpu, "attractive", 1)
    try:
        for call, code, word in ((lambda: mc.global_move("site"), _lib.ERR_STATE, "dqmc_prepare"),
                                 (lambda: mc.set_global_rate(-1, "site"), _lib.ERR_INVALID, "rate"),
                                 (lambda: mc.set_global_rate(2, 7), _lib.ERR_INVALID, "kind")):
            with pytest.raises(_lib.DQMCError) as e:
                call()
            assert e.value.code == code and word in str(e.value), str(e.value)
        mc.prepare()
        with pytest.raises(_lib.DQMCError) as e:
            mc.global_move(5)
        assert e.value.code == _lib.ERR_INVALID and "kind" in str(e.value)
        with pytest.raises(_lib.DQMCError) as e:
            mc.global_move("site", walker=3)
        assert e.value.code == _lib.ERR_INVALID
        st = _lib.GlobalStats()
        assert _lib.lib().dqmc_get_global_stats(mc._h, 4, C.byref(st)) == _lib.ERR_INVALID
        assert mc.global_stats(0) == dict(prop_global=0, acc_global=0, moves_drawn=0)
    finally:
        mc.close()


# ---- 9. decisions at TriangularLattice(8), with negative weights ----------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _p_ref(model, dtau, conf, new, cur, prop, w):
    """weight_ratio's formulas on the golden log-determinants -> mpf"""
    with mp.workdps(ref.DPS):
        l0, l1 = [mp.mpf(x) for x in cur["logabsdet"][w]], [mp.mpf(x) for x in prop["logabsdet"][w]]
        if model.flv == 1:
            dS = int(conf.astype(np.int64).sum() - new.astype(np.int64).sum())
            return mp.exp(mp.mpf(ref.hs_lambda(model.U, dtau)) * dS + 2 * (l1[0] - l0[0]))
        sp = cur["sign"][w][0] * cur["sign"][w][1] * prop["sign"][w][0] * prop["sign"][w][1]
        return sp * mp.exp((l1[0] - l0[0]) + (l1[1] - l0[1]))


def _p_tol(p, tol):
    return math.expm1(4 * tol) + 2.0 ** -52 * (abs(float(mp.log(abs(p)))) + 1)


def _seed_for_site(site, n, start):
    """the first walker seed from `start` on whose site uniform u(0, 0) lands on `site`"""
    s = start
    while ref.pick_site(ref.move_uniform(s, 0, 0), n) != site:
        s += 1
    return s


@pytest.mark.parametrize("kind", ["all", "site"])
def test_decisions_at_64_sites_with_negative_weights(gpu, golden, kind):
    """TriangularLattice(8), U = 8, beta = 4, the four golden fields, the device's own Philox uniforms: the walkers are
    seeded so that u(0, 0) picks the golden site.  last_p within the bound of the module docstring, the decision that of
    ref.decide with u(0, 1), the counters, the fields, and one negative_probability entry per negative p."""
    mv = golden["moves"]["triangular8"]
    case = golden["logdet"][mv["case"]]
    model = ref.golden_model(gpu, case)
    n, M = case["n"], case["slices"]
    mc = gpu.DQMC(model, n_walkers=4, beta=case["beta"], delta_tau=golden["delta_tau"], safe_mult=golden["safe_mult"])
    try:
        expect = []
        for w, s in enumerate(mv["seeds"]):
            c = ref.field(s, n, M)
            new = ref.apply_flip(c, ref.FLIP_ALL if kind == "all" else ref.FLIP_SITE, mv["sites"][w])
            p = _p_ref(model, golden["delta_tau"], c, new, case, mv[kind], w)
            seed = _seed_for_site(mv["sites"][w], n, 1000 * (w + 1)) if kind == "site" else 1000 * (w + 1)
            u = ref.move_uniform(seed, 0, 1)
            acc, _ = ref.decide(p, lambda: u)
            tol = _p_tol(p, LOGDET_TOL_T8)
            assert p > 1 + tol or abs(u - float(p)) > 2 * tol * abs(float(p)), "the decision hangs on rounding"
            mc.set_conf(w, c)
            mc.seed(w, seed)
            expect.append(dict(p=p, acc=acc, conf=new if acc else c, tol=tol))
        negative = sum(e["p"] < 0 for e in expect)
        print("moves triangular8 %s: %d negative p of 4" % (kind, negative))
        if kind == "site":
            assert negative >= 1
        mc.prepare()
        mc.global_move(kind)
        for w, e in enumerate(expect):
            last, st = mc.global_last(w), mc.global_stats(w)
            err = abs(float(mp.mpf(last["p"]) / e["p"] - 1))
            print("  walker %d: p = %.6e, |p / p_ref - 1| = %.3e, bound %.3e" % (w, last["p"], err, e["tol"]))
            assert err <= e["tol"]
            if kind == "site":
                assert last["site"] == mv["sites"][w]
            assert last["accepted"] == e["acc"]
            assert (st["prop_global"], st["acc_global"], st["moves_drawn"]) == (1, int(e["acc"]), 1)
            assert np.array_equal(mc.conf(w), e["conf"]), w
            a = mc.analysis(w)
            assert (a.prop_global, a.acc_global) == (1, int(e["acc"]))
            assert a.negative_probability.count == int(e["p"] < 0)
    finally:
        mc.close()


# ---- 10. state after a move at 64 and 256 sites ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "site"])
@pytest.mark.parametrize("where", ["triangular8", "square16_attractive"])
def test_state_after_a_move_is_the_prepared_state_at_larger_sizes(gpu, golden, where, kind):
    """test_state_after_a_move_is_the_prepared_state at TriangularLattice(8), U = 8, beta = 4 (n = 64) and at 16 x 16
    attractive, beta = 1 (n = 256: the one-launch UDT and the slab kernels rebuild the stack), same bound TOL_G"""
    case = golden["logdet"][where]
    model = ref.golden_model(gpu, case)
    kw = dict(n_walkers=4, beta=case["beta"], delta_tau=golden["delta_tau"], safe_mult=golden["safe_mult"], seed=77)
    _state_after_a_move(gpu.DQMC(model, **kw), gpu.DQMC(model, **kw), kind)


# ---- 11. FLIP_SITE over more than 256 slices ---------------------------------------------------------------------------------
def test_flip_site_over_300_slices(gpu, golden):
    """4 x 4 attractive, dtau = 0.01, beta = 3: gm_flip walks the 300 slices of a site in two turns of its 256 threads.
    Host streams [site uniform][acceptance uniform]; walkers with p <= 1 alternate between u = (1 + p) / 2 (rejected)
    and p / 2 (accepted).  The field afterwards is apply_flip's or the original, entry for entry; dS - twice the sum
    over all 300 entries of the line - is in last_p, which is held to weight_ratio's value on the golden
    log-determinants."""
    mv = golden["moves"]["slices300"]
    model = ref.golden_model(gpu, mv)
    n, M, dtau = mv["n"], mv["slices"], mv["delta_tau"]
    assert M > 256
    mc = gpu.DQMC(model, n_walkers=4, beta=mv["beta"], delta_tau=dtau, safe_mult=golden["safe_mult"])
    try:
        assert mc.p.slices == M
        expect, toggle = [], 0
        for w, s in enumerate(mv["seeds"]):
            c = ref.field(s, n, M)
            new = ref.apply_flip(c, ref.FLIP_SITE, mv["sites"][w])
            p = _p_ref(model, dtau, c, new, mv["cur"], mv["site"], w)
            u = 0.25
            if p <= 1:
                u = (1 + float(p)) / 2 if toggle % 2 == 0 else float(p) / 2
                toggle += 1
            acc, drawn = ref.decide(p, lambda: u)
            mc.set_conf(w, c)
            mc.set_uniforms(w, np.array([(mv["sites"][w] + 0.5) / n, u, 0.5, 0.5]))
            expect.append(dict(p=p, acc=acc, used=1 + int(drawn), conf=new if acc else c))
        assert {e["acc"] for e in expect} == {True, False}
        mc.prepare()
        mc.global_move("site")
        for w, e in enumerate(expect):
            last = mc.global_last(w)
            err, tol = abs(float(mp.mpf(last["p"]) / e["p"] - 1)), _p_tol(e["p"], LOGDET_TOL_300)
            print("300 slices walker %d: p = %.6e, |p / p_ref - 1| = %.3e, bound %.3e" % (w, last["p"], err, tol))
            assert err <= tol
            assert (last["site"], last["accepted"]) == (mv["sites"][w], e["acc"])
            assert np.array_equal(mc.conf(w), e["conf"]), w
            assert mc.uniforms_used(w) == e["used"]
    finally:
        mc.close()
