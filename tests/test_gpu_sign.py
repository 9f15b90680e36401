"""Sign-reweighted measurements on the device (include/dqmc_hip.h "sign reweighting"; csrc/sign.hip, global_move.inl):
dqmc_get_sign against the golden signs, the signed sums of every section against s_w x_w of single walkers, the
all-positive case bit for bit against a handle with weighting off, the Markov chain left alone, and the interface.

Fields: global_move_ref.field(seed, n, M), the seeds of tests/golden/logdet_sizes.json (test_sign_reference.py checks on
the CPU that they hold both signs):  triangular8 seeds 2, 3, 4, 12 -> - + + -;  triangular10 0, 2, 3, 4 -> + - + -;
triangular16 0, 64, 71, 73 -> + - - -;  square16_attractive -> +1.

Tolerance of test_weighted_sums: the device adds s_w x_w over the walkers in order, the host adds the same terms in its
own order; x_w of a one-walker handle is the sample the four-walker handle sees for that field.  Re-associating a sum of
W = 4 terms moves it by at most (W - 1) 2^-53 sum_w |x_w| to first order: the bound is 4 2^-53 sum_w |x_w| per element.
The sums of signs are small integers: exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_move_ref as ref  # noqa: E402
import sign_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SECTIONS = S.SECTIONS
EVERY = 10


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def make(gpu, golden, name, seeds=None, **kw):
    """a handle on the model of a golden case with the seeded fields of `seeds` (default: the case's four)"""
    case = golden["logdet"][name]
    seeds = case["seeds"] if seeds is None else seeds
    mc = gpu.DQMC(ref.golden_model(gpu, case), n_walkers=len(seeds), beta=case["beta"], delta_tau=golden["delta_tau"],
                  safe_mult=golden["safe_mult"], **kw)
    assert (mc.N, mc.p.slices) == (case["n"], case["slices"])
    for w, s in enumerate(seeds):
        mc.set_conf(w, ref.field(s, case["n"], case["slices"]))
    return mc


def configure_all(gpu, mc, every=EVERY):
    mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))  # the pair directions with them
    mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(mc.model.l))
    mc.set_time_displaced(every, ("greens", "density"))


def accumulate_all(mc):
    mc.accumulate_greens()
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    mc.accumulate_susceptibilities(recalculate=mc.p.safe_mult)  # feeds the time-displaced rows as well


def raw_sections(mc):
    """{section: (sums without the count, count)}"""
    return {sec: (mc._section(sec)[:-1].copy(), mc._section(sec)[-1]) for sec in SECTIONS}


# ---- 1. the sign of the current field ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["triangular8", "triangular10", "triangular16"])
def test_sign_equals_the_golden_products(gpu, golden, name):
    mc = make(gpu, golden, name)
    try:
        mc.prepare()
        want = S.sign_products(golden["logdet"][name])
        got = mc.sign()
        print("sign %s: device %s golden %s" % (name, got.tolist(), want.tolist()))
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert not mc.sign_weighting()  # (works with weighting off)
        assert np.array_equal(mc.sign(), want)  # from the kept values this time
        _, sg = mc.logdet()
        assert np.array_equal(sg.prod(axis=1), want)
        assert mc.sign_failures().tolist() == [0] * mc.n_walkers
    finally:
        mc.close()


def test_attractive_sign_is_one_without_a_launch(gpu, golden):
    mc = make(gpu, golden, "square16_attractive", sign_weighting=True)
    try:
        mc.prepare()
        mc.timing_enable(True)
        mc.synchronize()
        before = mc.timing()
        assert mc.sign().tolist() == [1, 1, 1, 1]
        mc.synchronize()
        assert {k: v[1] for k, v in mc.timing().items()} == {k: v[1] for k, v in before.items()}  # no launch at all
        # and a signed sum runs no slice chain: one small launch (the signs) next to the ones of an unsigned sum
        mc.accumulate_greens()
        mc.synchronize()
        after = mc.timing()
        assert after["qr"][1] == before["qr"][1] and after["trsm"][1] == before["trsm"][1]
        assert after["gemm"][1] == before["gemm"][1] + 2  # greens!(mc): two products
        assert mc.mean_sign("greens") == 1.0
    finally:
        mc.close()


# ---- 2. weighted sums ----------------------------------------------------------------------------------------------
T8_SEEDS = (2, 3, 4, 12)


@pytest.fixture(scope="module")
def single_walkers(gpu, golden):
    """x_w: the sums of every section after one pass of an unweighted one-walker handle on each triangular8 field"""
    out = {}
    for s in T8_SEEDS:
        mc = make(gpu, golden, "triangular8", seeds=[s])
        try:
            configure_all(gpu, mc)
            mc.prepare()
            mc.replay_greens(0)  # no update, the fields stay the seeded ones: mc.s.greens for them at current_slice = 1
            accumulate_all(mc)
            raw = raw_sections(mc)
            assert all(cnt == 1 for _, cnt in raw.values())
            out[s] = {sec: v for sec, (v, _) in raw.items()}
        finally:
            mc.close()
    return out


def weighted_handle(gpu, golden, seeds):
    mc = make(gpu, golden, "triangular8", seeds=list(seeds), sign_weighting=True)
    configure_all(gpu, mc)
    mc.prepare()
    mc.replay_greens(0)
    return mc


def check_weighted(mc, single, seeds, signs):
    raw = raw_sections(mc)
    for sec in SECTIONS:
        got, cnt = raw[sec]
        assert cnt == len(seeds), sec
        want = sum(float(sg) * single[s][sec] for s, sg in zip(seeds, signs))
        bound = 4 * 2.0 ** -53 * sum(np.abs(single[s][sec]) for s in seeds)
        err = np.abs(got - want)
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print("weighted %s: %d elements, max |device - host| = %.3e, worst error / bound = %.3f"
              % (sec, got.size, float(err.max()), worst))
        assert (err <= bound).all(), sec


def test_weighted_sums_of_four_walkers(gpu, golden, single_walkers):
    signs = S.sign_products(golden["logdet"]["triangular8"])
    mc = weighted_handle(gpu, golden, T8_SEEDS)
    try:
        accumulate_all(mc)
        assert np.array_equal(mc.sign(), signs)
        check_weighted(mc, single_walkers, T8_SEEDS, signs)
        sums = mc._section("sign")
        assert sums.shape == (5,) and sums.tolist() == [0.0] * 5  # - + + -
        assert mc.mean_sign("greens") == 0.0
        with pytest.raises(ValueError, match="sum of signs is 0"):
            mc.signed("greens")
        assert mc.sign_failures().tolist() == [0, 0, 0, 0]
    finally:
        mc.close()


def test_weighted_sums_of_three_walkers_and_the_ratio(gpu, golden, single_walkers):
    seeds, signs = T8_SEEDS[:3], S.sign_products(golden["logdet"]["triangular8"])[:3]
    mc = weighted_handle(gpu, golden, seeds)
    try:
        accumulate_all(mc)
        check_weighted(mc, single_walkers, seeds, signs)
        assert mc._section("sign").tolist() == [1.0] * 5  # - + +
        assert mc.mean_sign("susceptibilities") == 1.0 / 3.0
        res = mc.signed("greens")
        n, nb = mc.N, mc.nb
        host = sum(float(sg) * single_walkers[s]["greens"] for s, sg in zip(seeds, signs)) / 1.0  # / sum of signs
        bound = 4 * 2.0 ** -53 * sum(np.abs(single_walkers[s]["greens"]) for s in seeds)
        for b in range(nb):
            G = res["G"][b].reshape(-1, order="F")
            assert np.isfinite(G).all()
            assert (np.abs(G - host[b * n * n:(b + 1) * n * n]) <= bound[b * n * n:(b + 1) * n * n]).all()
        assert (res["count"], res["sign_sum"]) == (3, 1.0)
        for sec in SECTIONS[1:]:  # every section's dict is formed, with finite entries
            r = mc.signed(sec)
            assert all(np.isfinite(np.asarray(v)).all() for v in r.values())
    finally:
        mc.close()


# ---- 3. all signs +1: nothing changes ------------------------------------------------------------------------------
def square6(gpu, **kw):
    mc = gpu.DQMC(gpu.HubbardModelRepulsive(l=gpu.SquareLattice(6), U=4.0), n_walkers=4, beta=1.0, delta_tau=0.1,
                  safe_mult=5, seed=100, **kw)
    assert mc.seeds == [100, 101, 102, 103] and (mc.N, mc.p.slices) == (36, 10)
    for w, s in enumerate(mc.seeds):
        mc.set_conf(w, ref.field(s, 36, 10))
    configure_all(gpu, mc, every=5)
    mc.prepare()
    mc.enable_binning(SECTIONS, capacity=7)
    return mc


def test_all_positive_is_bitwise_the_unsigned_run(gpu):
    on, off = square6(gpu, sign_weighting=True), square6(gpu)
    try:
        for mc in (on, off):
            for _ in range(3):  # three pushes: levels 0 and 1 and a compressor carry
                mc.update_until_measure()
                accumulate_all(mc)
        assert (on.sign() == 1).all()
        for sec in SECTIONS:
            assert on._section(sec).tobytes() == off._section(sec).tobytes(), sec
            E, L, T = on.binner_size(sec)
            assert (E, L, T) == off.binner_size(sec) and T == 3
            for w in range(4):
                for lv in range(L):
                    a, b = on.binner_level(sec, w, lv), off.binner_level(sec, w, lv)
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], (sec, w, lv)
            assert on.mean_sign(sec) == 1.0
        assert on._section("sign").tolist() == [12.0] * 5
        assert off._section("sign").tolist() == [0.0] * 5
    finally:
        on.close()
        off.close()


# ---- 4. the Markov chain is left alone -----------------------------------------------------------------------------
def test_sign_evaluations_leave_the_chain_alone(gpu, golden, O):
    case = golden["logdet"]["triangular8"]
    on = make(gpu, golden, "triangular8", sign_weighting=True, seed=31)
    off = make(gpu, golden, "triangular8", seed=31)
    try:
        for mc in (on, off):
            mc.prepare()
            mc.sweep(2)
            mc.accumulate_greens()
            mc.sweep(2)
            mc.accumulate_greens()
        fields = [on.conf(w) for w in range(4)]
        for w in range(4):
            assert fields[w].tobytes() == off.conf(w).tobytes(), w
            assert on.uniforms_used(w) == off.uniforms_used(w), w
            assert np.array_equal(on.greens_eff(w), off.greens_eff(w)), w
        assert (on.current_slice, on.direction) == (off.current_slice, off.direction)
        got = on.sign()
        # the float64 oracle on the fields read back; a field counts only where a second float64 route with another
        # stabilisation agrees in both signs and to the tolerance the golden values of this case were accepted with
        tol = 4.7e-9
        want, left_out = [], []
        for w in range(4):
            lad, sg, _ = ref.oracle_logdet(O, on.model, golden["delta_tau"], golden["safe_mult"], fields[w])
            lad2, sg2 = ref.second_route_logdet(O, on.model, golden["delta_tau"], golden["safe_mult"], fields[w])
            if sg != sg2 or max(abs(a - b) for a, b in zip(lad, lad2)) > tol:
                left_out.append(w)
            want.append(int(np.prod(sg)))
        print("chain: signs after the sweeps device %s oracle %s, left out %s" % (got.tolist(), want, left_out))
        assert left_out == []
        assert got.tolist() == want
        assert on._section("greens")[-1] == 8 and on.sign_failures().tolist() == [0, 0, 0, 0]
        assert case["n"] == 64
    finally:
        on.close()
        off.close()


# ---- 5. interface ---------------------------------------------------------------------------------------------------
def parent_reduce_size(mc):
    """dqmc_reduce_size as it was before the sign section: the packed sums of the configured sections (the
    time-displaced rows without their count), six counter sums, two maxima, two minima"""
    n = mc._section_size("greens") + mc._section_size("correlations") + mc._section_size("pairing")
    n += mc._section_size("susceptibilities") + mc._section_size("time_displaced") - 1
    return n + 6 + 4


def test_interface(gpu):
    mc = square6(gpu)
    try:
        mc.update_until_measure()
        lib = gpu.lib()
        assert mc.reduce_size() == parent_reduce_size(mc)  # weighting off: the packed format is the old one
        with pytest.raises(gpu.DQMCError) as e:  # nothing packed for the section while weighting is off
            mc.reduce(None)
            mc.reduced("sign")
        assert e.value.code == gpu._lib.ERR_STATE
        mc.accumulate_greens()
        assert lib.dqmc_set_sign_weighting(mc._h, 1) == gpu._lib.ERR_STATE  # samples present
        assert not mc.sign_weighting()
        mc.reset_accumulators()
        mc.set_sign_weighting(True)
        assert mc.sign_weighting() and mc.reduce_size() == parent_reduce_size(mc) + 5
        accumulate_all(mc)
        assert lib.dqmc_set_sign_weighting(mc._h, 0) == gpu._lib.ERR_STATE
        assert mc._section("sign").tolist() == [4.0] * 5
        # export / import round trip of the packed buffer with the sign sums in it
        buf = mc.reduce_export()
        off = parent_reduce_size(mc) - 10
        assert buf[off:off + 5].tolist() == [4.0] * 5
        mc.reduce_import(2.0 * buf)  # what two ranks with the same sums reduce to
        assert mc.reduced("sign").tolist() == [8.0] * 5
        assert mc.sign_sums(reduced=True)["pairing"] == 8.0
        assert np.array_equal(mc.reduced("greens"), 2.0 * mc._section("greens"))
        mc.reduce(None)
        assert mc.reduced("sign").tolist() == [4.0] * 5
        mc.reset_accumulators()
        assert mc._section("sign").tolist() == [0.0] * 5
        mc.set_sign_weighting(False)
        assert mc.reduce_size() == parent_reduce_size(mc)
    finally:
        mc.close()


def test_jackknife_error_from_the_binners(gpu, golden):
    # five walkers on the fields of seeds 2, 3, 4, 3, 4: signs - + + + +, so that the sum of signs (3 per push) and every
    # sum with one walker left out (4, 2, 2, 2, 2) is away from 0; two pushes on the seeded fields
    seeds, signs = (2, 3, 4, 3, 4), [-1, 1, 1, 1, 1]
    mc = make(gpu, golden, "triangular8", seeds=list(seeds), sign_weighting=True)
    try:
        mc.prepare()
        mc.enable_binning(("greens",), capacity=7)
        mc.accumulate_greens()
        mc.accumulate_greens()
        assert mc.sign().tolist() == signs
        sx, sw = mc.signed_walker_sums("greens")
        assert sx.shape == (5, mc.binner_size("greens")[0]) and sw.tolist() == [2.0 * s for s in signs]
        assert sw.sum() == mc._section("sign")[0] == 6.0
        # the same field gives the same sample: walkers 1 and 3
        assert mc.binner_level("greens", 1, 0)[0].tobytes() == mc.binner_level("greens", 3, 0)[0].tobytes()
        ratio, err = S.jackknife_ratio(sx, sw)
        assert (err[:mc.nb * mc.N * mc.N] > 0).any()
        res = mc.signed("greens")
        n, nb = mc.N, mc.nb
        for b in range(nb):
            want = err[b * n * n:(b + 1) * n * n]
            assert np.allclose(res["G_std_error"][b].reshape(-1, order="F"), want, rtol=1e-12, atol=1e-15)
            # the ratio itself, level 0 of the binners against the accumulator: the same 10 terms s g, |g| <= 1 up to
            # rounding, added in another order: 10 2^-53 10 = 1.1e-14 on the sum, and |sum of signs| = 6
            assert np.allclose(res["G"][b].reshape(-1, order="F"), ratio[b * n * n:(b + 1) * n * n], rtol=0, atol=2e-14)
        assert np.allclose(np.concatenate(res["occupation_std_error"]), err[nb * n * n:], rtol=1e-12, atol=1e-15)
        with pytest.raises(ValueError):  # one walker: no jackknife
            one = make(gpu, golden, "triangular8", seeds=[3], sign_weighting=True)
            try:
                one.prepare()
                one.enable_binning(("greens",), capacity=3)
                one.accumulate_greens()
                one.signed("greens")
            finally:
                one.close()
    finally:
        mc.close()
