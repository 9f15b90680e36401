"""wrap_greens! on the factored n = 256 path as ONE launch (kron.hip: kron_wrap_kernel, both one-step chains with a hand-off
per unit) against the two-launch form it replaces (DQMC_WRAP_TWO_LAUNCH=1, read when a handle is created).  The two forms
run the same products in the same order on the same operands, so everything is compared bit for bit.  Against
DQMC_NO_WRAP_FLUSH=1 (stand-alone flush of a sweep's last chunk) the update is re-associated, and G is compared within
the bound tests/test_gpu_wrap_flush.py uses for that comparison.  The one-launch form needs its whole grid co-resident
(16 workgroups per unit, units padded to eights): 32 and 2 attractive walkers take it, 80 units do not."""
import os

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu
TOL_FLUSH = 1e-13


def _handle(gpu, model, switch, **kw):
    if switch:
        os.environ[switch] = "1"
    try:
        mc = gpu.DQMC(model, **kw)
    finally:
        if switch:
            os.environ.pop(switch, None)
    assert mc.kron_hopping()
    return mc


def _same_chain(a, b, walkers):
    for w in range(walkers):
        assert np.array_equal(a.conf(w), b.conf(w)), "HS field of walker %d differs" % w
        sa, sb = a.analysis(w), b.analysis(w)
        assert (sa.prop_local, sa.acc_local) == (sb.prop_local, sb.acc_local), w
        assert a.uniforms_used(w) == b.uniforms_used(w), w


def _same_bits(a, b, walkers, what):
    for w in range(walkers):
        for ga, gb in zip(a.greens_eff(w), b.greens_eff(w)):
            assert np.array_equal(ga, gb), "%s: greens of walker %d differs, max |diff| %.3g" % (what, w, np.abs(ga - gb).max())


def _clean(*mcs):
    for mc in mcs:
        assert mc.device_errors() == 0
        assert mc.qr_fallbacks() == 0
        assert mc.kron_hopping()
        mc.close()


def _gemm_launches_of_a_sweep(mc):
    mc.timing_enable(True)
    mc.sweep(1)
    n = mc.timing()["gemm"][1]
    mc.timing_enable(False)
    return n


# config 3's shape (attractive 16 x 16, beta = 8, M = 80, safe_mult 10); 2 walkers: a grid padded to eight units
@pytest.mark.parametrize("walkers", [32, 2])
def test_one_launch_bit_identical_to_two_launches(gpu, walkers):
    kw = dict(beta=8.0, delta_tau=0.1, safe_mult=10, n_walkers=walkers, seed=77)
    one = _handle(gpu, gpu.HubbardModelAttractive(16, 2), None, **kw)
    two = _handle(gpu, gpu.HubbardModelAttractive(16, 2), "DQMC_WRAP_TWO_LAUNCH", **kw)
    for mc in (one, two):
        mc.prepare()
        mc.sweep(2)
    _same_chain(one, two, walkers)
    _same_bits(one, two, walkers, "prepare + 2 sweeps")
    # single wraps (no sweep update pending: the form without the pending chunk), up and back down again, which leaves
    # greens where it was up to rounding
    for mc in (one, two):
        assert (mc.current_slice, mc.direction) == (one.current_slice, one.direction)
    sl = max(1, min(one.current_slice, one.p.slices - 1))
    for step, (s, d) in enumerate([(sl, +1), (sl + 1, -1)]):
        for mc in (one, two):
            mc.wrap_greens(s, d)
        _same_bits(one, two, walkers, "wrap %d (slice %d, direction %+d)" % (step, s, d))
    # which form ran: every wrap is one launch of the gemm family instead of two.  A sweep wraps greens once per slice step
    # (2 M of them) except where it is recomputed from the stack (2 M / safe_mult boundaries)
    n1, n2 = _gemm_launches_of_a_sweep(one), _gemm_launches_of_a_sweep(two)
    M, sm = one.p.slices, one.p.safe_mult
    print("%d walkers: gemm-family launches per sweep %d (two-launch form %d)" % (walkers, n1, n2))
    assert n2 - n1 >= 2 * M - 2 * M // sm, (n1, n2)
    _same_chain(one, two, walkers)
    _same_bits(one, two, walkers, "third sweep")
    _clean(one, two)


@pytest.mark.parametrize("walkers", [32, 2])
def test_one_launch_matches_stand_alone_flush(gpu, walkers):
    kw = dict(beta=8.0, delta_tau=0.1, safe_mult=10, n_walkers=walkers, seed=78)
    one = _handle(gpu, gpu.HubbardModelAttractive(16, 2), None, **kw)
    ref = _handle(gpu, gpu.HubbardModelAttractive(16, 2), "DQMC_NO_WRAP_FLUSH", **kw)
    for mc in (one, ref):
        mc.prepare()
        mc.sweep(1)
        # a sweep that starts (and ends) three slices into the up pass: the G compared comes out of wraps that took the
        # pending chunk, not out of calculate_greens (a pending chunk lives only inside one call: update() alone ends with
        # the stand-alone flush in both handles)
        for _ in range(3):
            mc.update()
        mc.sweep(1)
    _same_chain(one, ref, walkers)
    worst = 0.0
    for w in range(walkers):
        for ga, gb in zip(one.greens_eff(w), ref.greens_eff(w)):
            worst = max(worst, relerr(ga, gb))
    print("%d walkers: max rel |G_one_launch - G_stand_alone_flush| = %.3g" % (walkers, worst))
    assert worst < TOL_FLUSH, worst
    _clean(one, ref)


def test_80_units_keep_two_launches_and_match_oracle(gpu, O):
    """40 repulsive walkers = 80 units = 1280 workgroups: not co-resident, so the handle keeps the two-launch form (the same
    number of gemm-family launches as under the switch, same bits), and the chain still follows the oracle"""
    kw = dict(beta=1.0, n_walkers=40, seed=79)
    one = _handle(gpu, gpu.HubbardModelRepulsive(16, 2), None, **kw)
    two = _handle(gpu, gpu.HubbardModelRepulsive(16, 2), "DQMC_WRAP_TWO_LAUNCH", **kw)
    refs = {}
    for w in (0, 39):
        o = O.OracleDQMC(16, "repulsive", beta=1.0, delta_tau=one.p.delta_tau, safe_mult=one.p.safe_mult, U=one.model.U)
        o.set_conf(one.conf(w))
        o.seed(one.seeds[w])
        o.prepare()
        o.update_until_measure()
        refs[w] = o
    for mc in (one, two):
        mc.prepare()
        mc.update_until_measure()
    for w, o in refs.items():
        assert np.array_equal(one.conf(w), o.conf()), "HS field of walker %d differs from the oracle" % w
        for g, g0 in zip(one.greens_eff(w), o.greens_eff()):
            assert relerr(g, g0) < 1e-10
        a, st = one.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
    n1, n2 = _gemm_launches_of_a_sweep(one), _gemm_launches_of_a_sweep(two)
    assert n1 == n2, (n1, n2)
    _same_chain(one, two, 40)
    _same_bits(one, two, 40, "80 units")
    _clean(one, two)
