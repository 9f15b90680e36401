"""Engine parity at the sizes where the size-selected kernel forms change, against the oracle (given the lattice's
hopping matrix), one propagate / sweep_spatial at a time through more than a full sweep (up and down chains, both wraps).

The forms each case reaches on a 256-CU MI355X, from the dispatch (dqmc_create's sweep_fused rule, launch_sweep_fused,
launch_sweep_flush_lu, launch_trsm_right_upper):
  n      lattice            sweep                                            engine TRSM
  192    Chain(192)         sweep_fused_kernel<NB, 4, 1>                     the n <= 256 MFMA solve
  257    Chain(257)         per chunk, last chunk 1 site, non-full flush     panels 256 + 1
  320    Chain(320)         sweep_fused_kernel<NB, 4, 1> above 256           panels 160 + 160
  324    SquareLattice(18)  per chunk, last chunk 4 sites, non-full flush    panels 256 + 68
  384    Chain(384)         sweep_fused_kernel<NB, 8, 1>                     panels 192 + 192
  1024   SquareLattice(32)  per chunk, flush in 16 column passes             panels 4 x 256
Every fused case asserts that the rule selects the fused launch and that the engine took it (one stand-alone flush per
sweep_spatial instead of one per chunk); the fused cases are also run against the split launches (DQMC_SWEEP_SPLIT), the
panelled TRSM cases against the substitution solve (DQMC_TRSM_SIMPLE)."""
import os

import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def sweep_fused_rule(n, walkers, nb, cus):
    """restatement of dqmc_create's choice of the fused chunk loop (elimination of chunk c beside the flush of chunk
    c - 1): n a multiple of 64, at least 128 sites, and the launch's grid (one workgroup per walker + the flush
    workgroups) no larger than the number of CUs"""
    if n % 64 != 0 or n < 128:
        return False
    ncp = 2 if n % 256 == 0 else 1
    nt = 8 if n % 128 == 0 else 4
    units = walkers * nb
    flush_blocks = ((units + 7) // 8) * 8 * (n // 64) * (n // (16 * nt * ncp))
    return walkers + flush_blocks <= cus


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lattice(gpu, n):
    if n in (324, 1024):
        L = int(round(n ** 0.5))
        assert L * L == n
        return gpu.SquareLattice(L)
    return gpu.Chain(n)


def _model(gpu, kind, n):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    return cls(l=_lattice(gpu, n))


def _dqmc(gpu, kind, n, walkers, env=None, seed=31):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # kernel switches are read when a handle is created
    try:
        mc = gpu.DQMC(_model(gpu, kind, n), beta=1.0, safe_mult=5, n_walkers=walkers, seed=seed)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert mc.N == n and mc.p.slices == 10 and not mc.kron_hopping()
    return mc


def _oracles(O, mc, kind):
    T = mc.model.hopping_matrix()[0]
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(mc.model.l.sites, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=T)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


def _stepwise(mc, refs, nupd):
    """prepare, then nupd x (propagate, sweep_spatial), compared after every call; returns the worst G error"""
    worst = [0.0]

    def compare(conf=True):
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                e = relerr(g, g0)
                worst[0] = max(worst[0], e)
                assert e < TOL, e
    mc.prepare()
    for o in refs:
        o.prepare()
    compare()
    for _ in range(nupd):
        mc.propagate()
        for o in refs:
            o.propagate()
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        compare(conf=False)
        mc.sweep_spatial()
        for o in refs:
            o.sweep_spatial()
        compare()
    for w, o in enumerate(refs):
        a, st = mc.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
        assert mc.uniforms_used(w) == o.uniforms_used()
    return worst[0]


def _calculate_greens_at(mc, refs, slices):
    worst = 0.0
    for k in slices:
        for w, o in enumerate(refs):
            for g, g0 in zip(mc.calculate_greens(k, w), o.calculate_greens_at(k)):
                e = relerr(g, g0)
                worst = max(worst, e)
                assert e < TOL, (k, w, e)
    return worst


# (n, kind, walkers, fused): the table of the module docstring
CASES = [
    pytest.param(192, "attractive", 2, True, id="n192-attractive-fused_1_4_1-mfma_trsm"),
    pytest.param(192, "repulsive", 2, True, id="n192-repulsive-fused_2_4_1-mfma_trsm"),
    pytest.param(257, "attractive", 1, False, id="n257-attractive-chunked_last1-panels_256_1"),
    pytest.param(257, "repulsive", 1, False, id="n257-repulsive-chunked_last1-panels_256_1"),
    pytest.param(320, "attractive", 2, True, id="n320-attractive-fused_1_4_1-panels_160_160"),
    pytest.param(320, "repulsive", 2, True, id="n320-repulsive-fused_2_4_1-panels_160_160"),
    pytest.param(324, "attractive", 2, False, id="n324-attractive-chunked_last4-panels_256_68"),
    pytest.param(324, "repulsive", 2, False, id="n324-repulsive-chunked_last4-panels_256_68"),
    pytest.param(384, "attractive", 2, True, id="n384-attractive-fused_1_8_1-panels_192_192"),
    pytest.param(384, "repulsive", 2, True, id="n384-repulsive-fused_2_8_1-panels_192_192"),
]


@pytest.mark.parametrize("n,kind,walkers,fused", CASES)
def test_stepwise_updates_match_oracle(gpu, O, n, kind, walkers, fused):
    """beta = 1, safe_mult = 5: prepare + 2 x slices + 3 updates, HS field bit for bit, G within 1e-10, counters exact"""
    nb = 1 if kind == "attractive" else 2
    assert sweep_fused_rule(n, walkers, nb, _cus()) == fused
    mc = _dqmc(gpu, kind, n, walkers)
    refs = _oracles(O, mc, kind)
    worst = _stepwise(mc, refs, 2 * mc.p.slices + 3)
    if n == 324:
        worst = max(worst, _calculate_greens_at(mc, refs, (0, 1, 5, mc.p.slices)))
    print("n = %d %s, %d walkers: worst rel |G - G_oracle| = %.3g" % (n, kind, walkers, worst))
    mc.close()


def test_n1024_matches_oracle(gpu, O):
    """n = 1024 (SquareLattice(32), the declared ceiling): per-chunk sweep with the separate flush in its multi-pass
    form (16 column passes), engine TRSM in 4 panels of 256, the panel QR on its largest matrix.  prepare + safe_mult + 1
    updates and calculate_greens at slices 0, 5 and slices; the oracle's dense products go through OpenBLAS."""
    assert not sweep_fused_rule(1024, 1, 1, _cus())
    blas = O.use_openblas_dgemm(True)
    try:
        mc = _dqmc(gpu, "attractive", 1024, 1)
        refs = _oracles(O, mc, "attractive")
        worst = _stepwise(mc, refs, mc.p.safe_mult + 1)
        worst = max(worst, _calculate_greens_at(mc, refs, (0, 5, mc.p.slices)))
        print("n = 1024 attractive, 1 walker: worst rel |G - G_oracle| = %.3g (OpenBLAS oracle: %s)" % (worst, blas))
        mc.close()
    finally:
        O.use_openblas_dgemm(False)


def _launches(mc):
    """stand-alone sweep and flush launches of one sweep_spatial call"""
    mc.timing_enable(True)
    mc.sweep_spatial()
    t = mc.timing()
    mc.timing_enable(False)
    return t["sweep"][1], t["flush"][1]


def _against_plain_form(gpu, n, kind, walkers, env, check_launches=False):
    """the default handle against one created with `env` set, same seeds: prepare, then propagate / sweep_spatial
    through 2 x slices + 3 updates; HS field identical, G within 1e-10, counters equal"""
    mcs = [_dqmc(gpu, kind, n, walkers), _dqmc(gpu, kind, n, walkers, env)]
    for mc in mcs:
        mc.prepare()
    worst = 0.0
    for step in range(2 * mcs[0].p.slices + 3):
        for mc in mcs:
            mc.propagate()
        if step == 0 and check_launches:
            nc = n // 64
            assert _launches(mcs[0]) == (nc, 1)   # fused: elimination beside the previous flush, one last flush
            assert _launches(mcs[1]) == (nc, nc)  # split: a flush after every chunk
        else:
            for mc in mcs:
                mc.sweep_spatial()
        for w in range(walkers):
            assert np.array_equal(mcs[0].conf(w), mcs[1].conf(w)), (step, w)
            for a, b in zip(mcs[0].greens_eff(w), mcs[1].greens_eff(w)):
                e = relerr(a, b)
                worst = max(worst, e)
                assert e < TOL, (step, w, e)
    for w in range(walkers):
        a, b = mcs[0].analysis(w), mcs[1].analysis(w)
        assert (a.prop_local, a.acc_local) == (b.prop_local, b.acc_local)
        assert mcs[0].uniforms_used(w) == mcs[1].uniforms_used(w)
    for mc in mcs:
        mc.close()
    return worst


@pytest.mark.parametrize("n", [192, 320, 384])
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_fused_sweep_against_split_launches(gpu, n, kind):
    assert sweep_fused_rule(n, 2, 1 if kind == "attractive" else 2, _cus())
    worst = _against_plain_form(gpu, n, kind, 2, {"DQMC_SWEEP_SPLIT": "1"}, check_launches=True)
    print("n = %d %s: worst rel |G_fused - G_split| = %.3g" % (n, kind, worst))


@pytest.mark.parametrize("n", [257, 324])
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_panel_trsm_against_substitution(gpu, n, kind):
    """the engine's panelled MFMA solve (a trailing panel of 1 or 68 columns) against the substitution solve"""
    worst = _against_plain_form(gpu, n, kind, 1, {"DQMC_TRSM_SIMPLE": "1"})
    print("n = %d %s: worst rel |G_panel - G_substitution| = %.3g" % (n, kind, worst))
