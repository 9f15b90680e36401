"""Engine runs at the unit counts where the launch forms switch (a unit is one walker x one block).  At n = 256 the engine
picks its kernels by the number of units as well as by n: the one-launch UDT, the cooperative QR, the fused chunk loop of the
site sweep and the one-launch factored wrap each need their whole grid co-resident, and every block map pads the units to
whole groups of eight.  dqmc_launch_plan reports what a handle decided; tests/launch_rules.py restates the rules from the
capacities the plan reports, and every case asserts that the two agree before it runs.

Each case: SquareLattice(16) (n = 256, factored hopping), beta = 1, delta_tau = 0.1 (10 slices), safe_mult 10, U = 1.
prepare, then 2 x slices + 3 x (propagate, sweep_spatial), then one whole sweep (its wraps take the pending chunk), with
  * every walker compared after every call with the same walkers run as handles of at most 8 walkers (same seeds): HS field
    and counters identical, G within 1e-10, bit for bit where both handles run the same forms;
  * walker 0, the first walker of the last group of eight units and the last walker compared with the oracle: HS field
    identical, G within 1e-10, counters exact;
  * a twin under DQMC_WRAP_TWO_LAUNCH: bit for bit, and the gemm-family launch count of a sweep tells the wrap forms apart;
  * stand-alone flushes per sweep_spatial: 1 = fused chunk loop, n / 64 = launch per chunk;
  * device_errors() == 0 and qr_fallbacks() == 0.
(The launch counts do not tell the cooperative QR from the tile QR: both are one timed step per factorisation.  That
choice is covered by the plan, whose admission expression is the launcher's own, and by test_gpu_linalg.py.)

Occupancies the runtime reported on the MI355X (256 CUs) when this file was written: one workgroup per CU for the one-launch
UDT (256 workgroups: up to 32 units), two for the cooperative QR (512: up to 64 units), three for the one-launch wrap
without a pending chunk (768: up to 48 units) and two with one (512: up to 32 units).  The forms they give:
  walkers, model   units  UDT          site sweep         wrap without / with a pending chunk
  9 attractive     9      one launch   fused (9 + 64)     one launch / one launch     partial second group
  33 attractive    33     cooperative  fused (33 + 160)   one launch / two launches   first count past the one-launch UDT
  48 attractive    48     cooperative  fused (48 + 192)   one launch / two launches   last count with the fused sweep
  49 attractive    49     cooperative  split (49 + 224)   two launches                first count with the split sweep
  32 repulsive     64     cooperative  split (32 + 256)   two launches                cooperative QR at its maximum, 512
  65 attractive    65     tile + tail  split              two launches                partial ninth group
  17 repulsive     34     cooperative  fused (17 + 160)   one launch / two launches   two blocks per walker, partial group
Every count from 33 to 48 units gives a handle that mixes the wrap forms (three of the cases above); test_mixed_wrap_forms
runs the largest such count if the table no longer holds one.
test_every_regime_is_reached asserts that the cases still reach every regime of REGIMES, so a runtime that changes its
occupancy answers makes the suite say so instead of testing less."""
import os

import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

import launch_rules as R
from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL_DENSE = 1e-10  # test_gpu_kron.test_factored_sweeps_match_dense
SHARD = 8

REGIMES = {"one-launch UDT with a partial later group", "cooperative QR with fused sweep", "cooperative QR with split sweep",
           "cooperative QR at its admitted maximum", "tile QR", "one-launch wrap", "two-launch wrap"}

# (kind, walkers) on SquareLattice(16)
CASES_256 = [("attractive", 9), ("attractive", 33), ("attractive", 48), ("attractive", 49), ("repulsive", 32),
             ("attractive", 65), ("repulsive", 17)]
_plans = {}  # (kind, walkers) -> plan of the n = 256 cases that ran


@pytest.fixture(scope="module")
def caps(gpu):
    c = R.capacities(gpu)
    print("capacities: %s (per CU: one-launch UDT %d, cooperative QR %d, wrap %d / %d)"
          % (c, c["udt_blocks"] // c["cus"], c["qr_coop_blocks"] // c["cus"], c["wrap_blocks"][0] // c["cus"],
             c["wrap_blocks"][1] // c["cus"]))
    return c


def _model(gpu, kind, lattice):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    return cls(l=lattice)


def _handle(gpu, kind, lattice, walkers, first=0, env=(), seed=41):
    for k in env:
        os.environ[k] = "1"  # kernel switches are read when a handle is created
    try:
        mc = gpu.DQMC(_model(gpu, kind, lattice), beta=1.0, delta_tau=0.1, n_walkers=walkers, seed=seed, first_walker=first)
    finally:
        for k in env:
            os.environ.pop(k, None)
    assert mc.p.slices == 10 and mc.p.safe_mult == 10 and mc.model.U == 1.0
    return mc


def _shards(gpu, kind, lattice, walkers, env=()):
    return [_handle(gpu, kind, lattice, min(SHARD, walkers - lo), first=lo, env=env) for lo in range(0, walkers, SHARD)]


def _oracle_walkers(walkers, nb):
    units = walkers * nb
    return sorted({0, 8 * ((units - 1) // 8) // nb, walkers - 1})


def _oracles(O, mc, kind, ws):
    T = mc.model.hopping_matrix()[0]
    refs = {}
    for w in ws:
        o = O.OracleDQMC(mc.model.l.sites, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=mc.model.U, hopping=T)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs[w] = o
    return refs


class _Worst:
    oracle = 0.0
    shard = 0.0
    twin = 0.0


def _same_chain(a, wa, b, wb, what):
    assert np.array_equal(a.conf(wa), b.conf(wb)), "%s: HS field of walker %d differs" % (what, wa)
    sa, sb = a.analysis(wa), b.analysis(wb)
    assert (sa.prop_local, sa.acc_local) == (sb.prop_local, sb.acc_local), (what, wa)
    assert a.uniforms_used(wa) == b.uniforms_used(wb), (what, wa)


def _compare_shards(big, shards, bits, worst, what):
    for s, sh in enumerate(shards):
        for v in range(sh.n_walkers):
            w = s * SHARD + v
            _same_chain(big, w, sh, v, what)
            for g, g0 in zip(big.greens_eff(w), sh.greens_eff(v)):
                if np.array_equal(g, g0):
                    continue
                e = relerr(g, g0)
                worst.shard = max(worst.shard, e)
                assert not bits[s], "%s: walker %d differs from its shard (same forms), rel %.3g" % (what, w, e)
                assert e < TOL, (what, w, e)


def _compare_oracles(big, refs, worst, what):
    for w, o in refs.items():
        assert np.array_equal(big.conf(w), o.conf()), "%s: HS field of walker %d differs from the oracle" % (what, w)
        a, st = big.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local), (what, w)
        assert big.uniforms_used(w) == o.uniforms_used(), (what, w)
        for g, g0 in zip(big.greens_eff(w), o.greens_eff()):
            e = relerr(g, g0)
            worst.oracle = max(worst.oracle, e)
            assert e < TOL, (what, w, e)


def _compare_twin(big, twin, worst, what):
    for w in range(big.n_walkers):
        _same_chain(big, w, twin, w, what)
        for g, g0 in zip(big.greens_eff(w), twin.greens_eff(w)):
            if not np.array_equal(g, g0):
                worst.twin = max(worst.twin, relerr(g, g0))
    assert worst.twin == 0.0, "%s: differs from the twin, rel %.3g" % (what, worst.twin)


def _timed(mc, call):
    mc.timing_enable(True)
    call()
    t = mc.timing()
    mc.timing_enable(False)
    return t


def _run_case(gpu, O, caps, kind, lattice, walkers, twin_env=None, steps=None):
    """the procedure of the module docstring; returns (plan, worst errors)"""
    n, nb = lattice.sites, 1 if kind == "attractive" else 2
    big = _handle(gpu, kind, lattice, walkers)
    factored = big.kron_hopping()
    assert factored == (n == 256)
    plan = big.launch_plan()
    assert plan == R.expected_plan(n, walkers, nb, factored, caps), (plan, R.expected_plan(n, walkers, nb, factored, caps))
    assert big.udt_one_launch_sites() == plan["udt_sites"]
    shards = _shards(gpu, kind, lattice, walkers)
    bits = []
    for sh in shards:
        sp = sh.launch_plan()
        assert sp == R.expected_plan(n, sh.n_walkers, nb, factored, caps)
        bits.append(R.forms(sp, n) == R.forms(plan, n))
    twin = _handle(gpu, kind, lattice, walkers, env=(twin_env,)) if twin_env else None
    refs = _oracles(O, big, kind, _oracle_walkers(walkers, nb))
    worst = _Worst()
    everyone = [big] + shards + ([twin] if twin else [])

    def step(name, what):
        for mc in everyone:
            getattr(mc, name)()
        for o in refs.values():
            getattr(o, name)()
        assert (big.current_slice, big.direction) == (next(iter(refs.values())).current_slice, next(iter(refs.values())).direction)
        _compare_shards(big, shards, bits, worst, what)
        _compare_oracles(big, refs, worst, what)

    step("prepare", "prepare")
    nc = n // 64
    for i in range(2 * big.p.slices + 3 if steps is None else steps):
        step("propagate", "propagate %d" % i)
        if i == 0 and n >= 128:  # which sweep form ran: stand-alone flushes of one sweep_spatial
            for mc in shards + ([twin] if twin else []):
                mc.sweep_spatial()
            for o in refs.values():
                o.sweep_spatial()
            t = _timed(big, big.sweep_spatial)
            assert (t["sweep"][1], t["flush"][1]) == (nc, 1 if plan["sweep_fused"] else nc), (t, plan)
            _compare_shards(big, shards, bits, worst, "sweep_spatial 0")
            _compare_oracles(big, refs, worst, "sweep_spatial 0")
        else:
            step("sweep_spatial", "sweep_spatial %d" % i)
    if twin:
        _compare_twin(big, twin, worst, "step by step")
    # one whole sweep in one call: with the fused chunk loop its wraps take the sweep's pending last chunk
    t1 = _timed(big, lambda: big.sweep(1))
    for sh in shards:
        sh.sweep(1)
    for o in refs.values():
        o.sweeps(1)
    _compare_shards(big, shards, bits, worst, "sweep")
    _compare_oracles(big, refs, worst, "sweep")
    if twin:
        t2 = _timed(twin, lambda: twin.sweep(1))
        _compare_twin(big, twin, worst, "sweep")
        if twin_env == "DQMC_WRAP_TWO_LAUNCH":
            # Every one-launch wrap is one launch of the gemm family less than in the twin.  With one stack segment
            # (slices = safe_mult) a sweep calls wrap_greens 2 M - 1 times: M - 1 plain wraps on the way up, the wrap behind
            # the recomputation at the top and M - 1 plain wraps on the way down (the wrap of greens_temp at the top of the
            # way up is part of the slice chain's launch).  With the fused chunk loop each has the sweep's last chunk
            # pending, except the one behind the recomputation (the chunk is dropped there) and the first of this call
            # (a plain wrap on the way up; the API call before it applied its chunk)
            assert big.p.slices == big.p.safe_mult
            wraps = 2 * big.p.slices - 1
            without = wraps if not plan["sweep_fused"] else 2
            one0, one1 = plan["wrap_one_launch"]
            saved = t2["gemm"][1] - t1["gemm"][1]
            assert saved == one0 * without + one1 * (wraps - without), (t1["gemm"], t2["gemm"], plan)
    for mc in everyone:
        assert mc.device_errors() == 0
        assert mc.qr_fallbacks() == 0
        assert mc.kron_hopping() == factored
        mc.close()
    print("n = %d, %d %s walkers: plan %s; forms %s; worst rel |G - G_oracle| = %.3g, |G - G_shard| = %.3g (bitwise shards: "
          "%d of %d), |G - G_twin| = %.3g; fallbacks 0" % (n, walkers, kind, plan, R.forms(plan, n), worst.oracle, worst.shard,
                                                            sum(bits), len(bits), worst.twin))
    return plan, worst


@pytest.mark.parametrize("kind,walkers", CASES_256, ids=["%s-%d" % c for c in CASES_256])
def test_n256_unit_counts(gpu, O, caps, kind, walkers):
    plan, _ = _run_case(gpu, O, caps, kind, gpu.SquareLattice(16), walkers, twin_env="DQMC_WRAP_TWO_LAUNCH")
    _plans[(kind, walkers)] = plan


def test_mixed_wrap_forms(gpu, O, caps):
    """a handle whose wraps are one launch without a pending chunk and two with one (or the other way round), at the largest
    unit count that yields one on this device; where the two occupancies are equal there is no such count"""
    units = [u for u in R.mixed_wrap_units(caps) if R.sweep_fused(256, u, 1, caps)] or R.mixed_wrap_units(caps)
    print("unit counts with mixed wrap forms: %s" % (("%d..%d" % (units[0], units[-1])) if units else "none"))
    if not units:
        return
    walkers = units[-1]
    if ("attractive", walkers) in _plans:  # (already run as a case of the table)
        plan = _plans[("attractive", walkers)]
    else:
        plan, _ = _run_case(gpu, O, caps, "attractive", gpu.SquareLattice(16), walkers, twin_env="DQMC_WRAP_TWO_LAUNCH")
    assert plan["wrap_one_launch"][0] != plan["wrap_one_launch"][1]


def test_every_regime_is_reached(gpu, caps):
    """the plans of the table's cases, taken from handles (nothing is run), meet every condition of REGIMES; the handle with
    mixed wrap forms is test_mixed_wrap_forms' own"""
    reached = {}
    for kind, walkers in CASES_256:
        if (kind, walkers) not in _plans:
            mc = _handle(gpu, kind, gpu.SquareLattice(16), walkers)
            _plans[(kind, walkers)] = mc.launch_plan()
            mc.close()
        for r in R.regimes(_plans[(kind, walkers)], 256, True):
            reached.setdefault(r, []).append("%d %s" % (walkers, kind))
    for r in sorted(reached):
        print("%-45s %s" % (r, ", ".join(reached[r])))
    assert REGIMES <= set(reached), "not reached: %s" % sorted(REGIMES - set(reached))


@pytest.mark.parametrize("kind,walkers", [("attractive", 9), ("attractive", 33), ("repulsive", 32)],
                         ids=["attractive-9", "attractive-33", "repulsive-32"])
def test_n256_dense_forms_match_factored(gpu, caps, kind, walkers):
    """DQMC_NO_KRON: slab_chain_kernel and the dense wrap with partial later groups, against the factored handle of the same
    case: HS field and counters identical, G within the bound of test_gpu_kron.test_factored_sweeps_match_dense"""
    lat = gpu.SquareLattice(16)
    f, d = _handle(gpu, kind, lat, walkers), _handle(gpu, kind, lat, walkers, env=("DQMC_NO_KRON",))
    assert f.kron_hopping() and not d.kron_hopping()
    nb = 1 if kind == "attractive" else 2
    assert d.launch_plan() == R.expected_plan(256, walkers, nb, False, caps)
    worst = 0.0
    for mc in (f, d):
        mc.prepare()
    for i in range(2 * f.p.slices + 3):
        for name in ("propagate", "sweep_spatial"):
            for mc in (f, d):
                getattr(mc, name)()
            for w in range(walkers):
                _same_chain(f, w, d, w, "%s %d" % (name, i))
                for gf, gd in zip(f.greens_eff(w), d.greens_eff(w)):
                    worst = max(worst, relerr(gf, gd))
    for mc in (f, d):
        mc.sweep(1)
    for w in range(walkers):
        _same_chain(f, w, d, w, "sweep")
        af, ad = f.analysis(w), d.analysis(w)
        assert af.propagation_error.count == ad.propagation_error.count
        for gf, gd in zip(f.greens_eff(w), d.greens_eff(w)):
            worst = max(worst, relerr(gf, gd))
    print("%d %s walkers: max rel |G_kron - G_dense| = %.3g" % (walkers, kind, worst))
    assert worst < TOL_DENSE
    for mc in (f, d):
        assert mc.device_errors() == 0 and mc.qr_fallbacks() == 0
        mc.close()


def test_n64_past_the_cooperative_qr(gpu, O, caps):
    """SquareLattice(8), 72 attractive walkers: more units than the cooperative QR admits, so the engine factors with
    qr_pivot_kernel<1, 4>"""
    plan, _ = _run_case(gpu, O, caps, "attractive", gpu.SquareLattice(8), 72)
    assert R.forms(plan, 64)[0] == "single"


@pytest.mark.parametrize("walkers", [80, 81])
def test_n128_either_side_of_the_fused_rule(gpu, O, caps, walkers):
    """Chain(128): 80 walkers + 160 flush workgroups fit 256 CUs, 81 + 176 do not; the split form is checked against the fused
    one's counts inside _run_case (one stand-alone flush per sweep_spatial against n / 64)"""
    plan, _ = _run_case(gpu, O, caps, "attractive", gpu.Chain(128), walkers)
    if caps["cus"] == 256:
        assert plan["sweep_fused"] == (walkers == 80)
