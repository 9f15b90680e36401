"""Hubbard models on HoneycombLattice(L) on the device, through the ABI: stepwise parity with the oracle (given the
honeycomb hopping matrix), the U = 0 known answers, and the measurement sums over the 3 L^2 directions of a lattice with a
basis - through the injective form of the Green's rows (tdm_greens_inj_kernel), the pair lists (DQMC_TDM_GENERAL=1) and
the numpy references of tests/measurement_ref.py / time_displaced_ref.py, with the tolerance of
test_gpu_measurement_sizes.py: |device - reference| <= 2 (P + 16) eps abs_sum per element.  L = 3: n = 18, 27 directions,
one partly idle wave; L = 6: n = 72 (past one 64-tile), 108 directions (two direction groups, past one momentum tile).
Every case asserts the form the plan getters report: a silent fallback would make the comparisons vacuous."""
import os
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import honeycomb_ref as HR  # noqa: E402
import ising_checkerboard_ref as icb  # noqa: E402
import lattice_tables as LT  # noqa: E402
import measurement_ref as MR  # noqa: E402
import test_gpu_measurement_sizes as MS  # noqa: E402
import test_gpu_time_displaced as TD  # noqa: E402
import time_displaced_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
KINDS = ["attractive", "repulsive"]

_pairs = {}


def pairs(L):
    if L not in _pairs:
        _pairs[L] = HR.fast_pairs(L)
    return _pairs[L]


def _model(gpu, kind, L, **kw):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    return cls(l=gpu.HoneycombLattice(L), **kw)


# ---- the sweep: oracle parity
def _oracles(O, mc, kind, exps=None):
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(mc.model.l.L, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=mc.model.hopping_matrix()[0], exps=exps)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


def _stepwise(mc, refs, nupd):
    def compare(conf=True):
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                assert relerr(g, g0) < TOL, relerr(g, g0)
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", [2, 3, 6])
def test_stepwise_updates_match_oracle(gpu, O, kind, L):
    """prepare, then propagate / sweep_spatial one call at a time through the first up chain, its wrap and into the way
    down (beta = 1, safe_mult = 5, 10 slices), mu != 0: n = 8, 18 and 72"""
    mc = gpu.DQMC(_model(gpu, kind, L, U=2.0, mu=-0.2), beta=1.0, safe_mult=5, n_walkers=2 if L < 6 else 1, seed=31)
    assert not mc.kron_hopping()
    _stepwise(mc, _oracles(O, mc, kind), mc.p.slices + 3)
    mc.close()


def test_stepwise_updates_with_the_checkerboard(gpu, O):
    """checkerboard=True on L = 3: the three bond groups multiplied out, against the oracle given the same products"""
    model = _model(gpu, "attractive", 3)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=2, seed=13, checkerboard=True)
    assert gpu.build_checkerboard(model.l)[2] == 3
    exps = gpu.checkerboard_exponentials(model.hopping_matrix()[0], model.l, mc.p.delta_tau)
    _stepwise(mc, _oracles(O, mc, "attractive", exps=exps), mc.p.slices + 3)
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", [3, 6])
def test_free_fermions_known_answers(gpu, kind, L):
    """U = 0, mu != 0: G = (1 + e^{-beta T})^-1 from numpy eigh whatever the field, and nk of momentum_time_displaced(),
    the occupation of both bands (2 - Re tr G(k): the sublattice trace from the same-sublattice directions), is the sum
    of the two bands' Fermi functions; |G_AB(k)| from the A -> B directions is |f_- - f_+| / 2"""
    mu, beta, t = -0.4, 2.0, 1.0
    model = _model(gpu, kind, L, U=0.0, mu=mu, t=t)
    mc = gpu.DQMC(model, beta=beta, safe_mult=5, n_walkers=2, seed=3)
    mc.set_pair_directions(pairs(L))
    mc.set_momenta("all")
    mc.set_time_displaced(5, ("greens",))
    assert mc.time_displaced_plan()["fast"] == 2
    G0 = HR.free_greens(model.hopping_matrix()[0], beta)
    mc.prepare()
    for _ in range(2):
        for wk in range(2):
            for g in mc.greens(wk):
                assert relerr(g, G0) < TOL, relerr(g, G0)
        mc.update_until_measure()
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=5)
    q = mc.momenta()
    assert q.shape == (L * L, 2)
    e = HR.band_energies(q, t)
    fermi = lambda x: 1.0 / (np.exp(beta * x) + 1.0)
    res = mc.momentum_time_displaced()
    nk = res["nk"]
    assert nk.shape == (mc.nb, L * L)
    for b in range(mc.nb):
        err = np.abs(nk[b] - (fermi(-mu - e) + fermi(-mu + e))).max()
        assert err < TOL, err
        ab = np.abs(res["Gk_l0_AB"][b, 0])
        assert np.abs(ab - 0.5 * np.abs(fermi(-mu - e) - fermi(-mu + e))).max() < TOL
    assert np.ptp(fermi(-mu - e) + fermi(-mu + e)) > 0.1  # (the occupation varies over the zone)
    mc.close()


# ---- the measurement sums: the new form, the general form and numpy
def _set_tables(mc, L):
    fp = pairs(L)
    loc, cc = HR.quads(fp, 7), HR.quads(fp, 7, synced=True)
    mc.set_local_targets(loc)
    mc.set_current_targets(cc)
    return fp, loc, cc


def _measure(gpu, mc, L, rep, tag, G, ref_sus, ref_td):
    """one pass of every section on a handle in the state of G; -> (correlations, pairing, susceptibilities, rows)"""
    fp, loc, cc = pairs(L), HR.quads(pairs(L), 7), HR.quads(pairs(L), 7, synced=True)
    n, nd, dir_of, W, K, nb = 2 * L * L, fp.ndirections(), fp.dir_of, mc.n_walkers, 7, mc.nb
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    assert set(pair_count) == {n, n // 2}
    M = mc.p.slices
    mc.reset_accumulators()
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    raw = mc.correlations_raw()
    assert raw[-1] == W
    ref = MS.sum_walkers([MR.equal_time(g, dir_of, nd) for g in G])
    corr = {k: raw[i * nd:(i + 1) * nd] for i, k in enumerate(("CDC", "SDCx", "SDCy", "SDCz"))}
    for k in corr:
        rep.check(tag + k, corr[k], ref[k][0], ref[k][1], pair_count * W)
    raw = MS.raw_sums(mc, gpu.lib().dqmc_pairing_size, gpu.lib().dqmc_get_pairing)
    assert raw[-1] == W
    val, ab = (sum(x) for x in zip(*[MR.pairing(g, dir_of, nd, loc.trg_of) for g in G]))
    pc = raw[:-1].reshape((nd, K, K), order="F")
    rep.check(tag + "PC", pc, val, ab, MS.quad_terms(dir_of, nd, loc.trg_of, False) * W)
    bodies = TD.record(mc, 1, 3, samples=1)
    assert mc.time_displaced_plan()["rows"] == M + 1
    TD.check_rows(rep, tag, mc, bodies, ref_td, pair_count, 3, 1)
    sus, cnt = MS.raw_susceptibilities(gpu, mc, nd, K, K)
    assert cnt == W
    terms = {k: pair_count * M * W for k in ("CDS", "SDSx", "SDSy", "SDSz")}
    terms["PS"] = MS.quad_terms(dir_of, nd, loc.trg_of, False) * M * W
    terms["CCS"] = MS.quad_terms(dir_of, nd, cc.trg_of, True) * M * W
    for k in terms:
        rep.check(tag + k, sus[k], ref_sus[k][0], ref_sus[k][1], terms[k])
    return corr, pc, sus, TR.split(bodies[0], nb, M + 1, nd, 3), terms, pair_count


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,W", [(3, 4), (6, 2)])
def test_measurement_sums_in_both_forms(gpu, kind, L, W):
    """equal-time correlations, pairing, susceptibilities with pairing and current-current at K = 7, and the rows of
    GREENS | DENSITY at every = 1 (10 slices): the handle with the injective form and a handle under DQMC_TDM_GENERAL=1
    in the same state, each against numpy, and against each other under the same bound"""
    l = gpu.HoneycombLattice(L)
    n, nd, dir_of = l.sites, pairs(L).ndirections(), pairs(L).dir_of
    assert nd == 3 * L * L and HR.greens_rows_form(dir_of, nd) == 2
    rep = MS.Report("honeycomb L=%d[%s]" % (L, kind))
    mc = TD.handle(gpu, l, kind, W, beta=1.0)
    assert mc.p.slices == 10
    fp, loc, cc = _set_tables(mc, L)
    assert LT.cc_plan(n, 7, W, cc.trg_of, dir_of, nd) is None  # n_dirs != n: the current-current sums keep cc_pairs_kernel
    assert not mc.current_targets_fast_path() and not any(mc.current_targets_plan().values())
    G, steps = TD.device_inputs(gpu, mc)
    T = mc.model.hopping_matrix()
    ref_sus = MS.sum_walkers([MR.susceptibilities(T, G[w], steps[w], dir_of, nd, MS.DELTA_TAU, trg_loc=loc.trg_of,
                                                  trg_cc=cc.trg_of) for w in range(W)])
    ref_td = TD.reference(G, steps, dir_of, nd, 1, 3)
    new = _measure(gpu, mc, L, rep, "inj ", G, ref_sus, ref_td)
    assert mc.time_displaced_plan() == dict(rows=11, every=1, what=3, fast=2)
    mc.close()
    mc = TD.handle(gpu, l, kind, W, beta=1.0, general=True)
    assert all(np.array_equal(a, b) for w in range(W) for a, b in zip(G[w], mc.greens(w)))
    _set_tables(mc, L)
    gen = _measure(gpu, mc, L, rep, "general ", G, ref_sus, ref_td)
    assert mc.time_displaced_plan() == dict(rows=11, every=1, what=3, fast=0)
    mc.close()
    terms, pair_count = new[4], new[5]
    for k in ("Gl0", "G0l"):  # the rows the two kernels write: equal within the summation order
        rep.check("inj vs general " + k, new[3][k], gen[3][k], ref_td[k][1], pair_count * W)
    # every other section takes the same kernels on both handles: the same bits
    for k in ("CDC", "SDCx", "SDCy", "SDCz"):
        assert np.array_equal(new[0][k], gen[0][k]) and np.array_equal(new[3][k], gen[3][k]), k
    assert np.array_equal(new[1], gen[1])
    for k in terms:
        assert np.array_equal(new[2][k], gen[2][k]), k
    print("%s worst err/bound: %s" % (rep.case, ", ".join("%s %.2g" % kv for kv in sorted(rep.worst.items()))))


def test_bravais_lattices_keep_their_forms(gpu):
    """SquareLattice(6): the Latin square form of the Green's rows and the LDS plan of the current-current kernel, as
    before"""
    l = gpu.SquareLattice(6)
    fp = LT.fast_pairs(l)
    mc = TD.handle(gpu, l, "attractive", 2)
    cc = LT.fast_quads(l, 5, pairs=fp, synced=True)
    mc.set_current_targets(cc)
    mc.set_time_displaced(1, 3)
    assert HR.greens_rows_form(fp.dir_of, fp.ndirections()) == 1
    assert mc.time_displaced_plan() == dict(rows=mc.p.slices + 1, every=1, what=3, fast=1)
    want = LT.cc_plan(36, 5, 2, cc.trg_of, fp.dir_of, 36)
    got = mc.current_targets_plan()
    assert mc.current_targets_fast_path() and got["fast"] == 1 and all(got[k] == want[k] for k in want)
    assert LT.plan_tuple(want) == (16, 3, 1, 3, 64)
    mc.close()


def test_staggered_structure_factor_and_channels(gpu):
    """S_AF of staggered_structure_factors() = the signed sum over all pairs of the numpy Wick terms / n; the same number
    through the phase tables of set_staggered_momentum(); the default pair channels; strips for the entanglement cut"""
    L, W = 3, 2
    l = gpu.HoneycombLattice(L)
    n = l.sites
    mc = TD.handle(gpu, l, "repulsive", W, beta=1.0)
    it = gpu.EachSitePairByDistance(l)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(l, pairs=it))
    mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(l, pairs=it))
    assert mc.response_plan()["K"] == 7 and mc.response_plan()["K_cc"] == 7
    mc.set_pair_channels("default")
    assert list(mc.pair_channels()) == ["s", "s*"]
    assert np.array_equal(mc.sublattice_signs(), gpu.sublattice_sign(it, l))
    mc.reset_accumulators()
    G = [mc.greens(w) for w in range(W)]
    mc.accumulate_greens()
    mc.accumulate_correlations()
    mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    saf = mc.staggered_structure_factors()
    pair = np.arange(n * n).reshape(n, n)  # every pair its own "direction": the Wick terms pair by pair
    for name, key in (("Sc", "CDC"), ("Sx", "SDCx"), ("Sz", "SDCz")):
        ref = sum(HR.signed_pair_sum(MR.equal_time(g, pair, n * n)[key][0].reshape(n, n), l.sublattice) for g in G) / W
        assert abs(saf[name] - ref) <= TOL * abs(ref), (name, saf[name], ref)
    assert saf["count"] == W and saf["Sz"] > 0
    chi = mc.staggered_static_susceptibilities()
    sus = mc.susceptibilities()
    assert chi["chi_z"] == float(sus["SDSz"] @ mc.sublattice_signs()) and chi["count"] == W
    mc.set_momenta("all")
    cr = mc.current_response()
    assert cr["Lambda"].shape == (7, L * L) and cr["kbond"].shape == (7,) and np.all(np.isfinite(cr["Lambda"]))
    assert cr["kbond"][0] == 0 and np.all(cr["kbond"][1:] < 0)  # each of the six bond directions carries kinetic energy
    for fn in (mc.superfluid_stiffness, mc.drude_weight, mc.dc_conductivity):
        with pytest.raises(NotImplementedError, match="HoneycombLattice"):
            fn(0)
    mc.set_staggered_momentum()
    assert mc.momenta_plan()["n_q"] == 1
    sf = mc.structure_factors()
    assert all(abs(sf[k][0] - saf[k]) <= 1e-14 * abs(saf[k]) for k in ("Sc", "Sx", "Sy", "Sz"))
    mc.set_entanglement({"half": gpu.strip_subsystem(l, 1), "two": gpu.strip_subsystem(l, 2, axis=1)})
    mc.close()


def test_model_errors(gpu):
    l = gpu.HoneycombLattice(2)
    for cls in (gpu.HubbardModelAttractive, gpu.HubbardModelRepulsive):
        with pytest.raises(ValueError, match="tp"):
            cls(l=l, tp=-0.2)
        with pytest.raises(ValueError, match="t_perp"):
            cls(l=l, t_perp=0.5)


def test_checkpoint_round_trip(gpu, tmp_path):
    """save at a measurement point, load: the file names the lattice, the tables come back with the injective form, and
    the next sweep gives the same HS field as the uninterrupted handle"""
    kw = dict(beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=4242, thermalization=0, sweeps=0, measure_rate=1)
    a = gpu.DQMC(_model(gpu, "repulsive", 3, U=2.0, mu=-0.2), **kw)
    a.set_pair_directions(gpu.EachSitePairByDistance(a.model.l))
    a.set_time_displaced(2, ("greens",))
    a.prepare()
    a.update_until_measure()
    a.sweep(1)
    path = str(tmp_path / "honeycomb.ckpt")
    a.save(path)
    assert a._preamble(0, False)["lattice"] == {"class": "HoneycombLattice", "args": [3]}
    a.sweep(1)
    b = gpu.DQMC.load(path)
    assert isinstance(b.model.l, gpu.HoneycombLattice) and (b.model.l.L, b.model.mu, b.model.U) == (3, -0.2, 2.0)
    assert all(np.array_equal(x, y) for x, y in zip(a.model.hopping_matrix(), b.model.hopping_matrix()))
    assert b.time_displaced_plan() == a.time_displaced_plan() and b.time_displaced_plan()["fast"] == 2
    assert b._dirs is not None and b._ndirs == 27
    b.sweep(1)
    for w in range(2):
        assert np.array_equal(a.conf(w), b.conf(w))
        assert a.uniforms_used(w) == b.uniforms_used(w)
        for ga, gb in zip(a.greens(w), b.greens(w)):
            assert relerr(gb, ga) < TOL
    for mc in (a, b):
        mc.close()


# ---- the classical flavor takes any neighbour table with z <= 8
@pytest.mark.parametrize("update", ["sequential", "checkerboard"])
def test_ising_on_the_honeycomb(gpu, update):
    """IsingModel(l=HoneycombLattice(4)), z = 3, two colours: 41 sweeps of 8 walkers, bit for bit against the host
    restatement (tests/ising_checkerboard_ref.py)"""
    l = gpu.HoneycombLattice(4)
    col = gpu.greedy_colouring(l)
    assert int(col.max()) + 1 == 2 and np.array_equal(col, l.sublattice) and icb.is_valid(l, col)
    W, seed, therm, cap = 8, 900, 2, 50
    betas = np.linspace(0.3, 0.9, W)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=W, seed=seed, thermalization=therm, measure_rate=1,
                series_capacity=cap, update=update)
    for k in (13, 1, 27):
        mc.sweep(k)
    lad = icb.Ladders(l, betas, [seed + w for w in range(W)], series_capacity=cap, update=update)
    lad.run(1, 41, therm, 1)
    for w in range(W):
        want, st = lad.stats(w), mc.stats(w)
        assert {k: getattr(st, k) for k in want} == want, (update, w)
        assert np.array_equal(mc.conf(w), lad.c[w]), (update, w)
        e, m = mc.series(w)
        assert list(e) == lad.serE[w] and list(m) == lad.serM[w], (update, w)
    assert sum(mc.stats(w).acc_local for w in range(W)) > 0
    mc.close()
