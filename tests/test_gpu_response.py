"""Pair structure factors, current response and superfluid stiffness on the device (include/dqmc_hip.h "pair structure
factors and superfluid stiffness"; csrc/response.hip, response.inl): the samples against numpy, free fermions against the
closed form, reproducibility, "off is off", the state rules, sign weighting and the version 5 - 8 checkpoint.

Shapes, the smallest at which the kernels can go wrong (2 - 3 walkers, beta = 2, delta_tau = 0.1): 4 x 4 (16 directions,
25 rows of the pairing sample, below one tile), 6 x 6 (36 directions: the k-tail inside the second 32-tile), 9 x 9 (81
directions: three k-tiles with a tail, and with qs = "all" n_q past 64), TriangularLattice(4) (K = 7, 49 rows),
CubicLattice(3, 4) (64 directions exactly); n_q = 5 (no multiple of 16) and n_ch = 1, 3 and 8.

Bounds.  The transform (derived): an element is one sum of n_terms products, so |device - reference| <= n_terms 2^-52
sum |terms| whatever the order and with or without FMA: with u = 2^-53 the sum costs at most (n_terms - 1) u and the
products n_terms u (none with FMA), the delta_tau scale of the tau-integrated samples one u on the device's sum and one
on each term of the reference (the source binner holds delta_tau x, rounded), together below 2 n_terms u + u, and the
second-order terms are far below the one u that n_terms >= 16 leaves.  The reference is the same sum in longdouble from
level 0 of the source's own binner after one push, i.e. from exactly the sample the device transformed.  kbond adds the agreement of the
G the kernel read with the G the host reads back, TOL of test_gpu_dqmc.py per element.  Free fermions: the CPU oracle's
G(tau) chain (oracle.py with unequal_time_oracle.py, 4 x 4, beta = 2, delta_tau = 0.1, safe_mult = 5, U = 0) deviates
from the closed form by at most 2.31e-14 (attractive) and 1.43e-14 (repulsive, mu = 0.3) in any element, measured on the
CPU; the device is allowed ten times the larger, EPS_G = 2.31e-13 per element of G, and an observable that is a sum of
products of two G with absolute weights summing to C is allowed 2 C Gmax EPS_G (kbond, linear in G: C EPS_G)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import response_ref as R  # noqa: E402
from test_gpu_dqmc import TOL  # noqa: E402  (the device-against-oracle bound on G, 1e-10)

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
EPS_G = 10 * 2.31e-14
RESP = ("response_pairing", "response_pairing_susceptibility", "response_current")


def lattice(gpu, name):
    return {"sq4": lambda: gpu.SquareLattice(4), "sq6": lambda: gpu.SquareLattice(6), "sq9": lambda: gpu.SquareLattice(9),
            "tri4": lambda: gpu.TriangularLattice(4), "cub34": lambda: gpu.CubicLattice(3, 4)}[name]()


def channels(K, n_ch):
    """n_ch reproducible weight vectors over K directions (None: the default ones)"""
    if n_ch is None:
        return "default"
    rng = np.random.Generator(np.random.Philox(key=K * 100 + n_ch))
    return {"c%d" % c: rng.uniform(-1, 1, K) for c in range(n_ch)}


def handle(gpu, lat, kind, W, n_q=5, n_ch=None, U=1.0, mu=0.0, seed=71, first_walker=0, momenta=True, chan=True, prepare=True, current=True, **kw):
    """a handle at its measurement point with local and current targets, momenta and pair channels set"""
    l = lattice(gpu, lat)
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(l=l, U=U, mu=mu), beta=2.0, delta_tau=0.1, safe_mult=5, n_walkers=W, seed=seed, first_walker=first_walker, **kw)
    try:
        pairs = gpu.EachSitePairByDistance(l)
        mc.set_local_targets(gpu.EachLocalQuadByDistance(l, pairs=pairs))
        if current:
            mc._set_current_targets(gpu.EachLocalQuadBySyncedDistance(l, pairs=pairs).trg_of, mc._K, None)
        if momenta:
            q = gpu.momentum_grid(l)[0]
            mc.set_momenta(q if n_q == "all" else q[1:1 + n_q])
        if chan:
            mc.set_pair_channels(channels(mc._K, n_ch))
        if prepare:
            mc.prepare()
            mc.update_until_measure()
    except BaseException:
        mc.close()
        raise
    return mc


def one_pass(mc, greens=False):
    if greens:
        mc.accumulate_greens()
    mc.accumulate_pairing()
    mc.accumulate_susceptibilities(recalculate=5)


def level0(mc, which, w):
    return mc.binner_level(which, w, 0)[0]


def F_of(mc):
    return np.stack([np.outer(f, f).reshape(-1, order="F") for f in mc.pair_channels().values()], axis=1)


def assert_samples(mc, label):
    """level 0 of the three response binners after one push against the transforms of level 0 of the real-space ones"""
    nd, K, Kcc, dtau = mc._ndirs, mc._K, mc._Kcc, mc.p.delta_tau
    Ct, St = mc._phase_tables()
    nq, F = Ct.shape[1], F_of(mc)
    signed = mc.sign_weighting()
    trg = mc._tables["current_targets"][0]
    T = [mc._cc_T[b * mc.N ** 2:(b + 1) * mc.N ** 2].reshape((mc.N, mc.N), order="F") for b in range(mc.nb)]
    sg = mc.sign() if signed else np.ones(mc.n_walkers)
    worst = 0.0
    for w in range(mc.n_walkers):
        sus = level0(mc, "susceptibilities", w)  # (already times delta_tau: the device scales the sum, this the terms)
        refs = {"response_pairing": R.pair_transform(level0(mc, "pairing", w), F, nd, Ct, St),
                "response_pairing_susceptibility": R.pair_transform(sus[4 * nd:4 * nd + nd * K * K], F, nd, Ct, St),
                "response_current": R.current_transform(sus[4 * nd + nd * K * K:4 * nd + nd * K * K + nd * Kcc], nd, Ct, St)}
        for which, (ref, ab, nt) in refs.items():
            dev = level0(mc, which, w)
            if signed:
                assert dev[-1] == sg[w]
                dev = dev[:-1]
            if which == "response_current":
                kb, kab, knt = R.bond_kinetic(mc.greens(w), T, trg)
                g = np.concatenate([np.abs(x).ravel() for x in mc.greens(w)]).max()
                kerr = np.abs(dev[2 * Kcc * nq:].astype(np.longdouble) - sg[w] * kb).astype(np.float64)
                kbound = knt * U52 * kab.astype(np.float64) + TOL * g * np.array(
                    [(2.0 if mc.nb == 1 else 1.0) * sum(np.abs(Tb[trg[trg[:, k] >= 0, k], np.nonzero(trg[:, k] >= 0)[0]]).sum() for Tb in T) / mc.N
                     for k in range(Kcc)]) + 1e-300
                assert np.all(kerr <= kbound), (label, "kbond", w, float((kerr / kbound).max()))
                assert np.abs(kb).max() > 1e-3
                dev = dev[:2 * Kcc * nq]
            assert dev.shape == ref.shape, (label, which, dev.shape, ref.shape)
            bound = nt * U52 * ab.astype(np.float64) + 1e-300
            err = np.abs(dev.astype(np.longdouble) - ref).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (label, which, w, float((err / bound).max()))
            assert np.abs(ref).max() > 1e-6  # (not vacuous)
    print("%s: largest err / bound %.3g" % (label, worst))


#        lattice  model        n_q   n_ch  W
CASES = [("sq4", "attractive", 5, None, 3),
         ("sq6", "repulsive", 5, 8, 2),
         ("sq9", "attractive", "all", 1, 2),
         ("tri4", "repulsive", 5, 3, 2),
         ("cub34", "attractive", 5, 8, 2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-q%s-c%s-w%d" % c)
def test_samples_against_numpy(gpu, case):
    lat, kind, n_q, n_ch, W = case
    mc = handle(gpu, lat, kind, W, n_q=n_q, n_ch=n_ch)
    try:
        nq, nc = mc.momenta().shape[0], len(mc.pair_channels())
        assert mc.response_plan() == dict(n_ch=nc, K=mc._K, K_cc=mc._Kcc, n_q=nq)
        mc.enable_binning(("pairing", "susceptibilities") + RESP, capacity=7)
        assert [mc.binner_size(k)[0] for k in RESP] == [2 * nc * nq, 2 * nc * nq, 2 * mc._Kcc * nq + mc._Kcc]
        one_pass(mc)
        assert all(mc.binner_size(k)[2] == 1 for k in RESP)
        assert_samples(mc, "%s %s" % (lat, kind))
        b = mc.binned("response_current")
        assert b["Lambda"].shape == (mc._Kcc, nq) and b["kbond"].shape == (mc._Kcc,) and b["Lambda_std_error_re"].shape == (mc._Kcc, nq)
        host = mc.current_response()
        assert np.allclose(b["Lambda"], host["Lambda"], rtol=1e-11, atol=1e-13)
        bp, hp = mc.binned("response_pairing"), mc.pair_structure_factors()
        for c in mc.pair_channels():
            assert np.allclose(bp[c], hp[c], rtol=1e-11, atol=1e-13) and bp[c + "_std_error_walkers_im"].shape == (nq,)
    finally:
        mc.close()


@pytest.mark.parametrize("kind,mu", [("attractive", 0.0), ("repulsive", 0.3)])
def test_free_fermions_against_the_closed_form(gpu, kind, mu):
    mc = handle(gpu, "sq4", kind, 3, n_q="all", U=0.0, mu=mu)
    try:
        from montecarlo_jl_amd import lattices as Lt
        l = mc.model.l
        ff, loc, cur = R.free_fermions(gpu, l, 2.0, 0.1, mu=mu)
        ch = Lt.default_pair_channels(l, ff.r, loc.K)
        rs, ms = ff.band_basis(ch)
        mc.enable_binning(RESP, capacity=3)
        one_pass(mc, greens=True)
        Gmax, nd, beta, t2 = 1.0, mc._ndirs, 2.0, 1.0
        P, chi, cr, st = mc.pair_structure_factors(), mc.pair_susceptibilities(), mc.current_response(), mc.superfluid_stiffness(0)
        for c, f in ch.items():
            C = nd * np.abs(f).sum() ** 2
            assert np.abs(P[c] - ms["P"][c]).max() <= 2 * C * Gmax * EPS_G, (c, np.abs(P[c] - ms["P"][c]).max())
            assert np.abs(chi[c] - ms["chi"][c]).max() <= 2 * C * beta * Gmax * EPS_G, (c, np.abs(chi[c] - ms["chi"][c]).max())
        C_cc = nd * 2 * 4 * t2 * beta  # 2 spin species, four products T T G G per quadruple, sum_l dtau = beta
        assert np.abs(cr["Lambda"] - ms["Lambda"]).max() <= 2 * C_cc * Gmax * EPS_G, np.abs(cr["Lambda"] - ms["Lambda"]).max()
        assert np.abs(cr["kbond"] - rs["kbond"]).max() <= 2 * max(1.0, abs(mu)) * EPS_G
        q, d = ff.q, ff.r[:cur.K]
        iL = next(i for i in range(len(q)) if np.allclose(q[i], [2 * np.pi / 4, 0]))
        iT = next(i for i in range(len(q)) if np.allclose(q[i], [0, 2 * np.pi / 4]))
        kp = next(k for k in range(cur.K) if np.allclose(d[k], [1, 0]))
        km = next(k for k in range(cur.K) if np.allclose(d[k], [-1, 0]))
        want = R.stiffness(rs["kbond"], ms["Lambda"], kp, km, iL, iT)
        for k, v in want.items():
            assert abs(st[k] - v) <= 4 * EPS_G + 2 * C_cc * Gmax * EPS_G, (k, st[k], v)
            assert st[k + "_std_error"] <= 4 * EPS_G + 2 * C_cc * Gmax * EPS_G  # every walker gives the same value
        assert -st["k_axis"] > 0 and abs(st["drude"]) < abs(st["k_axis"])
        for which in RESP:  # all walkers the same, to rounding
            x = np.stack([level0(mc, which, w) for w in range(3)])
            assert np.abs(x - x[0]).max() <= 2 * C_cc * Gmax * EPS_G
    finally:
        mc.close()


def test_two_passes_and_another_walker_count_give_the_same_bits(gpu):
    one = three = None
    try:
        three, one = handle(gpu, "sq6", "repulsive", 3, n_ch=3), handle(gpu, "sq6", "repulsive", 1, n_ch=3)
        first = {}
        for mc in (three, one):
            mc.enable_binning(RESP, capacity=3)
            one_pass(mc)
            first[mc] = {k: [level0(mc, k, w) for w in range(mc.n_walkers)] for k in RESP}
            mc.reset_accumulators()
            assert mc.binner_size(RESP[0])[2] == 0 and not level0(mc, RESP[2], 0).any()
            one_pass(mc)
            for k in RESP:
                for w in range(mc.n_walkers):
                    assert np.array_equal(level0(mc, k, w), first[mc][k][w]), "a second pass differs bitwise: " + k
        for k in RESP:
            assert np.array_equal(first[one][k][0], first[three][k][0]), "walker 0 depends on n_walkers: " + k
    finally:
        for m in (one, three):
            if m is not None:
                m.close()


def test_off_is_off(gpu):
    """channels and momenta set but no response binner on: the accumulators, the reduce_export buffer and the state blob
    are byte for byte those of a handle that never called set_pair_channels"""
    a = b = None
    try:
        a, b = handle(gpu, "sq4", "repulsive", 2, chan=False), handle(gpu, "sq4", "repulsive", 2, chan=True)
        assert a.response_plan()["n_ch"] == 0 and b.response_plan()["n_ch"] == 3
        for mc in (a, b):
            mc.enable_binning(("pairing", "susceptibilities"), capacity=7)
            for s in range(2):
                if s:
                    mc.update_until_measure()
                one_pass(mc, greens=True)
        for sec in ("greens", "pairing", "susceptibilities"):
            assert np.array_equal(a._section(sec), b._section(sec)), sec
        for m in (a, b):
            m.reduce()
        assert a.reduce_size() == b.reduce_size() and np.array_equal(a.reduce_export(), b.reduce_export())
        sa, sb = a.state(), b.state()
        assert sa.size == sb.size and np.array_equal(sa, sb) and int.from_bytes(bytes(sb[8:12]), "little") == 1
        b.enable_binning("response_pairing", capacity=3)
        assert int.from_bytes(bytes(b.state()[8:12]), "little") == 5 and b.state_size() > sa.size
        b.set_pair_channels(None)
        assert np.array_equal(b.state(), sa)
    finally:
        for m in (a, b):
            if m is not None:
                m.close()


def test_state_rules(gpu):
    from montecarlo_jl_amd import _lib
    lib = _lib.lib()
    size = lambda mc, k: lib.dqmc_binner_size(mc._h, _lib.BIN_RESPONSE[k], None, None, None)
    fresh = gpu.DQMC(gpu.HubbardModelAttractive(l=gpu.SquareLattice(4)), beta=2.0, delta_tau=0.1, safe_mult=5, n_walkers=1)
    try:  # channels need the local targets
        one = np.ones(25)
        assert lib.dqmc_set_pair_channels(fresh._h, 1, _lib.dptr(one)) == _lib.ERR_STATE
        assert b"dqmc_set_local_targets" in lib.dqmc_last_error(fresh._h)
    finally:
        fresh.close()
    bare = handle(gpu, "sq4", "attractive", 1, current=False)
    try:  # momenta and channels, but no current targets: the current binner has no source
        with pytest.raises(_lib.DQMCError) as e:
            bare.enable_binning("response_current", capacity=3)
        assert e.value.code == _lib.ERR_STATE and "dqmc_set_current_targets" in str(e.value)
        assert size(bare, "response_current") == _lib.ERR_STATE and bare.response_plan()["K_cc"] == 0
        bare.enable_binning(RESP[:2], capacity=3)  # the pairing ones need none
    finally:
        bare.close()
    cold = handle(gpu, "sq4", "attractive", 1, prepare=False)
    try:  # not prepared: the two binners fed by the susceptibility pass need dqmc_prepare, the equal-time one does not
        for k in RESP[1:]:
            with pytest.raises(_lib.DQMCError) as e:
                cold.enable_binning(k, capacity=3)
            assert e.value.code == _lib.ERR_STATE and "dqmc_prepare" in str(e.value), k
            assert size(cold, k) == _lib.ERR_STATE
        cold.enable_binning("response_pairing", capacity=3)
        assert size(cold, "response_pairing") == _lib.OK
    finally:
        cold.close()
    mc = handle(gpu, "sq4", "attractive", 1, momenta=False, chan=False)
    try:
        q = gpu.momentum_grid(mc.model.l)[0]
        for k in RESP:  # before set_momenta
            with pytest.raises(_lib.DQMCError) as e:
                mc.enable_binning(k, capacity=3)
            assert e.value.code == _lib.ERR_STATE and "dqmc_set_momenta" in str(e.value)
        mc.set_momenta(q[:3])
        for k in RESP[:2]:  # before set_pair_channels
            with pytest.raises(_lib.DQMCError) as e:
                mc.enable_binning(k, capacity=3)
            assert e.value.code == _lib.ERR_STATE and "dqmc_set_pair_channels" in str(e.value)
        mc.enable_binning("response_current", capacity=3)  # needs no channels
        mc.set_pair_channels("default")
        F = np.ones(25 * 9)
        for n_ch, ptr in ((9, _lib.dptr(F)), (-1, _lib.dptr(F)), (2, None)):  # DQMC_ERR_INVALID, and the setting is kept
            assert lib.dqmc_set_pair_channels(mc._h, n_ch, ptr) == _lib.ERR_INVALID
        assert mc.response_plan() == dict(n_ch=3, K=5, K_cc=5, n_q=3)
        # the capacity: refused before anything is accumulated
        mc.enable_binning(RESP[:2], capacity=1)
        one_pass(mc)
        before = (mc._section("pairing"), mc._section("susceptibilities"))
        for call in (mc.accumulate_pairing, lambda: mc.accumulate_susceptibilities(recalculate=5)):
            with pytest.raises(_lib.DQMCError) as e:
                call()
            assert e.value.code == _lib.ERR_STATE and "capacity" in str(e.value)
        assert np.array_equal(mc._section("pairing"), before[0]) and np.array_equal(mc._section("susceptibilities"), before[1])
        assert [mc.binner_size(k)[2] for k in RESP] == [1, 1, 1]
        # the frees: channels -> the two pairing binners; current targets -> the current one; momenta -> all
        mc.set_pair_channels({"s": [1, 0, 0, 0, 0]})
        assert [size(mc, k) for k in RESP] == [_lib.ERR_STATE, _lib.ERR_STATE, _lib.OK]
        mc.enable_binning(RESP[:2], capacity=3)
        assert mc.binner_size(RESP[0])[0] == 2 * 1 * 3
        l = mc.model.l
        mc._set_current_targets(gpu.EachLocalQuadBySyncedDistance(l, K=3).trg_of, 3, None)
        assert [size(mc, k) for k in RESP] == [_lib.OK, _lib.OK, _lib.ERR_STATE]
        mc.enable_binning("response_current", capacity=3)
        assert mc.binner_size("response_current")[0] == 2 * 3 * 3 + 3
        mc.set_momenta(q[:2])
        assert [size(mc, k) for k in RESP] == [_lib.ERR_STATE] * 3
        mc.enable_binning(RESP, capacity=3)
        mc._set_local_targets(gpu.EachLocalQuadByDistance(l).trg_of, 5)  # turns the channels off
        assert mc.response_plan()["n_ch"] == 0 and mc.pair_channels() is None
        assert [size(mc, k) for k in RESP] == [_lib.ERR_STATE, _lib.ERR_STATE, _lib.OK]
        mc.set_pair_channels("default")
        mc.enable_binning(RESP[:2], capacity=3)
        mc.set_pair_directions(gpu.EachSitePairByDistance(l))  # momenta off: all three go
        assert [size(mc, k) for k in RESP] == [_lib.ERR_STATE] * 3
        mc._set_current_targets(gpu.EachLocalQuadBySyncedDistance(l).trg_of, 5, None)
        mc.set_momenta(q[:2])
        # a refused set_pair_channels keeps the setting, the engine's binners and the host's record of them
        mc.enable_binning(RESP[:2], capacity=3)
        for bad in ({"x": [1, 2]}, "nonsense", {"c%d" % i: [1, 0, 0, 0, 0] for i in range(9)}, {"x": [1, 0, 0, 0, np.nan]}):
            with pytest.raises(ValueError):
                mc.set_pair_channels(bad)
            assert list(mc.pair_channels()) == ["s", "s*", "d"] and mc.response_plan()["n_ch"] == 3
            assert all(size(mc, k) == _lib.OK and mc._binning_enabled(k) and k in mc._bin_caps for k in RESP[:2])
        mc.accumulate_greens()
        mc.accumulate_susceptibilities(recalculate=5)
        with pytest.raises(ValueError) as e:  # q[:2] holds (0, 0) and q_L = (pi/2, 0), not q_T: the one that is missing is named
            mc.superfluid_stiffness(0)
        assert "q_T" in str(e.value) and "q_L" not in str(e.value)
        mc.set_momenta(q[2:4])
        mc.accumulate_susceptibilities(recalculate=5)
        with pytest.raises(ValueError) as e:  # neither
            mc.superfluid_stiffness(0)
        assert "q_L" in str(e.value) and "q_T" in str(e.value)
    finally:
        mc.close()


def test_sign_weighting(gpu):
    """the doped repulsive model at 4 x 4, mu = 0.5: the sample is s_w times the unweighted one with a trailing s_w;
    binned() and superfluid_stiffness() are jackknife_ratio applied by hand.  At this size the fields' own signs are
    all +1 for most seeds, which would make every check the unweighted case, so the per-unit signs are imposed
    (dqmc_impose_unit_signs, as test_gpu_sign_sizes.py does) before every pass: walkers with s = -1 through either block,
    at the first measurement point (s = +1 through two negative blocks later), asserted through sign()"""
    from montecarlo_jl_amd.dqmc import jackknife_ratio
    mc = plain = None
    try:
        mc = handle(gpu, "sq4", "repulsive", 3, n_q="all", U=4.0, mu=0.5, sign_weighting=True)
        plain = handle(gpu, "sq4", "repulsive", 3, n_q="all", U=4.0, mu=0.5)
        nq, K = 16, mc._Kcc
        for m in (mc, plain):
            m.enable_binning(("pairing", "susceptibilities") + RESP, capacity=7)
        assert [mc.binner_size(k)[0] for k in RESP] == [2 * 3 * nq + 1, 2 * 3 * nq + 1, 2 * K * nq + K + 1]
        IMPOSED = [np.array([[1, 1], [-1, 1], [1, -1]]), np.array([[1, 1], [-1, -1], [1, 1]]), np.array([[-1, -1], [1, 1], [1, 1]])]
        mc.impose_unit_signs(IMPOSED[0])
        sg = mc.sign()
        assert list(sg) == [1, -1, -1]
        one_pass(mc, greens=True)
        one_pass(plain, greens=True)
        assert_samples(mc, "signed sq4")
        for k in RESP:
            for w in range(3):
                x, y = level0(mc, k, w), level0(plain, k, w)
                assert x[-1] == sg[w] and sg[w] in (-1, 1) and np.array_equal(x[:-1], sg[w] * y), k
        for s in range(2):
            mc.update_until_measure()
            mc.impose_unit_signs(IMPOSED[s + 1])
            assert list(mc.sign()) == list(IMPOSED[s + 1].prod(axis=1))
            one_pass(mc, greens=True)
        lv0 = np.stack([level0(mc, "response_current", w) for w in range(3)])
        # sums of s over the three passes: two walkers carry one negative sample each, so the ratio is not the plain mean
        # (and no walker left out makes the jackknife's denominator 0: 5 - 3, 5 - 1, 5 - 1)
        assert list(lv0[:, -1]) == [3, 1, 1]
        val, err = jackknife_ratio(lv0[:, :-1], lv0[:, -1])
        b = mc.binned("response_current")
        n = K * nq
        assert np.array_equal(b["Lambda"], val[:n].reshape(K, nq) - 1j * val[n:2 * n].reshape(K, nq))
        assert np.array_equal(b["kbond"], val[2 * n:]) and np.array_equal(b["kbond_std_error"], err[2 * n:])
        assert np.array_equal(b["Lambda_std_error_re"], err[:n].reshape(K, nq)) and "s" not in b
        st = mc.superfluid_stiffness(0)
        kp, km, iL, iT = mc._stiffness_indices(0)
        three = np.stack([lv0[:, 2 * n + kp] + lv0[:, 2 * n + km], -lv0[:, kp * nq + iL], -lv0[:, kp * nq + iT]], axis=1)
        v3, e3 = jackknife_ratio(three, lv0[:, -1])
        for i, k in enumerate(("k_axis", "Lambda_L", "Lambda_T")):
            assert st[k + "_std_error"] == e3[i] and np.isfinite(e3[i])
            assert abs(st[k] - v3[i]) <= 1e-11 * max(1.0, abs(v3[i]))  # (the mean: from the accumulators, the same ratio)
        _, e2 = jackknife_ratio(np.stack([(-three[:, 0] - three[:, 2]) / 4.0, -three[:, 0] - three[:, 1]], axis=1), lv0[:, -1])
        assert st["rho_s_std_error"] == e2[0] and st["drude_std_error"] == e2[1]
        mc.reset_accumulators()
        mc.set_sign_weighting(False)  # re-created, empty, without the trailing s
        assert [mc.binner_size(k)[::2] for k in RESP] == [(2 * 3 * nq, 0), (2 * 3 * nq, 0), (2 * K * nq + K, 0)]
    finally:
        for m in (mc, plain):
            if m is not None:
                m.close()


def binner_state(mc):
    out = {}
    for k in RESP:
        E, L, T = mc.binner_size(k)
        out[k] = (E, L, T, [mc.binner_level(k, w, lv)[:2] for w in range(mc.n_walkers) for lv in range(L)])
    return out


def test_checkpoint(gpu, tmp_path):
    """save with the three binners on after 3 pushes, load, push 2 more: every binner level equals, exactly, that of the
    handle that kept its binners and was fed the same 5 samples (it imports the same blob, so that both continue from the
    same rebuilt state: the futures of two imports of one blob are exact); the blob version is the parent's + 4.
    The restored compressor, which no level shows at push 3, is checked by hand at push 4 on the loaded handle: level 1
    must grow by (s3 + s4) / 2 with s3, s4 the increments of level 0 (s3 from the saving handle's level 0 before and after
    its third push).  Each of the three differences of sums is off by at most 2 u |sum|, u = 2^-53: the bound is
    4 2^-52 max(|level 0|, |level 1|) per element, where a compressor from a wrong offset is off by the size of a sample.
    superfluid_stiffness() on the loaded handle (the directions are rebuilt from the lattice) equals the saver's."""
    from montecarlo_jl_amd import _lib, checkpoint
    a = b = c = None
    p = tmp_path / "resp.ckpt"
    try:
        a = handle(gpu, "sq4", "attractive", 2, n_q=5, mu=0.3)
        a.enable_binning(RESP, capacity=7)
        lv0_2 = None
        for s in range(3):
            if s:
                a.update_until_measure()
            if s == 2:
                lv0_2 = {k: [level0(a, k, w) for w in range(2)] for k in RESP}
            one_pass(a, greens=True)
        a.save(p)
        pre, blob = checkpoint.read(p)
        assert int.from_bytes(bytes(blob[8:12]), "little") == 5 and set(RESP) <= set(pre["binning"]["sections"])
        assert [k for k, _ in pre["pair_channels"]] == ["s", "s*", "d"]
        b = gpu.DQMC.load(p)
        assert {k: list(v) for k, v in b.pair_channels().items()} == {k: list(v) for k, v in a.pair_channels().items()}
        sa, sb = binner_state(a), binner_state(b)
        for k in RESP:
            assert sa[k][:3] == sb[k][:3] and sb[k][2] == 3
            for (x1, y1), (x2, y2) in zip(sa[k][3], sb[k][3]):
                assert np.array_equal(x1, x2) and np.array_equal(y1, y2), k
        sta, stb = a.superfluid_stiffness(0), b.superfluid_stiffness(0)
        assert set(sta) == set(stb) and "rho_s_std_error" in stb and all(sta[k] == stb[k] for k in sta), (sta, stb)
        a.set_state(blob)
        before4 = {k: [(level0(b, k, w), b.binner_level(k, w, 1)[0]) for w in range(2)] for k in RESP}
        for s in range(2):
            for m in (a, b):
                m.update_until_measure()
                one_pass(m, greens=True)
            if s == 0:  # push 4 empties the restored compressor into level 1
                for k in RESP:
                    for w in range(2):
                        l0_3, l1_3 = before4[k][w]
                        l0_4, l1_4 = level0(b, k, w), b.binner_level(k, w, 1)[0]
                        s3, s4 = l0_3 - lv0_2[k][w], l0_4 - l0_3
                        bound = 4 * U52 * np.maximum(np.abs(l0_4), np.abs(l1_4)) + 1e-300
                        assert np.all(np.abs((l1_4 - l1_3) - (s3 + s4) / 2) <= bound), (k, w)
                        assert np.abs(s3).max() > 1e-6 and np.abs(s3 - s4).max() > 1e-9  # (not vacuous: the samples differ)
        sa, sb = binner_state(a), binner_state(b)
        for k in RESP:
            assert sa[k][:3] == sb[k][:3] and sb[k][2] == 5
            for (x1, y1), (x2, y2) in zip(sa[k][3], sb[k][3]):
                assert np.array_equal(x1, x2) and np.array_equal(y1, y2), k
        # with a momentum binner on as well the version is 2 + 4; a handle without the binners refuses the blob, named
        c = handle(gpu, "sq4", "attractive", 2, n_q=5, mu=0.3)
        c._section_size("susceptibilities")  # (the section laid out, as the saved handle's is)
        before = c.state()
        with pytest.raises(_lib.DQMCError) as e:
            c.set_state(blob)
        assert e.value.code == _lib.ERR_INVALID and "binner response_pairing on" in str(e.value)
        assert np.array_equal(c.state(), before)
        c.enable_binning(RESP + ("momentum_correlations",), capacity=7)
        assert int.from_bytes(bytes(c.state()[8:12]), "little") == 6
        with pytest.raises(_lib.DQMCError) as e:
            c.set_state(before)
        assert e.value.code == _lib.ERR_INVALID and "on" in str(e.value)
    finally:
        for m in (a, b, c):
            if m is not None:
                m.close()
