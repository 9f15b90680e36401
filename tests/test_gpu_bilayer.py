"""Hubbard models on BilayerSquareLattice(L) on the device: stepwise parity with the oracle (given the bilayer hopping
matrix), the factored path Ez (x) Ey (x) Ex at 16 x 16 x 2 (bilayer.hip) against the dense path (DQMC_NO_KRON=1, read
when a handle is created), the U = 0 known answers including n(k) at q_z = 0 and pi, the measurements with K = 6 and the
checkpoint.  Every factored case asserts the path taken: a silent fallback would make the comparisons vacuous."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
EPS = np.finfo(np.float64).eps


def _model(gpu, kind, L, **kw):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    return cls(l=gpu.BilayerSquareLattice(L), **kw)


def _oracles(O, mc, kind):
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(mc.model.l.L, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=mc.model.hopping_matrix()[0])
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


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
@pytest.mark.parametrize("L", [4, 6])
def test_stepwise_updates_match_oracle(gpu, O, kind, L):
    """propagate / sweep_spatial one call at a time through more than a full sweep (up and down chains, both wraps) at
    beta = 1, safe_mult = 5, t_perp = 1.5: n = 32 and n = 72 (off the tile grid)"""
    mc = gpu.DQMC(_model(gpu, kind, L, t_perp=1.5), beta=1.0, safe_mult=5, n_walkers=2 if L == 4 else 1, seed=31)
    assert not mc.kron_hopping()
    _stepwise(mc, _oracles(O, mc, kind), 2 * mc.p.slices + 3)
    mc.close()


def _handle(gpu, model, dense, **kw):
    if dense:
        os.environ["DQMC_NO_KRON"] = "1"
    try:
        mc = gpu.DQMC(model, **kw)
    finally:
        os.environ.pop("DQMC_NO_KRON", None)
    assert mc.kron_hopping() == (not dense)
    return mc


@pytest.mark.parametrize("kind,walkers,mu", [("attractive", 2, -0.5), ("repulsive", 1, -0.4)])
def test_factored_sweeps_match_dense_at_L16(gpu, kind, walkers, mu):
    """prepare, update_until_measure, one sweep at 16 x 16 x 2, t_perp = 1.3, beta = 1: HS field and counters identical, G
    within 1e-10.  Two units either way: two walkers of one block, one walker of two blocks"""
    kw = dict(beta=1.0, n_walkers=walkers, seed=77)
    mcs = [_handle(gpu, _model(gpu, kind, 16, t_perp=1.3, mu=mu), dense, **kw) for dense in (False, True)]
    for mc in mcs:
        mc.prepare()
        mc.update_until_measure()
        mc.sweep(1)
    f, d = mcs
    worst = 0.0
    for w in range(walkers):
        assert np.array_equal(f.conf(w), d.conf(w)), "HS field of walker %d differs" % w
        af, ad = f.analysis(w), d.analysis(w)
        assert (af.prop_local, af.acc_local) == (ad.prop_local, ad.acc_local)
        assert af.propagation_error.count == ad.propagation_error.count
        assert f.uniforms_used(w) == d.uniforms_used(w)
        for gf, gd in zip(f.greens_eff(w), d.greens_eff(w)):
            worst = max(worst, relerr(gf, gd))
    print("%s, %d walkers: max rel |G_factored - G_dense| = %.3g" % (kind, walkers, worst))
    assert worst < TOL
    for mc in mcs:
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_wrap_greens_both_directions_match_dense_at_L16(gpu, kind):
    mcs = [_handle(gpu, _model(gpu, kind, 16, t_perp=1.3), dense, beta=1.0, n_walkers=1, seed=5) for dense in (False, True)]
    for mc in mcs:
        mc.prepare()
    for sl, direction in ((3, 1), (7, -1), (10, -1), (1, 1)):
        for mc in mcs:
            mc.wrap_greens(sl, direction)
        for gf, gd in zip(mcs[0].greens_eff(0), mcs[1].greens_eff(0)):
            e = relerr(gf, gd)
            assert e < TOL, (sl, direction, e)
    for mc in mcs:
        mc.close()


class _OneStrongBond:
    """HubbardModelAttractive on 16 x 16 x 2 with the bond 1 - 2 at 1.2 t: its exponentials are no Kronecker products"""

    def __init__(self, gpu):
        self._m = _model(gpu, "attractive", 16, t_perp=1.3)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def hopping_matrix(self):
        T = self._m.hopping_matrix()[0]
        T[0, 1] = T[1, 0] = -1.2
        return [T]


def test_paths_that_stay_dense(gpu):
    for model, kw in ((_model(gpu, "attractive", 8, t_perp=1.3), {}), (_OneStrongBond(gpu), {}),
                      (_model(gpu, "attractive", 16, t_perp=1.3), dict(checkerboard=True))):
        mc = gpu.DQMC(model, beta=1.0, n_walkers=1, **kw)
        assert not mc.kron_hopping()
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_free_fermions_known_answers(gpu, kind):
    """U = 0, L = 4, t_perp = 2: G = (I + exp(-beta T))^-1 whatever the field, and n(k) of momentum_time_displaced() is the
    Fermi function of eps(k) - t_perp at q_z = 0 (bonding) and eps(k) + t_perp at q_z = pi (antibonding)"""
    tperp, mu, beta = 2.0, -0.3, 2.0
    model = _model(gpu, kind, 4, U=0.0, t_perp=tperp, mu=mu)
    mc = gpu.DQMC(model, beta=beta, safe_mult=5, n_walkers=2, seed=3)
    mc.set_pair_directions(gpu.EachSitePairByDistance(model.l))
    mc.set_momenta("all")
    mc.set_time_displaced(5, ("greens",))
    w, V = np.linalg.eigh(model.hopping_matrix()[0])
    G0 = (V / (1.0 + np.exp(-beta * w))) @ V.T
    mc.prepare()
    for _ in range(2):
        for wk in range(2):
            for g in mc.greens(wk):
                assert relerr(g, G0) < TOL, relerr(g, G0)
        mc.update_until_measure()
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=5)
    q = mc.momenta()
    assert q.shape == (32, 3)
    eps = -2.0 * (np.cos(q[:, 0]) + np.cos(q[:, 1])) - tperp * np.cos(q[:, 2]) - mu
    assert np.allclose(np.cos(q[:, 2]), np.where(np.arange(32) < 16, 1.0, -1.0))  # q_z = 0, then q_z = pi
    fermi = 1.0 / (np.exp(beta * eps) + 1.0)
    nk = mc.momentum_time_displaced()["nk"]
    assert nk.shape == (mc.nb, 32)
    for b in range(mc.nb):
        assert np.abs(nk[b] - fermi).max() < TOL, np.abs(nk[b] - fermi).max()
    assert np.abs(fermi[:16] - fermi[16:]).max() > 0.3  # (the two bands differ: a swapped label would show)
    mc.close()


# ---- measurements at L = 4, repulsive: inputs read from the device, the sums against tests/measurement_ref.py
def _raw(mc, size_fn, get_fn):
    size = C.c_size_t()
    mc._c(size_fn(mc._h, C.byref(size)))
    out = np.zeros(size.value)
    mc._c(get_fn(mc._h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _read_pass(gpu, mc, recalculate):
    """one CombinedGreensIterator pass: steps[w] = [(G0l, Gl0, Gll), ...] of every walker, per-block matrices"""
    lib = gpu.lib()
    steps = [[] for _ in range(mc.n_walkers)]
    mc._c(lib.dqmc_combined_iterator_begin(mc._h, recalculate))
    l = C.c_int32()
    while True:
        mc._c(lib.dqmc_combined_iterator_next(mc._h, C.byref(l)))
        if l.value < 0:
            return steps
        for w in range(mc.n_walkers):
            steps[w].append(tuple(mc._ut_result(i, w) for i in range(3)))


def _check(name, dev, ref, ab, P):
    """|dev - ref| <= 2 (P + 16) eps abs_sum elementwise: device and reference each sum at most P terms of fewer than 16
    flops, abs_sum the sum of the absolute values of the same terms (the bound of test_gpu_measurement_sizes.py); and the
    bound is small against the values"""
    dev, ref, ab = np.asarray(dev, dtype=float), np.asarray(ref, dtype=float), np.asarray(ab, dtype=float)
    assert dev.shape == ref.shape == ab.shape, (name, dev.shape, ref.shape)
    bound = 2.0 * (P + 16.0) * EPS * ab
    err = np.abs(dev - ref)
    print("%s: max err %.3g, max bound %.3g, max |ref| %.3g" % (name, err.max(), bound.max(), np.abs(ref).max()))
    assert bound.max() <= 1e-9 * np.abs(ref).max(), (name, "vacuous bound")
    assert np.all(err <= bound), (name, float(err.max()))


def test_measurements_match_the_numpy_references(gpu):
    """correlations, pairing and susceptibilities with set_current_targets on 4 x 4 x 2, K = 6 (the five nearest neighbours),
    n_dirs == n_sites == 32: the fast forms apply"""
    W, s, dtau = 2, 5, 0.1
    model = _model(gpu, "repulsive", 4, t_perp=1.5)
    l = model.l
    mc = gpu.DQMC(model, beta=0.5, delta_tau=dtau, safe_mult=s, n_walkers=W, seed=41)
    pairs = gpu.EachSitePairByDistance(l)
    loc = gpu.EachLocalQuadByDistance(l, pairs=pairs)
    cc = gpu.EachLocalQuadBySyncedDistance(l, pairs=pairs)
    n, nd, K, dir_of = l.sites, pairs.ndirections(), loc.K, pairs.dir_of
    assert (n, nd, K, cc.K) == (32, 32, 6, 6)
    mc.set_local_targets(loc)
    mc.set_current_targets(cc)
    assert mc.current_targets_fast_path()
    mc.prepare()
    mc.update_until_measure()
    mc.reset_accumulators()
    G = [mc.greens(w) for w in range(W)]
    T = model.hopping_matrix()
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    raw = mc.correlations_raw()
    assert raw[-1] == W
    per = [MR.equal_time(g, dir_of, nd) for g in G]
    for i, k in enumerate(("CDC", "SDCx", "SDCy", "SDCz")):
        _check(k, raw[i * nd:(i + 1) * nd], sum(p[k][0] for p in per), sum(p[k][1] for p in per), n * W)
    _check("Mz", raw[4 * nd + 2 * n:4 * nd + 3 * n], sum(p["Mz"][0] for p in per), sum(p["Mz"][1] for p in per), W)
    raw = _raw(mc, gpu.lib().dqmc_pairing_size, gpu.lib().dqmc_get_pairing)
    assert raw[-1] == W
    val, ab = (sum(x) for x in zip(*[MR.pairing(g, dir_of, nd, loc.trg_of) for g in G]))
    _check("PC", raw[:-1].reshape((nd, K, K), order="F"), val, ab, n * W)
    steps = _read_pass(gpu, mc, s)
    M = len(steps[0])
    assert M == mc.p.slices == 5
    per = [MR.susceptibilities(T, G[w], steps[w], dir_of, nd, dtau, trg_loc=loc.trg_of, trg_cc=cc.trg_of) for w in range(W)]
    mc.accumulate_susceptibilities(recalculate=s)
    raw = _raw(mc, gpu.lib().dqmc_susceptibilities_size, gpu.lib().dqmc_get_susceptibilities)
    assert raw.size == 4 * nd + nd * K * K + nd * K + 1 and raw[-1] == W
    dev = {k: raw[i * nd:(i + 1) * nd] for i, k in enumerate(("CDS", "SDSx", "SDSy", "SDSz"))}
    dev["PS"] = raw[4 * nd:4 * nd + nd * K * K].reshape((nd, K, K), order="F")
    dev["CCS"] = raw[4 * nd + nd * K * K:-1].reshape((nd, K), order="F")
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS", "CCS"):
        _check(k, dev[k], sum(p[k][0] for p in per), sum(p[k][1] for p in per), n * M * W)
    mc.close()


def test_momenta_channels_and_stiffness(gpu):
    """structure_factors() over all 32 momenta including (pi, pi, pi) against numpy from the site positions, the four
    default pair channels, superfluid_stiffness along the in-plane axes and its refusal of the interlayer one"""
    model = _model(gpu, "repulsive", 4, t_perp=1.5)
    l = model.l
    mc = gpu.DQMC(model, beta=0.5, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=43)
    pairs = gpu.EachSitePairByDistance(l)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(l, pairs=pairs))
    mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(l, pairs=pairs))
    mc.set_momenta("all")
    mc.set_pair_channels("default")
    ch = mc.pair_channels()
    assert list(ch) == ["s", "s*", "d", "s_perp"] and ch["s_perp"].sum() == 1.0 and ch["s_perp"].shape == (6,)
    mc.prepare()
    mc.update_until_measure()
    mc.reset_accumulators()
    G = [mc.greens(w) for w in range(2)]
    mc.accumulate_greens()
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    mc.accumulate_susceptibilities(recalculate=5)
    q = mc.momenta()
    assert q.shape == (32, 3) and np.allclose(q[2 + 4 * 2 + 16], [np.pi, np.pi, np.pi])  # label (2, 2, 1)
    sf = mc.structure_factors()
    assert sf["count"] == 2 and sf["Sz"].shape == (32,)
    n = l.sites
    pos = np.array(gpu.lattices._positions(l))
    cosp = np.cos(np.einsum("ijx,qx->qij", pos[:, None, :] - pos[None, :, :], q))
    pair = np.arange(n * n).reshape(n, n)  # every pair its own "direction": the Wick terms pair by pair
    for name, key in (("Sc", "CDC"), ("Sz", "SDCz")):
        ref = sum(np.einsum("qij,ij->q", cosp, MR.equal_time(g, pair, n * n)[key][0].reshape(n, n)) for g in G) / 2
        assert np.abs(sf[name] - ref).max() <= TOL * np.abs(ref).max(), name
    P = mc.pair_structure_factors()
    assert all(k in P for k in ch)
    for axis in (0, 1):
        st = mc.superfluid_stiffness(axis)
        assert all(np.isfinite(st[k]) for k in ("k_axis", "Lambda_L", "Lambda_T", "rho_s", "drude")) and st["k_axis"] < 0
    for fn in (mc.superfluid_stiffness, mc._axis_bonds):
        with pytest.raises(ValueError, match="axis 2"):
            fn(2)
    mc.close()


def test_checkpoint_restores_the_bilayer_model(gpu, tmp_path):
    """save at a measurement point, load: the file names the lattice and t_perp, the loaded model's hopping matrix is equal,
    and the next sweep gives the same HS field as the uninterrupted handle"""
    kw = dict(beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=4242, thermalization=0, sweeps=0, measure_rate=1)
    a = gpu.DQMC(_model(gpu, "repulsive", 4, t_perp=1.5, mu=-0.2), **kw)
    a.prepare()
    a.update_until_measure()
    a.sweep(1)
    path = str(tmp_path / "bilayer.ckpt")
    a.save(path)
    pre = a._preamble(0, False)
    assert pre["lattice"] == {"class": "BilayerSquareLattice", "args": [4]} and pre["model"]["t_perp"] == 1.5
    a.sweep(1)
    b = gpu.DQMC.load(path)
    assert type(b.model) is type(a.model) and isinstance(b.model.l, gpu.BilayerSquareLattice)
    assert (b.model.t_perp, b.model.mu, b.model.l.L) == (1.5, -0.2, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a.model.hopping_matrix(), b.model.hopping_matrix()))
    b.sweep(1)
    for w in range(2):
        assert np.array_equal(a.conf(w), b.conf(w))
        assert a.uniforms_used(w) == b.uniforms_used(w)
        for ga, gb in zip(a.greens(w), b.greens(w)):
            assert relerr(gb, ga) < TOL
    # a model on another lattice writes the preamble of before
    c = gpu.DQMC(gpu.HubbardModelRepulsive(4, 2), **kw)
    assert "t_perp" not in c._preamble(0, False)["model"]
    for mc in (a, b, c):
        mc.close()
