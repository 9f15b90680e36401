"""Hubbard and Ising models on RectangularLattice(Lx, Ly) on the device: stepwise parity with the oracle (given the
lattice's hopping matrix), the factored path Ey (x) Ex of unequal factors at 32 x 8 (rect.hip) against the dense path
(DQMC_NO_KRON=1, in a fresh child process), dqmc_wrap_greens from a non-symmetric matrix, the U = 0 n(k) on the (Lx, Ly)
grid, the paths that stay dense, the measurements at 6 x 4 with K = 5, the stiffness along both axes, the checkpoint and
the Ising sweep.  Every factored case asserts the path taken: a silent fallback would make the comparisons vacuous."""
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest

from conftest import ROOT, relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402
import response_ref as RR  # noqa: E402
from test_gpu_bilayer import _check, _raw, _read_pass, _stepwise  # noqa: E402
from test_gpu_ising import _stats, restate  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _model(gpu, kind, Lx, Ly, **kw):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    return cls(l=gpu.RectangularLattice(Lx, Ly), **kw)


def _oracles(O, mc, kind):
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(0, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=mc.model.U,
                         hopping=mc.model.hopping_matrix()[0])
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


@pytest.mark.parametrize("kind,kw", [("attractive", {}), ("repulsive", {}), ("repulsive", dict(mu=-0.4, tp=-0.25))],
                         ids=["attractive", "repulsive", "repulsive_doped_tp"])
@pytest.mark.parametrize("Lx,Ly", [(4, 3), (6, 4), (8, 2)])
def test_stepwise_updates_match_oracle(gpu, O, kind, kw, Lx, Ly):
    """prepare, then propagate / sweep_spatial one call at a time through two sweeps (up and down chains, both wraps) at
    beta = 1, safe_mult = 5: n = 12, 24 and 16 (8 x 2: the doubled bonds of a length-2 axis)"""
    mc = gpu.DQMC(_model(gpu, kind, Lx, Ly, **kw), beta=1.0, safe_mult=5, n_walkers=2, seed=31)
    assert not mc.kron_hopping()
    _stepwise(mc, _oracles(O, mc, kind), 4 * mc.p.slices)
    mc.close()


# ---- 32 x 8: the factored path against the dense one of a child process started with DQMC_NO_KRON=1
KINDS = ("attractive", "repulsive")
WRAPS = ((3, 1), (7, -1), (10, -1), (1, 1))


def _run_32x8(gpu, kind, want_kron):
    """prepare plus two sweeps from the seeded random field, then the wraps from a seeded non-symmetric greens_eff"""
    out = {}
    mc = gpu.DQMC(_model(gpu, kind, 32, 8, mu=-0.4), beta=1.0, n_walkers=2, seed=77)
    assert mc.kron_hopping() == want_kron
    mc.prepare()
    out["G0"] = np.array([mc.greens_eff(w) for w in range(2)])
    mc.sweep(2)
    out["conf"] = np.array([mc.conf(w) for w in range(2)])
    out["G2"] = np.array([mc.greens_eff(w) for w in range(2)])
    out["counters"] = np.array([[mc.analysis(w).prop_local, mc.analysis(w).acc_local, mc.uniforms_used(w)] for w in range(2)])
    rng = np.random.default_rng(5)
    for w in range(2):
        mc.set_greens_eff(w, [rng.standard_normal((256, 256)) for _ in range(mc.nb)])
    for i, (sl, direction) in enumerate(WRAPS):
        mc.wrap_greens(sl, direction)
        out["W%d" % i] = np.array([mc.greens_eff(w) for w in range(2)])
    mc.close()
    return out


@pytest.fixture(scope="module")
def dense_32x8(gpu, tmp_path_factory):
    """the dense side, computed once: this module's _run_32x8 in a child process whose handles are created under
    DQMC_NO_KRON=1 (asserted there through kron_hopping())"""
    path = str(tmp_path_factory.mktemp("rect") / "dense.npz")
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import __graft_entry__ as g
        gpu = g.load_package()
        import test_gpu_rectangular as T
        res = {}
        for kind in T.KINDS:
            for k, v in T._run_32x8(gpu, kind, False).items():
                res[kind + "_" + k] = v
        np.savez(%r, **res)
        print("dense side written")
    """ % (ROOT, os.path.join(ROOT, "tests"), path))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DQMC_NO_KRON="1"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "dense side written" in p.stdout, p.stdout + p.stderr
    return dict(np.load(path))


@pytest.fixture(scope="module")
def factored_32x8(gpu):
    return {kind: _run_32x8(gpu, kind, True) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_factored_sweeps_match_dense_at_32x8(factored_32x8, dense_32x8, kind):
    """HS fields and counters identical, G within 1e-10 after prepare and after two sweeps.  Measured: see DESIGN 4.24."""
    f = factored_32x8[kind]
    d = {k[len(kind) + 1:]: v for k, v in dense_32x8.items() if k.startswith(kind + "_")}
    assert np.array_equal(f["conf"], d["conf"]), "HS fields differ"
    assert np.array_equal(f["counters"], d["counters"]), (f["counters"], d["counters"])
    worst = max(relerr(f[k], d[k]) for k in ("G0", "G2"))
    print("%s: max |G_factored - G_dense| / max|G| = %.3g" % (kind, worst))
    assert worst < TOL


@pytest.mark.parametrize("kind", KINDS)
def test_wrap_greens_both_directions_match_dense_at_32x8(factored_32x8, dense_32x8, kind):
    """four chained wraps in both directions from a non-symmetric random matrix: a swapped axis or a missed transpose in
    one of the two one-step launches shows here directly"""
    f = factored_32x8[kind]
    for i in range(len(WRAPS)):
        d = dense_32x8["%s_W%d" % (kind, i)]
        assert np.abs(d - np.swapaxes(d, -1, -2)).max() > 1e-3 * np.abs(d).max()  # (far from symmetric)
        e = relerr(f["W%d" % i], d)
        print("%s wrap %d %r: %.3g" % (kind, i, WRAPS[i], e))
        assert e < TOL, (WRAPS[i], e)


@pytest.mark.parametrize("Lx,Ly,factored", [(6, 4, False), (32, 8, True)])
def test_free_fermions_nk(gpu, Lx, Ly, factored):
    """U = 0, mu = -0.3: n(k) of momentum_time_displaced() is the Fermi function of eps(k) = -2 t (cos kx + cos ky) - mu on
    the (Lx, Ly) grid; exchanging kx and ky changes the answer"""
    mu, beta = -0.3, 2.0
    model = _model(gpu, "attractive", Lx, Ly, U=0.0, mu=mu)
    mc = gpu.DQMC(model, beta=beta, safe_mult=5, n_walkers=2, seed=3)
    assert mc.kron_hopping() == factored
    if factored:  # (the package's iterator takes ten seconds of host time at 256 sites: the same table from coordinates)
        n = Lx * Ly
        x, y = np.arange(n) % Lx, np.arange(n) // Lx
        dx, dy = (x[:, None] - x[None, :]) % Lx, (y[:, None] - y[None, :]) % Ly  # pos[src] - pos[trg], folded
        r = [(a if a <= Lx // 2 else a - Lx, b if b <= Ly // 2 else b - Ly) for b in range(Ly) for a in range(Lx)]
        it = types.SimpleNamespace(dir_of=dx + Lx * dy, directions=r, ndirections=lambda: n)
    else:
        it = gpu.EachSitePairByDistance(model.l)
    mc.set_pair_directions(it)
    mc.set_momenta("all")
    mc.set_time_displaced(5, ("greens",))
    mc.prepare()
    mc.update_until_measure()
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=5)
    q = mc.momenta()
    lab = np.array([(a, b) for b in range(Ly) for a in range(Lx)])
    assert q.shape == (Lx * Ly, 2) and np.allclose(q, lab * np.array([2 * np.pi / Lx, 2 * np.pi / Ly]), rtol=0, atol=1e-13)
    fermi = lambda kx, ky: 1.0 / (np.exp(beta * (-2.0 * (np.cos(kx) + np.cos(ky)) - mu)) + 1.0)
    nk = mc.momentum_time_displaced()["nk"]
    assert nk.shape == (mc.nb, Lx * Ly)
    err = np.abs(nk[0] - fermi(q[:, 0], q[:, 1])).max()
    print("%d x %d: max |n(k) - f(eps_k)| = %.3g" % (Lx, Ly, err))
    assert err < TOL
    swapped = fermi(lab[:, 0] * 2 * np.pi / Ly, lab[:, 1] * 2 * np.pi / Lx)  # the grid with the lengths exchanged
    assert np.abs(swapped - fermi(q[:, 0], q[:, 1])).max() > 0.1
    mc.close()


def _prepare_matches_oracle(O, mc, kind, exps=None):
    mc.prepare()
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(0, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=mc.model.U,
                         hopping=mc.model.hopping_matrix()[0], exps=exps)
        o.set_conf(mc.conf(w))
        o.prepare()
        for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
            assert relerr(g, g0) < TOL, relerr(g, g0)


@pytest.mark.parametrize("Lx,Ly,mkw,kw,env", [(8, 32, {}, {}, {}), (64, 4, {}, {}, {}), (32, 8, dict(tp=-0.25), {}, {}),
                                               (32, 8, {}, dict(checkerboard="sparse"), {}), (32, 8, {}, {}, {"DQMC_NO_KRON": "1"})],
                         ids=["8x32", "64x4", "32x8_tp", "32x8_checkerboard", "32x8_no_kron"])
def test_paths_that_stay_dense(gpu, O, Lx, Ly, mkw, kw, env):
    """kron_hopping() False and a prepare within TOL of the oracle (with the checkerboard: of the oracle given the same
    group-product exponentials).  The checkerboard is the engine's own, the sparse-factor form: see the next test for
    checkerboard=True."""
    os.environ.update(env)  # (read when the handle is created)
    try:
        mc = gpu.DQMC(_model(gpu, "attractive", Lx, Ly, **mkw), beta=1.0, n_walkers=1, seed=9, **kw)
    finally:
        for k in env:
            os.environ.pop(k, None)
    assert not mc.kron_hopping()
    exps = None
    if kw.get("checkerboard"):
        exps = (mc.hopping_matrix_exp[0], mc.hopping_matrix_exp_inv[0], mc.hopping_matrix_exp_squared[0],
                mc.hopping_matrix_exp_inv_squared[0])
    _prepare_matches_oracle(O, mc, "attractive", exps)
    mc.close()


def test_multiplied_out_checkerboard_at_32x8_matches_oracle(gpu, O):
    """checkerboard=True at n = 256 hands the engine the bond groups multiplied out, and never tells it of a checkerboard.
    On this lattice those products are Kronecker products Ey (x) Ex themselves, so the gate, which reads the matrices,
    accepts them (observed: kron_hopping() True); what is asserted is the result: a prepare within TOL of the oracle given
    the same products.  These products are not symmetric, which no exponential of the lattice's own hopping is; the chains,
    wraps and sweeps of rect.hip on non-symmetric factors, in both spin blocks, are in test_gpu_factored_generic.py."""
    mc = gpu.DQMC(_model(gpu, "attractive", 32, 8), beta=1.0, n_walkers=1, seed=9, checkerboard=True)
    print("checkerboard=True at 32 x 8: kron_hopping() = %r" % mc.kron_hopping())
    _prepare_matches_oracle(O, mc, "attractive", (mc.hopping_matrix_exp[0], mc.hopping_matrix_exp_inv[0],
                                                  mc.hopping_matrix_exp_squared[0], mc.hopping_matrix_exp_inv_squared[0]))
    mc.close()


def test_factored_prepare_matches_oracle_at_32x8(gpu, O):
    """the factored path against the oracle itself (not only against the dense path)"""
    mc = gpu.DQMC(_model(gpu, "repulsive", 32, 8, mu=-0.4), beta=1.0, n_walkers=1, seed=9)
    assert mc.kron_hopping()
    _prepare_matches_oracle(O, mc, "repulsive")
    mc.close()


# ---- measurements at 6 x 4, repulsive: inputs read from the device, the sums against tests/measurement_ref.py
def test_measurements_match_the_numpy_references(gpu):
    """correlations, pairing and susceptibilities with set_current_targets on 6 x 4, K = 5, n_dirs == n_sites == 24: the fast
    forms apply"""
    W, s, dtau = 2, 5, 0.1
    model = _model(gpu, "repulsive", 6, 4)
    l = model.l
    mc = gpu.DQMC(model, beta=0.5, delta_tau=dtau, safe_mult=s, n_walkers=W, seed=41)
    pairs = gpu.EachSitePairByDistance(l)
    loc = gpu.EachLocalQuadByDistance(l, pairs=pairs)
    cc = gpu.EachLocalQuadBySyncedDistance(l, pairs=pairs)
    n, nd, K, dir_of = l.sites, pairs.ndirections(), loc.K, pairs.dir_of
    assert (n, nd, K, cc.K) == (24, 24, 5, 5)
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


def test_momenta_and_pair_channels(gpu):
    """structure_factors() over the 24 momenta against numpy from the site positions, and the three default channels"""
    model = _model(gpu, "repulsive", 6, 4)
    l = model.l
    mc = gpu.DQMC(model, beta=0.5, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=43)
    pairs = gpu.EachSitePairByDistance(l)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(l, pairs=pairs))
    mc.set_momenta("all")
    mc.set_pair_channels("default")
    ch = mc.pair_channels()
    d = np.array(pairs.directions[:5])
    assert list(ch) == ["s", "s*", "d"] and all(ch["d"][k] == (0.5 if d[k, 0] != 0 else -0.5) for k in range(1, 5))
    mc.prepare()
    mc.update_until_measure()
    mc.reset_accumulators()
    G = [mc.greens(w) for w in range(2)]
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    q = mc.momenta()
    assert q.shape == (24, 2) and np.allclose(q[3 + 6 * 2], [np.pi, np.pi])  # label (3, 2)
    sf = mc.structure_factors()
    assert sf["count"] == 2 and sf["Sz"].shape == (24,)
    n = l.sites
    pos = np.array(gpu.lattices._positions(l))
    cosp = np.cos(np.einsum("ijx,qx->qij", pos[:, None, :] - pos[None, :, :], q))
    pair = np.arange(n * n).reshape(n, n)  # every pair its own "direction": the Wick terms pair by pair
    for name, key in (("Sc", "CDC"), ("Sz", "SDCz")):
        ref = sum(np.einsum("qij,ij->q", cosp, MR.equal_time(g, pair, n * n)[key][0].reshape(n, n)) for g in G) / 2
        assert np.abs(sf[name] - ref).max() <= TOL * np.abs(ref).max(), name
    P = mc.pair_structure_factors()
    assert all(k in P and P[k].shape == (24,) for k in ch)
    mc.close()


def test_superfluid_stiffness_takes_each_axis_own_momentum(gpu):
    """free fermions at 6 x 4, mu = -0.3: superfluid_stiffness(0) and (1) against tests/response_ref.py with q_L = 2 pi / Lx
    along x and 2 pi / Ly along y (q_T the other one); the two axes differ"""
    Lx, Ly, mu, beta, dtau = 6, 4, -0.3, 2.0, 0.1
    model = _model(gpu, "attractive", Lx, Ly, U=0.0, mu=mu)
    l = model.l
    mc = gpu.DQMC(model, beta=beta, delta_tau=dtau, safe_mult=5, n_walkers=2, seed=71)
    ff, loc, cur = RR.free_fermions(gpu, l, beta, dtau, mu=mu)
    mc.set_local_targets(loc)
    mc.set_current_targets(cur)
    mc.set_momenta("all")
    mc.set_pair_channels("default")
    mc.prepare()
    mc.update_until_measure()
    mc.reset_accumulators()
    mc.accumulate_greens()
    mc.accumulate_susceptibilities(recalculate=5)
    rs, ms = ff.band_basis(mc.pair_channels())
    q, d = ff.q, ff.r[:cur.K]
    qx, qy = [2 * np.pi / Lx, 0], [0, 2 * np.pi / Ly]
    find_q = lambda v: next(i for i in range(len(q)) if np.allclose(q[i], v))
    find_d = lambda v: next(k for k in range(cur.K) if np.allclose(d[k], v))
    eps_g = 10 * 2.31e-14  # the bound of tests/test_gpu_response.py: ten times the device-against-exact error of G
    bound = 4 * eps_g + 2 * (l.sites * 2 * 4 * beta) * eps_g
    got = []
    for axis, (qL, qT, e) in enumerate(((qx, qy, [1, 0]), (qy, qx, [0, 1]))):
        st = mc.superfluid_stiffness(axis)
        want = RR.stiffness(rs["kbond"], ms["Lambda"], find_d(e), find_d([-e[0], -e[1]]), find_q(qL), find_q(qT))
        for k, v in want.items():
            print("axis %d %s: %.12g (reference %.12g)" % (axis, k, st[k], v))
            assert abs(st[k] - v) <= bound, (axis, k, st[k], v)
        assert mc._stiffness_indices(axis)[2:] == (find_q(qL), find_q(qT))
        got.append(st)
    assert abs(got[0]["Lambda_L"] - got[1]["Lambda_L"]) > 1e-3 and abs(got[0]["rho_s"] - got[1]["rho_s"]) > 1e-3
    mc.close()


def test_checkpoint_restores_the_rectangular_model(gpu, tmp_path):
    """save at a measurement point, load: the file names the lattice with (Lx, Ly), the loaded model's hopping matrix is
    equal, and the next sweep gives the same HS field as the uninterrupted handle"""
    kw = dict(beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=4242, thermalization=0, sweeps=0, measure_rate=1)
    a = gpu.DQMC(_model(gpu, "repulsive", 4, 3, mu=-0.2, tp=-0.25), **kw)
    a.prepare()
    a.update_until_measure()
    a.sweep(1)
    path = str(tmp_path / "rect.ckpt")
    a.save(path)
    pre = a._preamble(0, False)
    assert pre["lattice"] == {"class": "RectangularLattice", "args": [4, 3]} and pre["model"]["tp"] == -0.25
    a.sweep(1)
    b = gpu.DQMC.load(path)
    assert type(b.model) is type(a.model) and isinstance(b.model.l, gpu.RectangularLattice)
    assert (b.model.tp, b.model.mu, b.model.l.Lx, b.model.l.Ly) == (-0.25, -0.2, 4, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a.model.hopping_matrix(), b.model.hopping_matrix()))
    b.sweep(1)
    for w in range(2):
        assert np.array_equal(a.conf(w), b.conf(w))
        assert a.uniforms_used(w) == b.uniforms_used(w)
        for ga, gb in zip(a.greens(w), b.greens(w)):
            assert relerr(gb, ga) < TOL
    # a model on another lattice writes the preamble of before
    c = gpu.DQMC(gpu.HubbardModelRepulsive(4, 2), **kw)
    assert c._preamble(0, False)["lattice"] == {"class": "SquareLattice", "args": [4]}
    for mc in (a, b, c):
        mc.close()


def test_ising_sweeps_match_the_restatement_bit_exactly(gpu, O):
    l = gpu.RectangularLattice(6, 4)
    betas, seed = [0.3, 0.55], 777
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=2, seed=seed, thermalization=0, sweeps=2, measure_rate=1)
    mc.sweep(2)
    for w, b in enumerate(betas):
        ref, c = restate(O, l, b, seed + w, 0, 2, 1)
        assert _stats(mc, w) == ref, w
        assert np.array_equal(np.asarray(mc.conf(w)).reshape(-1, order="F"), c)
    mc.close()
