"""Renyi-2 entanglement entropy from walker pairs on the device (csrc/entangle.hip, entangle.inl; include/dqmc_hip.h
"entanglement"): every pair's sample against the numpy restatement (tests/entanglement_ref.py) fed with the same Green's
functions, at every tile edge and at the static / dynamic LDS switch of the pair kernel; independence of the batch; free
fermions against the closed form; sums, reset, the off state and the refusals; the way through run() and the checkpoint.

Tolerance of device against numpy on the same G (only GEMM / LU rounding separates them): relative
64 max(e_ref, 2^-52 N_A), e_ref the numpy reference's own error against extended precision on those very inputs."""
import shutil

import numpy as np
import pytest

import entanglement_ref as ER

pytestmark = pytest.mark.gpu
KINDS = ("attractive", "repulsive")


def make(gpu, l, kind, W, U=1.0, beta=1.0, seed=31, **kw):
    model = gpu.HubbardModelAttractive(l=l, U=U, mu=0.3) if kind == "attractive" else gpu.HubbardModelRepulsive(l=l, U=U)
    return gpu.DQMC(model, beta=beta, safe_mult=5, n_walkers=W, seed=seed, **kw)


def tolerance(e_ref, na):
    return 64.0 * max(e_ref, 2.0 ** -52 * na)


def assert_sample(x, greens, sites, label):
    """one subsystem's [W, W] device sample against numpy on the same G; -> the tolerance used"""
    ref, e_ref = ER.reference_error(greens, sites)
    tol = tolerance(e_ref, len(sites))
    iu = np.triu_indices(x.shape[0], 1)
    err = np.abs(x[iu] - ref[iu]) / np.abs(ref[iu])
    print("%s: N_A = %d, e_ref = %.3g, device - numpy = %.3g, tolerance %.3g" % (label, len(sites), e_ref, err.max(), tol))
    assert np.all(err <= tol), (label, len(sites), err.max(), tol)
    assert np.all(np.tril(x) == 0.0), label  # the lower triangle and the diagonal are exactly 0
    return tol


SMALL_SUBS = {"site": [5], "two": [10, 2], "strip": [0, 1, 4, 5, 8, 9, 12, 13], "all": list(range(16))}


def small(gpu, kind, W=3, subs=None, **kw):
    """the fixture of most cases: SquareLattice(4), 10 slices, safe_mult 5, two sweeps, one sample"""
    mc = make(gpu, gpu.SquareLattice(4), kind, W, **kw)
    mc.set_entanglement(SMALL_SUBS if subs is None else subs)
    mc.prepare()
    mc.sweep(2)
    mc.accumulate_entanglement()
    return mc


@pytest.mark.parametrize("kind", KINDS)
def test_samples_equal_numpy_on_the_same_greens_function(gpu, kind):
    """one site, two non-adjacent sites in descending order, the 8-site strip (strip_subsystem) and all 16 sites"""
    assert gpu.lattices.strip_subsystem(gpu.SquareLattice(4), 2).tolist() == SMALL_SUBS["strip"]
    mc = small(gpu, kind)
    try:
        x = mc.entanglement_sample()
        assert x.shape == (4, 3, 3)
        greens = [mc.greens(w) for w in range(3)]
        for s, (name, sites) in enumerate(SMALL_SUBS.items()):
            assert_sample(x[s], greens, sites, "%s %s" % (kind, name))
        res = mc.entanglement()
        assert res["names"] == list(SMALL_SUBS) and res["count"] == 1 and res["failures"] == 0
        assert np.array_equal(res["pair_sums"], x)
        assert np.allclose(res["purity"], x.sum(axis=(1, 2)) / 3.0, rtol=1e-15)
        assert np.all(res["S2"] > 0) and np.all(res["S2_std_error"] >= 0)
    finally:
        mc.close()


FORM_SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128)


def form_sites(gpu, l, na):
    """strips where N_A is a multiple of the lattice's edge, else the ragged prefix of a strip"""
    if na % 16 == 0:
        return gpu.lattices.strip_subsystem(l, na // 16, axis=1).tolist()
    return gpu.lattices.strip_subsystem(l, na // 16 + 1).tolist()[:na]


def test_every_kernel_form_and_the_refusals(gpu):
    """SquareLattice(16), attractive, 3 walkers, one sweep; N_A = 1, 15, 16, 17 (one tile and its edges), 63, 64, 65 (the
    last static size, the first dynamic one), 127, 128 (the limit) on one handle.  Then N_A = 129, an empty list, a
    duplicate site and a site = n: ERR_INVALID each, and the configuration of before goes on working."""
    from montecarlo_jl_amd import _lib
    l = gpu.SquareLattice(16)
    mc = make(gpu, l, "attractive", 3)
    try:
        subs = [form_sites(gpu, l, na) for na in FORM_SIZES]
        assert [len(a) for a in subs] == list(FORM_SIZES) and all(len(set(a)) == len(a) for a in subs)
        mc.set_entanglement(subs)
        mc.prepare()
        mc.sweep(1)
        mc.accumulate_entanglement()
        x = mc.entanglement_sample()
        greens = [mc.greens(w) for w in range(3)]
        for s, sites in enumerate(subs):
            assert_sample(x[s], greens, sites, "16x16")
        assert mc.entanglement()["failures"] == 0
        for bad in ([list(range(129))], [subs[1], []], [[3, 7, 3]], [[0, 256]], [[-1]], [[0]] * 65):
            with pytest.raises(_lib.DQMCError) as e:
                mc.set_entanglement(bad)
            assert e.value.code == _lib.ERR_INVALID, bad
        mc.accumulate_entanglement()
        assert np.array_equal(mc.entanglement_sample(), x)  # the same fields, the same bits
        res = mc.entanglement()
        assert res["count"] == 2 and np.array_equal(res["pair_sums"], x + x)
    finally:
        mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_pair_does_not_depend_on_the_batch(gpu, kind):
    """pair (0, 1) of a 2-, a 3- and a 5-walker handle (same seed, first_walker = 0), and the subsystem listed alone or as
    the last of four: bit for bit"""
    strip = SMALL_SUBS["strip"]
    got = {}
    for W, subs in ((2, [strip]), (3, [strip]), (5, [strip]), (3, [[5], [10, 2], list(range(16)), strip])):
        mc = small(gpu, kind, W=W, subs=subs)
        try:
            x = mc.entanglement_sample()
            got[(W, len(subs))] = x[-1, 0, 1]
            if W == 5:
                x3 = x[-1, :3, :3]
        finally:
            mc.close()
    vals = list(got.values())
    assert vals[0] != 0.0 and all(v == vals[0] for v in vals), got
    mc = small(gpu, kind, W=3, subs=[strip])
    try:
        assert np.array_equal(mc.entanglement_sample()[0], x3)  # and so do the other pairs of the first three walkers
    finally:
        mc.close()


FREE = [("square4", "attractive"), ("square4", "repulsive"), ("chain8", "attractive"), ("chain8", "repulsive")]


@pytest.mark.parametrize("name,kind", FREE)
def test_free_fermions_against_the_closed_form(gpu, name, kind):
    """U = 0 (dqmc_create accepts it), beta = 2, 3 walkers, prepare() only: the field drops out, every pair gives
    prod_b det(I - 2 C_A + 2 C_A^2) with C = (I + e^{beta T})^-1 from eigh of the model's hopping matrix.  Tolerance: the
    project's device-versus-oracle agreement on G, 1e-10, propagated through d log det M = tr(M^-1 dM):
    3 N_A ||M^-1||_1 1e-10 relative, ||M^-1||_1 computed here; S2_std_error is below the same bound."""
    l = gpu.SquareLattice(4) if name == "square4" else gpu.Chain(8)
    subs = {"square4": [[5], SMALL_SUBS["strip"], list(range(16))], "chain8": [[0, 1, 2, 3], [6, 1], list(range(8))]}[name]
    mc = make(gpu, l, kind, 3, U=0.0, beta=2.0)
    try:
        mc.set_entanglement(subs)
        mc.prepare()
        mc.accumulate_entanglement()
        x = mc.entanglement_sample()
        res = mc.entanglement()
        Ts = mc.model.hopping_matrix()
        for s, sites in enumerate(subs):
            exact, bound = 1.0, 0.0
            for T in (Ts if len(Ts) == 2 else [Ts[0], Ts[0]]):
                w, V = np.linalg.eigh(T)
                Cm = (V / (1.0 + np.exp(2.0 * w))) @ V.T
                Ca = ER.restrict(Cm, sites)
                M = np.eye(len(sites)) - 2.0 * Ca + 2.0 * Ca @ Ca
                exact *= np.linalg.det(M)
                bound = max(bound, 3.0 * len(sites) * np.linalg.norm(np.linalg.inv(M), 1) * 1e-10)
            iu = np.triu_indices(3, 1)
            err = np.abs(x[s][iu] - exact) / exact
            print("%s %s N_A = %d: purity %.15g, device - exact = %.3g, bound %.3g" % (name, kind, len(sites), exact, err.max(), bound))
            assert np.all(err <= bound), (sites, err, bound)
            assert abs(res["purity"][s] - exact) <= bound * exact
            assert abs(res["S2"][s] + np.log(exact)) <= bound
            assert res["S2_std_error"][s] <= bound
    finally:
        mc.close()


def test_sums_reset_off_and_refusals(gpu):
    from montecarlo_jl_amd import _lib
    mc = small(gpu, "repulsive")
    try:
        s1 = mc.entanglement_sample()
        mc.update()
        mc.accumulate_entanglement()
        s2 = mc.entanglement_sample()
        assert not np.array_equal(s1, s2)
        res = mc.entanglement()
        assert res["count"] == 2 and res["failures"] == 0 and np.array_equal(res["pair_sums"], s1 + s2)
        on = (mc.accumulator_size(), mc.reduce_size())
        mc.reset_accumulators()
        res = mc.entanglement()
        assert res["count"] == 0 and res["failures"] == 0 and not res["pair_sums"].any() and "purity" not in res
        mc.accumulate_entanglement()
        assert mc.entanglement()["count"] == 1
        mc.set_entanglement(None)
        assert (mc.accumulator_size(), mc.reduce_size()) == on
        for call in (mc.accumulate_entanglement, mc.entanglement_sample, mc.entanglement):
            with pytest.raises((_lib.DQMCError, TypeError)) as e:
                call()
            assert e.type is TypeError or e.value.code == _lib.ERR_STATE
        with pytest.raises(_lib.DQMCError) as e:
            mc.accumulate_entanglement()
        assert e.value.code == _lib.ERR_STATE
        mc.set_entanglement([])  # off twice is fine
        mc.set_entanglement([[1, 2]])  # and on again starts from zero
        assert mc.entanglement()["count"] == 0
    finally:
        mc.close()
    mc = make(gpu, gpu.SquareLattice(4), "repulsive", 3, sign_weighting=True)
    try:
        mc.set_entanglement([[1, 2]])
        mc.prepare()
        with pytest.raises(_lib.DQMCError) as e:
            mc.accumulate_entanglement()
        assert e.value.code == _lib.ERR_STATE
    finally:
        mc.close()
    mc = make(gpu, gpu.SquareLattice(4), "attractive", 1)
    try:
        with pytest.raises(_lib.DQMCError) as e:
            mc.set_entanglement([[1, 2]])
        assert e.value.code == _lib.ERR_STATE  # one walker has no pair
    finally:
        mc.close()


def test_run_checkpoint_and_resume(gpu, tmp_path):
    """run(measurements=("greens", "entanglement"), checkpoint=...) over 4 sweeps; the file saved in sweep 2 is loaded:
    sums, count and site lists come back exactly, and the finished run's pair sums agree with the uninterrupted run's to
    the tolerance of the sample test (G is rebuilt on import, as for every other section).  A file saved without the
    measurement has no "entanglement" key."""
    from montecarlo_jl_amd import checkpoint
    p, p2 = tmp_path / "run.ckpt", tmp_path / "at2.ckpt"
    subs = {"strip": SMALL_SUBS["strip"], "two": [10, 2]}
    kept = {}
    a = b = None

    def look(mc, i):
        if i == 3:  # (the file still holds sweep 2)
            shutil.copy(p, p2)
        if i == 2:
            kept["raw"] = mc._entanglement_raw()
    try:
        a = make(gpu, gpu.SquareLattice(4), "repulsive", 3, thermalization=0, sweeps=4, measure_rate=1)
        a.set_entanglement(subs)
        a.run(measurements=("greens", "entanglement"), on_measure=look, checkpoint=p, checkpoint_every=2)
        pre, _ = checkpoint.read(p2)
        assert pre["last_sweep"] == 2 and pre["entanglement"]["count"] == 2
        assert pre["entanglement"]["sites"] == list(subs.values()) and pre["entanglement"]["names"] == list(subs)
        b = gpu.DQMC.load(p2)
        assert b._ent == (list(subs), list(subs.values()))
        assert np.array_equal(b._entanglement_raw(), kept["raw"]) and kept["raw"][-2] == 2
        b.run(measurements=("greens", "entanglement"))
        ra, rb = a.entanglement(), b.entanglement()
        assert ra["count"] == rb["count"] == 4 and ra["failures"] == rb["failures"] == 0
        greens = [a.greens(w) for w in range(3)]
        for s, sites in enumerate(subs.values()):
            tol = tolerance(ER.reference_error(greens, sites)[1], len(sites))
            iu = np.triu_indices(3, 1)
            err = np.abs(ra["pair_sums"][s][iu] - rb["pair_sums"][s][iu]) / np.abs(ra["pair_sums"][s][iu])
            print("resumed - uninterrupted, N_A = %d: %.3g, tolerance %.3g" % (len(sites), err.max(), tol))
            assert np.all(err <= tol), (sites, err, tol)
        a.close()
        a = make(gpu, gpu.SquareLattice(4), "repulsive", 3, thermalization=0, sweeps=2, measure_rate=1)
        a.run(checkpoint=p, checkpoint_every=2)
        pre, _ = checkpoint.read(p)
        assert "entanglement" not in pre
    finally:
        for mc in (a, b):
            if mc is not None:
                mc.close()
