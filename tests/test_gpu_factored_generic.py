"""The factored hopping kernels (kron.hip, rect.hip, kron3.hip, bilayer.hip, tri.hip, ttp.hip) on exponentials that no
physical lattice gives (tests/factored_exps.py; their properties are asserted in test_factored_exps_host.py): factors
that are not symmetric, not circulant (tri.hip / ttp.hip, whose forms need commuting parts: circulant and asymmetric), and
different in the two spin blocks.  With the lattices' own exponentials a factor set in the place of its transpose, an
operand index reversed or rotated, or a block offset left out of a factor address reads equal numbers; here it does not.

The matrices reach the engine through the package's hopping_exponentials (called once per block in DQMC.__init__) and,
for the two commuting forms, triangular_factors / square_tp_factors, all three replaced for the duration of one
constructor.  The model is the ordinary one of the lattice, so the handle is created as always and the gates of
dqmc_create decide on the matrices alone.  Every factored handle asserts kron_hopping(): a silent fallback would make the
comparisons vacuous.  The oracle is given the same matrices, per block.

All runs: beta = 1, delta_tau = 0.1, safe_mult = 5, two walkers; every comparison of G at the project's 1e-10."""
import os
import subprocess
import sys
import textwrap
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT, relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factored_exps as FE  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
KW = dict(beta=1.0, delta_tau=FE.DELTA_TAU, safe_mult=5, n_walkers=2)
WRAPS = ((3, 1), (7, -1), (10, -1), (1, 1))
CASES = FE.ALL_CASES
IDS = ["%s-%s" % fc for fc in CASES]
_inputs = {}


def _case_inputs(family, case):
    if (family, case) not in _inputs:
        _inputs[family, case] = FE.case_inputs(family, case)
    return _inputs[family, case]


def _kind(case):
    return "repulsive" if case == "repulsive" else "attractive"


def _model(gpu, family, case):
    cls = gpu.HubbardModelRepulsive if _kind(case) == "repulsive" else gpu.HubbardModelAttractive
    if family == "square16":
        return cls(16, 2)
    if family == "rect32x8":
        return cls(l=gpu.RectangularLattice(32, 8))
    if family == "cubic8":
        return cls(8, 3)
    if family == "bilayer16":
        return cls(l=gpu.BilayerSquareLattice(16), t_perp=1.3)
    if family == "tri16":
        return cls(l=gpu.TriangularLattice(16))
    return cls(16, 2, tp=-0.25)


def _handle(gpu, family, case, dense=False, seed=31):
    """the lattice's ordinary model with the case's matrices in the place of its own exponentials (and factors)"""
    exps, farr = _case_inputs(family, case)
    model = _model(gpu, family, case)
    assert model.flv == len(exps)
    handed = iter(exps)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(gpu.dqmc, "hopping_exponentials", lambda T, delta_tau: next(handed))
        if farr is not None:
            m.setattr(gpu.dqmc, "triangular_factors" if family == "tri16" else "square_tp_factors", lambda model, delta_tau: farr)
        if dense:
            m.setenv("DQMC_NO_KRON", "1")  # (read when the handle is created)
        else:
            m.delenv("DQMC_NO_KRON", raising=False)
        mc = gpu.DQMC(model, seed=seed, **KW)
    assert next(handed, None) is None
    assert mc.kron_hopping() == (not dense), "%s %s: kron_hopping() = %r" % (family, case, mc.kron_hopping())
    for b, e in enumerate(exps):
        assert np.array_equal(mc.hopping_matrix_exp_squared[b], e[2])
    return mc


def _oracles(O, mc, family, case, exps=None):
    exps = _case_inputs(family, case)[0] if exps is None else exps
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(0, _kind(case), beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=mc.model.U,
                         hopping=np.zeros((mc.N, mc.N)), exps=exps)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


@pytest.mark.parametrize("family,case", CASES, ids=IDS)
def test_stepwise_updates_match_oracle(gpu, O, family, case):
    """prepare, then propagate / sweep_spatial one call at a time: 2 * slices + 3 steps at n = 256 (both chain directions,
    the daggered products and both wraps), one full up-and-down sweep at n = 512.  HS fields and counters identical, G
    within 1e-10 at every step.  In the repulsive case block 1 must also be far from what block 0's matrices would give
    (a condition on the inputs, from two oracle runs): a kernel that ignored the block in a factor address cannot pass."""
    mc = _handle(gpu, family, case)
    refs = _oracles(O, mc, family, case)
    worst = [0.0]
    pool = ThreadPoolExecutor(len(refs))
    # one host thread per walker's oracle (the calls release the GIL; the oracles share no state that these calls change
    # in value): at n = 512 the host side is most of the test's time
    each = lambda objs, name: list(pool.map(lambda o: getattr(o, name)(), objs))

    def compare(conf=True):
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                e = relerr(g, g0)
                worst[0] = max(worst[0], e)
                assert e < TOL, e

    mc.prepare()
    each(refs, "prepare")
    compare()
    if case == "repulsive":
        exps = _case_inputs(family, case)[0]
        shared = _oracles(O, mc, family, case, exps=[exps[0], exps[0]])[0]
        shared.prepare()
        own, other = refs[0].greens_eff()[1], shared.greens_eff()[1]
        assert relerr(own, other) > 1e-3 and relerr(mc.greens_eff(0)[1], other) > 1e-3
    for _ in range(2 * mc.p.slices + 3 if mc.N == 256 else 2 * mc.p.slices):
        mc.propagate()
        each(refs, "propagate")
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        compare(conf=False)
        mc.sweep_spatial()
        each(refs, "sweep_spatial")
        compare()
    for w, o in enumerate(refs):
        a, st = mc.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
        assert mc.uniforms_used(w) == o.uniforms_used()
    print("%s %s: worst rel |G - G_oracle| over the steps = %.3g" % (family, case, worst[0]))
    pool.shutdown()
    mc.close()


# ---- prepare, two sweeps and the four wraps from a seeded non-symmetric matrix: against the oracle and the dense twin
def _run(gpu, family, case, dense):
    out = {}
    mc = _handle(gpu, family, case, dense=dense, seed=77)
    W, n = mc.n_walkers, mc.N
    mc.prepare()
    out["G0"] = np.array([mc.greens_eff(w) for w in range(W)])
    mc.sweep(2)
    out["conf"] = np.array([mc.conf(w) for w in range(W)])
    out["G2"] = np.array([mc.greens_eff(w) for w in range(W)])
    out["counters"] = np.array([[mc.analysis(w).prop_local, mc.analysis(w).acc_local, mc.uniforms_used(w)] for w in range(W)])
    rng = np.random.default_rng(5)
    out["start"] = rng.standard_normal((W, mc.nb, n, n))
    for w in range(W):
        mc.set_greens_eff(w, list(out["start"][w]))
    for i, (sl, direction) in enumerate(WRAPS):
        mc.wrap_greens(sl, direction)
        out["W%d" % i] = np.array([mc.greens_eff(w) for w in range(W)])
    mc.close()
    return out


_factored = {}


def _factored_run(gpu, family, case):
    if (family, case) not in _factored:
        _factored[family, case] = _run(gpu, family, case, False)
    return _factored[family, case]


RECT = [fc for fc in CASES if fc[0] == "rect32x8"]


@pytest.fixture(scope="module")
def dense_rect(gpu, tmp_path_factory):
    """the dense side at 32 x 8 as test_gpu_rectangular.py computes its own: this module's _run in a fresh child process
    whose handles are created under DQMC_NO_KRON=1 (asserted there through kron_hopping()), once for the three cases"""
    path = str(tmp_path_factory.mktemp("generic") / "dense.npz")
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import __graft_entry__ as g
        gpu = g.load_package()
        import test_gpu_factored_generic as T
        res = {}
        for family, case in T.RECT:
            for k, v in T._run(gpu, family, case, True).items():
                res[case + "_" + k] = v
        np.savez(%r, **res)
        print("dense side written")
    """ % (ROOT, os.path.join(ROOT, "tests"), path))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DQMC_NO_KRON="1"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and "dense side written" in p.stdout, p.stdout + p.stderr
    return dict(np.load(path))


@pytest.mark.parametrize("family,case", CASES, ids=IDS)
def test_wraps_from_a_nonsymmetric_matrix_match_oracle(gpu, O, family, case):
    """four chained dqmc_wrap_greens calls in both directions from a seeded random matrix per block, against
    OracleDQMC.wrap_greens on the same blocks with the same HS field"""
    f = _factored_run(gpu, family, case)
    exps = _case_inputs(family, case)[0]
    n = f["start"].shape[-1]
    worst = 0.0
    for w in range(f["start"].shape[0]):
        o = O.OracleDQMC(0, _kind(case), beta=KW["beta"], delta_tau=KW["delta_tau"], safe_mult=KW["safe_mult"],
                         hopping=np.zeros((n, n)), exps=exps)
        o.set_conf(f["conf"][w])
        G = list(f["start"][w])
        for i, (sl, direction) in enumerate(WRAPS):
            G = o.wrap_greens(G, sl, direction)
            e = relerr(f["W%d" % i][w], np.array(G))
            worst = max(worst, e)
            assert e < TOL, (WRAPS[i], w, e)
    print("%s %s: worst rel |wrap - oracle| = %.3g" % (family, case, worst))


@pytest.mark.parametrize("family,case", CASES, ids=IDS)
def test_dense_twin(gpu, request, family, case):
    """the same prepare, two sweeps and four wraps on a handle created under DQMC_NO_KRON=1 (kron_hopping() False): HS
    fields and counters identical, G within 1e-10.  When a comparison with the oracle fails, this one tells a wrong
    factored path from an engine that is wrong for non-symmetric matrices on both paths."""
    f = _factored_run(gpu, family, case)
    if family == "rect32x8":
        dense = request.getfixturevalue("dense_rect")
        d = {k[len(case) + 1:]: v for k, v in dense.items() if k.startswith(case + "_")}
    else:
        d = _run(gpu, family, case, True)
    assert np.array_equal(f["conf"], d["conf"]), "HS fields differ"
    assert np.array_equal(f["counters"], d["counters"]), (f["counters"], d["counters"])
    worst = max(relerr(f[k], d[k]) for k in ["G0", "G2"] + ["W%d" % i for i in range(len(WRAPS))])
    print("%s %s: worst rel |G_factored - G_dense| = %.3g" % (family, case, worst))
    assert worst < TOL
