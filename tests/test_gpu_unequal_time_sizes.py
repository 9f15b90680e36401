"""Unequal-time Green's functions (csrc/unequal_time.inl) against oracle/unequal_time_oracle.py, entry by entry, at every
size at which a kernel under that path changes its form.  tests/test_gpu_unequal_time.py does this at n = 16 only, where
every kernel runs in its smallest, fully predicated form.  beta = 1, dtau = 0.1, safe_mult = 5 (M = 10, two stack ranges),
U = 1; the shapes (tests/unequal_time_shapes.py, each the smallest n that reaches its form):

  n     lattice            what it reaches
  64    Chain(64)          gemm_kernel<.., FULL, KSM = 0 / 1 / 2 / 3>, one tile; LDS-resident QR; block 1 of the repulsive
                           model in FULL form
  100   SquareLattice(10)  partial tiles on both edges at n <= 256
  128   Chain(128)         FULL, 2 x 2 tiles; scale_mat / set_diag / sub_identity fill their capped grid (64 x 256 threads)
  256   SquareLattice(16)  one-launch pre-pivoted UDT (every ut_udt) mixed with the pivoted UDT + rdivp of full1 / full2 on
                           one QrSet; Kronecker hopping active on the handle
  256   same, DQMC_QR_NOBLOCKED=1 around handle creation: the reference's pivot rule at 256 (cooperative QR + tail)
  257   Chain(257)         panel QR, TRSM panels 256 + 1, one-element partial GEMM tile
  320   Chain(320)         FULL forms above 256, TRSM panels 160 + 160

Scalings of the fused GEMM epilogue that only this path issues (row / column modes 4 and 5, row_first with a column
scale, alpha = -1 without ident, the conf-derived row and k scales with eTinv2) are thereby compared at all of them.
One walker for the attractive model, two for the repulsive one up to n = 128 and one above.  The misc kernels of
sweep.hip loop more than once per thread from n = 256 on (n^2 > 64 x 256; at n = 128 the grid covers the matrix exactly);
mat_add's grid is capped at 4096 x 256 threads and covers every shape here in one pass.

Bounds.  Device against oracle: |G - ref|.max() < 1e-10 max(1, |ref|.max()) (the suite's bar), stack D to rtol 1e-10
(numpy.allclose, as the n = 16 test; the worst relative deviation is printed).  The two derived bounds come from the
reference's own error, measured on the CPU by `python tests/unequal_time_shapes.py` (same expression):

  oracle's stabilised G(k,l) against brute_force_greens, pairs (0,0), (7,2), (2,7), (M,0), after prepare:
      n = 64: 9.87e-15 (both models);  n = 256: 1.63e-14 attractive, 2.15e-14 repulsive
    -> device against brute force: 10 x 2.15e-14 = 2.15e-13 (ANCHOR_BOUND)
  oracle's iterators against the oracle's own greens(k,l), walker 0, after one update_until_measure
  (GreensIterator(0, r) and CombinedGreensIterator(r) | GreensIterator(3, s)):
      n     model       r = s      r = 4 s    (3, s)
      64    attractive  1.56e-14   1.03e-13   6.88e-15
      64    repulsive   1.56e-14   2.68e-13   6.88e-15
      128   attractive  2.13e-14   8.61e-14   6.03e-15
      128   repulsive   2.23e-14   8.62e-14   1.09e-14
      256   attractive  1.55e-14   5.85e-13   4.78e-15
      256   repulsive   2.03e-14   7.86e-13   6.96e-15
    -> ten times each is below the 1e-10 bar, so the bar is the bound of every iterator step (ITERATOR_MEASURED,
       iterator_bound); the n = 16 test's fitted 2e-9 / 5e-9 for r = 4 s are not carried over.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (at import time, before the library opens the device: see tests/test_gpu_sizes.py)

import unequal_time_shapes as H
from test_gpu_sizes import TOL
from unequal_time_shapes import ANCHOR_PAIRS, PAIRS, ROW, ROWS, M, S, dist

pytestmark = pytest.mark.gpu

KINDS = ["attractive", "repulsive"]
ANCHOR_MEASURED = 2.15e-14
ANCHOR_BOUND = 10 * ANCHOR_MEASURED
# (n, kind) -> {recalculate: the oracle iterator's distance from the oracle's own greens(k, l)}, see the docstring
ITERATOR_MEASURED = {
    (64, "attractive"): {S: 1.56e-14, 4 * S: 1.03e-13, "l3": 6.88e-15},
    (64, "repulsive"): {S: 1.56e-14, 4 * S: 2.68e-13, "l3": 6.88e-15},
    (128, "attractive"): {S: 2.13e-14, 4 * S: 8.61e-14, "l3": 6.03e-15},
    (128, "repulsive"): {S: 2.23e-14, 4 * S: 8.62e-14, "l3": 1.09e-14},
    (256, "attractive"): {S: 1.55e-14, 4 * S: 5.85e-13, "l3": 4.78e-15},
    (256, "repulsive"): {S: 2.03e-14, 4 * S: 7.86e-13, "l3": 6.96e-15},
}


@pytest.fixture(scope="module")
def UT():
    from oracle import unequal_time_oracle
    return unequal_time_oracle


def iterator_bound(n, kind, recalc):
    return max(TOL, 10 * ITERATOR_MEASURED[(n, kind)][recalc])


def _handle(gpu, rid, kind, walkers=None, spec=None):
    """the device engine of one row of the table, with the dispatch facts that the row relies on"""
    _, n, rspec, env, _ = ROW[rid]
    spec = spec or rspec
    walkers = walkers or H.walkers_of(n, kind)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # kernel switches are read when a handle is created
    try:
        mc = gpu.DQMC(H.model(gpu, kind, spec), beta=H.BETA, delta_tau=H.DELTA_TAU, safe_mult=S, n_walkers=walkers,
                      seed=H.SEED)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert mc.N == n and mc.p.slices == M and mc.p.safe_mult == S and mc.n_walkers == walkers
    assert mc.kron_hopping() == (n == 256)
    assert (mc.udt_one_launch_sites() != 0) == (rid == "n256")
    return mc


_REFS = {}


def _reference(gpu, O, UT, mc, key, kind, sweeps):
    """the oracle side of one shape, model and point of the chain, built as tests/test_gpu_sizes.py::_oracles does (the
    lattice's hopping matrix, the walker's initial HS field and seed) and advanced like the device; built once and shared
    by every test that needs it.  Its HS field is compared with the device's at every use, so the field that the oracle
    was given is the handle's, and after a sweep the two chains agree bit for bit."""
    key = (key, kind, mc.n_walkers, sweeps)
    if key not in _REFS:
        confs, seeds = H.initial_confs(gpu, mc.N, mc.n_walkers)
        assert seeds == list(mc.seeds)
        _REFS[key] = H.Reference(O, UT, mc.model, kind, confs, seeds, sweeps)
    ref = _REFS[key]
    for w, o in enumerate(ref.oracles):
        assert np.array_equal(o.conf(), mc.conf(w)), "HS field of walker %d differs" % w
    return ref


def _compare_pairs(mc, ref, pairs=PAIRS):
    """calculate_greens_kl (effective) and greens_kl of every walker and block against the oracle; returns the worst"""
    worst = 0.0
    for k, l in pairs:
        g_all = mc.greens_kl(k, l)
        for w in range(mc.n_walkers):
            g_eff = mc.calculate_greens_kl(k, l, w)
            for b in range(mc.nb):
                e = max(dist(g_eff[b], ref.greens_eff(w, b, k, l)), dist(g_all[w][b], ref.greens(w, b, k, l)))
                worst = max(worst, e)
                assert e < TOL, (k, l, w, b, e)
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_greens_kl_every_entry(gpu, O, UT, rid, kind):
    """G(k,l), effective and true, for the pairs that walk every branch of ut_compute_inverse_udt_block, full1 and full2:
    after prepare, and at n = 64 and the default n = 256 also after one update_until_measure"""
    mc = _handle(gpu, rid, kind)
    mc.prepare()
    for sweeps in ((0, 1) if rid in ("n64", "n256") else (0,)):
        if sweeps:
            mc.update_until_measure()
        worst = _compare_pairs(mc, _reference(gpu, O, UT, mc, rid, kind, sweeps))
        print("%s %s, %d walkers, %d sweeps: worst |G(k,l) - G_oracle| / max(1, |G_oracle|) = %.3g"
              % (rid, kind, mc.n_walkers, sweeps, worst))
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_stacks(gpu, O, UT, rid, kind):
    """build_stack: U diag(D) T of every forward and backward slot, and D of every slot (inverse slots: D only), against
    the oracle.  D is compared where both sides use the same pivot rule: the oracle as it is for every row but the default
    n = 256, whose one-launch UDT takes the column order from the input's norms - there against the oracle's stack built
    with the same pre-sorted order (orc_set_udt_presort)."""
    mc = _handle(gpu, rid, kind)
    mc.prepare()
    ref = _reference(gpu, O, UT, mc, rid, kind, 0)
    mc.ut_build_stack()
    nr = M // S
    worst_p = worst_d = 0.0
    for w in range(mc.n_walkers):
        fwd = [mc.ut_stack("forward", idx, w) for idx in range(nr + 1)]
        bwd = [mc.ut_stack("backward", idx, w) for idx in range(nr + 1)]
        inv = [mc.ut_stack("inverse", idx, w) for idx in range(nr)]
        for b in range(mc.nb):
            ut = ref.ut[w][b]
            ut.build_stack()
            utd = ut
            if rid == "n256":
                utd = ref.fresh_ut(w, b)
                O.lib().orc_set_udt_presort(1)
                try:
                    utd.build_stack()
                finally:
                    O.lib().orc_set_udt_presort(0)
            for idx in range(nr + 1):
                for (U, D, T), ru, rd, rt, dd in ((fwd[idx], ut.fu[idx], ut.fd[idx], ut.ft[idx], utd.fd[idx]),
                                                  (bwd[idx], ut.bu[idx], ut.bd[idx], ut.bt[idx], utd.bd[idx])):
                    # U D T is the contract (UDT.jl:192-306); the factors themselves are unique up to signs
                    e = np.abs((U[b] * D[b]) @ T[b] - (ru * rd) @ rt).max() / max(1.0, rd.max())
                    worst_p = max(worst_p, e)
                    assert e < TOL, (w, b, idx, e)
                    e = np.abs(D[b] / dd - 1).max()
                    worst_d = max(worst_d, e)
                    assert np.allclose(D[b], dd, rtol=1e-10), (w, b, idx, e)
            for idx in range(nr):
                e = np.abs(inv[idx][1][b] / utd.id[idx] - 1).max()
                worst_d = max(worst_d, e)
                assert np.allclose(inv[idx][1][b], utd.id[idx], rtol=1e-10), (w, b, idx, e)
    print("%s %s stacks: worst |UDT - UDT_oracle| / max(1, D_max) = %.3g, worst |D / D_oracle - 1| = %.3g"
          % (rid, kind, worst_p, worst_d))
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rid", ["n64", "n128", "n256"])
def test_iterators(gpu, O, UT, rid, kind):
    """GreensIterator(0, r), GreensIterator(3, s) and CombinedGreensIterator(r), r = s and 4 s (the branches k % r == 0,
    k % s == 0 and the plain step, with the (U D) T products in FULL form), walker 0: every step against the device's own
    greens_kl and against the oracle's iterator; bounds from iterator_bound"""
    mc = _handle(gpu, rid, kind)
    n, w = mc.N, 0
    mc.prepare()
    mc.update_until_measure()
    ref = _reference(gpu, O, UT, mc, rid, kind, 1)
    o = ref.oracles[w]
    assert max(dist(g, g0) for g, g0 in zip(mc.greens_eff(w), o.greens_eff())) < TOL
    Gk0 = [mc.greens_kl(k, 0, w) for k in range(M + 1)]
    G0k = [mc.greens_kl(0, k, w) for k in range(M + 1)]
    Gkk = [mc.greens_kl(k, k, w) for k in range(M + 1)]
    Gk3 = [mc.greens_kl(k, 3, w) for k in range(3, M + 1)]
    worst = {"own": 0.0, "oracle": 0.0}

    def check(what, dev, own, orc, bound, at):
        for b in range(mc.nb):
            e_own, e_orc = dist(dev[b], own[b]), dist(dev[b], orc[b])
            worst["own"], worst["oracle"] = max(worst["own"], e_own), max(worst["oracle"], e_orc)
            assert e_own < bound and e_orc < bound, (what, at, b, e_own, e_orc, bound)

    for recalc in (S, 4 * S):
        bound = iterator_bound(n, kind, recalc)
        orc = list(zip(*[ref.ut[w][b].greens_iterator(0, recalc) for b in range(mc.nb)]))
        dev = list(mc.greens_iterator(0, recalc, walker=w))
        assert len(dev) == len(orc) == M + 1
        for k in range(M + 1):
            check("GreensIterator(0)", dev[k], Gk0[k], orc[k], bound, (recalc, k))
        orc = list(zip(*[ref.ut[w][b].combined_greens_iterator(o.greens_eff()[b], recalc) for b in range(mc.nb)]))
        dev = list(mc.combined_greens_iterator(recalc, walker=w))
        assert len(dev) == len(orc) == M
        for i in range(M):
            for q, (name, own) in enumerate((("G0l", G0k), ("Gl0", Gk0), ("Gll", Gkk))):
                check("Combined " + name, dev[i][q], own[i + 1], [blk[q] for blk in orc[i]], bound, (recalc, i + 1))
    orc = list(zip(*[ref.ut[w][b].greens_iterator(3, S) for b in range(mc.nb)]))
    dev = list(mc.greens_iterator(3, S, walker=w))
    assert len(dev) == len(orc) == M + 1 - 3
    for i in range(len(dev)):
        check("GreensIterator(3)", dev[i], Gk3[i], orc[i], iterator_bound(n, kind, "l3"), (S, 3 + i))
    print("%s %s iterators: worst step against the device's greens_kl = %.3g, against the oracle's iterator = %.3g"
          % (rid, kind, worst["own"], worst["oracle"]))
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_susceptibilities_8x8(gpu, O, R, UT, kind):
    """charge / spin / pairing susceptibility sums at n = 64 on SquareLattice(8) with EachLocalQuadByDistance (64
    directions, launch_sus_slice beyond one 16-site row), one walker, against the oracle's CombinedGreensIterator fed
    through the generic packed kernels (generic.jl:226-243), as tests/test_gpu_unequal_time.py does at L = 4"""
    L = 8
    mc = _handle(gpu, "n64", kind, walkers=1, spec=("square", L))
    mc.prepare()
    mc.update_until_measure()
    ref = _reference(gpu, O, UT, mc, "square8", kind, 1)
    it = gpu.EachLocalQuadByDistance(mc.model.l)
    mc.set_local_targets(it)
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=S)
    res = mc.susceptibilities()
    assert res["count"] == 1 and res["PS"].shape == (L * L, 5, 5)
    o = ref.oracles[0]
    its = [u.combined_greens_iterator(o.greens_eff()[b], S) for b, u in enumerate(ref.ut[0])]
    steps = [tuple([blk[q] for blk in per_block] for q in range(3)) for per_block in zip(*its)]
    want = R.susceptibilities(o.greens(), steps, L, kind == "attractive", 5, o.delta_tau)
    worst = 0.0
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS"):
        e = dist(res[k], want[k])
        worst = max(worst, e)
        assert e < TOL, (k, e)
    print("8x8 %s susceptibilities: worst |X - X_oracle| / max(1, |X_oracle|) = %.3g" % (kind, worst))
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rid", ["n64", "n256"])
def test_brute_force_anchor(gpu, O, UT, rid, kind):
    """device and oracle against brute_force_greens, the dense evaluation of the definition that shares no code with the
    stabilised path; bound ANCHOR_BOUND = ten times the oracle's own distance from it (measured on the CPU, docstring)"""
    mc = _handle(gpu, rid, kind, walkers=1)
    mc.prepare()
    ref = _reference(gpu, O, UT, mc, rid, kind, 0)
    worst_dev = worst_orc = 0.0
    fails = []
    for k, l in ANCHOR_PAIRS:
        g = mc.calculate_greens_kl(k, l, 0)
        for b in range(mc.nb):
            bf = UT.brute_force_greens(ref.oracles[0], b, k, l)
            e_dev, e_orc = dist(g[b], bf), dist(ref.greens_eff(0, b, k, l), bf)
            print("%s %s (%d,%d) block %d: device - brute force %.3g, oracle - brute force %.3g, device - oracle %.3g"
                  % (rid, kind, k, l, b, e_dev, e_orc, dist(g[b], ref.greens_eff(0, b, k, l))))
            worst_dev, worst_orc = max(worst_dev, e_dev), max(worst_orc, e_orc)
            if not (e_dev < ANCHOR_BOUND and e_orc < ANCHOR_BOUND):
                fails.append((k, l, b, e_dev, e_orc))
    print("%s %s anchor: worst device - brute force %.3g, oracle - brute force %.3g (bound %.3g)"
          % (rid, kind, worst_dev, worst_orc, ANCHOR_BOUND))
    assert not fails, fails
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_sweep_state_untouched_n256(gpu, kind):
    """the default n = 256 handle after stack build, G(k,l) and both iterators continues bit for bit like an equally seeded
    handle that never measured (the path owns its buffers: unequal_time.inl)"""
    mcs = [_handle(gpu, "n256", kind), _handle(gpu, "n256", kind)]
    for mc in mcs:
        mc.prepare()
        mc.update_until_measure()
    mc = mcs[0]
    mc.ut_build_stack()
    for k, l in ((7, 2), (2, 7), (M, 0), (3, 3)):
        mc.calculate_greens_kl(k, l)
        mc.greens_kl(k, l)
    for recalc in (S, 4 * S):
        assert len(list(mc.greens_iterator(0, recalc))) == M + 1
        assert len(list(mc.combined_greens_iterator(recalc))) == M
    for mc in mcs:
        mc.update_until_measure()
    assert np.array_equal(mcs[0].conf(0), mcs[1].conf(0))
    for a, b in zip(mcs[0].greens_eff(0), mcs[1].greens_eff(0)):
        assert np.array_equal(a, b)
    for mc in mcs:
        mc.close()
