"""current_current_susceptibility on the device (CCS section of dqmc_accumulate_susceptibilities) against the numpy
restatement of cc_kernel (tests/cc_reference.py) summed over the oracle's CombinedGreensIterator, and against exact
diagonalisation statistically (test/ED/ED_tests.jl:100-140,353-366)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_reference as CC  # noqa: E402
from test_gpu_unequal_time import _pair  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def UT():
    from oracle import unequal_time_oracle
    return unequal_time_oracle


def _oracle_ccs(oracles, it, T, attractive, recalc, UT):
    ref = None
    for o in oracles:
        uts = [UT.UnequalTimeOracle(o, b) for b in range(o.nb)]
        its = [u.combined_greens_iterator(o.greens_eff()[b], recalc) for b, u in enumerate(uts)]
        steps = [tuple([blk[q] for blk in per_block] for q in range(3)) for per_block in zip(*its)]
        r = CC.current_current_susceptibility(o.greens(), steps, T, it, attractive, o.delta_tau)
        ref = r if ref is None else ref + r
    return ref / len(oracles)


def _relerr(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
@pytest.mark.parametrize("K", [4, 5, 9])
@pytest.mark.parametrize("mult", [1, 4])
def test_ccs_against_oracle(gpu, O, UT, kind, K, mult):
    mc, oracles = _pair(gpu, O, kind, walkers=2)
    recalc = mult * mc.p.safe_mult
    it = gpu.EachLocalQuadBySyncedDistance(mc.model.l, K)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))
    mc.set_current_targets(it)
    assert mc.current_targets_fast_path() == (K <= 8)  # K = 9: the general kernel
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=recalc)
    res = mc.susceptibilities()
    assert res["count"] == 2 and res["CCS"].shape == (16, K) and res["PS"].shape == (16, 5, 5)
    ref = _oracle_ccs(oracles, it, mc.model.hopping_matrix(), kind == "attractive", recalc, UT)
    # recalculate = 4 safe_mult: both CombinedGreensIterators drift by ~1e-9 (test_iterators), so does the sum
    assert _relerr(res["CCS"], ref) < (1e-10 if mult == 1 else 1e-8), _relerr(res["CCS"], ref)
    # a second sample adds up; reset clears
    mc.accumulate_susceptibilities(recalculate=recalc)
    r2 = mc.susceptibilities()
    assert r2["count"] == 4 and np.abs(r2["CCS"] - res["CCS"]).max() < 1e-12 * max(1.0, np.abs(ref).max())
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=recalc)
    assert mc.susceptibilities()["count"] == 2
    mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_other_susceptibilities_unchanged(gpu, O, kind):
    """the same chain with and without current targets: CDS, SDS and PS are bit-identical"""
    out = []
    for with_cc in (False, True):
        mc, _ = _pair(gpu, O, kind, walkers=2)
        mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))
        if with_cc:
            mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(mc.model.l))
        mc.reset_accumulators()
        mc.accumulate_susceptibilities()
        out.append(mc.susceptibilities())
        mc.close()
    assert "CCS" not in out[0] and "CCS" in out[1]
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS", "count"):
        assert np.array_equal(out[0][k], out[1][k]), k


def test_ccs_full_size(gpu, O, UT):
    """n = 256: 16x16 attractive, beta = 2, K = 5 (the LDS path at the config-3 lattice)"""
    mc, oracles = _pair(gpu, O, "attractive", L=16, beta=2.0, walkers=2, safe_mult=10)
    it = gpu.EachLocalQuadBySyncedDistance(mc.model.l, 5)
    mc.set_current_targets(it)
    assert mc.current_targets_fast_path()
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=mc.p.safe_mult)
    res = mc.susceptibilities()
    ref = _oracle_ccs(oracles, it, mc.model.hopping_matrix(), True, mc.p.safe_mult, UT)
    assert res["CCS"].shape == (256, 5)
    assert _relerr(res["CCS"], ref) < 1e-10, _relerr(res["CCS"], ref)
    mc.close()


def _sus_section(mc, buf):
    n = C.c_size_t()
    mc._c(mc_lib().dqmc_susceptibilities_size(mc._h, C.byref(n)))
    return buf[-(10 + n.value):-10]


def mc_lib():
    import __graft_entry__ as g
    return g.load_package().lib()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_ccs_reduction(gpu, kind):
    model = lambda: (gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive)(4, 2)

    def run(walkers, first):
        mc = gpu.DQMC(model(), beta=1.0, safe_mult=5, n_walkers=walkers, seed=9, first_walker=first)
        mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))
        mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(mc.model.l))
        mc.prepare()
        mc.update_until_measure()
        mc.reset_accumulators()
        mc.accumulate_susceptibilities()
        return mc

    a, b, full = run(2, 0), run(2, 2), run(4, 0)
    sa, sb, sf = (_sus_section(m, m.reduce_export()) for m in (a, b, full))
    assert np.abs(sa + sb - sf).max() < 1e-12 * max(1.0, np.abs(sf).max())
    # reduce(None) carries the section; the last entries are the CCS block and the count
    full.reduce(None)
    red = full.reduced("susceptibilities")
    n = C.c_size_t()
    full._c(mc_lib().dqmc_susceptibilities_size(full._h, C.byref(n)))
    raw = np.zeros(n.value)
    full._c(mc_lib().dqmc_get_susceptibilities(full._h, raw.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.array_equal(red, raw) and np.array_equal(red, sf)
    assert raw.size == 4 * 16 + 16 * 25 + 16 * 5 + 1
    # two identical runs are bit-identical
    again = run(4, 0)
    assert np.array_equal(_sus_section(again, again.reduce_export()), sf)
    for m in (a, b, full, again):
        m.close()


def test_set_current_targets_errors(gpu):
    lib = mc_lib()
    mc = gpu.DQMC(gpu.HubbardModelAttractive(4, 2), beta=1.0, n_walkers=1)
    it = gpu.EachLocalQuadBySyncedDistance(mc.model.l)
    T = np.ascontiguousarray(mc.model.hopping_matrix()[0].reshape(-1, order="F"))
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))

    def call(tab, K, Tptr):
        t = np.asfortranarray(tab.astype(np.int32))
        return lib.dqmc_set_current_targets(mc._h, t.ctypes.data_as(C.POINTER(C.c_int32)), K, Tptr)

    assert call(it.trg_of, 5, Tp) == -4                   # no pair directions yet: DQMC_ERR_STATE
    mc.set_pair_directions(it.pairs_by_dir)
    assert call(it.trg_of, 0, Tp) == -1                   # K < 1
    big = np.zeros((16, 17), dtype=np.int32)
    assert call(big, 17, Tp) == -1                        # K > n_dirs
    bad = it.trg_of.copy(); bad[3, 1] = 16
    assert call(bad, 5, Tp) == -1                         # target out of range
    bad[3, 1] = -2
    assert call(bad, 5, Tp) == -1
    assert call(it.trg_of, 5, None) == -1                 # NULL T
    assert call(it.trg_of, 5, Tp) == 0
    mc.close()


def _ed_ccs(O, R, kind, U, mu, beta, dtau, it):
    """ED_CCS / N of ED_tests.jl:353-366: sum over the synced quads of the Riemann sum over
    tau = beta, beta - dtau, ..., dtau of <J1(tau) J2(0)> times dtau, divided by N"""
    L, N = 2, 4
    neighs = O.square_neighs(L)
    Ued = -U if kind == "attractive" else U
    rho, c, cd = R.ed_hubbard_greens(neighs, N, Ued, 1.0, mu, beta, return_state=True)
    T1 = np.zeros((N, N))
    for src in range(N):
        for trg in neighs[:, src] - 1:
            T1[trg, src] -= 1.0
    H = np.zeros_like(rho)
    Id = np.eye(rho.shape[0])
    for s_ in range(2):
        for src in range(N):
            for trg in neighs[:, src] - 1:
                H -= cd[N * s_ + trg] @ c[N * s_ + src]
    for i in range(N):
        nu, nd_ = cd[i] @ c[i], cd[N + i] @ c[N + i]
        H += Ued * (nu - 0.5 * Id) @ (nd_ - 0.5 * Id) - mu * (nu + nd_)
    w, V = np.linalg.eigh(H)

    def J(src, trg):
        out = np.zeros_like(rho)
        for s_ in range(2):
            a, b = N * s_ + src, N * s_ + trg
            out += T1[trg, src] * cd[b] @ c[a] - T1[src, trg] * cd[a] @ c[b]
        return V.T @ out @ V  # eigenbasis

    p = np.exp(-beta * (w - w.min()))
    p /= p.sum()
    ed = np.zeros(it.ndirections()[0] * it.K)
    taus = [beta - m * dtau for m in range(int(round(beta / dtau)))]
    cache = {}
    for lin, s1, t1, s2, t2 in it:
        key = (s1, t1, s2, t2)
        if key not in cache:
            A, B = J(s1 - 1, t1 - 1), J(s2 - 1, t2 - 1)
            v = 0.0
            for tau in taus:  # tr(rho e^{tau H} A e^{-tau H} B) in the eigenbasis
                E = np.exp(tau * (w[:, None] - w[None, :]))
                v += dtau * np.sum(p[:, None] * E * A * B.T)
            cache[key] = v
        ed[lin - 1] += cache[key]
    return ed.reshape(it.ndirections(), order="F") / N


@pytest.mark.parametrize("kind,U,mu", [("repulsive", 1.0, 0.0), ("attractive", 1.0, 1.0)])
def test_ccs_against_ed_statistically(gpu, O, R, kind, U, mu):
    beta, dtau = 1.0, 0.1
    if kind == "attractive":
        model = gpu.HubbardModelAttractive(2, 2, U=U, mu=mu)
    else:
        model = gpu.HubbardModelRepulsive(2, 2, U=U)
    mc = gpu.DQMC(model, beta=beta, delta_tau=dtau, safe_mult=5, n_walkers=128, seed=77,
                  thermalization=200, sweeps=400, measure_rate=2)
    it = gpu.EachLocalQuadBySyncedDistance(model.l, 4)
    mc.set_current_targets(it)
    snaps = []
    mc.run(measurements=("susceptibilities",),
           on_measure=lambda m, i: snaps.append(m.susceptibilities()["CCS"] * m.susceptibilities()["count"]))
    sums = np.array(snaps)
    per = np.diff(np.concatenate([np.zeros((1,) + sums.shape[1:]), sums]), axis=0) / mc.n_walkers
    bins = per.reshape((20, -1) + per.shape[1:]).mean(axis=1)
    mean, se = bins.mean(axis=0), bins.std(axis=0, ddof=1) / np.sqrt(len(bins))
    ed = _ed_ccs(O, R, kind, U, mu, beta, dtau, it)
    tol = 2 * dtau ** 2
    assert np.all(np.abs(mean - ed) <= tol + tol * np.abs(ed) + 4.5 * se), np.abs(mean - ed).max()
    mc.close()


def test_isa_budget_of_the_current_current_kernels():
    from test_isa_guard import _load_shipped, _runs_and_flat
    shipped = _load_shipped()
    names = [n for n in shipped if "(" in n and any(f in n for f in ("cc_b_kernel", "cc_lds_kernel", "cc_fold_kernel",
                                                                        "cc_pairs_kernel"))]
    assert len(names) == 4, names
    for n in names:
        run, flat = _runs_and_flat(shipped[n])
        assert run <= 1 and flat == 0, (n[:60], run, flat)
