"""The imaginary-time current recording on the device (include/dqmc_hip.h "current response in imaginary time";
csrc/current_tau.hip, current_tau.inl, the hooks in unequal_time.inl), through the ABI: every row against numpy, the sum
rule against current_response(), free fermions against the closed form, "nothing else moves", signs, and the contract.

Shapes (10 slices, safe_mult 5, 1 - 5 walkers; every case a few seconds): 4 x 4 both models with every = 1, 2, 5; 6 x 6
(36 directions, off the 64 grid) with one momentum and with all 36; TriangularLattice(5) (K_cc = 7, a non-orthogonal
reciprocal basis); 9 x 9 with all 81 momenta (a second 64-wide momentum tile); 6 x 6 with holes in a K = 9 target table,
which takes the pair-list form of the cc kernels.

Bounds.  Rows: the bound tests/test_gpu_measurement_sizes.py applies to the ccs section, |device - reference| <= 2 (P + 16)
eps abs_sum per element, P the number of terms summed into the element and abs_sum the sum of their absolute values: a
row element sums the quads of all directions of one k, each times a phase factor, so P = sum_d quads(d, k) + n_dirs (the
contraction's own terms) and abs_sum = sum_d |phase| abs_sum_x[d].  Sum rule: 1e-12 of the largest magnitude (both sides
are fp64 sums of at most slices n_dirs terms of that size).  Free fermions: the bound of tests/test_gpu_response.py at
U = 0, 2 C Gmax EPS_G with C = n_dirs 2 4 t^2 the absolute weight of one row (no delta_tau sum), EPS_G = 2.31e-13 the
device's allowance per element of G there (same beta, delta_tau, safe_mult).  Everything else is bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import current_tau_ref as CT  # noqa: E402
import lattice_tables as LT  # noqa: E402
import response_ref as R  # noqa: E402
from test_gpu_dqmc import TOL  # noqa: E402  (the device-against-oracle bound on G, 1e-10)
from test_gpu_measurement_sizes import holes  # noqa: E402
from test_gpu_response import EPS_G, U52  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SAFE_MULT = 5
RESP = ("response_pairing", "response_pairing_susceptibility", "response_current")
_tables = {}


def tables(gpu, lat):
    """(lattice, fast_pairs) built once per lattice name"""
    if lat not in _tables:
        l = {"sq4": lambda: gpu.SquareLattice(4), "sq6": lambda: gpu.SquareLattice(6), "sq9": lambda: gpu.SquareLattice(9),
             "tri5": lambda: gpu.TriangularLattice(5)}[lat]()
        _tables[lat] = (l, LT.fast_pairs(l))
    return _tables[lat]


def handle(gpu, lat, kind, W, n_q=5, every=None, trg=None, U=1.0, mu=0.0, beta=1.0, seed=83, signed=False, local=False):
    """a handle at its measurement point with current targets and momenta (n_q: a count taken from the grid behind q = 0,
    or "all"), recording every `every` slices"""
    l, fp = tables(gpu, lat)
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(l=l, U=U, mu=mu), beta=beta, delta_tau=0.1, safe_mult=SAFE_MULT, n_walkers=W, seed=seed, sign_weighting=signed)
    try:
        cur = LT.QuadTables(fp, LT.fast_quads(l, pairs=fp).trg_of if trg is None else trg, synced=True)
        if local:  # (set_local_targets sets the pair directions; setting them again would drop nothing but costs a call)
            mc.set_local_targets(LT.QuadTables(fp, LT.fast_quads(l, pairs=fp).trg_of))
            mc._set_current_targets(cur.trg_of, cur.K, None)
        else:
            mc.set_current_targets(cur)
        q = gpu.momentum_grid(l)[0]
        mc.set_momenta(q if n_q == "all" else q[:n_q])
        if local:
            mc.set_pair_channels("default")
        mc.prepare()
        mc.update_until_measure()
        if every:
            mc.set_current_time_displaced(every)
    except BaseException:
        mc.close()
        raise
    return mc


def read_pass(gpu, mc):
    """one CombinedGreensIterator pass: steps[w] = [(G0l, Gl0, Gll), ...] of every walker, per-block matrices"""
    lib = gpu.lib()
    steps = [[] for _ in range(mc.n_walkers)]
    mc._c(lib.dqmc_combined_iterator_begin(mc._h, SAFE_MULT))
    l = C.c_int32()
    while True:
        mc._c(lib.dqmc_combined_iterator_next(mc._h, C.byref(l)))
        if l.value < 0:
            return steps
        for w in range(mc.n_walkers):
            steps[w].append(tuple(mc._ut_result(i, w) for i in range(3)))


def split(mc, raw):
    """[W, P] -> C, S [W, R, K, n_q], kbond [W, K], tail [W, 3]"""
    p = mc.current_time_displaced_plan()
    R_, K, nq = p["R"], p["K_cc"], p["n_q"]
    n = R_ * K * nq
    assert raw.shape == (mc.n_walkers, 2 * n + K + 3)
    return (raw[:, :n].reshape((-1, R_, K, nq)), raw[:, n:2 * n].reshape((-1, R_, K, nq)), raw[:, 2 * n:2 * n + K], raw[:, 2 * n + K:])


def hopping(mc):
    return [mc._cc_T[b * mc.N ** 2:(b + 1) * mc.N ** 2].reshape((mc.N, mc.N), order="F") for b in range(mc.nb)]


#         lattice kind          W  n_q    every  punched
ROWS = [("sq4", "attractive", 3, 5, 1, False), ("sq4", "attractive", 3, 5, 2, False), ("sq4", "attractive", 3, 5, 5, False),
        ("sq4", "repulsive", 3, 5, 1, False), ("sq4", "repulsive", 3, 5, 2, False), ("sq4", "repulsive", 3, 5, 5, False),
        ("sq6", "repulsive", 2, 1, 5, False), ("sq6", "attractive", 2, "all", 2, False),
        ("tri5", "repulsive", 2, 5, 2, False), ("sq9", "attractive", 2, "all", 5, False),
        ("sq6", "repulsive", 2, 5, 1, True), ("sq6", "attractive", 2, 5, 2, True)]


@pytest.mark.parametrize("case", ROWS, ids=lambda c: "%s-%s-w%d-q%s-e%d-%s" % (c[:5] + ("holes" if c[5] else "full",)))
def test_rows_against_numpy(gpu, case):
    lat, kind, W, n_q, every, punched = case
    l, fp = tables(gpu, lat)
    trg = holes(LT.fast_quads(l, 9, pairs=fp).trg_of, 3) if punched else None
    mc = handle(gpu, lat, kind, W, n_q=n_q, every=every, trg=trg)
    try:
        fast = C.c_int32(-1)
        mc._c(gpu.lib().dqmc_current_targets_fast_path(mc._h, C.byref(fast)))
        assert fast.value == (0 if punched else 1)  # holes in a K = 9 table: the pair-list form of the cc kernels
        trg_cc, nd, dir_of = mc._tables["current_targets"][0], fp.ndirections(), fp.dir_of
        K = trg_cc.shape[1]
        assert K == {"sq4": 5, "sq6": 9 if punched else 5, "sq9": 5, "tri5": 7}[lat]
        Ct, St = mc._phase_tables()
        nq, M = Ct.shape[1], mc.p.slices
        assert M == 10 and mc.current_time_displaced_plan() == dict(R=1 + M // every, every=every, K_cc=K, n_q=nq)
        mc.enable_binning(("response_current",), capacity=3)
        mc.reset_accumulators()
        G = [mc.greens(w) for w in range(W)]
        steps = read_pass(gpu, mc)
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        Cd, Sd, kb, tail = split(mc, mc._current_tau_raw())
        assert np.array_equal(tail, np.tile([1.0, 1.0, 0.0], (W, 1)))
        T, P = hopping(mc), CT.terms(dir_of, nd, trg_cc)[:, None]
        worst = 0.0
        for w in range(W):
            for r in range(1 + M // every):
                tup = CT.row0_tuple(G[w]) if r == 0 else (G[w],) + steps[w][r * every - 1]
                Cr, Sr, Ca, Sa, _ = CT.row(T, *tup, dir_of, nd, trg_cc, Ct, St)
                for name, dev, ref, ab in (("C", Cd[w, r], Cr, Ca), ("S", Sd[w, r], Sr, Sa)):
                    bound = 2.0 * (P + 16.0) * EPS * ab
                    err = np.abs(dev - ref)
                    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (case, name, w, r, ratio, err.max())
                    assert bound.max() <= 1e-9 * np.abs(Cr).max(), (case, "vacuous bound")
                assert np.abs(Cr).max() > 1e-3
            # kbond: the bits of DQMC_BIN_RESPONSE_CURRENT's, and numpy's value within that test's bound
            lv0 = mc.binner_level("response_current", w, 0)[0]
            assert np.array_equal(kb[w], lv0[2 * K * nq:2 * K * nq + K])
            ref, kab, knt = R.bond_kinetic(G[w], T, trg_cc)
            g = np.concatenate([np.abs(x).ravel() for x in G[w]]).max()
            wsum = np.array([(2.0 if mc.nb == 1 else 1.0) * sum(np.abs(Tb[trg_cc[trg_cc[:, k] >= 0, k], np.nonzero(trg_cc[:, k] >= 0)[0]]).sum()
                                                                 for Tb in T) / mc.N for k in range(K)])
            assert np.all(np.abs(kb[w] - ref.astype(np.float64)) <= knt * U52 * kab.astype(np.float64) + TOL * g * wsum + 1e-300)
        print("%s: largest err / bound %.3g" % (case, worst))
    finally:
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_sum_rule(gpu, kind):
    """every = 1: delta_tau times the sum of the rows r >= 1 is the transform of the ccs sums of the same pass"""
    mc = handle(gpu, "sq4", kind, 3, n_q="all", every=1)
    try:
        mc.reset_accumulators()
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        td, cr = mc.current_time_displaced(), mc.current_response()
        assert td["count"] == cr["count"] == 3 and td["left_out"] == 0 and td["tau"].shape == (11,)
        mine = -mc.p.delta_tau * (td["Lambda_cos"][1:].sum(axis=0) - 1j * td["Lambda_sin"][1:].sum(axis=0))
        assert np.abs(mine - cr["Lambda"]).max() <= 1e-12 * np.abs(cr["Lambda"]).max()
        assert np.abs(cr["Lambda"]).max() > 1e-2 and td["Lambda_cos_std_error"].shape == (11, 5, 16)
    finally:
        mc.close()


@pytest.mark.parametrize("lat,kind,mu", [("sq4", "attractive", 0.0), ("sq6", "repulsive", 0.3)])
def test_free_fermions(gpu, lat, kind, mu):
    """U = 0: every row against the closed form (route 1 of tests/response_ref.py); the q = 0 current commutes with H, so
    its diagonal rows are constant in tau and D / pi = -k_axis at every Matsubara index"""
    beta, every = 2.0, 2
    mc = handle(gpu, lat, kind, 3, n_q="all", every=every, U=0.0, mu=mu, beta=beta)
    try:
        l = mc.model.l
        ff, _loc, cur = R.free_fermions(gpu, l, beta, 0.1, mu=mu)
        assert np.array_equal(cur.trg_of, mc._tables["current_targets"][0]) and np.allclose(ff.q, mc.momenta())
        mc.reset_accumulators()
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        td = mc.current_time_displaced()
        nd, K, Rr = ff.nd, cur.K, 1 + 20 // every
        tol = 2 * (nd * 2 * 4 * 1.0) * 1.0 * EPS_G
        for r in range(Rr):
            g00, g0l, gl0, gll = ff.matrices(r * every)
            x = R.MR.cc_step([ff.T], [g00], [g0l], [gl0], [gll], ff.dir_of, nd, cur.trg_of)[0]
            assert np.abs(td["Lambda_cos"][r] + x.T @ ff.Ct).max() <= tol, (r, np.abs(td["Lambda_cos"][r] + x.T @ ff.Ct).max())
            assert np.abs(td["Lambda_sin"][r] + x.T @ ff.St).max() <= tol
        i0 = next(i for i in range(len(ff.q)) if np.allclose(ff.q[i], 0.0))
        diag = td["Lambda_cos"][:, :, i0]
        assert np.abs(diag - diag[0]).max() <= 2 * tol and diag[0, 1:].min() > 1e-2  # constant in tau, and not 0
        assert np.abs(td["kbond"] - R.bond_kinetic([ff.matrices(0)[0]], [ff.T], cur.trg_of)[0].astype(float)).max() <= 2 * max(1.0, abs(mu)) * EPS_G
        dw = mc.drude_weight(0, m=(1, 2, 3))
        assert dw["D_over_pi_m"].shape == (3,) and -dw["k_axis"] > 0.1
        assert np.abs(dw["D_over_pi_m"] + dw["k_axis"]).max() <= 2 * beta * tol  # (the trapezoid sum of deviations <= 2 tol)
        assert np.abs(dw["D_over_pi_m_std_error"]).max() <= 2 * beta * tol      # every walker gives the same value
        dc = mc.dc_conductivity(0)
        kp = mc._axis_bonds(0)[0]
        assert abs(dc["sigma_dc"] - beta ** 2 / np.pi * diag[0, kp]) <= beta ** 2 / np.pi * 2 * tol
    finally:
        mc.close()


def test_nothing_else_moves(gpu):
    """two handles with the same seeds, one recording: everything but the recording is bit for bit the same; a second
    pass adds the same bits; walker 0 does not depend on n_walkers"""
    on = off = one = None
    try:
        on, off = (handle(gpu, "sq6", "repulsive", 3, every=e, local=True) for e in (2, None))
        one = handle(gpu, "sq6", "repulsive", 1, every=2, local=True)
        assert off.current_time_displaced_plan() == dict(R=0, every=0, K_cc=0, n_q=0)
        size = C.c_size_t(7)
        off._c(gpu.lib().dqmc_current_time_displaced_size(off._h, C.byref(size)))
        assert size.value == 0
        for m in (on, off, one):
            m.enable_binning(("susceptibilities",) + RESP, capacity=3)
            m.reset_accumulators()
            m.accumulate_pairing()
            m.accumulate_susceptibilities(recalculate=SAFE_MULT)
        first = on._current_tau_raw()
        assert np.abs(first).max() > 1e-3
        assert np.array_equal(on._section("susceptibilities"), off._section("susceptibilities"))
        for k in ("susceptibilities",) + RESP:
            for w in range(3):
                for a, b in zip(on.binner_level(k, w, 0), off.binner_level(k, w, 0)):
                    assert np.array_equal(a, b), (k, w)
        for w in range(3):
            assert np.stack(on.greens_eff(w)).tobytes() == np.stack(off.greens_eff(w)).tobytes()
            assert np.array_equal(on.conf(w), off.conf(w)) and on.uniforms_used(w) == off.uniforms_used(w)
        assert on.state().tobytes() == off.state().tobytes()  # accumulators, binners, fields, cursors: one blob
        assert np.array_equal(one._current_tau_raw()[0], first[0]), "walker 0 depends on n_walkers"
        on.accumulate_susceptibilities(recalculate=SAFE_MULT)
        assert np.array_equal(on._current_tau_raw(), 2.0 * first), "a second pass differs bitwise"
    finally:
        for m in (on, off, one):
            if m is not None:
                m.close()


def test_signs(gpu):
    """repulsive 4 x 4, five walkers with the signs + - 0 + + imposed: rows are s_w x, the zero-sign walker is left out"""
    units = np.array([[1, 1], [-1, 1], [0, 1], [1, 1], [-1, -1]])
    s = units.prod(axis=1)
    assert s.tolist() == [1, -1, 0, 1, 1] and s.sum() != 0 and all(s.sum() - v != 0 for v in s)
    mc = twin = None
    try:
        mc, twin = (handle(gpu, "sq4", "repulsive", 5, every=2, U=4.0, signed=sg) for sg in (True, False))
        mc.impose_unit_signs(units)
        assert np.array_equal(mc.sign(), s)
        for m in (mc, twin):
            m.reset_accumulators()
            m.accumulate_susceptibilities(recalculate=SAFE_MULT)
        raw, x = mc._current_tau_raw(), twin._current_tau_raw()
        E = raw.shape[1] - 3
        for w in range(5):
            assert np.array_equal(raw[w, :E], s[w] * x[w, :E] if s[w] else np.zeros(E)), w
            assert raw[w, E:].tolist() == ([s[w], 1, 0] if s[w] else [0, 0, 1])
        assert np.abs(x[2, :E]).max() > 1e-3
        td = mc.current_time_displaced()
        assert td["count"] == 4 and td["left_out"] == 1
        val, err = CT.jackknife(raw[:, :E], raw[:, E])
        p = mc.current_time_displaced_plan()
        n = p["R"] * p["K_cc"] * p["n_q"]
        for name, got, ref in (("Lambda_cos", td["Lambda_cos"].ravel(), -val[:n]), ("Lambda_sin", td["Lambda_sin"].ravel(), -val[n:2 * n]),
                               ("kbond", td["kbond"], val[2 * n:])):
            assert np.abs(got - ref).max() <= 1e-13 * np.abs(val).max(), name
        assert np.abs(td["Lambda_cos_std_error"].ravel() - err[:n]).max() <= 1e-13 * err.max() and err.min() >= 0 and err.max() > 0
        assert np.abs(td["kbond_std_error"] - err[2 * n:]).max() <= 1e-13 * err.max()
        # s and -s cancel: the same error as signed()
        mc.reset_accumulators()
        mc.impose_unit_signs(np.array([[1, 1], [-1, 1], [0, 1], [1, 1], [1, -1]]))
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        with pytest.raises(ValueError, match="sum of signs is 0"):
            mc.current_time_displaced()
    finally:
        for m in (mc, twin):
            if m is not None:
                m.close()


def test_contract(gpu, tmp_path):
    from montecarlo_jl_amd import _lib, checkpoint as ckpt
    lib = gpu.lib()
    l, fp = tables(gpu, "sq4")
    quads = LT.QuadTables(fp, LT.fast_quads(l, pairs=fp).trg_of, synced=True)
    q = gpu.momentum_grid(l)[0]
    mc = gpu.DQMC(gpu.HubbardModelAttractive(l=l), beta=1.0, delta_tau=0.1, safe_mult=SAFE_MULT, n_walkers=2, seed=5)
    a = b = c = None
    try:
        call = lambda every: lib.dqmc_set_current_time_displaced(mc._h, every)
        plan = mc.current_time_displaced_plan
        off = dict(R=0, every=0, K_cc=0, n_q=0)
        # the prerequisites, one after the other
        for step, need in ((lambda: mc.set_pair_directions(fp), b"dqmc_set_pair_directions"),
                           (lambda: mc.set_current_targets(quads), b"dqmc_set_current_targets"),
                           (lambda: mc.set_momenta(q[:3]), b"dqmc_set_momenta"),
                           (lambda: (mc.prepare(), mc.update_until_measure()), b"dqmc_prepare")):
            assert call(1) == _lib.ERR_STATE and need in lib.dqmc_last_error(mc._h) and plan() == off
            step()
        assert call(0) == _lib.OK and plan() == off
        mc.set_current_time_displaced(2)
        assert plan() == dict(R=6, every=2, K_cc=5, n_q=3)
        for bad in (-1, 3, 4, 20):  # 10 slices
            assert call(bad) == _lib.ERR_INVALID and plan()["every"] == 2
        with pytest.raises(gpu.DQMCError) as e:
            mc.set_current_time_displaced(7)
        assert e.value.code == _lib.ERR_INVALID and mc._ctd == 2
        size = C.c_size_t()
        mc._c(lib.dqmc_current_time_displaced_size(mc._h, C.byref(size)))
        assert size.value == 2 * (2 * 6 * 5 * 3 + 5 + 3)
        assert not mc._current_tau_raw().any()
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        assert mc._current_tau_raw().any()
        with pytest.raises(ValueError, match="not a recorded row"):  # slice 5 of 10, every 2
            mc.dc_conductivity(0)
        with pytest.raises(ValueError, match="n_max"):
            mc.current_matsubara(3)
        assert mc.current_matsubara()["Lambda"].shape == (3, 5, 3) and abs(mc.current_matsubara()["omega"][1] - 2 * np.pi) < 1e-12
        mc.reset_accumulators()
        assert not mc._current_tau_raw().any()
        mc.set_current_time_displaced(5)
        assert "sigma_dc_std_error" in _pass(mc).dc_conductivity(0)
        # a successful call zeroes the sums; the three setters turn the recording off
        mc.set_current_time_displaced(5)
        assert not mc._current_tau_raw().any()
        for setter in (lambda: mc.set_momenta(q[:3]), lambda: mc.set_current_targets(quads), lambda: mc.set_pair_directions(fp)):
            mc.set_momenta(q[:3]), mc.set_current_targets(quads), mc.set_momenta(q[:3])
            mc.set_current_time_displaced(1)
            assert plan()["every"] == 1
            setter()
            assert plan() == off and mc._ctd == 0
            assert lib.dqmc_get_current_time_displaced(mc._h, None) == _lib.ERR_STATE
        # ---- checkpoint: the sums go through the preamble, the blob is that of a handle without the recording
        a, b = (handle(gpu, "sq4", "repulsive", 2, every=e, seed=9) for e in (5, None))
        for m in (a, b):
            m.reset_accumulators()
            _pass(m)
        path = str(tmp_path / "ctd.ckpt")
        a.save(path)
        pre, blob = ckpt.read(path)
        assert pre["current_time_displaced"]["every"] == 5
        assert bytes(blob) == b.state().tobytes() and int.from_bytes(bytes(blob)[8:12], "little") == int.from_bytes(b.state().tobytes()[8:12], "little")
        pb = str(tmp_path / "plain.ckpt")
        b.save(pb)
        assert "current_time_displaced" not in ckpt.read(pb)[0]
        c = gpu.DQMC.load(path)
        assert c.current_time_displaced_plan() == a.current_time_displaced_plan() and c._ctd == 5
        assert np.array_equal(c._current_tau_raw(), a._current_tau_raw()) and a._current_tau_raw().any()
        assert c.state().tobytes() == a.state().tobytes()
        bad = a._current_tau_raw().copy()
        bad[1, -1] = 0.5
        assert lib.dqmc_set_current_time_displaced_sums(a._h, _lib.dptr(np.ascontiguousarray(bad.ravel()))) == _lib.ERR_INVALID
    finally:
        for m in (mc, a, b, c):
            if m is not None:
                m.close()


def _pass(mc):
    mc.accumulate_greens()
    mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
    return mc
