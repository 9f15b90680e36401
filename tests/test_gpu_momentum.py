"""Momentum-space observables on the device (include/dqmc_hip.h "momentum-space observables"; csrc/momentum.hip): the
transform of every walker's sample against numpy, against the site positions directly, the means, reproducibility, "off
is free", the errors, sign weighting and the version-2 checkpoint.

The bound of the transform (derived, not measured): an output is one dot product of n_dirs terms, so whatever the order of
the sum and with or without FMA  |device - reference| <= 2 n_dirs 2^-53 sum_d |X[d] Tab[d, q]|  per element (the standard
gamma_n bound with a factor two of room, which also covers the one extra rounding of the delta_tau scale); 1e-300 is
allowed for exact zeros.  The reference is the same product in numpy.longdouble, from level 0 of the source section's own
binner after one push, i.e. from exactly the sample the device transformed.

Shapes, the small ones where the 64 x 64 tiling of the kernel can go wrong: 8, 9, 16 and 36 directions (36 and 9 are no
multiple of 4 or 16), n_q in {1, 3, 17, n_dirs}, one and two blocks, 1 and 3 walkers, R = 3 .. 21 rows per block, so that
no row count per walker is a multiple of 16."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402
from test_gpu_dqmc import TOL  # noqa: E402  (the device-against-oracle bound on G, 1e-10)

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
MOM = ("momentum_correlations", "momentum_susceptibilities", "momentum_time_displaced")
SRC = ("correlations", "susceptibilities", "time_displaced")
GREENS, DENSITY = 1, 2


def lattice(gpu, name):
    return {"chain8": lambda: gpu.Chain(8), "sq4": lambda: gpu.SquareLattice(4), "sq6": lambda: gpu.SquareLattice(6),
            "tri3": lambda: gpu.TriangularLattice(3)}[name]()


def handle(gpu, lat, kind, W, slices=10, n_q="all", every=None, what=GREENS | DENSITY, seed=53, first_walker=0, **kw):
    """a prepared handle at its measurement point with directions, momenta (the first n_q of the grid) and recording set"""
    l = lattice(gpu, lat)
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(l=l), beta=0.1 * slices, delta_tau=0.1, safe_mult=5, n_walkers=W, seed=seed, first_walker=first_walker, **kw)
    try:
        it = gpu.EachSitePairByDistance(l)
        mc.set_pair_directions(it)
        if n_q is not None:
            q = gpu.momentum_grid(l)[0]
            mc.set_momenta(q if n_q == "all" else q[:n_q])
        if every:
            mc.set_time_displaced(every, what)
        mc.prepare()
        mc.update_until_measure()
    except BaseException:
        mc.close()
        raise
    return mc


def one_pass(mc, sections=SRC):
    if "correlations" in sections:
        mc.accumulate_correlations()
    if "susceptibilities" in sections or "time_displaced" in sections:
        mc.accumulate_susceptibilities(recalculate=5)


def level0(mc, which, w):
    return mc.binner_level(which, w, 0)[0]


def transform_reference(mc, which, x):
    """the momentum sample of one walker from its source sample x, in longdouble -> (value, abs_sum) flat, sample order"""
    Ct, St = (t.astype(np.longdouble) for t in mc._phase_tables())
    nd = mc._ndirs

    def rows(v, tab):
        v = v.astype(np.longdouble).reshape(-1, nd)
        return (v @ tab).ravel(), (np.abs(v) @ np.abs(tab)).ravel()
    parts = []
    if which != "momentum_time_displaced":
        parts.append(rows(x[:4 * nd], Ct))
    else:
        p, B = mc.time_displaced_plan(), mc.nb
        off = 0
        if p["what"] & GREENS:
            for _ in range(2):
                g = x[off:off + B * p["rows"] * nd]
                parts += [rows(g, Ct), rows(g, St)]
                off += g.size
        if p["what"] & DENSITY:
            parts.append(rows(x[off:off + 4 * p["rows"] * nd], Ct))
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])


def assert_transform(mc, which, src, label):
    nd, worst = mc._ndirs, 0.0
    for w in range(mc.n_walkers):
        ref, ab = transform_reference(mc, which, level0(mc, src, w))
        dev = level0(mc, which, w)
        if mc.sign_weighting():
            dev = dev[:-1]
        assert dev.shape == ref.shape, (label, which, dev.shape, ref.shape)
        bound = 2 * nd * U53 * ab.astype(np.float64) + 1e-300
        err = np.abs(dev.astype(np.longdouble) - ref).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (label, which, w, float((err / bound).max()))
        assert np.abs(ref).max() > 1e-6  # (not vacuous)
    print("%s %s: largest err / bound %.3g over %d elements" % (label, which, worst, ref.size))


#        lattice   model         n_q  W  slices every what
CASES = [("chain8", "attractive", 1, 1, 10, 1, GREENS | DENSITY),
         ("chain8", "repulsive", 8, 3, 10, 5, GREENS),
         ("sq4", "attractive", 3, 3, 20, 1, DENSITY),
         ("sq4", "repulsive", 16, 1, 10, 5, GREENS | DENSITY),
         ("sq6", "attractive", 17, 3, 10, 1, GREENS | DENSITY),
         ("sq6", "repulsive", 36, 1, 20, 5, GREENS | DENSITY),
         ("tri3", "repulsive", 9, 3, 10, 1, GREENS | DENSITY),
         ("tri3", "attractive", 3, 1, 20, 5, GREENS)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-q%d-w%d-m%d-e%d-what%d" % c)
def test_transform_against_numpy(gpu, case):
    lat, kind, n_q, W, slices, every, what = case
    mc = handle(gpu, lat, kind, W, slices=slices, n_q=n_q, every=every, what=what)
    try:
        nd, B, R = mc._ndirs, mc.nb, 1 + slices // every
        assert mc.momenta_plan() == dict(n_q=n_q, n_dirs=nd, tile_rows=64, tile_cols=64)
        mc.enable_binning(SRC + MOM, capacity=7)
        E_td = ((4 * B if what & GREENS else 0) + (4 if what & DENSITY else 0)) * R * n_q
        assert [mc.binner_size(k)[0] for k in MOM] == [4 * n_q, 4 * n_q, E_td]
        one_pass(mc)
        for which, src in zip(MOM, SRC):
            assert mc.binner_size(which)[2] == 1
            assert_transform(mc, which, src, "%s %s" % (lat, kind))
    finally:
        mc.close()


def test_momentum_binner_runs_without_its_source_binner(gpu):
    """the momentum binners alone give the bits they give next to the real-space binners"""
    a = b = None
    try:
        a, b = handle(gpu, "tri3", "repulsive", 3, every=5), handle(gpu, "tri3", "repulsive", 3, every=5)
        a.enable_binning(SRC + MOM, capacity=3)
        b.enable_binning(MOM, capacity=3)
        one_pass(a)
        one_pass(b)
        for which in MOM:
            for w in range(3):
                assert np.array_equal(level0(a, which, w), level0(b, which, w)), which
    finally:
        for m in (a, b):
            if m is not None:
                m.close()


@pytest.mark.parametrize("lat,kind", [("sq4", "attractive"), ("sq4", "repulsive"), ("tri3", "repulsive"), ("tri3", "attractive")])
def test_nk_and_structure_factors_from_the_site_positions(gpu, lat, kind):
    """n(k), Im G(k, tau = 0), Sc and Sz of one configuration against numpy from mc.greens(w) and the site positions alone - no
    direction table, no minimum image: 1 - (1/N) sum_ij cos(k . (r_i - r_j)) G_ij, and the Wick expressions of
    tests/measurement_ref.py evaluated pair by pair and summed with the phase of r_i - r_j.  1e-10 relative, the project's
    device-against-oracle gate on G.  A wrong sign or order convention of the directions shows in the imaginary part."""
    mc = handle(gpu, lat, kind, 2, every=5)
    try:
        l = mc.model.l
        n, B = len(l), mc.nb
        mc.enable_binning(("momentum_correlations", "momentum_time_displaced"), capacity=3)
        G = [mc.greens(w) for w in range(2)]
        one_pass(mc)
        pos = np.array(gpu.lattices._positions(l))
        q = mc.momenta()
        dr = pos[:, None, :] - pos[None, :, :]              # r_i - r_j at [i, j]
        ph = np.einsum("ijx,qx->qij", dr, q)
        cosp, sinp = np.cos(ph), np.sin(ph)
        pair = np.arange(n * n).reshape(n, n)                # every pair its own "direction": the Wick terms pair by pair
        for w in range(2):
            td = mc._bin_shape("momentum_time_displaced", level0(mc, "momentum_time_displaced", w))
            for b in range(B):
                nk_ref = 1.0 - np.einsum("qij,ij->q", cosp, G[w][b]) / n
                im_ref = -np.einsum("qij,ij->q", sinp, G[w][b]) / n
                nk_dev, im_dev = 1.0 - td["Gl0_C"][b, 0, :], -td["Gl0_S"][b, 0, :]
                scale = max(np.abs(nk_ref).max(), np.abs(im_ref).max())
                assert np.abs(nk_dev - nk_ref).max() <= TOL * scale
                assert np.abs(im_dev - im_ref).max() <= TOL * scale
                assert np.abs(im_ref).max() > 1e-4 * scale  # (the imaginary part of one configuration is not zero)
            et = MR.equal_time(G[w], pair, n * n)
            sf = mc._bin_shape("momentum_correlations", level0(mc, "momentum_correlations", w))
            for name, key in (("Sc", "CDC"), ("Sz", "SDCz")):
                ref = np.einsum("qij,ij->q", cosp, et[key][0].reshape(n, n))
                assert np.abs(sf[name] - ref).max() <= TOL * np.abs(ref).max(), (name, w)
    finally:
        mc.close()


@pytest.mark.parametrize("lat,kind", [("sq4", "repulsive"), ("tri3", "attractive")])
def test_binner_means_agree_with_the_host_transform_of_the_accumulators(gpu, lat, kind):
    """after several sweeps with measurements the level-0 mean over the walkers equals structure_factors() and its
    siblings, the host transform of the accumulated sums.  Bound: the dot-product bound times the sample count S, with the
    mean absolute sample bounded by Cauchy-Schwarz from the source binner's own squares: sum_s |x_s| <= sqrt(S sum_s
    x_s^2), i.e.  |a - b| <= S 2 n_dirs 2^-53 sum_d sqrt(sum x^2 / S)[d] |Tab[d, q]|."""
    W, T = 3, 3
    mc = handle(gpu, lat, kind, W, every=5)
    try:
        mc.enable_binning(SRC + MOM, capacity=7)
        for s in range(T):
            if s:
                mc.update_until_measure()
            one_pass(mc)
        S, nd = W * T, mc._ndirs
        Ct, St = (np.abs(t) for t in mc._phase_tables())
        host = dict(mc.structure_factors(), **mc.static_susceptibilities())
        host.update(mc.momentum_time_displaced())
        assert host["count"] == S
        for which, src in zip(MOM, SRC):
            raw = mc.binned_raw(which)
            assert raw["count"] == T
            dev = mc._bin_shape(which, raw["mean"])
            x2 = sum(mc.binner_level(src, w, 0)[1] for w in range(W))
            rms = mc._bin_shape(src, np.sqrt(x2 / S))
            for name, v in dev.items():
                if which == "momentum_time_displaced" and name[:3] in ("Gl0", "G0l"):
                    ref = host["Gk_l0" if name[:3] == "Gl0" else "Gk_0l"]
                    ref, tab = (ref.real, Ct) if name.endswith("_C") else (-ref.imag, St)
                    a = rms[name[:3]] @ tab
                else:
                    ref, tab = host[name], Ct
                    a = rms[{"Sc": "CDC", "Sx": "SDCx", "Sy": "SDCy", "Sz": "SDCz", "chi_c": "CDS", "chi_x": "SDSx",
                             "chi_y": "SDSy", "chi_z": "SDSz"}.get(name, name[:-1])] @ tab
                bound = S * 2 * nd * U53 * a + 1e-300
                err = np.abs(v - ref)
                assert np.all(err <= bound), (which, name, float((err / bound).max()))
        b = mc.binned("momentum_time_displaced")
        assert np.allclose(b["nk"], host["nk"], rtol=0, atol=1e-12) and b["Gk_l0"].dtype.kind == "c"
        for k in ("nk_std_error", "Gk_l0_std_error_re", "Gk_l0_std_error_im", "Gk_0l_std_error_walkers_im", "CDCk_std_error",
                  "SDCzk_tau", "reliable_level", "tau", "count"):
            assert k in b, k
        c = mc.binned("momentum_correlations")
        assert set(c) >= {"Sc", "Sz", "Sz_std_error", "Sz_std_error_walkers", "Sz_tau", "reliable_level"}
        assert np.all(np.isfinite(c["Sz_std_error_walkers"])) and c["Sz"].shape == (nd,)
        assert set(mc.binned("momentum_susceptibilities")) >= {"chi_c", "chi_z_std_error"}
    finally:
        mc.close()


def test_two_passes_and_another_walker_count_give_the_same_bits(gpu):
    one = three = None
    try:
        three, one = handle(gpu, "sq6", "repulsive", 3, n_q=17, every=5), handle(gpu, "sq6", "repulsive", 1, n_q=17, every=5)
        first = {}
        for mc in (three, one):
            mc.enable_binning(MOM, capacity=3)
            one_pass(mc)
            first[mc] = {k: [level0(mc, k, w) for w in range(mc.n_walkers)] for k in MOM}
            mc.reset_accumulators()
            assert mc.binner_size(MOM[0])[2] == 0 and not level0(mc, MOM[2], 0).any()
            one_pass(mc)
            for k in MOM:
                for w in range(mc.n_walkers):
                    assert np.array_equal(level0(mc, k, w), first[mc][k][w]), "a second pass differs bitwise: " + k
        for k in MOM:
            assert np.array_equal(first[one][k][0], first[three][k][0]), "walker 0 depends on n_walkers: " + k
    finally:
        for m in (one, three):
            if m is not None:
                m.close()


def snapshot(mc):
    out = {"state": mc.state(), "reduce_size": mc.reduce_size()}
    for sec in ("greens", "correlations", "susceptibilities", "time_displaced"):
        out["acc:" + sec] = mc._section(sec)
    for sec in ("greens",) + SRC:
        E, L, T = mc.binner_size(sec)
        out["bin:" + sec] = (E, L, T, [mc.binner_level(sec, w, lv) for w in range(mc.n_walkers) for lv in range(L)])
    return out


def test_off_is_free(gpu):
    """set_momenta with no momentum binner on: state(), reduce_size(), every accumulator and every binner level are byte
    for byte those of a handle that never called it; n_q = 0 after use frees everything"""
    from montecarlo_jl_amd import _lib
    a = b = None
    try:
        a, b = handle(gpu, "sq4", "repulsive", 2, n_q=None, every=5), handle(gpu, "sq4", "repulsive", 2, n_q="all", every=5)
        assert a.momenta() is None and a.momenta_plan()["n_q"] == 0 and b.momenta_plan()["n_q"] == 16
        for mc in (a, b):
            mc.enable_binning(("greens",) + SRC, capacity=7)
            for s in range(2):
                if s:
                    mc.update_until_measure()
                mc.accumulate_greens()
                one_pass(mc)
        sa, sb = snapshot(a), snapshot(b)
        assert sa["state"].size == sb["state"].size and np.array_equal(sa["state"], sb["state"])
        assert int.from_bytes(bytes(sb["state"][8:12]), "little") == 1  # format version 1
        assert sa["reduce_size"] == sb["reduce_size"]
        for k in sa:
            if k.startswith("acc:"):
                assert np.array_equal(sa[k], sb[k]), k
            if k.startswith("bin:"):
                assert sa[k][:3] == sb[k][:3], k
                for (x1, y1, c1), (x2, y2, c2) in zip(sa[k][3], sb[k][3]):
                    assert np.array_equal(x1, x2) and np.array_equal(y1, y2) and c1 == c2, k
        # with a momentum binner on the blob is version 2, and n_q = 0 takes everything away again
        b.enable_binning("momentum_correlations", capacity=3)
        assert int.from_bytes(bytes(b.state()[8:12]), "little") == 2 and b.state_size() > sa["state"].size
        b.set_momenta(None)
        assert b.momenta() is None and b.momenta_plan() == dict(n_q=0, n_dirs=0, tile_rows=0, tile_cols=0)
        with pytest.raises(_lib.DQMCError) as e:
            b.binner_size("momentum_correlations")
        assert e.value.code == _lib.ERR_STATE
        assert np.array_equal(b.state(), sa["state"])
    finally:
        for m in (a, b):
            if m is not None:
                m.close()


def test_errors(gpu):
    from montecarlo_jl_amd import _lib
    import ctypes as C
    mc = handle(gpu, "sq4", "attractive", 1, n_q=None)
    try:
        lib = _lib.lib()
        for k in MOM:  # before set_momenta
            with pytest.raises(_lib.DQMCError) as e:
                mc.enable_binning(k, capacity=3)
            assert e.value.code == _lib.ERR_STATE and "dqmc_set_momenta" in str(e.value)
        q = gpu.momentum_grid(mc.model.l)[0]
        mc.set_momenta(q[:3])
        with pytest.raises(_lib.DQMCError) as e:  # before set_time_displaced
            mc.enable_binning("momentum_time_displaced", capacity=3)
        assert e.value.code == _lib.ERR_STATE and "dqmc_set_time_displaced" in str(e.value)
        # n_q > n_dirs, a negative n_q and NULL tables: DQMC_ERR_INVALID, and the handle keeps its setting
        big = np.zeros(16 * 17)
        assert lib.dqmc_set_momenta(mc._h, 17, _lib.dptr(big), _lib.dptr(big)) == _lib.ERR_INVALID
        assert lib.dqmc_set_momenta(mc._h, -1, _lib.dptr(big), _lib.dptr(big)) == _lib.ERR_INVALID
        assert lib.dqmc_set_momenta(mc._h, 2, None, _lib.dptr(big)) == _lib.ERR_INVALID
        assert mc.momenta_plan()["n_q"] == 3
        # the capacity: refused before anything is accumulated
        mc.enable_binning("momentum_correlations", capacity=1)
        mc.accumulate_correlations()
        before = mc.correlations_raw()
        with pytest.raises(_lib.DQMCError) as e:
            mc.accumulate_correlations()
        assert e.value.code == _lib.ERR_STATE and "capacity" in str(e.value)
        assert np.array_equal(mc.correlations_raw(), before) and mc.binner_size("momentum_correlations")[2] == 1
        # set_time_displaced disables the time-displaced momentum binner, set_momenta all of them
        mc.set_time_displaced(5, ("greens",))
        mc.enable_binning("momentum_time_displaced", capacity=3)
        mc.set_time_displaced(1, ("greens",))
        assert lib.dqmc_binner_size(mc._h, _lib.BIN_MOMENTUM["momentum_time_displaced"], None, None, None) == _lib.ERR_STATE
        assert mc.binner_size("momentum_correlations")[0] == 12
        mc.set_momenta(q[:2])
        assert lib.dqmc_binner_size(mc._h, _lib.BIN_MOMENTUM["momentum_correlations"], None, None, None) == _lib.ERR_STATE
        # a new direction table turns momenta off
        mc.set_pair_directions(gpu.EachSitePairByDistance(mc.model.l))
        assert mc.momenta_plan()["n_q"] == 0 and mc.momenta() is None
        # and without directions there are no momenta
        fresh = gpu.DQMC(gpu.HubbardModelAttractive(l=gpu.Chain(8)), beta=1.0, n_walkers=1)
        try:
            one = np.ones(8)
            assert lib.dqmc_set_momenta(fresh._h, 1, _lib.dptr(one), _lib.dptr(one)) == _lib.ERR_STATE
            assert b"dqmc_set_pair_directions" in lib.dqmc_last_error(fresh._h)
        finally:
            fresh.close()
    finally:
        mc.close()


def test_sign_weighting(gpu):
    """the repulsive model on TriangularLattice(3) with weighting on: the sample has E + 1 elements, the last is s_w, the
    others are the transform of the source binner's signed sample; binned() gives finite ratio errors from 3 walkers"""
    mc = handle(gpu, "tri3", "repulsive", 3, every=5, sign_weighting=True)
    try:
        n_q, R = 9, 3
        mc.enable_binning(SRC + MOM, capacity=7)
        assert [mc.binner_size(k)[0] for k in MOM] == [4 * n_q + 1, 4 * n_q + 1, 12 * R * n_q + 1]
        sg = mc.sign()
        one_pass(mc)
        for which, src in zip(MOM, SRC):
            for w in range(3):
                assert level0(mc, which, w)[-1] == sg[w] and sg[w] in (-1, 1)
            assert_transform(mc, which, src, "signed tri3")
        for s in range(3):
            mc.update_until_measure()
            one_pass(mc)
        b = mc.binned("momentum_correlations")
        host = mc.structure_factors()
        for k in ("Sc", "Sx", "Sy", "Sz"):
            assert np.all(np.isfinite(b[k + "_std_error"])) and b[k].shape == (n_q,)
            assert np.allclose(b[k], host[k], rtol=1e-12, atol=1e-13)
        assert "s" not in b
        # turning the weighting off again re-creates the binners, empty, without the trailing s
        mc.reset_accumulators()
        mc.set_sign_weighting(False)
        assert [mc.binner_size(k)[::2] for k in MOM] == [(4 * n_q, 0), (4 * n_q, 0), (12 * R * n_q, 0)]
        one_pass(mc)
        assert_transform(mc, "momentum_time_displaced", "time_displaced", "unsigned tri3")
    finally:
        mc.close()


def run_object(gpu, n_q="all"):
    m = gpu.HubbardModelAttractive(l=gpu.SquareLattice(4), U=1.0, mu=0.3)
    mc = gpu.DQMC(m, n_walkers=2, beta=1.0, delta_tau=0.1, safe_mult=5, seed=31, thermalization=2, sweeps=4, measure_rate=1)
    mc.set_pair_directions(gpu.EachSitePairByDistance(m.l))
    q = gpu.momentum_grid(m.l)[0]
    mc.set_momenta(q if n_q == "all" else q[:n_q])
    mc.set_time_displaced(5)
    return mc


def binner_state(mc):
    out = {}
    for k in MOM:
        E, L, T = mc.binner_size(k)
        out[k] = (E, L, T, [mc.binner_level(k, w, lv)[:2] for w in range(mc.n_walkers) for lv in range(L)])
    return out


def test_run_with_checkpoints_and_resume(gpu, tmp_path):
    """run(checkpoint=...) at 4 x 4 with the three momentum binners on (run(binning=True) enables them because momenta are
    set): after DQMC.load every momentum binner level and the push counts are exactly what they were at the save; the
    continued run matches the uninterrupted one as test_gpu_checkpoint.py asks of resumed runs (TOL per sample); a
    version-2 blob is refused by a handle with another n_q, which names the field and stays as it was"""
    from montecarlo_jl_amd import _lib, checkpoint
    p, p4 = tmp_path / "run.ckpt", tmp_path / "at4.ckpt"
    meas = ("correlations", "susceptibilities", "time_displaced")
    saved = {}
    a = b = c = None

    def look(mc, i):
        if i == 4:
            saved.update(binner_state(mc))  # (the sweep's save comes behind its measurements)
        if i == 5:
            shutil.copy(p, p4)
    try:
        a = run_object(gpu)
        a.run(measurements=meas, binning=True, on_measure=look, checkpoint=p, checkpoint_every=2)
        pre, blob = checkpoint.read(p4)
        assert pre["last_sweep"] == 4 and set(MOM) <= set(pre["binning"]["sections"]) and len(pre["momenta"]["q"]) == 16
        assert int.from_bytes(bytes(blob[8:12]), "little") == 2
        b = gpu.DQMC.load(p4)
        assert np.array_equal(b.momenta(), a.momenta())
        got = binner_state(b)
        for k in MOM:
            assert got[k][:3] == saved[k][:3] and got[k][2] == 2, k
            for (x1, y1), (x2, y2) in zip(got[k][3], saved[k][3]):
                assert np.array_equal(x1, x2) and np.array_equal(y1, y2), k
        b.run(measurements=meas, binning=True)
        assert b.last_sweep == 6
        for w in range(2):
            assert np.array_equal(b.conf(w), a.conf(w)) and b.uniforms_used(w) == a.uniforms_used(w)
        for k in MOM:
            assert b.binner_size(k) == a.binner_size(k) and a.binner_size(k)[2] == 4
            for w in range(2):
                xa, xb = level0(a, k, w), level0(b, k, w)
                cnt = 4
                assert np.abs(xa - xb).max() <= TOL * cnt * max(1.0, np.abs(xa).max() / cnt), k
        # another n_q on the importing side
        c = run_object(gpu, n_q=3)
        c.prepare()
        c.update_until_measure()
        c.enable_binning(meas + MOM)
        before = c.state()
        with pytest.raises(_lib.DQMCError) as e:
            c.set_state(blob)
        assert e.value.code == _lib.ERR_INVALID and "n_q" in str(e.value)
        assert np.array_equal(c.state(), before)
    finally:
        for m in (a, b, c):
            if m is not None:
                m.close()
