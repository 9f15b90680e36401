"""Scalar thermodynamics on the device (csrc/thermo.hip, thermo.inl): every walker's ten-element sample against the
numpy restatement (tests/thermo_ref.py) of include/dqmc_hip.h's table on the same Green's function, at the sizes where the
kernel's tile loops change shape; bit reproducibility; the doped repulsive model against the CPU oracle; means against
exact diagonalisation; and the section's way through binner, sign weighting, reduction, checkpoint and run()."""
import ctypes as C
import os

import numpy as np
import pytest

import thermo_ref as TR
from conftest import relerr

pytestmark = pytest.mark.gpu
NE = 10
# device against host, relative to max(1, |value|): the project's bar; the worst-case rounding of the largest sum here,
# n^2 = 331 776 products of O(1) in fp64, is about 4e-11
TOL = 1e-10


def lattice(gpu, name):
    return {"2x2": lambda: gpu.SquareLattice(2), "6x6": lambda: gpu.SquareLattice(6), "chain33": lambda: gpu.Chain(33),
            "16x16": lambda: gpu.SquareLattice(16), "24x24": lambda: gpu.SquareLattice(24),
            "tri4": lambda: gpu.TriangularLattice(4), "tri10": lambda: gpu.TriangularLattice(10),
            "cubic3": lambda: gpu.CubicLattice(3, 3), "cubic5": lambda: gpu.CubicLattice(3, 5),
            "chain64": lambda: gpu.Chain(64), "chain65": lambda: gpu.Chain(65), "chain128": lambda: gpu.Chain(128),
            "chain129": lambda: gpu.Chain(129)}[name]()


def make(gpu, name, kind, W, seed=77, U=1.0, **kw):
    l = lattice(gpu, name) if isinstance(name, str) else name
    model = gpu.HubbardModelAttractive(l=l, U=U, mu=0.5) if kind == "attractive" else gpu.HubbardModelRepulsive(l=l, U=U, mu=0.4)
    return gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=W, seed=seed, **kw)


def u_s(mc):
    return mc.model.U if mc.model.kind == 1 else -mc.model.U


def one_sample(mc, updates=2):
    """prepare, `updates` updates, one accumulate with the binner on -> [W, E] level-0 sums = the samples"""
    mc.set_thermodynamics()
    mc.enable_binning("thermodynamics", capacity=3)
    mc.prepare()
    for _ in range(updates):
        mc.update()
    mc.accumulate_thermodynamics()
    return np.stack([mc.binner_level("thermodynamics", w, 0)[0] for w in range(mc.n_walkers)])


# off-diagonal non-zeros per row of the hopping matrix on the lattices whose neighbour list is not the square lattice's
NEIGHBOURS = {"tri4": 6, "tri10": 6, "cubic3": 6, "cubic5": 6, "chain64": 2, "chain65": 2, "chain128": 2, "chain129": 2}
SAMPLE_CASES = [(name, kind, W) for name in ("2x2", "6x6", "chain33", "16x16", "24x24") for kind in ("attractive", "repulsive")
                for W in (1, 3)]
SAMPLE_CASES += [(name, kind, W) for name in NEIGHBOURS for kind in ("attractive", "repulsive")
                 for W in ((1, 3) if name in ("chain65", "tri10") else (1,))]


@pytest.mark.parametrize("name,kind,W", SAMPLE_CASES)
def test_samples_equal_numpy_on_the_same_greens_function(gpu, name, kind, W):
    """n = 4 (below a wavefront), 36 (no multiple of 16, one partial tile), 33 (odd), 256 (4 x 4 full tiles), 576 (9 x 9
    tiles, more than one per lane stride of the diagonal loop); one and three walkers; both models, doped.  The
    triangular (n = 16, 100) and cubic (n = 27, 125) lattices: six neighbours per row, non-bipartite, and at cubic L = 3
    the periodic images at distance 1; the exact tile edges n = 64, 65, 128, 129 on chains."""
    mc = make(gpu, name, kind, W)
    if name in NEIGHBOURS:  # (a degenerate lattice would make the bond sum trivial)
        for t in mc.model.hopping_matrix():
            assert np.all(np.count_nonzero(t - np.diag(np.diag(t)), axis=1) == NEIGHBOURS[name]), name
    x = one_sample(mc)
    assert x.shape == (W, NE)
    T = mc.model.hopping_matrix()
    for w in range(W):
        ref = TR.thermo_ref(mc.greens(w), T, u_s(mc))
        for k, a, b in zip(TR.FIELDS, x[w], ref):
            print(name, kind, W, w, k, a, b, abs(a - b) / max(1.0, abs(b)))
            assert abs(a - b) <= TOL * max(1.0, abs(b)), (name, kind, w, k, a, b)
    raw = mc._section("thermodynamics")
    assert raw.shape == (NE + 2,) and raw[NE] == W and raw[NE + 1] == W
    tot = np.zeros(NE)
    for w in range(W):  # the kernel's order
        tot = tot + x[w]
    assert np.array_equal(raw[:NE], tot)
    if name == "16x16":  # the doped exponentials are still Kronecker products: the factored path is kept
        assert mc.kron_hopping()
    mc.close()


@pytest.mark.parametrize("name,kind", [("6x6", "repulsive"), ("chain33", "attractive"), ("16x16", "repulsive")])
def test_walker_sample_is_bit_reproducible_and_independent_of_the_walker_count(gpu, name, kind):
    runs = []
    for W in (1, 3, 3):
        mc = make(gpu, name, kind, W)
        x = one_sample(mc)
        runs.append((x[0].copy(), [g.copy() for g in mc.greens(0)]))
        mc.close()
    for x, G in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(G, runs[0][1])), "the Green's function itself differs"
        assert x.tobytes() == runs[0][0].tobytes()


def test_doped_repulsive_model_follows_the_oracle(gpu, O):
    """4x4, U = 4, mu = 0.5, beta = 1, two walkers: the oracle created with the doped exponentials; after prepare and 12
    updates the HS fields are identical and G agrees within the sweep tests' 1e-10"""
    model = gpu.HubbardModelRepulsive(4, 2, U=4.0, mu=0.5)
    mc = gpu.DQMC(model, beta=1.0, n_walkers=2, seed=123)
    refs = []
    for w in range(2):
        o = O.OracleDQMC(4, "repulsive", beta=1.0, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=4.0,
                         hopping=np.asfortranarray(model.hopping_matrix()[0]))
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    assert np.array_equal(np.diag(refs[0].T), np.full(16, -0.5))
    mc.prepare()
    for o in refs:
        o.prepare()
    for _ in range(12):
        mc.update()
        for o in refs:
            o.update()
    for w, o in enumerate(refs):
        assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
        for b, (g, g0) in enumerate(zip(mc.greens_eff(w), o.greens_eff())):
            assert relerr(g, g0) < 1e-10, (w, b, relerr(g, g0))
    mc.close()


def ed_bounds(G, T, U_s, ed):
    """The reference's bound on a mean Green's element against ED, d = 2 dtau^2 = 0.02, propagated to first order through
    each scalar's formula (G, n from ED; N sites):
      n_up, n_dn  (1/N) sum_i d                                   = d
      n           2 d
      D           (1/N) sum_i (n_up,i + n_dn,i) d                 = d n
      m2 = n - 2D 2 d + 2 d n
      E_kin       d (1/N) sum_s sum_{i != j} |T_ij|
      E_int       |U_s| (d n + d)          (D and n/2)
      E           E_kin's + d (1/N) sum_s sum_i |T_ii| + E_int's
      N2          (1/N) [ 2 |N_tot| 2 N d + sum_s (N d + 2 d sum_ij |G_ij|) ]
      Mz2         (1/N) [ 2 |M_z| 2 N d + the same second term ]"""
    d, N = 0.02, G[0].shape[0]
    n = ed[2]
    off = sum(np.abs(t - np.diag(np.diag(t))).sum() for t in T) / N
    dia = sum(np.abs(np.diag(t)).sum() for t in T) / N
    wick = sum(N * d + 2 * d * np.abs(g).sum() for g in G)
    e_int = abs(U_s) * (d * n + d)
    return np.array([d, d, 2 * d, d * n, 2 * d + 2 * d * n, d * off, e_int, d * off + d * dia + e_int,
                     (2 * abs(N * n) * 2 * N * d + wick) / N, (2 * abs(N * (ed[0] - ed[1])) * 2 * N * d + wick) / N])


@pytest.mark.parametrize("kind", ["repulsive", "attractive"])
def test_means_against_exact_diagonalisation(gpu, O, R, kind):
    """The setup of test_ed_known_answer_on_gpu (2x2, U = 1, beta = 1, dtau = 0.1, safe_mult 5, 64 walkers, 100 + 150
    sweeps, measure_rate 1): the repulsive model at mu = 0.5 with sign weighting, the attractive one at mu = 1"""
    N, beta = 4, 1.0
    if kind == "repulsive":
        model, mu, U_s = gpu.HubbardModelRepulsive(2, 2, U=1.0, mu=0.5), 0.5, 1.0
    else:
        model, mu, U_s = gpu.HubbardModelAttractive(2, 2, U=1.0, mu=1.0), 1.0, -1.0
    mc = gpu.DQMC(model, beta=beta, safe_mult=5, n_walkers=64, seed=2024, thermalization=100, sweeps=150, measure_rate=1,
                  sign_weighting=kind == "repulsive")
    mc.set_thermodynamics()
    mc.run(measurements=("thermodynamics",), binning=True)
    res = mc.signed("thermodynamics") if kind == "repulsive" else mc.thermodynamics()
    assert res["count"] == 64 * 150
    assert mc.mean_sign("thermodynamics") > 0.5
    neighs = O.square_neighs(2)
    rho, c, cd = R.ed_hubbard_greens(neighs, N, U_s, 1.0, mu, beta, return_state=True)
    ed = TR.ed_thermo(rho, c, cd, neighs, N, U_s, 1.0, mu)
    T = model.hopping_matrix()
    if len(T) == 1:
        T = [T[0], T[0]]
    assert np.array_equal(T[0], TR.hopping_from_neighs(neighs, N, 1.0, mu))
    bound = ed_bounds(TR.ed_greens_blocks(rho, c, cd, N), T, U_s, ed)
    for k, e, b in zip(TR.FIELDS, ed, bound):
        print(kind, k, res[k], e, abs(res[k] - e), b, res.get(k + "_std_error"))
        assert np.isfinite(res[k]) and abs(res[k] - e) <= b, (kind, k, res[k], e, b)
    for k, e in zip(("kappa", "chi_s"), TR.derived(ed, beta, N)):
        err = res[k + "_std_error"]
        print(kind, k, res[k], e, abs(res[k] - e), err)
        assert np.isfinite(res[k]) and np.isfinite(err) and abs(res[k] - e) <= 5 * err, (kind, k, res[k], e, err)
    mc.close()


def test_binner_means_errors_and_sign_on_off(gpu):
    """attractive 4x4, three walkers, 5 samples: the binner's means are the accumulator's, std_error_walkers is numpy's
    standard error over the per-walker means, and with the sign (+1 by construction) on every number is the same"""
    out = []
    for sign in (False, True):
        mc = make(gpu, gpu.SquareLattice(4), "attractive", 3, sign_weighting=sign)
        mc.set_thermodynamics()
        mc.enable_binning("thermodynamics", capacity=7)
        assert mc.binner_size("thermodynamics")[0] == NE + (1 if sign else 0)
        mc.prepare()
        for _ in range(5):
            mc.update_until_measure()
            mc.accumulate_thermodynamics()
        raw = mc._section("thermodynamics")
        assert raw[NE] == 15 and raw[NE + 1] == 15
        lv0 = np.stack([mc.binner_level("thermodynamics", w, 0)[0] for w in range(3)])
        b = mc.binned("thermodynamics")
        th = mc.thermodynamics()
        per_walker = lv0[:, :NE] / 5
        for i, k in enumerate(TR.FIELDS):
            assert abs(b[k] - raw[i] / 15) <= 1e-13 * max(1.0, abs(b[k])), k
            assert th[k] == raw[i] / 15
            sew = per_walker[:, i].std(ddof=1) / np.sqrt(3)
            assert abs(b[k + "_std_error_walkers"] - sew) <= 1e-12 * max(1.0, sew) + 1e-9 * sew, (k, b[k + "_std_error_walkers"], sew)
            assert th[k + "_std_error"] >= 0
        assert b["count"] == 5 and "s" not in b
        k_, c_ = TR.derived(raw[:NE] / 15, 1.0, 16)
        assert th["kappa"] == k_ and th["chi_s"] == c_ and th["count"] == 15 and th["mean_sign"] == 1.0
        if sign:
            assert np.array_equal(lv0[:, NE], np.full(3, 5.0))
            sg = mc.signed("thermodynamics")
            assert all(sg[k] == th[k] for k in TR.FIELDS)
        out.append((raw.copy(), lv0[:, :NE].copy()))
        # reset zeroes the section and its binner
        mc.reset_accumulators()
        assert not mc._section("thermodynamics").any() and mc.binner_size("thermodynamics")[2] == 0
        mc.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_sign_weighted_sums_are_the_signed_samples(gpu):
    """repulsive, doped: sums = sum_w s_w x_w, the sum of signs inside the section, the DQMC_RED_SIGN section untouched"""
    mc = make(gpu, gpu.SquareLattice(4), "repulsive", 3, U=6.0, sign_weighting=True)
    x = one_sample(mc, updates=4)
    assert x.shape == (3, NE + 1)
    s = mc.sign().astype(float)
    assert np.array_equal(x[:, NE], s)
    T = mc.model.hopping_matrix()
    tot = np.zeros(NE)
    for w in range(3):
        ref = s[w] * TR.thermo_ref(mc.greens(w), T, u_s(mc))
        assert np.all(np.abs(x[w, :NE] - ref) <= TOL * np.maximum(1.0, np.abs(ref)))
        tot = tot + x[w, :NE]
    raw = mc._section("thermodynamics")
    assert np.array_equal(raw[:NE], tot) and raw[NE] == s.sum() and raw[NE + 1] == 3
    assert not mc._section("sign").any() and mc._section("sign").shape == (5,)
    # signed and unsigned sums never mix
    with pytest.raises(gpu.DQMCError) as e:
        mc.set_sign_weighting(False)
    assert e.value.code == -4
    mc.reset_accumulators()
    mc.set_sign_weighting(False)
    assert mc.binner_size("thermodynamics")[0] == NE  # made again, empty, without the sign element
    mc.accumulate_thermodynamics()
    assert mc._section("thermodynamics")[NE] == 3
    mc.close()


def test_reduce_on_one_rank_returns_the_local_sums(gpu):
    for sign in (False, True):
        mc = make(gpu, gpu.SquareLattice(4), "repulsive", 2, sign_weighting=sign)
        n0 = mc.reduce_size()
        mc.set_thermodynamics()
        assert mc.reduce_size() == n0 + NE + 2
        mc.prepare()
        mc.accumulate_greens()
        mc.accumulate_thermodynamics()
        mc.accumulate_thermodynamics()
        mc.reduce()
        raw = mc._section("thermodynamics")
        assert raw[NE + 1] == 4 and np.array_equal(mc.reduced("thermodynamics"), raw)
        assert np.array_equal(mc.reduced("greens"), mc.accumulators())
        if sign:
            assert np.array_equal(mc.reduced("sign"), mc._section("sign"))
        mc.set_thermodynamics(False)
        assert mc.reduce_size() == n0
        with pytest.raises(gpu.DQMCError) as e:
            mc.reduced("thermodynamics")
        assert e.value.code == -4
        mc.close()


def test_call_order_and_bad_matrices(gpu):
    mc = make(gpu, gpu.Chain(66), "attractive", 1)
    mc.prepare()
    lib, h = gpu.lib(), mc._h
    assert lib.dqmc_accumulate_thermodynamics(h) == -4  # ERR_STATE before dqmc_set_thermodynamics
    with pytest.raises(gpu.DQMCError) as e:
        mc.enable_binning("thermodynamics")
    assert e.value.code == -4
    n = C.c_size_t(9)
    assert lib.dqmc_thermodynamics_size(h, C.byref(n)) == 0 and n.value == 0
    mc.set_thermodynamics()
    mc.accumulate_thermodynamics()
    before = mc._section("thermodynamics")
    dense = np.ones((66, 66))  # 65 off-diagonal non-zeros in every row
    with pytest.raises(gpu.DQMCError) as e:
        mc.set_thermodynamics(hopping=dense)
    assert e.value.code == -1 and "64" in str(e.value)
    bad = mc.model.hopping_matrix()[0].copy()
    bad[3, 4] = np.nan
    with pytest.raises(gpu.DQMCError) as e:
        mc.set_thermodynamics(hopping=bad)
    assert e.value.code == -1
    assert np.array_equal(mc._section("thermodynamics"), before)  # a refused call leaves the handle as it was
    band = np.zeros((66, 66))  # exactly 64 off-diagonal non-zeros per row: taken
    for i in range(66):
        for k in range(1, 33):
            band[i, (i + k) % 66] = band[i, (i - k) % 66] = -0.01 * k
    mc.set_thermodynamics(hopping=band)
    mc.enable_binning("thermodynamics", capacity=1)
    mc.accumulate_thermodynamics()
    x = mc.binner_level("thermodynamics", 0, 0)[0]
    ref = TR.thermo_ref(mc.greens(0), [band], u_s(mc))
    assert np.all(np.abs(x - ref) <= TOL * np.maximum(1.0, np.abs(ref)))
    with pytest.raises(gpu.DQMCError) as e:  # the binner is full: refused before anything is accumulated
        mc.accumulate_thermodynamics()
    assert e.value.code == -4 and mc._section("thermodynamics")[NE + 1] == 1
    mc.close()


def version_of(blob):
    return int(np.frombuffer(blob[8:12].tobytes(), dtype="<u4")[0])


def test_checkpointed_run_restores_the_section(gpu, tmp_path):
    """run(checkpoint=...) with the section and its binner, sign weighting on; load() gives back the sums, the sum of
    signs, the count and every binner level exactly, and goes on"""
    path = str(tmp_path / "thermo.ckpt")
    model = gpu.HubbardModelRepulsive(4, 2, U=4.0, mu=0.4)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=3, seed=5, thermalization=2, sweeps=6, measure_rate=1,
                  sign_weighting=True)
    mc.set_thermodynamics()
    mc.run(measurements=("greens", "thermodynamics"), binning=True, checkpoint=path, checkpoint_every=4)
    raw = mc._section("thermodynamics")
    assert raw[NE + 1] == 18
    E, L, T = mc.binner_size("thermodynamics")
    assert (E, T) == (NE + 1, 6)
    levels = [[mc.binner_level("thermodynamics", w, l) for l in range(L)] for w in range(3)]
    back = gpu.DQMC.load(path)
    assert back.model.mu == 0.4 and back.last_sweep == 8
    assert np.array_equal(back._section("thermodynamics"), raw)
    assert back.binner_size("thermodynamics") == (E, L, T)
    for w in range(3):
        for l in range(L):
            a, b = back.binner_level("thermodynamics", w, l), levels[w][l]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(back.accumulators(), mc.accumulators())
    assert back.thermodynamics()["E"] == mc.thermodynamics()["E"]
    # the file's state goes on: one more sample
    back.update_until_measure()
    back.accumulate_thermodynamics()
    assert back._section("thermodynamics")[NE + 1] == 21
    back.close()
    mc.close()


def test_blob_versions_and_refusals(gpu):
    """Without the section the blob is the version-1 (or, with a momentum binner, version-2) blob of before, with it
    version 3 (4); a blob goes only into a handle configured the same way, and the refusal names the field"""
    def fresh(thermo, momenta=False):
        mc = make(gpu, gpu.SquareLattice(4), "repulsive", 2, seed=3)
        if momenta:
            mc.set_pair_directions(gpu.EachSitePairByDistance(mc.model.l))
            mc.set_momenta([(0, 0), (2, 2)])
            mc.enable_binning("momentum_correlations", capacity=3)
        if thermo:
            mc.set_thermodynamics()
        mc.prepare()
        mc.update_until_measure()
        return mc
    for momenta in (False, True):
        plain, with_t = fresh(False, momenta), fresh(True, momenta)
        b0 = plain.state()
        assert version_of(b0) == (2 if momenta else 1)
        with_t.accumulate_thermodynamics()
        b1 = with_t.state()
        assert version_of(b1) == (4 if momenta else 3)
        assert b1.size == b0.size + 64 + (NE + 2) * 8 + 8
        # the front part is the old blob but for the version field and the header's checksum (bytes 8..12, 552..560)
        same = b0 == b1[:b0.size]
        same[8:12] = same[552:560] = True
        assert same.all()
        # switched off again: the old bytes, all of them
        with_t.set_thermodynamics(False)
        assert np.array_equal(with_t.state(), b0)
        with pytest.raises(gpu.DQMCError) as e:
            plain.set_state(b1)
        assert e.value.code == -1 and "section thermodynamics n" in str(e.value)
        with_t.set_thermodynamics()
        with pytest.raises(gpu.DQMCError) as e:
            with_t.set_state(b0)
        assert e.value.code == -1 and "section thermodynamics n" in str(e.value)
        # another hopping matrix is another configuration
        T = [t.copy() for t in with_t.model.hopping_matrix()]
        T[1][0, 0] += 0.25
        with_t.set_thermodynamics(hopping=T)
        with pytest.raises(gpu.DQMCError) as e:
            with_t.set_state(b1)
        assert e.value.code == -1 and "hopping matrix" in str(e.value)
        with_t.set_thermodynamics()
        with_t.set_state(b1)
        assert with_t._section("thermodynamics")[NE + 1] == 2
        # a binner on one side only
        with_t.enable_binning("thermodynamics", capacity=3)
        with pytest.raises(gpu.DQMCError) as e:
            with_t.set_state(b1)
        assert e.value.code == -1 and "binner thermodynamics on" in str(e.value)
        plain.close()
        with_t.close()
