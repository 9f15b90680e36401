"""The classical MC flavor on the MI355X (ising.hip): bit-exact against the oracle's orc_ising_run and a sequential
restatement of sweep(mc) (MC.jl:316-333, IsingModel.jl:85-101) on every lattice family, independent of the batch and of
how a run is split, and right in distribution against exact enumeration and the reference's golden run
(test/integration_tests.jl:1-26)."""
import ctypes as C
import math

import numpy as np
import pytest

from golden_stats import Z

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "acc_local", "prop_local", "uniforms_used",
               "energy", "magnetization")


def _stats(mc, w):
    st = mc.stats(w)
    return {f: getattr(st, f) for f in STAT_FIELDS}


def restate(O, l, beta, seed, therm, sweeps, rate=1, conf=None):
    """sweep(mc) + run!'s measurement rule, site by site, from the walker's Philox stream and the host's exp"""
    N = len(l)
    neighs = np.asarray(l.neighs) - 1
    bonds = np.asarray(l.bonds)[:, :2] - 1
    u = O.philox_uniforms(seed, N * (therm + sweeps + 1))
    draw = 0
    if conf is None:
        c = np.where(u[:N] < 0.5, -1, 1).astype(np.int64)
        draw = N
    else:
        c = np.asarray(conf, dtype=np.int64).copy()
    E = -int(np.sum(c[bonds[:, 0]] * c[bonds[:, 1]]))
    r = dict(sum_E=0.0, sum_E2=0.0, sum_absM=0.0, sum_M2=0.0, n_meas=0, acc_local=0, prop_local=0)
    nb = [list(neighs[:, i]) for i in range(N)]
    for sw in range(1, therm + sweeps + 1):
        for i in range(N):
            dE = 2.0 * c[i] * sum(int(c[j]) for j in nb[i])
            r["prop_local"] += 1
            if dE <= 0 or u[draw] < math.exp(-beta * dE):
                E += int(dE)
                c[i] = -c[i]
                r["acc_local"] += 1
            if dE > 0:
                draw += 1
        if sw > therm and sw % rate == 0:
            M = abs(int(c.sum()))
            r["sum_E"] += E
            r["sum_E2"] += float(E) * E
            r["sum_absM"] += M
            r["sum_M2"] += float(M) * M
            r["n_meas"] += 1
    r.update(uniforms_used=draw, energy=E, magnetization=int(c.sum()))
    return r, c


def test_square_8x8_matches_the_oracle_bit_exactly(gpu, O):
    W, seed, therm, sweeps = 100, 4242, 10, 300
    betas = np.linspace(0.2, 0.6, W)
    model = gpu.IsingModel(dims=2, L=8)
    mc = gpu.MC(model, beta=betas, n_walkers=W, seed=seed, thermalization=therm, sweeps=sweeps)
    for n in (37, 150, 123):
        mc.sweep(n)
    assert mc.last_sweep == therm + sweeps
    for w in range(W):
        o = O.ising_run(8, float(betas[w]), therm, sweeps, seed + w)
        st = mc.stats(w)
        assert (st.sum_E, st.sum_E2, st.sum_absM, st.sum_M2) == (o.E, o.E2, o.M, o.M2), w
        assert (st.n_meas, st.acc_local, st.prop_local) == (o.n_meas, o.accepted, o.proposed), w
    # the conf_io path: a configuration set from the host, the stream keyed afresh (cursor at 0)
    rng = np.random.default_rng(7)
    confs = [(2 * rng.integers(0, 2, 64) - 1).astype(np.int8) for _ in range(W)]
    mc2 = gpu.MC(model, beta=betas, n_walkers=W, seed=0, thermalization=therm, sweeps=sweeps)
    for w in range(W):
        mc2.set_conf(w, confs[w])
        mc2.seed(w, 9000 + w)
    for n in (101, 9, 200):
        mc2.sweep(n)
    for w in (0, 1, 63, 64, 99):
        ref, c_ref = restate(O, model.l, float(betas[w]), 9000 + w, therm, sweeps, conf=confs[w])
        assert mc2.uniforms_used(w) == ref["uniforms_used"], w
    for w in range(W):
        buf = confs[w].copy()
        res = O.IsingResult()
        O.lib().orc_ising_run(8, float(betas[w]), therm, sweeps, 9000 + w, buf.ctypes.data_as(C.c_void_p),
                              C.byref(res))
        st = mc2.stats(w)
        assert (st.sum_E, st.sum_E2, st.sum_absM, st.sum_M2) == (res.E, res.E2, res.M, res.M2), w
        assert (st.n_meas, st.acc_local, st.prop_local) == (res.n_meas, res.accepted, res.proposed), w
        assert np.array_equal(mc2.conf(w), buf), w
    mc.close()
    mc2.close()


@pytest.mark.parametrize("name,make", [
    ("chain10", lambda g: g.Chain(10)),
    ("cubic4", lambda g: g.CubicLattice(3, 4)),
    ("cubic6", lambda g: g.CubicLattice(3, 6)),
    ("triangular4", lambda g: g.TriangularLattice(4)),
    ("triangular6", lambda g: g.TriangularLattice(6)),
])
def test_other_lattices_match_the_restatement_bit_exactly(gpu, O, name, make):
    l = make(gpu)
    therm, sweeps, rate, seed = 5, 25, 3, 777
    betas = [0.15, 0.3, 0.55]
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=3, seed=seed, thermalization=therm, sweeps=sweeps,
                measure_rate=rate)
    mc.sweep(11)
    mc.sweep(therm + sweeps - 11)
    for w, b in enumerate(betas):
        ref, c = restate(O, l, b, seed + w, therm, sweeps, rate)
        assert _stats(mc, w) == ref, (name, w)
        assert np.array_equal(mc.conf(w), c), (name, w)
    mc.close()


def test_results_do_not_depend_on_the_batch_or_the_split(gpu):
    """walker k of a 16384-walker handle (sweeps split into several launches by the work bound) equals a 1-walker
    handle keyed with the same seed, and a whole run equals many short sweep calls"""
    model = gpu.IsingModel(dims=2, L=8)
    seed, therm, sweeps = 31337, 20, 300
    big = gpu.MC(model, beta=0.44, n_walkers=16384, seed=seed, thermalization=therm, sweeps=sweeps)
    big.run()
    for k in (0, 1, 199, 8191, 16383):
        one = gpu.MC(model, beta=0.44, n_walkers=1, seed=seed, first_walker=k, thermalization=therm, sweeps=sweeps)
        one.run()
        assert _stats(one, 0) == _stats(big, k), k
        assert np.array_equal(one.conf(0), big.conf(k)), k
        one.close()
    mid = gpu.MC(model, beta=0.44, n_walkers=200, seed=seed, thermalization=therm, sweeps=sweeps)
    rng = np.random.default_rng(3)
    while mid.last_sweep < therm + sweeps:
        mid.sweep(int(min(rng.integers(1, 17), therm + sweeps - mid.last_sweep)))
    for k in (0, 57, 199):
        assert _stats(mid, k) == _stats(big, k), k
    big.close()
    mid.close()


def _exact_4x4(beta):
    """<E>, <E^2>, <|M|>, <M^2> over all 2^16 states"""
    n = 16
    states = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1) * 2 - 1
    from montecarlo_jl_amd import SquareLattice
    l = SquareLattice(4)
    b = l.bonds[:, :2] - 1
    E = -np.sum(states[:, b[:, 0]] * states[:, b[:, 1]], axis=1).astype(float)
    M = np.abs(states.sum(axis=1)).astype(float)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    return {"E": w @ E, "E2": w @ E ** 2, "M": w @ M, "M2": w @ M ** 2}


def test_4x4_against_exact_enumeration(gpu):
    betas = (0.2, 0.44, 0.7)
    Wb = 512
    model = gpu.IsingModel(dims=2, L=4)
    mc = gpu.MC(model, beta=np.repeat(betas, Wb), n_walkers=3 * Wb, seed=99, thermalization=200, sweeps=2000)
    mc.run()
    for bi, beta in enumerate(betas):
        ex = _exact_4x4(beta)
        per = {"E": [], "E2": [], "M": [], "M2": []}
        for w in range(bi * Wb, (bi + 1) * Wb):
            st = mc.stats(w)
            assert st.n_meas == 2000
            per["E"].append(st.sum_E / st.n_meas)
            per["E2"].append(st.sum_E2 / st.n_meas)
            per["M"].append(st.sum_absM / st.n_meas)
            per["M2"].append(st.sum_M2 / st.n_meas)
        for k, v in per.items():
            v = np.array(v)
            se = v.std(ddof=1) / np.sqrt(Wb)
            assert abs(v.mean() - ex[k]) <= 4.5 * se, (beta, k, v.mean(), ex[k], se)
    mc.close()


def test_reference_golden_8x8(gpu):
    """integration_tests.jl:1-26 (one run: 10 thermalization + 1000 sweeps at beta = 0.35).  Rule 1 of
    golden_stats.py: |ours - golden| <= Z sqrt(se_golden^2 + se_ours^2).  chi and C carry no published std_error; the
    scatter of one run's value is taken from the walkers themselves (each walker is one such run)."""
    Wn = 256
    mc = gpu.MC(gpu.IsingModel(dims=2, L=8), beta=0.35, n_walkers=Wn, seed=2024, thermalization=10, sweeps=1000)
    mc.run()
    vals = {k: [] for k in ("M", "E", "chi", "C", "m", "e")}
    for w in range(Wn):
        ms = mc.measurements(w)
        assert ms["n_meas"] == 1000
        for k in ("M", "m", "chi"):
            vals[k].append(ms["Magn"][k])
        for k in ("E", "e", "C"):
            vals[k].append(ms["Energy"][k])
    golden = {"M": (25.47, 0.82), "E": (-59.10, 0.88), "m": (0.398, 0.013), "e": (-0.924, 0.014),
              "chi": (1.300, None), "C": (0.585, None)}
    for k, (g, gse) in golden.items():
        v = np.array(vals[k])
        se_ours = v.std(ddof=1) / np.sqrt(Wn)
        if gse is None:
            gse = v.std(ddof=1)
        assert abs(v.mean() - g) <= Z * math.sqrt(gse ** 2 + se_ours ** 2), (k, v.mean(), g, gse, se_ours)
    mc.close()


def test_interface_consistency(gpu):
    model = gpu.IsingModel(dims=2, L=16)
    W, cap = 70, 40
    mc = gpu.MC(model, beta=[0.3 + 0.005 * w for w in range(W)], n_walkers=W, seed=5, thermalization=7, sweeps=60,
                measure_rate=2, series_capacity=cap)
    rec = gpu.ConfigRecorder(rate=10)
    mc.run(recorder=rec, sweeps=63)
    assert mc.last_sweep == 70 and len(rec) == 7  # sweeps 10, 20, ..., 70
    assert np.array_equal(gpu.decompress(rec[-1]).reshape(-1), mc.conf(0))
    for w in (0, 33, 69):
        c = mc.conf(w)
        st = mc.stats(w)
        assert set(np.unique(c)) <= {-1, 1}
        assert st.energy == model.energy(c) and st.magnetization == int(c.sum())
        assert st.n_meas == 32 and st.n_series == 32  # sweeps 8..70, every second one
        e, m = mc.series(w)
        assert len(e) == 32 and e.sum() == st.sum_E and (e.astype(float) ** 2).sum() == st.sum_E2
        assert m.sum() == st.sum_absM and (m.astype(float) ** 2).sum() == st.sum_M2
        assert st.acc_local == mc.analysis(w)["acc_local"] and st.prop_local == 70 * 256
    # past the capacity the series stops, the sums go on
    mc.sweep(40)
    st = mc.stats(0)
    e, m = mc.series(0)
    assert st.n_meas == 52 and st.n_series == cap and len(e) == cap
    mc.reset_accumulators()
    st = mc.stats(0)
    assert st.n_meas == 0 and st.n_series == 0 and st.sum_E == 0.0 and st.prop_local == 110 * 256
    mc.close()


# ---- the kernel's limits: the N ceiling (512 LDS spin words per lane), every z = 1..8, the threshold edges
def _check_against_restatement(O, mc, l, betas, seed, therm, sweeps, rate=1, walkers=None):
    for w in (range(len(betas)) if walkers is None else walkers):
        ref, c = restate(O, l, float(betas[w]), seed + w, therm, sweeps, rate)
        assert _stats(mc, w) == ref, w
        assert np.array_equal(mc.conf(w), c), w


@pytest.mark.parametrize("name,make", [
    ("square128_N16384_z4", lambda g: g.SquareLattice(128)),
    ("cubic4d_11_N14641_z8", lambda g: g.CubicLattice(4, 11)),   # 14641 = 457 words of 32 spins + 17
])
def test_the_site_ceiling_matches_the_restatement(gpu, O, name, make):
    """N = 16384 (the most the LDS holds) and a 4D lattice just below it whose last spin word is partial, three walkers
    at different betas, the run split over two sweep calls"""
    l = make(gpu)
    assert len(l) <= 16384
    therm, sweeps, seed = 2, 3, 4711
    betas = [0.2, 0.44, 0.7]
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=3, seed=seed, thermalization=therm, sweeps=sweeps)
    mc.sweep(2)
    mc.sweep(therm + sweeps - 2)
    _check_against_restatement(O, mc, l, betas, seed, therm, sweeps)
    mc.close()


class _RingTable:
    """N sites (0-based i) with the neighbours i ^ 1 (z = 1) or i +- 1..(z - 1)/2 and i + N/2 (odd z), 1-based as the
    project's lattices; the bonds are the undirected edges of that table"""

    def __init__(self, N, z):
        assert N % 2 == 0 and (z == 1 or (z % 2 == 1 and N // 2 > (z - 1) // 2))
        i = np.arange(N)
        if z == 1:
            rows = [i ^ 1]
        else:
            rows = [(i + s * d) % N for d in range(1, (z - 1) // 2 + 1) for s in (1, -1)] + [(i + N // 2) % N]
        self.sites = N
        self.neighs = np.vstack(rows).astype(np.int64) + 1
        edges = sorted({(min(a, b), max(a, b)) for r in rows for a, b in zip(i, r)})
        assert len(edges) * 2 == N * z  # every neighbour distinct: each edge seen once from each end
        self.bonds = np.array(edges, dtype=np.int64) + 1

    def __len__(self):
        return self.sites


@pytest.mark.parametrize("N,z", [(50, 1), (70, 3), (94, 5), (1000, 7)])
def test_odd_z_tables_match_the_restatement(gpu, O, N, z):
    """z = 1, 3, 5, 7 (the instantiations of ising_sweep_kernel<Z> no project lattice selects), N even and not a
    multiple of 32 (a partial last spin word)"""
    l = _RingTable(N, z)
    model = gpu.IsingModel(l=l)
    therm, sweeps, rate, seed = 4, 21, 2, 606
    betas = [0.15, 0.4, 0.9]
    mc = gpu.MC(model, beta=betas, n_walkers=3, seed=seed, thermalization=therm, sweeps=sweeps, measure_rate=rate)
    mc.sweep(9)
    mc.sweep(therm + sweeps - 9)
    _check_against_restatement(O, mc, l, betas, seed, therm, sweeps, rate)
    for w in range(3):
        assert mc.stats(w).energy == model.energy(mc.conf(w))
    mc.close()


def test_z8_many_walkers_matches_the_restatement(gpu, O):
    """CubicLattice(4, 4): z = 8, every entry of a padded neighbour row and all eight thresholds, 300 walkers"""
    l = gpu.CubicLattice(4, 4)
    assert l.neighs.shape == (8, 256)
    W, therm, sweeps, rate, seed = 300, 5, 20, 2, 8080
    betas = np.linspace(0.02, 0.4, W)
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=W, seed=seed, thermalization=therm, sweeps=sweeps,
                measure_rate=rate)
    mc.sweep(7)
    mc.sweep(therm + sweeps - 7)
    _check_against_restatement(O, mc, l, betas, seed, therm, sweeps, rate, walkers=(0, 1, 63, 64, 150, 255, 299))
    mc.close()


@pytest.mark.parametrize("name,make", [
    ("ring70_z3", lambda g: _RingTable(70, 3)),
    ("square8_z4", lambda g: g.SquareLattice(8)),
    ("cubic4d_4_z8", lambda g: g.CubicLattice(4, 4)),
])
def test_threshold_edges_match_the_restatement(gpu, O, name, make):
    """beta = 0: every proposal accepted, a uniform still drawn for every dE > 0.  beta = 185: exp(-2 beta k) is normal
    for k = 1, subnormal for k = 2 (exp(-740)) and 0 from k = 3 on; beta = 1000: every threshold is 0, so only dE <= 0 is
    accepted, and the draws for dE > 0 are still counted"""
    l = make(gpu)
    therm, sweeps, seed = 3, 8, 99
    betas = [0.0, 185.0, 1000.0]
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=3, seed=seed, thermalization=therm, sweeps=sweeps)
    mc.sweep(5)
    mc.sweep(therm + sweeps - 5)
    _check_against_restatement(O, mc, l, betas, seed, therm, sweeps)
    st = mc.stats(0)
    assert st.acc_local == st.prop_local == (therm + sweeps) * len(l)
    assert st.uniforms_used > len(l)
    mc.close()
