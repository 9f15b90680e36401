"""The momentum transform (csrc/momentum.hip, momentum.inl) past one 64 x 64 tile of the sample: more than one q-tile
(blockIdx.y > 0, the table tile at q0 + c and the epilogue's q0 + c * 16 + li), two to five k-tiles with and without a tail
(n_dirs = 64, 65, 81, 100, 130), row counts at and around the row tile (32, 64, 65, 84, 260), a source whose per-walker
stride is not 4 n_dirs, tables without any symmetry, and a three-component q.

Bound and reference are those of test_gpu_momentum.py, imported from there and unchanged:
|device - reference| <= 2 n_dirs 2^-53 sum_d |X[d] Tab[d, q]| + 1e-300 per element against the same product in
numpy.longdouble, from level 0 of the source section's own binner after one push.  Every case prints its largest
err / bound (DESIGN.md 4.14 records them per family).

The direction tables come from tests/lattice_tables.py: fast_pairs (the package's iterator is a Python double loop); on
every lattice used here it gives n_dirs = n.  U = 1, delta_tau = 0.1, beta = 0.1 slices, safe_mult 5 unless a case says
otherwise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_tables as LT  # noqa: E402
import measurement_ref as MR  # noqa: E402
from test_gpu_dqmc import TOL  # noqa: E402  (the device-against-oracle bound on G, 1e-10)
from test_gpu_momentum import MOM, SRC, U53, assert_transform, level0, one_pass, transform_reference  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GREENS, DENSITY = 1, 2
_tables = {}


def tables(gpu, spec):
    """(lattice, fast_pairs) of ("chain", n) / ("square", L) / ("cubic", L) / ("tri", L), built once"""
    if spec not in _tables:
        kind, L = spec
        l = {"chain": lambda: gpu.Chain(L), "square": lambda: gpu.SquareLattice(L), "cubic": lambda: gpu.CubicLattice(3, L),
             "tri": lambda: gpu.TriangularLattice(L)}[kind]()
        fp = LT.fast_pairs(l)
        assert fp.ndirections() == l.sites and np.all(np.bincount(fp.dir_of.ravel(), minlength=l.sites) == l.sites)
        _tables[spec] = (l, fp)
    return _tables[spec]


def handle(gpu, spec, kind, W, slices=10, n_q="all", every=5, what=GREENS | DENSITY, seed=53, safe_mult=5, random_tables=None,
           quads=0, **kw):
    """a prepared handle at its measurement point with directions, momenta (the first n_q of the grid, or with
    random_tables = seed two independent standard-normal tables of that shape) and recording set; quads = K: local and
    current targets of the K shortest directions first, so that the susceptibility section holds PS and CCS too"""
    l, fp = tables(gpu, spec)
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(l=l), beta=0.1 * slices, delta_tau=0.1, safe_mult=safe_mult, n_walkers=W, seed=seed, **kw)
    try:
        mc.set_pair_directions(fp)
        if quads:
            trg = LT.fast_quads(l, quads, pairs=fp).trg_of
            mc.set_local_targets(LT.QuadTables(fp, trg))
            mc.set_current_targets(LT.QuadTables(fp, trg, synced=True))
        q = gpu.momentum_grid(l)[0]
        q = q if n_q == "all" else q[:n_q]
        if random_tables is None:
            mc.set_momenta(q)
        else:
            rng = np.random.default_rng(random_tables)
            nd = fp.ndirections()
            mc._set_momenta(q, rng.standard_normal(nd * len(q)), rng.standard_normal(nd * len(q)))
        if every:
            mc.set_time_displaced(every, what)
        mc.prepare()
        mc.update_until_measure()
    except BaseException:
        mc.close()
        raise
    return mc


def closing(*handles):
    for m in handles:
        if m is not None:
            m.close()


def run_transform_case(gpu, case, label=None, **kw):
    spec, kind, n_q, W, slices, every, what = case[:7]
    mc = handle(gpu, spec, kind, W, slices=slices, n_q=n_q, every=every, what=what, **kw)
    try:
        nd, B, R = mc._ndirs, mc.nb, 1 + slices // every
        plan = mc.momenta_plan()
        assert plan == dict(n_q=n_q, n_dirs=nd, tile_rows=64, tile_cols=64)
        if n_q > 64:
            assert plan["n_q"] > plan["tile_cols"]  # a second q-tile runs
        mc.enable_binning(SRC + MOM, capacity=7)
        E_td = ((4 * B if what & GREENS else 0) + (4 if what & DENSITY else 0)) * R * n_q
        assert [mc.binner_size(k)[0] for k in MOM] == [4 * n_q, 4 * n_q, E_td]
        one_pass(mc)
        for which, src in zip(MOM, SRC):
            assert mc.binner_size(which)[2] == 1
            assert_transform(mc, which, src, label or "%s%d %s" % (spec + (kind,)))
    finally:
        mc.close()


def case_id(c):
    return "%s%d-%s-q%d-w%d-m%d-e%d-what%d" % (c[0] + tuple(c[1:7]))


# ---- 1. the tile edges ----------------------------------------------------------------------------------------------
#        lattice         model        n_q  W  slices every what                what it reaches
CASES = [(("chain", 64), "attractive", 64, 1, 10, 5, GREENS | DENSITY),     # exactly two k-tiles, one q-tile, no tail code
         (("chain", 65), "repulsive", 65, 3, 10, 5, GREENS),                # third k-tile of one entry; second q-tile one column wide
         (("chain", 65), "attractive", 64, 1, 10, 1, GREENS | DENSITY),     # k tail with a full single q-tile
         (("square", 10), "repulsive", 100, 1, 20, 1, GREENS | DENSITY),    # R = 21: 42 Green's rows, 84 density rows; 4 k-, 2 q-tiles
         (("square", 10), "attractive", 97, 3, 10, 5, DENSITY),             # n_q off every grid
         (("chain", 130), "repulsive", 129, 1, 10, 5, GREENS | DENSITY),    # 5 k-tiles, a tail of 2; 3 q-tiles, the last one column wide
         (("cubic", 3), "repulsive", 27, 3, 10, 5, GREENS | DENSITY),       # three-component q, one partial k-tile
         (("cubic", 4), "attractive", 64, 1, 10, 5, GREENS),                # 3-D at the exact tile
         (("tri", 9), "repulsive", 81, 1, 10, 5, DENSITY)]                  # non-orthogonal reciprocal basis past one tile


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_transform_at_the_tile_edges(gpu, case):
    run_transform_case(gpu, case)


# the row tile, independent of n_dirs: Chain(8), n_q = 8
#            lattice       model        n_q W slices every what            safe_mult   rows
ROW_CASES = [(("chain", 8), "attractive", 8, 1, 64, 1, GREENS | DENSITY, 8),  # R = 65: 65 Green's rows, 260 density rows
             (("chain", 8), "repulsive", 8, 1, 15, 1, GREENS | DENSITY, 5),   # R = 16: 32 Green's rows, exactly 64 density rows
             (("chain", 8), "attractive", 8, 1, 64, 1, GREENS, 8),
             (("chain", 8), "attractive", 8, 1, 64, 1, DENSITY, 8)]


@pytest.mark.parametrize("case", ROW_CASES, ids=case_id)
def test_transform_at_the_row_tile_edges(gpu, case):
    R, B = 1 + case[4] // case[5], 1 if case[1] == "attractive" else 2
    assert (R, B * R, 4 * R) in ((65, 65, 260), (16, 32, 64))
    run_transform_case(gpu, case, safe_mult=case[7])


# ---- 2. tables without symmetry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1][:6] + (GREENS | DENSITY, 11), CASES[3] + (12,)], ids=case_id)
def test_transform_with_random_tables(gpu, case):
    """both tables standard normal, drawn independently: every (d, q) entry is distinct, so a transposed table, two swapped
    columns (q for -q among them) or the cosine table where the sine table belongs all fail"""
    run_transform_case(gpu, case, label="random tables %s%d %s" % (case[0] + (case[1],)), random_tables=case[7])


# ---- 3. a source stride that is not 4 n_dirs --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,signed", [("attractive", False), ("repulsive", False), ("repulsive", True)],
                         ids=["attractive", "repulsive", "repulsive-signed"])
@pytest.mark.parametrize("L", [6, 10])
def test_susceptibility_source_with_local_and_current_targets(gpu, L, kind, signed):
    """local and current targets (K = 5) put PS and CCS behind the four susceptibility rows of every walker: x_stride =
    4 n_dirs + 25 n_dirs + 5 n_dirs.  With sign weighting (repulsive model) the sample ends with s_w and the rest is the
    transform of the signed source sample."""
    K, W = 5, 2
    mc = handle(gpu, ("square", L), kind, W, every=0, quads=K, sign_weighting=signed)
    try:
        nd = n_q = L * L
        assert mc.momenta_plan() == dict(n_q=n_q, n_dirs=nd, tile_rows=64, tile_cols=64)
        mc.enable_binning(("susceptibilities", "momentum_susceptibilities"), capacity=3)
        E = mc.binner_size("susceptibilities")[0]  # (the source's own binner carries no s_w)
        assert E == 4 * nd + nd * K * K + nd * K and E > 4 * nd
        assert mc.binner_size("momentum_susceptibilities")[0] == 4 * n_q + (1 if signed else 0)
        sg = mc.sign() if signed else None
        one_pass(mc, ("susceptibilities",))
        if signed:
            for w in range(W):
                assert level0(mc, "momentum_susceptibilities", w)[-1] == sg[w] and sg[w] in (-1, 1)
        assert_transform(mc, "momentum_susceptibilities", "susceptibilities",
                         "stride %d n_dirs, square%d %s%s" % (E // nd, L, kind, " signed" if signed else ""))
    finally:
        mc.close()


# ---- 4. n(k) from the site positions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,kind", [(("chain", 65), "attractive"), (("square", 10), "repulsive"),
                                       (("cubic", 3), "attractive"), (("cubic", 3), "repulsive")],
                         ids=lambda v: v if isinstance(v, str) else "%s%d" % v)
def test_nk_from_the_site_positions(gpu, spec, kind):
    """test_gpu_momentum.py's test of the same name at n_q = n = 65, 100 (two q-tiles) and on the cubic lattice: n(k) and
    Im G(k, 0) from mc.greens(w) and the site positions alone, 1e-10 relative to the largest reference value; Sc and Sz
    through measurement_ref.equal_time with one direction per pair on CubicLattice(3) only (n^2 = 729 directions)"""
    mc = handle(gpu, spec, kind, 2, every=5)
    try:
        l = mc.model.l
        n, B = len(l), mc.nb
        mc.enable_binning(("momentum_correlations", "momentum_time_displaced"), capacity=3)
        G = [mc.greens(w) for w in range(2)]
        one_pass(mc)
        pos = np.array(gpu.lattices._positions(l))
        q = mc.momenta()
        assert q.shape == (n, pos.shape[1])
        dr = pos[:, None, :] - pos[None, :, :]              # r_i - r_j at [i, j]
        ph = np.einsum("ijx,qx->qij", dr, q)
        cosp, sinp = np.cos(ph), np.sin(ph)
        for w in range(2):
            td = mc._bin_shape("momentum_time_displaced", level0(mc, "momentum_time_displaced", w))
            for b in range(B):
                nk_ref = 1.0 - np.einsum("qij,ij->q", cosp, G[w][b]) / n
                im_ref = -np.einsum("qij,ij->q", sinp, G[w][b]) / n
                nk_dev, im_dev = 1.0 - td["Gl0_C"][b, 0, :], -td["Gl0_S"][b, 0, :]
                scale = max(np.abs(nk_ref).max(), np.abs(im_ref).max())
                print("%s%d %s walker %d block %d: nk %.3g, Im %.3g of TOL scale" % (
                    spec + (kind, w, b, np.abs(nk_dev - nk_ref).max() / (TOL * scale), np.abs(im_dev - im_ref).max() / (TOL * scale))))
                assert np.abs(nk_dev - nk_ref).max() <= TOL * scale
                assert np.abs(im_dev - im_ref).max() <= TOL * scale
                assert np.abs(im_ref).max() > 1e-4 * scale  # (the imaginary part of one configuration is not zero)
            if spec == ("cubic", 3):
                pair = np.arange(n * n).reshape(n, n)        # every pair its own "direction"
                et = MR.equal_time(G[w], pair, n * n)
                sf = mc._bin_shape("momentum_correlations", level0(mc, "momentum_correlations", w))
                for name, key in (("Sc", "CDC"), ("Sz", "SDCz")):
                    ref = np.einsum("qij,ij->q", cosp, et[key][0].reshape(n, n))
                    assert np.abs(sf[name] - ref).max() <= TOL * np.abs(ref).max(), (name, w)
    finally:
        mc.close()


# ---- 5. bits ------------------------------------------------------------------------------------------------------------
def test_two_passes_and_another_walker_count_give_the_same_bits_over_two_q_tiles(gpu):
    one = three = None
    try:
        three, one = handle(gpu, ("chain", 65), "repulsive", 3), handle(gpu, ("chain", 65), "repulsive", 1)
        first = {}
        for mc in (three, one):
            assert mc.momenta_plan()["n_q"] == 65 > mc.momenta_plan()["tile_cols"]
            mc.enable_binning(MOM, capacity=3)
            one_pass(mc)
            first[mc] = {k: [level0(mc, k, w) for w in range(mc.n_walkers)] for k in MOM}
            assert all(np.abs(first[mc][k][0][64::65]).max() > 1e-6 for k in MOM)  # (the second q-tile's column is written)
            mc.reset_accumulators()
            assert mc.binner_size(MOM[0])[2] == 0 and not level0(mc, MOM[2], 0).any()
            one_pass(mc)
            for k in MOM:
                for w in range(mc.n_walkers):
                    assert np.array_equal(level0(mc, k, w), first[mc][k][w]), "a second pass differs bitwise: " + k
        for k in MOM:
            assert np.array_equal(first[one][k][0], first[three][k][0]), "walker 0 depends on n_walkers: " + k
    finally:
        closing(one, three)


# ---- 6. checkpoint at a multi-tile table ----------------------------------------------------------------------------------
def binner_levels(mc, sections):
    out = {}
    for k in sections:
        E, L, T = mc.binner_size(k)
        out[k] = (E, L, T, [mc.binner_level(k, w, lv) for w in range(mc.n_walkers) for lv in range(L)])
    return out


def assert_same_levels(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k][:3] == b[k][:3], k
        for (x1, y1, c1), (x2, y2, c2) in zip(a[k][3], b[k][3]):
            assert np.array_equal(x1, x2) and np.array_equal(y1, y2) and c1 == c2, k


def test_checkpoint_with_a_multi_tile_table(gpu):
    """Chain(65), n_q = 65, two pushes into momentum_correlations and momentum_time_displaced: the blob is version 2; a
    fresh, identically configured handle takes it and then holds every level of both binners exactly; a third pass gives
    equal bits on both handles once both stand on the blob (an import rebuilds G from the HS field, so the exporting
    chain as it runs on agrees with an import within TOL only - test_gpu_checkpoint.py - while two imports of one blob have
    one future: the exporter takes its own blob back before the pass); a handle with n_q = 64 refuses the blob, names n_q
    and stays as it was"""
    from montecarlo_jl_amd import _lib
    on, src = ("momentum_correlations", "momentum_time_displaced"), ("correlations", "time_displaced")
    a = b = c = None
    try:
        a = handle(gpu, ("chain", 65), "repulsive", 2)
        a.enable_binning(on, capacity=7)
        one_pass(a, src)
        a.update_until_measure()
        one_pass(a, src)
        blob = a.state()
        assert int.from_bytes(bytes(blob[8:12]), "little") == 2
        saved = binner_levels(a, on)
        assert all(saved[k][2] == 2 for k in on) and saved[on[0]][0] == 4 * 65
        b = handle(gpu, ("chain", 65), "repulsive", 2, seed=7)
        b.enable_binning(on, capacity=7)
        one_pass(b, src)  # (the first pass lays the susceptibility section out: part of the configuration a blob asks for)
        assert not np.array_equal(level0(b, on[0], 0), saved[on[0]][3][0][0])
        b.set_state(blob)
        assert_same_levels(binner_levels(b, on), saved)
        a.set_state(blob)
        assert_same_levels(binner_levels(a, on), saved)
        for mc in (a, b):
            mc.update_until_measure()
            one_pass(mc, src)
        third = binner_levels(a, on)
        assert all(third[k][2] == 3 for k in on)
        assert_same_levels(binner_levels(b, on), third)
        for w in range(2):
            assert np.array_equal(a.conf(w), b.conf(w))
        # another n_q on the importing side
        c = handle(gpu, ("chain", 65), "repulsive", 2, n_q=64)
        c.enable_binning(on, capacity=7)
        one_pass(c, src)
        before = c.state()
        with pytest.raises(_lib.DQMCError) as e:
            c.set_state(blob)
        assert e.value.code == _lib.ERR_INVALID and "n_q" in str(e.value)
        assert np.array_equal(c.state(), before)
    finally:
        closing(a, b, c)
