"""The teeth of tests/checkerboard_products_ref.py, without a device: every way cb_apply_kernel (csrc/cb.hip) could go
wrong that tests/test_gpu_checkerboard_products.py is meant to catch is applied to the REFERENCE as a mutant, and the
mutant must leave the derived bound of the unmutated reference by a wide margin.  The margin asked for is 1e6 bounds: a
mutant is an O(dtau t) = 0.05 relative change of some entry (a factor dropped or moved) or larger (a wrong exponential,
a wrong column), the bound is a few hundred eps of the same magnitude.  Inputs are those of the device tests.

Where a mutant is the identity on a shape it is not asked for there: rows k >= 256 exist only on Chain(257), and the last
slab of Chain(257) (16 columns per slab, 257 = 16 * 16 + 1) starts at column n - 1 itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checkerboard_products_ref as CR  # noqa: E402

DTAU, U, MARGIN = 0.1, 4.0, 1e6
SHAPES = [("square", 6), ("chain", 257)]


def lattice(pkg, spec):
    kind, L = spec[0], spec[1:]
    return {"square": pkg.SquareLattice, "chain": pkg.Chain, "triangular": pkg.TriangularLattice,
            "cubic": pkg.CubicLattice}[kind](*L)


def model(pkg, spec, kind, U=U):
    if kind == "attractive":
        return pkg.HubbardModelAttractive(l=lattice(pkg, spec), U=U, mu=0.3)
    return pkg.HubbardModelRepulsive(l=lattice(pkg, spec), U=U)


def inputs(n, nb, W, seed):
    """X standard normal, distinct per walker and block; one HS slice of random +-1 per walker; a qscale graded over
    e^+-20 like the D of a stabilisation step, distinct per unit"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((W * nb, n, n))
    conf = rng.choice(np.array([-1, 1], dtype=np.int8), size=(W, n))
    q = np.exp(np.linspace(20.0, -20.0, n)[None, :] + rng.uniform(-0.5, 0.5, (W * nb, n)))
    return X, conf, q


_CASES = {}


def case(mc_amd, spec, kind):
    key = (spec, kind)
    if key not in _CASES:
        m = model(mc_amd, spec, kind)
        tabs = CR.tables(mc_amd, m, DTAU)
        X, conf, q = inputs(len(m.l), m.flv, 2, 11)
        _CASES[key] = (m, tabs, X, conf, q, CR.lambdas(U, DTAU))
    return _CASES[key]


def worst(mut, ref, base, tabs, which):
    """largest |mutant - reference| / bound"""
    b = CR.bound(tabs, which, base)
    return float((np.abs(mut - ref) / b).max())


def reference(c, which, qscale=None):
    m, tabs, X, conf, q, (epl, eml) = c
    return CR.apply(which, X, tabs, conf, epl, eml, m.flv, qscale=qscale)


@pytest.mark.parametrize("spec", SHAPES)
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_reference_is_not_vacuous_and_follows_the_dense_factors(mc_amd, spec, kind):
    """the ELL reference equals the longdouble product of the dense group matrices exactly (two nonzeros per row: the
    zero terms of a dense row add nothing), and its bound is far below its values"""
    c = case(mc_amd, spec, kind)
    m, tabs, X, conf, q, (epl, eml) = c
    assert tabs["kmax"] == 2
    fac = [mc_amd.checkerboard_exponentials(T, m.l, DTAU, return_factors=True) for T in m.hopping_matrix()]
    nb, W = m.flv, conf.shape[0]
    w0 = 0 if len(m.l) <= 64 else W - 1  # (dense longdouble products at n = 257 are slow: the last walker only)
    for which in range(7):
        val, base = reference(c, which)
        assert CR.bound(tabs, which, base).max() <= 1e-9 * np.abs(val).max()
        dense = CR.apply_dense(which, X[w0 * nb:], fac, conf[w0:], epl, eml, nb)
        assert np.array_equal(dense, val[w0 * nb:]), CR.NAMES[which]


@pytest.mark.parametrize("spec", SHAPES)
def test_mutants_of_the_factor_sequence(mc_amd, spec):
    c = case(mc_amd, spec, "attractive")
    m, tabs, X, conf, q, (epl, eml) = c
    groups = (len(tabs["seqs"][0]) + 1) // 2
    for which in range(7):
        val, base = reference(c, which)
        seq = tabs["seqs"][which]
        for drop in (0, len(seq) // 2, len(seq) - 1):  # one factor dropped: first, middle (C_1 of a sandwich), last
            t = dict(tabs, seqs=[s if i != which else seq[:drop] + seq[drop + 1:] for i, s in enumerate(tabs["seqs"])])
            r = worst(CR.apply(which, X, t, conf, epl, eml, 1)[0], val, base, tabs, which)
            print("%s %s drop %d: %.3g bounds" % (spec, CR.NAMES[which], drop, r))
            assert r > MARGIN
        # two neighbouring factors of different groups swapped (groups share sites, so they do not commute)
        assert groups > 2
        i = 0
        sw = list(seq)
        sw[i], sw[i + 1] = sw[i + 1], sw[i]
        assert sw != seq
        t = dict(tabs, seqs=[s if k != which else sw for k, s in enumerate(tabs["seqs"])])
        r = worst(CR.apply(which, X, t, conf, epl, eml, 1)[0], val, base, tabs, which)
        print("%s %s swap %d,%d: %.3g bounds" % (spec, CR.NAMES[which], i, i + 1, r))
        assert r > MARGIN


@pytest.mark.parametrize("spec", SHAPES)
def test_mutant_block_1_sign_not_swapped(mc_amd, spec):
    c = case(mc_amd, spec, "repulsive")
    m, tabs, X, conf, q, (epl, eml) = c
    for which in range(5):  # the conf-scaled sequences
        val, base = reference(c, which)
        mut = CR.apply(which, X, tabs, conf, epl, eml, 2, swap_block1=False)[0]
        assert np.array_equal(mut[0::2], val[0::2])  # block 0 is not affected
        r = worst(mut[1::2], val[1::2], base[1::2], tabs, which)
        print("%s %s block 1 sign: %.3g bounds" % (spec, CR.NAMES[which], r))
        assert r > MARGIN


@pytest.mark.parametrize("spec", SHAPES)
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_mutant_pre_and_post_scaling_exchanged(mc_amd, spec, kind):
    c = case(mc_amd, spec, kind)
    m, tabs, X, conf, q, (epl, eml) = c
    for which in range(5):
        val, base = reference(c, which)
        side, pre, post = CR.SCALINGS[which]
        mut = CR.apply(which, X, tabs, conf, epl, eml, m.flv, scalings={which: (side, post, pre)})[0]
        r = worst(mut, val, base, tabs, which)
        print("%s %s pre <-> post: %.3g bounds" % (spec, CR.NAMES[which], r))
        assert r > MARGIN


def test_mutant_clamped_column_leaks_into_the_last_slab(mc_amd):
    """SquareLattice(6): slabs of 32, the last holds columns 32..35; its loads of columns 36.. are clamped to column 35"""
    c = case(mc_amd, ("square", 6), "attractive")
    m, tabs, X, conf, q, (epl, eml) = c
    n, q0 = 36, 32
    assert mc_amd.checkerboard_slab(n)[0] == 32
    for which in range(7):
        val, base = reference(c, which)
        Xm = X.copy()
        if CR.SCALINGS[which][0] == 0:
            Xm[:, :, q0] = X[:, :, n - 1]  # a left product slabs the columns
        else:
            Xm[:, q0, :] = X[:, n - 1, :]  # a right product the rows
        r = worst(CR.apply(which, Xm, tabs, conf, epl, eml, 1)[0], val, base, tabs, which)
        print("%s clamp leak: %.3g bounds" % (CR.NAMES[which], r))
        assert r > MARGIN


def test_mutant_rows_of_the_second_pass_left_unmixed(mc_amd):
    """Chain(257): one thread per row and 256 threads, so row 256 belongs to a second pass of the factor loop"""
    c = case(mc_amd, ("chain", 257), "attractive")
    m, tabs, X, conf, q, (epl, eml) = c
    vals, cols = tabs["vals"].copy(), tabs["cols"].copy()
    vals[:, 256:, :] = 0.0
    vals[:, 256:, 0] = 1.0
    cols[:, 256:, :] = np.arange(256, 257)[None, :, None]
    t = dict(tabs, vals=vals, cols=cols)
    for which in range(7):
        val, base = reference(c, which)
        r = worst(CR.apply(which, X, t, conf, epl, eml, 1)[0], val, base, tabs, which)
        print("%s rows >= 256 unmixed: %.3g bounds" % (CR.NAMES[which], r))
        assert r > MARGIN


@pytest.mark.parametrize("spec", SHAPES)
def test_mutant_qscale_of_the_neighbouring_unit(mc_amd, spec):
    c = case(mc_amd, spec, "repulsive")
    m, tabs, X, conf, q, (epl, eml) = c
    for which in (0, 2):
        val, base = reference(c, which, qscale=q)
        assert CR.bound(tabs, which, base).max() <= 1e-9 * np.abs(val).max()
        mut = CR.apply(which, X, tabs, conf, epl, eml, 2, qscale=np.roll(q, 1, axis=0))[0]
        r = worst(mut, val, base, tabs, which)
        print("%s %s qscale of unit u on u + 1: %.3g bounds" % (spec, CR.NAMES[which], r))
        assert r > MARGIN


def test_padded_tables_are_the_same_products(mc_amd):
    c = case(mc_amd, ("square", 6), "repulsive")
    m, tabs, X, conf, q, (epl, eml) = c
    p = CR.padded(tabs, 5)
    assert p["vals"].shape[2] == 5 and np.all(p["vals"][:, :, 2:] == 0) and np.all(p["cols"][:, :, 2:] == np.arange(36)[None, :, None])
    for which in range(7):
        a, b = reference(c, which), CR.apply(which, X, p, conf, epl, eml, 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_slab_widths_and_the_size_no_width_fits(mc_amd):
    """checkerboard_slab restates cb_slab_width (csrc/cb.hip); the device tests hold it against dqmc_checkerboard_plan"""
    f = mc_amd.checkerboard_slab
    assert f(16) == (32, 16 * 544) and f(256) == (32, 139264) and f(257) == (16, 257 * 288)
    assert f(568) == (16, 163584) and f(576) == (8, 576 * 160) and f(1024) == (8, 160 * 1024)
    with pytest.raises(ValueError, match="dense"):
        f(1025)
