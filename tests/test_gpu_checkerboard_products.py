"""The sparse checkerboard products on the device (csrc/cb.hip: cb_apply_kernel), one product at a time through
dqmc_checkerboard_apply, at every form of the slab: the three slab widths, one and several slabs with a partial last one,
one and two row passes, the generic kmax > 4 branch, qscale, in place and out of place.

Reference and tolerance: tests/checkerboard_products_ref.py (np.longdouble ELL gathers written from the header; per
element |device - reference| <= 2 (kmax seq_len + 6) eps bound_base; non-vacuity asserted: the largest bound is at most
1e-9 of the largest |reference|).  tests/test_checkerboard_products_ref.py shows without a device that the bound catches a
dropped or moved factor, a wrong sign in block 1, exchanged scalings, a leaking clamp, an unmixed second row pass and a
qscale of the wrong unit.  Each case prints its worst err / bound per sequence (DESIGN.md section 2 records them).

Inputs: X standard normal and distinct per walker and block, the HS field random +-1 and distinct per walker, slice 4 of
10, mu = 0.3 where the model takes one, U = 4 (no Markov chain is run), 2 walkers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checkerboard_products_ref as CR  # noqa: E402
import test_checkerboard_products_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

DTAU, U, SLICE, M = H.DTAU, H.U, 4, 10
KINDS = ["attractive", "repulsive"]
# lattice -> (n, slab width, groups); what each reaches is in the table of DESIGN.md section 2
SHAPES = {
    ("square", 4): (16, 32, 4),        # one partial slab
    ("square", 5): (25, 32, 5),        # 5 bond groups, sequences of 9
    ("square", 6): (36, 32, 4),        # two slabs, the last with 4 of 32 columns
    ("square", 16): (256, 32, 4),      # 8 full slabs, 139264 B of LDS, one row per thread
    ("chain", 257): (257, 16, 3),      # first 16-column size, a second row pass of one row, 17 slabs, the last of 1
    ("square", 18): (324, 16, 4),      # 21 slabs, the last with 4 of 16
    ("chain", 512): (512, 16, 2),      # two full row passes, 32 full slabs
    ("chain", 568): (568, 16, 2),      # the last size 16 columns fit (163584 B)
    ("square", 24): (576, 8, 4),       # the first size they do not: 8 columns
    ("triangular", 6): (36, 32, 16),   # 16 groups, sequences of 31 of the 32 the engine takes
    ("cubic", 3, 6): (216, 32, 6),     # sequences of 11, a partial last slab
    ("square", 32): (1024, 8, 4),      # the ceiling: 160 KiB of LDS, four row passes (attractive only: host tables)
}
CASES = [(s, k) for s in SHAPES for k in KINDS if not (s == ("square", 32) and k == "repulsive")]
IDS = ["%s%s-%s" % (s[0], "x".join(map(str, s[1:])), k) for s, k in CASES]

_TABS = {}


def tables(gpu, spec, kind):
    if (spec, kind) not in _TABS:
        _TABS[(spec, kind)] = CR.tables(gpu, H.model(gpu, spec, kind), DTAU)
    return _TABS[(spec, kind)]


def field(n, W, seed):
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(rng.choice(np.array([-1, 1], dtype=np.int8), size=(n, M))) for _ in range(W)]


def handle(gpu, spec, kind, W=2, checkerboard="sparse", U=U, seed=23):
    """a handle with a HS field of its own making; -> (mc, field of slice SLICE [W][n])"""
    m = H.model(gpu, spec, kind, U=U)
    mc = gpu.DQMC(m, beta=M * DTAU, delta_tau=DTAU, n_walkers=W, seed=seed, checkerboard=checkerboard)
    conf = field(len(m.l), W, seed)
    for w in range(W):
        mc.set_conf(w, conf[w])
    return mc, conf


def slice_of(conf, l):
    return np.stack([c[:, l - 1] for c in conf])


def set_tables(gpu, mc, tabs):
    """dqmc_set_checkerboard with tables of the caller's (the padded ones)"""
    from montecarlo_jl_amd import _lib
    seqs, lens = gpu.checkerboard_seqs(tabs)
    vals, cols = np.ascontiguousarray(tabs["vals"]), np.ascontiguousarray(tabs["cols"], dtype=np.int32)
    mu, mui = np.ascontiguousarray(tabs["mu"].ravel()), np.ascontiguousarray(tabs["mu_inv"].ravel())
    i32 = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().dqmc_set_checkerboard(mc._h, tabs["kmax"], vals.shape[0], _lib.dptr(vals), cols.ctypes.data_as(i32),
                                                _lib.dptr(mu), _lib.dptr(mui), seqs.ctypes.data_as(i32),
                                                lens.ctypes.data_as(i32)), mc._h)


def expected_plan(n, qw, kmax=2):
    return dict(sparse=1, kmax=kmax, slab_width=qw, lds_bytes=(2 * n * (qw + 1) + 2 * n) * 8)


def check(tag, dev, val, base, tabs, which, worst, coeff=None):
    """|dev - val| <= bound per element, non-vacuous; the worst err / bound goes into `worst`"""
    b = CR.bound(tabs, which, base, kmax=2) if coeff is None else 2.0 * coeff * CR.EPS * base
    assert b.max() <= 1e-9 * np.abs(val).max(), "%s: vacuous bound" % tag
    r = float((np.abs(dev.astype(CR.LD) - val) / b).max())
    worst[tag] = max(worst.get(tag, 0.0), r)
    return r


def products(gpu, mc, tabs, conf, nb, X, q, label, against=None):
    """all seven sequences out of place and in place, 0 and 2 also with qscale; -> {(which, scaled): device result}"""
    epl, eml = CR.lambdas(U, DTAU)
    worst, out, bad = {}, {}, []
    for which, qs in [(w, None) for w in range(7)] + [(0, q), (2, q)]:
        tag = CR.NAMES[which] + (" D" if qs is not None else "")
        dev = mc.checkerboard_apply(which, SLICE, X, qscale=qs)
        inp = mc.checkerboard_apply(which, SLICE, X, qscale=qs, in_place=True)
        assert np.array_equal(dev, inp), "%s %s: in place and out of place differ" % (label, tag)
        val, base = CR.apply(which, X, tabs, conf, epl, eml, nb, qscale=qs)
        if check(tag, dev, val, base, tabs, which, worst) > 1.0:
            bad.append(tag)
        if against is not None:  # padding adds zeros only: also within the bound of the unpadded handle's result
            d = float((np.abs(dev - against[(which, qs is not None)]) / CR.bound(tabs, which, base, kmax=2)).max())
            worst[tag + " vs kmax 2"] = d
            if d > 1.0:
                bad.append(tag + " vs kmax 2")
        out[(which, qs is not None)] = dev
    print("%s worst err/bound: %s" % (label, ", ".join("%s %.2g" % kv for kv in worst.items())))
    assert not bad, "%s: beyond the bound: %s" % (label, bad)
    return out


@pytest.mark.parametrize("spec,kind", CASES, ids=IDS)
def test_every_sequence_at_every_slab_form(gpu, spec, kind):
    n, qw, groups = SHAPES[spec]
    tabs = tables(gpu, spec, kind)
    assert tabs["vals"].shape[1] == n and [len(s) for s in tabs["seqs"]] == [2 * groups - 1] * 5 + [groups] * 2
    mc, conf = handle(gpu, spec, kind)
    assert mc.checkerboard_plan() == expected_plan(n, qw)
    assert gpu.checkerboard_slab(n) == (qw, mc.checkerboard_plan()["lds_bytes"])
    X, _, q = H.inputs(n, mc.nb, 2, 11)
    products(gpu, mc, tabs, slice_of(conf, SLICE), mc.nb, X, q, "%s[%s]" % (spec, kind))
    mc.close()


@pytest.mark.parametrize("spec", [("square", 6), ("chain", 257)])
@pytest.mark.parametrize("kind", KINDS)
def test_generic_branch_with_padded_tables(gpu, spec, kind):
    """kmax = 5 > 4 takes the branch that reads the coefficients from memory; the padding (val 0, col = the row) adds zeros"""
    n, qw, _ = SHAPES[spec]
    tabs = tables(gpu, spec, kind)
    mc, conf = handle(gpu, spec, kind)
    X, _, q = H.inputs(n, mc.nb, 2, 11)
    s = slice_of(conf, SLICE)
    plain = products(gpu, mc, tabs, s, mc.nb, X, q, "%s[%s] kmax 2" % (spec, kind))
    set_tables(gpu, mc, CR.padded(tabs, 5))
    assert mc.checkerboard_plan() == expected_plan(n, qw, kmax=5)
    products(gpu, mc, tabs, s, mc.nb, X, q, "%s[%s] kmax 5" % (spec, kind), against=plain)
    mc.close()


@pytest.mark.parametrize("spec", [("square", 6), ("chain", 257), ("square", 18)])
@pytest.mark.parametrize("kind", KINDS)
def test_through_the_call_sites_of_the_engine(gpu, spec, kind):
    """the wrap (two products in place on mc.s.greens) and greens() (two products through the scratch matrices), each
    against the composition of the two reference products with the bound composed: the second product's absolute chain
    applied to the first one's bound_base, coefficients added"""
    n = SHAPES[spec][0]
    tabs = tables(gpu, spec, kind)
    mc, conf = handle(gpu, spec, kind)
    nb, W = mc.nb, 2
    X = H.inputs(n, nb, W, 12)[0]
    epl, eml = CR.lambdas(U, DTAU)
    worst, bad = {}, []

    def load():
        for w in range(W):
            mc.set_greens_eff(w, list(X[w * nb:(w + 1) * nb]))

    def composed(first, second, l):
        s = slice_of(conf, l) if l else slice_of(conf, 1)  # (sequences 5 and 6 read no field)
        v1, b1 = CR.apply(first, X, tabs, s, epl, eml, nb)
        v2, b2 = CR.apply(second, v1, tabs, s, epl, eml, nb, Xabs=b1)
        return v2, b2, CR.roundings(tabs, first) + CR.roundings(tabs, second)

    # wrap_greens(l, +1) = B_l G B_l^-1; wrap_greens(l, -1) = B_{l-1}^-1 G B_{l-1}; greens() = eTinv G eT
    for tag, first, second, l, run, read in [
            ("wrap +1", 0, 4, SLICE, lambda: mc.wrap_greens(SLICE, +1), mc.greens_eff),
            ("wrap -1", 1, 3, SLICE - 1, lambda: mc.wrap_greens(SLICE, -1), mc.greens_eff),
            ("greens()", 5, 6, 0, lambda: None, mc.greens)]:
        load()
        run()
        dev = np.stack([g for w in range(W) for g in read(w)])
        val, base, coeff = composed(first, second, l)
        if check(tag, dev, val, base, tabs, None, worst, coeff=coeff) > 1.0:
            bad.append(tag)
    print("%s[%s] call sites worst err/bound: %s" % (spec, kind, ", ".join("%s %.2g" % kv for kv in worst.items())))
    assert not bad, bad
    mc.close()


@pytest.mark.parametrize("spec", [("square", 6), ("chain", 257), ("square", 18)])
@pytest.mark.parametrize("kind", KINDS)
def test_sparse_and_dense_chains_agree(gpu, spec, kind):
    """calculate_greens(slice) runs B' and the qscale of every stabilisation through the UDT: sparse factors against the
    multiplied-out constants at the model's default U, to the 1e-11 of test_sparse_and_dense_checkerboard_paths_agree"""
    a, _ = handle(gpu, spec, kind, checkerboard="sparse", U=1.0)
    b, _ = handle(gpu, spec, kind, checkerboard="dense", U=1.0)
    assert a.checkerboard_plan()["sparse"] == 1 and b.checkerboard_plan() == dict(sparse=0, kmax=0, slab_width=0, lds_bytes=0)
    for w in range(2):
        ga, gb = a.calculate_greens(SLICE, w), b.calculate_greens(SLICE, w)
        for blk in range(a.nb):
            d, s = np.abs(ga[blk] - gb[blk]).max(), max(1.0, np.abs(gb[blk]).max())
            print("%s[%s] walker %d block %d: max|dG| %.3g, scale %.3g" % (spec, kind, w, blk, d, s))
            assert d < 1e-11 * s
    a.close(); b.close()


def test_selection_of_the_form(gpu):
    zeros = dict(sparse=0, kmax=0, slab_width=0, lds_bytes=0)
    for spec, cb, want in [(("square", 16), True, zeros), (("chain", 257), True, expected_plan(257, 16)),
                           (("chain", 257), "dense", zeros)]:
        mc = gpu.DQMC(H.model(gpu, spec, "attractive", U=1.0), beta=1.0, n_walkers=1, seed=3, checkerboard=cb)
        assert mc.checkerboard_plan() == want, (spec, cb)
        mc.close()


def test_apply_refuses_what_it_cannot_run(gpu):
    from montecarlo_jl_amd import _lib
    n = 16
    X = np.zeros((1, n, n))
    mc = gpu.DQMC(H.model(gpu, ("square", 4), "attractive"), beta=1.0, n_walkers=1, seed=3, checkerboard="dense")
    with pytest.raises(_lib.DQMCError) as e:
        mc.checkerboard_apply(0, 1, X)
    assert e.value.code == _lib.ERR_STATE
    mc.close()
    mc = gpu.DQMC(H.model(gpu, ("square", 4), "attractive"), beta=1.0, n_walkers=1, seed=3, checkerboard="sparse")
    for which, l in [(-1, 1), (7, 1), (0, 0), (4, 11), (3, -1)]:
        with pytest.raises(_lib.DQMCError) as e:
            mc.checkerboard_apply(which, l, X)
        assert e.value.code == _lib.ERR_INVALID, (which, l)
    X = np.random.default_rng(1).standard_normal((1, n, n))
    for which in (5, 6):  # the greens() sandwiches read no field: any slice is the same launch
        assert np.array_equal(mc.checkerboard_apply(which, 0, X), mc.checkerboard_apply(which, 99, X))
    mc.close()


@pytest.mark.parametrize("spec", [("chain", 257), ("square", 24)])
def test_the_default_works_where_it_is_chosen(gpu, spec):
    """checkerboard=True above 256 sites is the sparse form: prepare() and one sweep against a dense twin"""
    m = H.model(gpu, spec, "attractive", U=1.0)
    a = gpu.DQMC(m, beta=1.0, n_walkers=1, seed=9, checkerboard=True)
    b = gpu.DQMC(m, beta=1.0, n_walkers=1, seed=9, checkerboard="dense")
    n, qw, _ = SHAPES[spec]
    assert a.checkerboard_plan() == expected_plan(n, qw) and b.checkerboard_plan()["sparse"] == 0
    for mc in (a, b):
        mc.prepare()
        mc.sweep(1)
    assert np.array_equal(a.conf(0), b.conf(0))
    ga, gb = a.greens_eff(0)[0], b.greens_eff(0)[0]
    d, s = np.abs(ga - gb).max(), max(1.0, np.abs(gb).max())
    print("%s: max|dG| %.3g, scale %.3g" % (spec, d, s))
    assert d < 1e-10 * s
    a.close(); b.close()
