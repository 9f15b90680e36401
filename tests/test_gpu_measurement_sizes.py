"""The measurement kernels beyond 4 x 4: the strided pair loops of corr_pairs / pairing / sus_pairs / sus_pairing /
cc_pairs, the grid-stride trip of accumulate_kernel and every launch plan of cc_lds_kernel (several chunks per
workgroup, partial last chunk and workgroup, more than 256 threads, missing targets).

Inputs come from the device, only the sums are under test: every case reads the matrices the kernels consume
(mc.greens(w); one CombinedGreensIterator pass read with dqmc_ut_get for all walkers), feeds them to
tests/measurement_ref.py and compares.  Precondition, asserted per handle: a second pass yields bit-identical matrices.

Tolerance (derived, not measured): |device - reference| <= 2 (P + 16) eps abs_sum per element, P the number of terms
summed into the element (pairs of the direction, times steps for the time-displaced sums, times walkers), abs_sum the
sum of the absolute values of the same terms: device and reference each sum at most P terms of fewer than 16 flops in
some order.  Non-vacuity, asserted: the largest bound of every observable is at most 1e-9 of its largest |reference|.
Each case prints its largest err / bound per observable (DESIGN.md section 2 records them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_tables as LT  # noqa: E402
import measurement_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BETA, DELTA_TAU, SAFE_MULT = 0.5, 0.1, 5

_tables = {}


def tables(gpu, spec):
    """(lattice, fast_pairs) of ("square", L) / ("chain", n), built once"""
    if spec not in _tables:
        l = gpu.SquareLattice(spec[1]) if spec[0] == "square" else gpu.Chain(spec[1])
        _tables[spec] = (l, LT.fast_pairs(l))
    return _tables[spec]


def ring_table(n):
    """dir_of = min(|i - j|, n - |i - j|): both senses of a distance share a direction, so n_dirs = n // 2 + 1 != n"""
    d = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
    return LT.Tables(np.minimum(d, n - d), n // 2 + 1)


def holes(trg_of, seed):
    """a seeded 20 % of the entries set to -1, source 7 without any target, direction 3 missing for every source"""
    t = trg_of.copy()
    t[np.random.default_rng(seed).random(t.shape) < 0.2] = -1
    t[7, :] = -1
    t[:, 3] = -1
    return t


def handle(gpu, l, kind, W, seed=41):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(l=l), beta=BETA, delta_tau=DELTA_TAU, safe_mult=SAFE_MULT, n_walkers=W, seed=seed)
    mc.prepare()
    mc.update_until_measure()  # G of a field the sweep has worked on, current_slice == 1
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


class Report:
    def __init__(self, case):
        self.case, self.worst = case, {}

    def check(self, name, dev, ref, ab, P):
        """|dev - ref| <= 2 (P + 16) eps abs_sum elementwise; the bound is small against the values"""
        dev, ref, ab = np.asarray(dev, dtype=float), np.asarray(ref, dtype=float), np.asarray(ab, dtype=float)
        assert dev.shape == ref.shape == ab.shape, (self.case, name, dev.shape, ref.shape)
        bound = 2.0 * (np.asarray(P, dtype=float) + 16.0) * EPS * ab
        err = np.abs(dev - ref)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        self.worst[name] = max(self.worst.get(name, 0.0), ratio)
        print("%s %s: err/bound = %.3g (max err %.3g, max |ref| %.3g)" % (self.case, name, ratio, err.max(), np.abs(ref).max()))
        assert bound.max() <= 1e-9 * np.abs(ref).max(), (self.case, name, "vacuous bound", bound.max(), np.abs(ref).max())
        assert ratio <= 1.0, (self.case, name, ratio, err.max())


def sum_walkers(per_walker):
    """[{name: (value, abs_sum)}, ...] -> {name: (sum of values, sum of abs_sums)}"""
    return {k: (sum(r[k][0] for r in per_walker), sum(r[k][1] for r in per_walker)) for k in per_walker[0]}


def quad_terms(dir_of, nd, trg_of, synced):
    """number of quads summed into every element of PS [nd, K, K] / CCS [nd, K]"""
    ok = (trg_of >= 0).astype(float)
    K = trg_of.shape[1]
    cnt = lambda k1, k2: np.bincount(dir_of.ravel(), weights=np.outer(ok[:, k1], ok[:, k2]).ravel(), minlength=nd)
    if synced:
        return np.stack([cnt(k, k) for k in range(K)], axis=1)
    return np.stack([np.stack([cnt(k1, k2) for k2 in range(K)], axis=1) for k1 in range(K)], axis=1)


def raw_sums(mc, size_fn, get_fn):
    """the accumulator of a section as the device holds it: sums, then the sample count"""
    size = C.c_size_t()
    mc._c(size_fn(mc._h, C.byref(size)))
    out = np.zeros(size.value)
    mc._c(get_fn(mc._h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def raw_susceptibilities(gpu, mc, nd, K_loc, K_cc):
    """-> (dict of raw sums in the layout of include/dqmc_hip.h, sample count)"""
    raw = raw_sums(mc, gpu.lib().dqmc_susceptibilities_size, gpu.lib().dqmc_get_susceptibilities)
    assert raw.size == 4 * nd + nd * K_loc * K_loc + nd * K_cc + 1
    res = {k: raw[i * nd:(i + 1) * nd] for i, k in enumerate(("CDS", "SDSx", "SDSy", "SDSz"))}
    off = 4 * nd
    if K_loc:
        res["PS"] = raw[off:off + nd * K_loc * K_loc].reshape((nd, K_loc, K_loc), order="F")
        off += nd * K_loc * K_loc
    if K_cc:
        res["CCS"] = raw[off:off + nd * K_cc].reshape((nd, K_cc), order="F")
    return res, raw[-1]


def run_case(gpu, case, spec, kind, W, plan, K_cc, K_loc=0, pairs=None, punch=False):
    """plan: None = the general kernel, else (C, chunks, chunks per workgroup, workgroups, threads) of cc_lds_kernel"""
    l, fp = tables(gpu, spec)
    std = fp
    fp = pairs if pairs is not None else fp
    n, nd, dir_of = l.sites, fp.ndirections(), fp.dir_of
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    rep = Report("%s[%s]" % (case, kind))
    mc = handle(gpu, l, kind, W)
    nb, T = mc.nb, mc.model.hopping_matrix()
    loc = None
    punched = holes(LT.fast_quads(l, 9, pairs=std).trg_of, 3) if punch else None  # one table for PS and CCS
    mc.set_pair_directions(fp)
    if K_loc:
        loc = LT.QuadTables(fp, punched[:, :K_loc] if punch else LT.fast_quads(l, K_loc, pairs=std).trg_of)
        mc.set_local_targets(loc)
    cc = LT.QuadTables(fp, punched[:, :K_cc] if punch else LT.fast_quads(l, K_cc, pairs=std).trg_of, synced=True)
    mc.set_current_targets(cc)
    expect = LT.cc_plan(n, K_cc, W, cc.trg_of, dir_of, nd)  # the restatement and the engine's own plan agree
    got = mc.current_targets_plan()
    fast = expect is not None
    assert mc.current_targets_fast_path() == fast
    if fast:
        assert got["fast"] == 1 and all(got[k] == expect[k] for k in expect), (got, expect)
    else:
        assert not any(got.values()), got
    assert LT.plan_tuple(expect) == plan, (case, expect)  # and both give the form this case is here for
    print("%s plan: %s" % (rep.case, got))
    mc.reset_accumulators()

    # ---- equal time: accumulate_kernel, corr_pairs / corr_reduce, pairing / pairing_reduce on mc.greens(w)
    G = [mc.greens(w) for w in range(W)]
    for sample in (1, 2):
        mc.accumulate_greens()
        mc.accumulate_correlations()
        if loc:
            mc.accumulate_pairing()
        acc = mc.accumulators()
        assert acc[-1] == sample * W
        ref = MR.greens_sums(G)
        per = nb * n * n
        rep.check("G", acc[:per], sample * ref["G"][0], ref["G"][1], W)
        rep.check("G2", acc[per:2 * per], sample * ref["G2"][0], ref["G2"][1], W)
        rep.check("occupation", acc[2 * per:2 * per + nb * n], sample * ref["occupation"][0], ref["occupation"][1], W)
        raw = mc.correlations_raw()
        assert raw[-1] == sample * W
        ref = sum_walkers([MR.equal_time(g, dir_of, nd) for g in G])
        for i, k in enumerate(("CDC", "SDCx", "SDCy", "SDCz")):
            rep.check(k, raw[i * nd:(i + 1) * nd], sample * ref[k][0], ref[k][1], pair_count * W)
        for i, k in enumerate(("Mx", "My", "Mz")):
            dev = raw[4 * nd + i * n:4 * nd + (i + 1) * n]
            if k == "Mz" and nb == 2:
                rep.check(k, dev, sample * ref[k][0], ref[k][1], W)
            else:
                assert not dev.any() and not ref[k][0].any(), k
        if loc:
            raw = raw_sums(mc, gpu.lib().dqmc_pairing_size, gpu.lib().dqmc_get_pairing)
            assert raw[-1] == sample * W
            val, ab = (sum(x) for x in zip(*[MR.pairing(g, dir_of, nd, loc.trg_of) for g in G]))
            rep.check("PC", raw[:-1].reshape((nd, K_loc, K_loc), order="F"), sample * val, ab,
                      quad_terms(dir_of, nd, loc.trg_of, False) * W)

    # ---- time-displaced: sus_pairs, sus_pairing, cc_b + cc_lds / cc_pairs + cc_fold on one iterator pass
    steps = read_pass(gpu, mc)
    again = read_pass(gpu, mc)
    assert all(np.array_equal(a, b) for w in range(W) for s1, s2 in zip(steps[w], again[w])
               for q1, q2 in zip(s1, s2) for a, b in zip(q1, q2)), "a second iterator pass differs bitwise"
    assert all(np.array_equal(a, b) for w in range(W) for a, b in zip(G[w], mc.greens(w)))
    del again
    M = len(steps[0])
    assert M == mc.p.slices == 5
    ref = sum_walkers([MR.susceptibilities(T, G[w], steps[w], dir_of, nd, DELTA_TAU, trg_loc=loc.trg_of if loc else None,
                                           trg_cc=cc.trg_of) for w in range(W)])
    terms = {k: pair_count * M * W for k in ("CDS", "SDSx", "SDSy", "SDSz")}
    if loc:
        terms["PS"] = quad_terms(dir_of, nd, loc.trg_of, False) * M * W
    terms["CCS"] = quad_terms(dir_of, nd, cc.trg_of, True) * M * W
    first = None
    for sample in (1, 2):
        mc.accumulate_susceptibilities(recalculate=SAFE_MULT)
        res, cnt = raw_susceptibilities(gpu, mc, nd, K_loc, K_cc)
        assert cnt == sample * W and sorted(res) == sorted(terms)
        for k in terms:
            rep.check(k, res[k], sample * ref[k][0], ref[k][1], terms[k])
        first = first if first is not None else res
    mc.close()

    # ---- wherever the LDS kernel ran: the same CCS from a handle forced onto the general kernel by K = 9 tables with
    # the same first columns
    if fast:
        mc2 = handle(gpu, l, kind, W)
        assert all(np.array_equal(a, b) for w in range(W) for a, b in zip(G[w], mc2.greens(w)))
        trg9 = punched if punch else LT.fast_quads(l, 9, pairs=std).trg_of
        assert np.array_equal(trg9[:, :K_cc], cc.trg_of)
        mc2.set_current_targets(LT.QuadTables(fp, trg9, synced=True))
        assert not mc2.current_targets_fast_path() and not any(mc2.current_targets_plan().values())
        mc2.reset_accumulators()
        mc2.accumulate_susceptibilities(recalculate=SAFE_MULT)
        r2, cnt = raw_susceptibilities(gpu, mc2, nd, 0, 9)
        assert cnt == W
        gen = r2["CCS"][:, :K_cc]
        rep.check("CCS general vs reference", gen, ref["CCS"][0], ref["CCS"][1], terms["CCS"])
        rep.check("CCS general vs fast", gen, first["CCS"], ref["CCS"][1], terms["CCS"])
        mc2.close()
    print("%s worst err/bound: %s" % (rep.case, ", ".join("%s %.2g" % kv for kv in sorted(rep.worst.items()))))


KINDS = ["attractive", "repulsive"]


@pytest.mark.parametrize("kind", KINDS)
def test_e1_off_the_tile_grid(gpu, kind):
    """SquareLattice(10), n = 100, 3 walkers: every sum with n off the tile grid; Mz over 3 blocks of corr_reduce"""
    run_case(gpu, "E1", ("square", 10), kind, 3, (16, 7, 1, 7, 128), K_cc=5, K_loc=5)


@pytest.mark.parametrize("kind", KINDS)
def test_e2_second_trip_of_one_thread(gpu, kind):
    """Chain(257): 257 pairs per direction, so thread 0 makes a second trip; repulsive accumulate_greens has
    nb n n = 132098 > 131072 entries, the last 1026 of them (diagonal entries among them) on the grid-stride trip"""
    run_case(gpu, "E2", ("chain", 257), kind, 2, (8, 33, 1, 33, 320), K_cc=3, K_loc=3)


@pytest.mark.parametrize("kind", KINDS)
def test_e3_second_trip_of_68_threads(gpu, kind):
    """SquareLattice(18), n = 324: 324 pairs per direction in all five pair kernels"""
    run_case(gpu, "E3", ("square", 18), kind, 2, (2, 162, 1, 162, 384), K_cc=5, K_loc=5)


def test_e4_three_trips_and_the_general_cc_kernel(gpu):
    """Chain(257) with the hand-made ring table (129 directions of 514 pairs, direction 0 of 257): three trips, the
    last partial; n_dirs != n sends CCS to cc_pairs_kernel"""
    run_case(gpu, "E4", ("chain", 257), "attractive", 2, None, K_cc=3, K_loc=3, pairs=ring_table(257))


@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_f1_partial_last_chunk(gpu, kind, K):
    """SquareLattice(6), n = 36: chunks of 16 / 16 / 4 sources; K = 8 fills CC_KMAX"""
    run_case(gpu, "F1-K%d" % K, ("square", 6), kind, 2, (16, 3, 1, 3, 64), K_cc=K, K_loc=5)


@pytest.mark.parametrize("kind", KINDS)
def test_f2_last_chunk_of_one_source(gpu, kind):
    run_case(gpu, "F2", ("chain", 33), kind, 2, (16, 3, 1, 3, 64), K_cc=5, K_loc=3)


@pytest.mark.parametrize("kind", KINDS)
def test_f3_two_chunks_in_one_workgroup(gpu, kind):
    """SquareLattice(6) with 256 walkers: 2 workgroups per walker, the first with two chunks (bins carried across
    chunks, the barrier at the loop head), the last with one"""
    run_case(gpu, "F3", ("square", 6), kind, 256, (16, 3, 2, 2, 64), K_cc=5)


@pytest.mark.parametrize("kind", KINDS)
def test_f4_inactive_threads_above_256(gpu, kind):
    """Chain(257), K = 5: C = 8, 33 chunks, 320 threads of which 63 are inactive, last chunk of one source"""
    run_case(gpu, "F4", ("chain", 257), kind, 2, (8, 33, 1, 33, 320), K_cc=5)


@pytest.mark.parametrize("kind,W,plan", [("attractive", 1, (1, 576, 2, 288, 576)), ("repulsive", 2, (1, 576, 3, 192, 576))])
def test_f5_production_lattice(gpu, kind, W, plan):
    """SquareLattice(24), n = 576: C = 1, nine waves, two resp. three chunks per workgroup"""
    run_case(gpu, "F5", ("square", 24), kind, W, plan, K_cc=5)


def test_g1_lds_budget_refuses(gpu):
    """SquareLattice(24), K = 7: no chunk size fits the LDS budget; cc_pairs_kernel with 576 pairs per direction"""
    run_case(gpu, "G1", ("square", 24), "attractive", 1, None, K_cc=7)


@pytest.mark.parametrize("K,plan", [(5, (16, 3, 1, 3, 64)), (9, None)])
@pytest.mark.parametrize("kind", KINDS)
def test_h1_missing_targets(gpu, kind, K, plan):
    """SquareLattice(6) with holes in the target tables: every t < 0 / j1 < 0 branch of cc_b_kernel, cc_lds_kernel
    (K = 5) and cc_pairs_kernel (K = 9), and of the pairing kernels through set_local_targets"""
    run_case(gpu, "H1-K%d" % K, ("square", 6), kind, 2, plan, K_cc=K, K_loc=5, punch=True)
