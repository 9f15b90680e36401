"""Time-displaced recording on the device (include/dqmc_hip.h; csrc/tdm.hip): the rows a dqmc_accumulate_susceptibilities
pass keeps, through both kernel forms of the Green's rows, the binner and the reduction.

Method of test_gpu_measurement_sizes.py: the matrices the kernels consume come from the device (mc.greens(w); one
CombinedGreensIterator pass read for all walkers, a second pass asserted bit-identical) and go to the numpy reference
tests/time_displaced_ref.py.  Tolerance (derived, not measured): |device - reference| <= 2 (P + 16) eps abs_sum per
element, P the number of terms summed into it (pairs of the direction x walkers x samples), abs_sum the sum of the
absolute values of the same terms.  Non-vacuity, asserted: the largest bound of every observable is at most 1e-9 of its
largest |reference|.  Each case prints its largest err / bound per observable (DESIGN.md section 2 records them).

Sizes, the smallest at which the loops change form (the fast form is 64 directions x 4 column quarters per workgroup):
SquareLattice(4) one partly idle wave; SquareLattice(10), n = 100: two direction groups, the second with 28 idle lanes,
quarters of 25 columns; Chain(257): a fifth direction group for one direction, a last quarter of 62 columns against 65;
SquareLattice(18), n = 324: six groups, the last with 4 directions, and 324 pairs per direction in the pair-list kernels;
Chain(33) with the ring table: n_dirs = 17 != n, unequal pair counts, the general form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measurement_ref as MR  # noqa: E402
import test_gpu_measurement_sizes as MS  # noqa: E402
import time_displaced_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = MS.EPS
KINDS = ["attractive", "repulsive"]
SUS = ("CDS", "SDSx", "SDSy", "SDSz")


def handle(gpu, l, kind, W, beta=MS.BETA, seed=41, first_walker=0, general=False):
    """as test_gpu_measurement_sizes.handle; general: DQMC_TDM_GENERAL=1 while the handle is created (read once there)"""
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    if general:
        os.environ["DQMC_TDM_GENERAL"] = "1"
    try:
        mc = gpu.DQMC(cls(l=l), beta=beta, delta_tau=MS.DELTA_TAU, safe_mult=MS.SAFE_MULT, n_walkers=W, seed=seed,
                      first_walker=first_walker)
    finally:
        os.environ.pop("DQMC_TDM_GENERAL", None)
    mc.prepare()
    mc.update_until_measure()
    return mc


def device_inputs(gpu, mc):
    """G00 and the iterator's tuples of every walker, with the precondition that a second pass gives the same bits"""
    W = mc.n_walkers
    G = [mc.greens(w) for w in range(W)]
    steps, again = MS.read_pass(gpu, mc), MS.read_pass(gpu, mc)
    assert all(np.array_equal(a, b) for w in range(W) for s1, s2 in zip(steps[w], again[w])
               for q1, q2 in zip(s1, s2) for a, b in zip(q1, q2)), "a second iterator pass differs bitwise"
    assert all(np.array_equal(a, b) for w in range(W) for a, b in zip(G[w], mc.greens(w)))
    assert len(steps[0]) == mc.p.slices
    return G, steps


def reference(G, steps, dir_of, nd, every, what):
    """sum over the walkers of the per-walker samples -> {name: (value, abs_sum)}"""
    return MS.sum_walkers([TR.rows(G[w], steps[w], dir_of, nd, every, what) for w in range(len(G))])


def record(mc, every, what, samples=2):
    """set, run `samples` passes, -> [accumulator body after each pass] with the count checked"""
    mc.set_time_displaced(every, what)
    R = 1 + mc.p.slices // every
    assert mc.time_displaced_plan()["rows"] == R and mc.time_displaced_plan()["every"] == every
    assert mc.time_displaced_size() == TR.size(mc.nb, R, mc._ndirs, what) + 1
    out = []
    for s in range(1, samples + 1):
        mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
        raw = mc.time_displaced_raw()
        assert raw[-1] == s * mc.n_walkers
        out.append(raw[:-1])
    return out


def check_rows(rep, tag, mc, bodies, ref, pair_count, what, every):
    nb, nd, R, W = mc.nb, mc._ndirs, 1 + mc.p.slices // every, mc.n_walkers
    for s, body in enumerate(bodies, 1):
        dev = TR.split(body, nb, R, nd, what)
        for k in TR.names(what):
            rep.check(tag + k, dev[k], s * ref[k][0], s * ref[k][1], pair_count * W * s)


def run_case(gpu, case, spec, kind, W, fast, pairs=None):
    l, fp = MS.tables(gpu, spec)
    fp = pairs if pairs is not None else fp
    nd, dir_of = fp.ndirections(), fp.dir_of
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    rep = MS.Report("%s[%s]" % (case, kind))
    mc = handle(gpu, l, kind, W)
    mc.set_pair_directions(fp)
    assert (TR.src_of_table(dir_of, nd) is not None) == fast
    G, steps = device_inputs(gpu, mc)
    ref = reference(G, steps, dir_of, nd, 1, 3)
    bodies = record(mc, 1, 3)
    assert mc.time_displaced_plan() == dict(rows=mc.p.slices + 1, every=1, what=3, fast=int(fast))
    check_rows(rep, "", mc, bodies, ref, pair_count, 3, 1)
    again = record(mc, 1, 3, samples=1)  # set again: sums start at zero; the same state gives the same bits
    assert np.array_equal(again[0], bodies[0]), "a second recording pass differs bitwise"
    td = mc.time_displaced()
    assert td["count"] == W and np.array_equal(td["tau"], np.arange(mc.p.slices + 1) * MS.DELTA_TAU)
    assert np.array_equal(td["Gl0"], TR.split(again[0], mc.nb, mc.p.slices + 1, nd, 3)["Gl0"] / W)
    mc.close()
    print("%s worst err/bound: %s" % (rep.case, ", ".join("%s %.2g" % kv for kv in sorted(rep.worst.items()))))
    return bodies, ref, G


@pytest.mark.parametrize("kind", KINDS)
def test_every_and_what(gpu, kind):
    """SquareLattice(4), 10 slices: every in {1, 2, 5, 10} are row subsets of every = 1, bitwise; GREENS only and
    DENSITY only are the matching parts of the full layout, bitwise"""
    l, fp = MS.tables(gpu, ("square", 4))
    nd, dir_of, W = fp.ndirections(), fp.dir_of, 2
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    rep = MS.Report("A1[%s]" % kind)
    mc = handle(gpu, l, kind, W, beta=1.0)
    assert mc.p.slices == 10
    mc.set_pair_directions(fp)
    G, steps = device_inputs(gpu, mc)
    full = record(mc, 1, 3)
    assert mc.time_displaced_plan()["fast"] == 1
    check_rows(rep, "", mc, full, reference(G, steps, dir_of, nd, 1, 3), pair_count, 3, 1)
    full = TR.split(full[-1], mc.nb, 11, nd, 3)
    for every in (2, 5, 10):
        sub = TR.split(record(mc, every, 3)[-1], mc.nb, 1 + 10 // every, nd, 3)
        for k in sub:
            ax = 1 if k in ("Gl0", "G0l") else 0
            assert np.array_equal(sub[k], np.take(full[k], np.arange(0, 11, every), axis=ax)), (every, k)
    for what in (TR.GREENS, TR.DENSITY):
        part = TR.split(record(mc, 1, what)[-1], mc.nb, 11, nd, what)
        assert sorted(part) == sorted(TR.names(what))
        for k in part:
            assert np.array_equal(part[k], full[k]), (what, k)
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_e1_off_the_tile_grid_and_the_general_form_forced(gpu, kind):
    """SquareLattice(10), W = 3: fast form with idle lanes; then DQMC_TDM_GENERAL=1 on a second handle: the plan
    reports general, and its rows meet the reference and the fast handle's rows under the same bound"""
    spec, W = ("square", 10), 3
    fast_bodies, ref, G = run_case(gpu, "E1", spec, kind, W, True)
    l, fp = MS.tables(gpu, spec)
    nd, dir_of = fp.ndirections(), fp.dir_of
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    rep = MS.Report("E1-general[%s]" % kind)
    mc = handle(gpu, l, kind, W, general=True)
    assert all(np.array_equal(a, b) for w in range(W) for a, b in zip(G[w], mc.greens(w)))
    mc.set_pair_directions(fp)
    bodies = record(mc, 1, 3)
    assert mc.time_displaced_plan()["fast"] == 0
    check_rows(rep, "", mc, bodies, ref, pair_count, 3, 1)
    a, b = (TR.split(x[0], mc.nb, mc.p.slices + 1, nd, 3) for x in (bodies, fast_bodies))
    for k in a:
        rep.check("vs fast " + k, a[k], b[k], ref[k][1], pair_count * W)
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_e2_one_direction_beyond_four_groups(gpu, kind):
    run_case(gpu, "E2", ("chain", 257), kind, 2, True)


@pytest.mark.parametrize("kind", KINDS)
def test_e3_last_group_of_four_directions(gpu, kind):
    run_case(gpu, "E3", ("square", 18), kind, 2, True)


@pytest.mark.parametrize("kind", KINDS)
def test_e4_ring_table_takes_the_general_form(gpu, kind):
    ring = MS.ring_table(33)
    counts = np.bincount(ring.dir_of.ravel(), minlength=17)
    assert ring.ndirections() == 17 and counts[0] == 33 and counts[1] == 66
    run_case(gpu, "E4", ("chain", 33), kind, 2, False, pairs=ring)


@pytest.mark.parametrize("L", [4, 10])
@pytest.mark.parametrize("kind", KINDS)
def test_identities(gpu, kind, L):
    """row 0 = the equal-time correlations; delta_tau sum of the rows r >= 1 = the susceptibilities of the same call;
    a recording handle and a plain one stay bitwise together"""
    l, fp = MS.tables(gpu, ("square", L))
    nd, dir_of, W = fp.ndirections(), fp.dir_of, 2
    pair_count = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    rep = MS.Report("I%d[%s]" % (L, kind))
    mc, plain = handle(gpu, l, kind, W), handle(gpu, l, kind, W)
    for m in (mc, plain):
        m.set_pair_directions(fp)
        m.reset_accumulators()
    mc.set_time_displaced(1, 3)
    G, steps = device_inputs(gpu, mc)
    ref = reference(G, steps, dir_of, nd, 1, TR.DENSITY)
    M = mc.p.slices
    mc.accumulate_correlations()
    corr = mc.correlations_raw()
    for m in (mc, plain):
        m.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    dev = TR.split(mc.time_displaced_raw()[:-1], mc.nb, M + 1, nd, 3)
    sus, cnt = MS.raw_susceptibilities(gpu, mc, nd, 0, 0)
    assert cnt == W and corr[-1] == W
    for i, (k, ks) in enumerate(zip(TR.DENSITY_NAMES, SUS)):
        rep.check(k + " row 0 vs correlations", dev[k][0], corr[i * nd:(i + 1) * nd], ref[k][1][0], pair_count * W)
        rep.check(ks + " vs dtau sum of rows", MS.DELTA_TAU * dev[k][1:].sum(axis=0), sus[ks],
                  MS.DELTA_TAU * ref[k][1][1:].sum(axis=0), pair_count * M * W)
    for m in (mc, plain):
        m.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
        m.sweep(1)
    a, _ = MS.raw_susceptibilities(gpu, mc, nd, 0, 0)
    b, _ = MS.raw_susceptibilities(gpu, plain, nd, 0, 0)
    assert all(np.array_equal(a[k], b[k]) for k in SUS)
    for w in range(W):
        assert all(np.array_equal(x, y) for x, y in zip(mc.greens(w), plain.greens(w)))
        assert np.array_equal(mc.conf(w), plain.conf(w))
        assert mc.uniforms_used(w) == plain.uniforms_used(w)
    mc.close()
    plain.close()


@pytest.mark.parametrize("kind", KINDS)
def test_binner(gpu, kind):
    """SquareLattice(4), W = 3, capacity 8, five pushes with a sweep between them"""
    l, fp = MS.tables(gpu, ("square", 4))
    W, seed = 3, 41
    mc = handle(gpu, l, kind, W, seed=seed)
    mc.set_pair_directions(fp)
    with pytest.raises(gpu.DQMCError) as e:  # recording is off
        mc.enable_binning("time_displaced", capacity=8)
    assert e.value.code == gpu._lib.ERR_STATE
    mc.set_time_displaced(1, 3)
    mc.reset_accumulators()
    mc.enable_binning("time_displaced", capacity=8)
    mc.enable_binning("susceptibilities", capacity=100)
    E = mc.time_displaced_size() - 1
    assert mc.binner_size("time_displaced") == (E, 4, 0)
    singles = [handle(gpu, l, kind, 1, seed=seed, first_walker=w) for w in range(W)]
    samples = [[] for _ in range(W)]
    for s, w in zip(singles, range(W)):
        s.set_pair_directions(fp)
        s.set_time_displaced(1, 3)
        assert all(np.array_equal(a, b) for a, b in zip(s.greens(0), mc.greens(w)))
    for push in range(5):
        for m in [mc] + singles:
            m.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
        for w, s in enumerate(singles):
            raw = s.time_displaced_raw()[:-1]
            samples[w].append(raw - sum(samples[w]) if samples[w] else raw)
        if push < 4:
            for m in [mc] + singles:
                m.sweep(1)
    assert all(np.array_equal(a, b) for w, s in enumerate(singles) for a, b in zip(s.greens(0), mc.greens(w)))
    for s in singles:
        s.close()
    absum = [np.sum(np.abs(x), axis=0) for x in samples]
    for w in range(W):
        xs, _, cnt = mc.binner_level("time_displaced", w, 0)
        assert cnt == 5
        err = np.abs(xs - np.sum(samples[w], axis=0))
        print("B[%s] walker %d: level-0 err/bound = %.3g" % (kind, w, (err / (16 * EPS * absum[w])).max()))
        assert np.all(err <= 16 * EPS * absum[w])
    for lv in range(4):
        assert mc.binner_level("time_displaced", 0, lv)[2] == 5 >> lv
    raw = mc.time_displaced_raw()
    assert raw[-1] == 5 * W
    b = mc.binned("time_displaced")
    assert b["count"] == 5 and b["reliable_level"] == 0 and np.array_equal(b["tau"], np.arange(6) * MS.DELTA_TAU)
    acc = TR.split(raw[:-1], mc.nb, 6, mc._ndirs, 3)
    tot = TR.split(sum(absum), mc.nb, 6, mc._ndirs, 3)
    for k in TR.names(3):
        assert b[k].shape == acc[k].shape and b[k + "_std_error"].shape == acc[k].shape
        assert k + "_std_error_walkers" in b and k + "_tau" in b
        assert np.all(np.abs(b[k] * raw[-1] - acc[k]) <= 16 * EPS * tot[k]), k
    for _ in range(3):
        mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    before = (mc.time_displaced_raw(), MS.raw_susceptibilities(gpu, mc, mc._ndirs, 0, 0),
              mc.binner_size("time_displaced"), mc.binner_size("susceptibilities"))
    assert before[2][2] == 8 and before[3][2] == 8
    with pytest.raises(gpu.DQMCError) as e:  # the ninth push: refused before anything of either section moves
        mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    assert e.value.code == gpu._lib.ERR_STATE
    after = (mc.time_displaced_raw(), MS.raw_susceptibilities(gpu, mc, mc._ndirs, 0, 0),
             mc.binner_size("time_displaced"), mc.binner_size("susceptibilities"))
    assert np.array_equal(before[0], after[0]) and before[1][1] == after[1][1] and before[2:] == after[2:]
    assert all(np.array_equal(before[1][0][k], after[1][0][k]) for k in SUS)
    mc.reset_accumulators()
    assert not mc.time_displaced_raw().any() and mc.binner_size("time_displaced") == (E, 4, 0)
    assert not mc.binner_level("time_displaced", 1, 0)[0].any()
    mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)  # and the handle goes on
    assert mc.time_displaced_raw()[-1] == W and mc.binner_size("time_displaced")[2] == 1
    mc.close()


def test_reduction(gpu):
    l, fp = MS.tables(gpu, ("square", 4))
    mc = handle(gpu, l, "repulsive", 2)
    mc.set_pair_directions(fp)
    mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    off = mc.reduce_size()
    off_buf = mc.reduce_export()
    mc.set_time_displaced(1, 3)
    assert mc.reduce_size() == off + mc.time_displaced_size() - 1
    mc.reset_accumulators()
    for _ in range(2):
        mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    mc.reduce(None)
    local = mc.time_displaced_raw()
    assert local[-1] == 4 and np.array_equal(mc.reduced("time_displaced"), local)
    sus = mc.reduced("susceptibilities")
    buf = mc.reduce_export()  # [... | susceptibilities | time-displaced sums | 6 counters | 4 extrema]
    assert np.array_equal(buf[-10 - (local.size - 1):-10], local[:-1])
    assert np.array_equal(buf[-10 - (local.size - 1) - sus.size:-10 - (local.size - 1)], sus)
    mc.set_time_displaced(0)
    assert mc.reduce_size() == off and mc.time_displaced_size() == 0
    assert not any(mc.time_displaced_plan().values())
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    assert np.array_equal(mc.reduce_export(), off_buf)  # recording off again: the buffer it was
    mc.close()


def test_argument_checks_on_a_live_handle(gpu):
    l, fp = MS.tables(gpu, ("square", 4))
    mc = handle(gpu, l, "attractive", 2, beta=1.0)
    E = gpu._lib
    with pytest.raises(gpu.DQMCError) as e:
        mc.set_time_displaced(1, 3)  # before set_pair_directions
    assert e.value.code == E.ERR_STATE
    mc.set_time_displaced(0)  # off is always accepted
    mc.set_pair_directions(fp)
    mc.set_time_displaced(2, 3)
    plan = mc.time_displaced_plan()
    assert plan == dict(rows=6, every=2, what=3, fast=1)
    for every, what in ((3, 3), (1, 0), (1, 4), (-1, 3), (-2, 1)):
        with pytest.raises(gpu.DQMCError) as e:
            mc.set_time_displaced(every, what)
        assert e.value.code == E.ERR_INVALID, (every, what)
        assert mc.time_displaced_plan() == plan  # the handle keeps its setting ...
        mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)  # ... and keeps working
    assert mc.time_displaced_raw()[-1] == 5 * mc.n_walkers
    mc.set_time_displaced(0)
    with pytest.raises(gpu.DQMCError) as e:
        mc.enable_binning("time_displaced", capacity=8)
    assert e.value.code == E.ERR_STATE
    with pytest.raises(gpu.DQMCError) as e:
        mc.time_displaced_raw()
    assert e.value.code == E.ERR_STATE
    with pytest.raises(gpu.DQMCError) as e:
        mc.run(measurements=("time_displaced",))
    assert e.value.code == E.ERR_STATE
    mc.accumulate_susceptibilities(recalculate=MS.SAFE_MULT)
    mc.close()


def test_run_takes_one_pass_per_measurement(gpu):
    """run(measurements=("susceptibilities", "time_displaced")): both sections count one sample per walker and
    measurement, and binning=True gives error bars for both"""
    l, fp = MS.tables(gpu, ("square", 4))
    mc = gpu.DQMC(gpu.HubbardModelAttractive(l=l), beta=MS.BETA, delta_tau=MS.DELTA_TAU, safe_mult=MS.SAFE_MULT,
                  n_walkers=2, seed=7, thermalization=1, sweeps=4, measure_rate=2)
    mc.set_pair_directions(fp)
    mc.set_time_displaced(1, ("greens", "density"))
    mc.run(measurements=("susceptibilities", "time_displaced"), binning=True)
    assert mc.time_displaced_raw()[-1] == 2 * 2 and mc.susceptibilities()["count"] == 2 * 2
    assert mc.binner_size("time_displaced")[2] == 2 and mc.binner_size("susceptibilities")[2] == 2
    td, b = mc.time_displaced(), mc.binned("time_displaced")
    assert td["Gl0"].shape == (1, 6, fp.ndirections()) and td["CDC"].shape == (6, fp.ndirections())
    assert np.allclose(b["CDC"], td["CDC"], rtol=1e-12, atol=1e-14)
    mc.close()
