"""The host layer under the two classical-MC engines (csrc/mc_host.h, csrc/mc_tables.h) on the device: the binner
sections and the colour tables are allocated, released and re-made by one piece of code now, so a handle that reached its
configuration through every one of those paths must be the handle that was created with it.  Everything is compared
with ==, NaN equal to NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flat(x):
    """the numbers of a nested result, in order"""
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _flat(x[k])]
    if isinstance(x, (list, tuple, np.ndarray)):
        return [v for y in x for v in _flat(y)]
    return [float(x)]


def _same(a, b):
    return np.array_equal(np.array(_flat(a)), np.array(_flat(b)), equal_nan=True)


def test_an_ising_handle_configured_in_steps_is_the_one_configured_in_one_go(gpu):
    """8 x 8, 4 walkers, 5 + 40 sweeps.  In steps: binning on; FSS on afterwards (the binner restarts with its FSS
    section); binning again with another capacity (both sections re-made); two valid colourings one after the other
    (the first one's tables released); a few sweeps, so that there is something to forget; reset_accumulators; every
    walker reseeded and redrawn.  In one go: the constructor with the final settings."""
    l = gpu.SquareLattice(8)
    model = gpu.IsingModel(l=l)
    W, seed, therm, n = 4, 31, 5, 45
    betas = np.linspace(0.36, 0.5, W)
    i, j = np.arange(64) % 8, np.arange(64) // 8
    two, four = ((i + j) % 2).astype(np.int32), ((i % 2) + 2 * (j % 2)).astype(np.int32)
    kw = dict(beta=betas, n_walkers=W, seed=seed, thermalization=therm, series_capacity=64)

    steps = gpu.MC(model, **kw)
    steps.enable_binning(1000)
    steps.set_fss(True)
    assert steps.binner_size() == (10, 0)
    steps.enable_binning(200)
    steps.set_update("checkerboard", two)
    steps.set_update("checkerboard", four)
    steps.sweep(9)
    assert steps.binner_size() == (8, 4) and steps.fss_sums(0).n_meas == 4
    steps.reset_accumulators()
    for w in range(W):
        steps.seed(w, seed + w)
    steps.rand_conf(-1)
    steps.last_sweep = 0

    fresh = gpu.MC(model, binning=True, binning_capacity=200, fss=True, update="checkerboard", colouring=four, **kw)
    for mc in (steps, fresh):
        mc.sweep(n)
    assert steps.binner_size() == fresh.binner_size() == (8, n - therm)
    for w in range(W):
        assert np.array_equal(steps.conf(w), fresh.conf(w)), w
        assert [list(x) for x in steps.series(w)] == [list(x) for x in fresh.series(w)], w
        assert len(fresh.series(w)[0]) == n - therm
        assert _same(steps.binned(w), fresh.binned(w)), w
        assert _same(steps.binned_fss(w), fresh.binned_fss(w)), w
        assert _same(steps.measurements(w), fresh.measurements(w)) and _same(steps.fss(w), fresh.fss(w)), w
        for level in range(8):  # and the raw sums of every level of both sections
            assert _same(steps.binner_level(w, level), fresh.binner_level(w, level)), (w, level)
            assert _same(steps.fss_binner_level(w, level), fresh.fss_binner_level(w, level)), (w, level)
        u = steps.update_stats(w)
        assert (u.kind, u.n_colours, u.sweeps_drawn) == (1, 4, n)
    assert fresh.binned(0)["count"] == n - therm and np.isfinite(_flat(fresh.binned_fss(1)["M4"])).all()
    steps.close()
    fresh.close()


def test_a_refused_colouring_leaves_no_trace_in_a_qstate_handle(gpu):
    """Potts q = 3 on 8 x 8: sweeps, a set_colouring that is refused, more sweeps, against a handle that never saw the
    refused call (the tables of a colouring are built in full before the handle is touched)"""
    l = gpu.SquareLattice(8)
    kw = dict(beta=[0.9, 1.05], n_walkers=2, seed=77, thermalization=2, series_capacity=32)
    a, b = (gpu.MC(gpu.PottsModel(3, l=l), **kw) for _ in range(2))
    clash = a.colouring.copy()
    clash[9] = clash[8]  # neighbours in a row
    for mc in (a, b):
        mc.sweep(5)
    with pytest.raises(gpu.DQMCError) as ei:
        a.set_colouring(clash)
    assert ei.value.code == -1 and "share colour" in str(ei.value) and "dqmc_qs_set_colouring" in str(ei.value)
    with pytest.raises(gpu.DQMCError):
        a.set_colouring(np.arange(64) % 17)  # 17 colours
    assert np.array_equal(a.colouring, b.colouring)
    for mc in (a, b):
        mc.sweep(10)
    names = [f[0] for f in a.stats(0)._fields_]
    for w in range(2):
        sa, sb = a.stats(w), b.stats(w)
        assert [getattr(sa, k) for k in names] == [getattr(sb, k) for k in names], w
        assert np.array_equal(a.conf(w), b.conf(w)), w
        assert [list(x) for x in a.series(w)] == [list(x) for x in b.series(w)] and len(a.series(w)[0]) == 13, w
    assert a.stats(0).n_meas == 13 and a.stats(0).n_colours == 2
    a.close()
    b.close()
