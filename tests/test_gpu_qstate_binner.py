"""The binner of the q-state engine on the device (csrc/qstate.hip: qs_bin_push in the BIN forms of the sweep kernel and in
qs_exchange_kernel) against the numpy restatement of tests/qstate_binner_ref.py, with the comparison rules of
test_gpu_qstate_tempering.py: every sum bit for bit except those that inherit the device's sqrt (1e-13 relative)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_binner_ref as bref  # noqa: E402
from test_gpu_qstate_tempering import check, pair  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,k", [(0, 0), (3, 2)])
def test_capacity_seven_filled_exactly_then_refused(gpu, R, k):
    """three levels; the eighth measurement is refused with DQMC_ERR_STATE before anything runs"""
    from montecarlo_jl_amd import _lib
    l = gpu.SquareLattice(3)
    mc, wk = pair(gpu, l, "potts", 3, [0.9, 1.0, 1.1], R, k, binner=7, cluster_rate=3)
    assert mc.binner_size() == (3, 0)
    with pytest.raises(gpu.DQMCError) as ei:
        mc.sweep(8)
    assert ei.value.code == _lib.ERR_STATE and "capacity" in str(ei.value)
    assert mc.stats(0).sweeps_drawn == 0 and mc.binner_size() == (3, 0)
    mc.sweep(3)
    mc.sweep(4)
    wk.run(1, 7, 0, 1, cluster_rate=3)
    check(mc, wk, "filled")
    assert mc.binner_size() == (3, 7) and [mc.binner_level(1, lv)[3] for lv in range(3)] == [7, 3, 1]
    with pytest.raises(gpu.DQMCError) as ei:
        mc.sweep(1)
    assert ei.value.code == _lib.ERR_STATE
    check(mc, wk, "after the refusal")  # nothing ran
    mc.reset_accumulators()
    wk.reset_accumulators()
    check(mc, wk, "after reset")
    assert mc.binner_size() == (3, 0)
    assert mc.last_sweep == 7  # (the refused calls did not advance it)
    mc.sweep(2)
    wk.run(8, 2, 0, 1, cluster_rate=3)
    check(mc, wk, "two more")
    mc.close()


@pytest.mark.parametrize("R,k", [(0, 0), (2, 7)])
def test_pushes_across_a_launch_boundary(gpu, R, k):
    """SquareLattice(4): a launch runs at most 2^19 / (16 + 512) = 992 sweeps, so the 100 pushes of 1100 sweeps (every 11th
    measured) come from two launches of the work bound; with k = 7 from many, and from both kernels (sweep 77 = 7 * 11 is
    measured by the exchange kernel)"""
    l = gpu.SquareLattice(4)
    mc, wk = pair(gpu, l, "clock", 5, [0.95, 1.05], R, k, binner=100, measure_rate=11, cap=100)
    mc.sweep(1100)
    wk.run(1, 1100, 0, 11)
    check(mc, wk, (R, k))
    assert mc.binner_size() == (7, 100) and mc.binner_reliable_level() == 1
    # finish and binned against the restatement's formulas on equal or near-equal sums
    for w in range(2):
        for level in (None, 0, 3):
            got, want = mc.binner_finish(w, level), wk.bin.finish(w, level)
            assert (got.count, got.level) == (want["count"], want["level"])
            for key in ("mean", "varN", "varN0", "tau", "covN"):
                g, r = np.array(getattr(got, key)), want[key]
                assert np.all(np.abs(g - r) <= 1e-12 * np.abs(r)), (w, level, key, g, r)
        b, f = mc.binned(w), wk.bin.finish(w)
        beta, N = float(mc.betas[w]), len(l)
        E, E2, M, M2, _, M4 = f["mean"]
        want = {"E": (E, f["varN"][0]), "E2": (E2, f["varN"][1]), "e": (E / N, f["varN"][0] / N ** 2),
                "C": (beta ** 2 / N * (E2 - E * E),
                      (beta ** 2 / N) ** 2 * (f["varN"][1] - 4 * E * f["covN"][0] + 4 * E * E * f["varN"][0])),
                "M": (M, f["varN"][2]), "M2": (M2, f["varN"][3]), "M4": (M4, f["varN"][5]), "m": (M / N, f["varN"][2] / N ** 2),
                "chi": (beta / N * (M2 - M * M),
                        (beta / N) ** 2 * (f["varN"][3] - 4 * M * f["covN"][1] + 4 * M * M * f["varN"][2])),
                "U4": (1 - M4 / (2 * M2 * M2),
                       (M4 / M2 ** 3) ** 2 * f["varN"][4] + f["varN"][5] / (2 * M2 * M2) ** 2
                       - 2 * (M4 / M2 ** 3) / (2 * M2 * M2) * f["covN"][2])}
        # std_error of C, chi and U4: three terms of either sign from inputs equal to 1e-12, summed in another order; with
        # a cancellation of up to 1e3 between them the variance agrees to 1e-9, far below any use of an error bar
        for group in ("Energy", "Magn"):
            for name, o in b[group].items():
                mean, var = want[name]
                assert abs(o["mean"] - mean) <= 1e-12 * abs(mean), (name, o, mean)
                assert abs(o["std_error"] - math.sqrt(max(var, 0.0))) <= 1e-9 * math.sqrt(abs(var)) + 1e-300, (name, o, var)
                assert "tau" in o
        assert abs(b["Energy"]["E"]["tau"] - f["tau"][0]) <= 1e-12 * abs(f["tau"][0])
        assert math.isnan(b["Energy"]["C"]["tau"]) and b["count"] == 50 and b["level"] == 1
        m = mc.measurements(w)  # the plain means are the binner's
        assert abs(m["Energy"]["E"] - b["Energy"]["E"]["mean"]) <= 1e-12 * abs(m["Energy"]["E"])
    pooled = mc.binned(walkers=[0]) if R == 0 else None
    assert pooled is None or pooled["n_walkers"] == 1
    with pytest.raises(ValueError, match="share one beta"):
        mc.binned(walkers=[0, 1])
    mc.close()


def test_the_binner_leaves_everything_else_alone_and_can_be_enabled_late(gpu):
    l = gpu.TriangularLattice(4)
    betas = [0.5, 0.6, 0.7]
    on, wk = pair(gpu, l, "potts", 3, betas, 3, 2, binner=16, cluster_rate=2)
    off, wk_off = pair(gpu, l, "potts", 3, betas, 3, 2, cluster_rate=2)
    on.sweep(9)
    off.sweep(9)
    wk.run(1, 9, 0, 1, cluster_rate=2)
    wk_off.run(1, 9, 0, 1, cluster_rate=2)
    check(on, wk, "on")
    check(off, wk_off, "off")
    for w in range(3):
        a, b = on.stats(w), off.stats(w)
        assert all(getattr(a, k) == getattr(b, k) for k, _ in a._fields_)
    with pytest.raises(gpu.DQMCError, match="binner is not enabled"):
        off.binner_size()
    off.enable_binning(4)  # from now on
    wk_off.bin = bref.QsBinnerRef(3, 4)
    off.sweep(4)
    wk_off.run(10, 4, 0, 1, cluster_rate=2)
    check(off, wk_off, "enabled late")
    on.enable_binning()  # enabling again starts anew, with the default capacity
    assert on.binner_size() == (17, 0)
    on.close()
    off.close()
