"""The accumulator section table of the engine (dqmc_handle::sec): Green's sums, correlations, pairing,
susceptibilities and time-displaced rows, each through its size / host get / device export entry points, the packed
reduction, the reset, the binners, and the setters that rebuild a layout.

Every case: SquareLattice(4) (n = 16), 2 walkers, 10 slices with safe_mult 5, both models (the Green's section's sizes
depend on the number of blocks), all five sections configured (pair directions, local targets, current targets, the
unequal-time stack, time-displaced recording with every = 5 and both parts), a binner on each, each accumulated twice
with a sweep in between.  All comparisons are between two reads of the same device sums, hence bitwise.

One point is stated as the library behaves and not as first written down: right after dqmc_set_pair_directions,
dqmc_get_reduced answers "call dqmc_reduce first" (the setter voids the reduction), with DQMC_ERR_STATE; the message
"accumulators were reconfigured after the last reduction" is what a reduction brought in by dqmc_reduce_import meets when
the layout has changed since it was packed.  test_retabling_voids_the_reduction_and_the_binners asserts both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_tables as LT  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["attractive", "repulsive"]
SECTIONS = ("greens", "correlations", "pairing", "susceptibilities", "time_displaced")
STEM = dict(greens="accumulators", correlations="correlations", pairing="pairing", susceptibilities="susceptibilities",
            time_displaced="time_displaced")
NEED = dict(correlations="call dqmc_set_pair_directions first", pairing="call dqmc_set_local_targets first",
            susceptibilities="nothing accumulated", time_displaced="call dqmc_set_time_displaced first")
CAPACITY = 15


def fresh(gpu, kind):
    cls = gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive
    mc = gpu.DQMC(cls(4, 2), beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=7)
    assert (mc.N, mc.p.slices, mc.nb) == (16, 10, 1 if kind == "attractive" else 2)
    mc.prepare()
    mc.update_until_measure()
    return mc


def accumulate_all(mc):
    mc.accumulate_greens()
    mc.accumulate_correlations()
    mc.accumulate_pairing()
    mc.accumulate_susceptibilities(recalculate=5)  # feeds the time-displaced rows as well


def configured(gpu, kind):
    mc = fresh(gpu, kind)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))  # the pair directions with them
    mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(mc.model.l))
    mc.set_time_displaced(5, ("greens", "density"))
    mc.enable_binning(SECTIONS, capacity=CAPACITY)
    accumulate_all(mc)
    mc.update_until_measure()
    accumulate_all(mc)
    return mc


def size(gpu, mc, sec):
    n = C.c_size_t()
    stem = "accumulator" if sec == "greens" else STEM[sec]
    mc._c(getattr(gpu.lib(), "dqmc_%s_size" % stem)(mc._h, C.byref(n)))
    return n.value


def host_get(gpu, mc, sec, n, fill=np.nan):
    out = np.full(n + 1, fill)  # one double more than the section: the getter must leave it alone
    rc = getattr(gpu.lib(), "dqmc_get_" + STEM[sec])(mc._h, out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def device_export(gpu, mc, sec, n):
    buf = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = getattr(gpu.lib(), "dqmc_export_" + STEM[sec])(mc._h, C.c_void_p(buf.data_ptr()))
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


LOCAL = dict(greens="accumulators", correlations="correlations_raw", time_displaced="time_displaced_raw")


def local(gpu, mc, sec):
    """the section's sums through the package's own getter where it has a raw one, else through the C getter"""
    if sec in LOCAL:
        return getattr(mc, LOCAL[sec])()
    rc, out = host_get(gpu, mc, sec, size(gpu, mc, sec))
    mc._c(rc)
    return out[:-1]


@pytest.fixture(scope="module", params=KINDS)
def done(request, gpu):
    """a configured handle with two samples per section and a local reduction; the tests that use it only read"""
    mc = configured(gpu, request.param)
    mc.reduce(None)
    yield mc
    mc.close()


def test_size_get_and_export_agree(gpu, done):
    mc = done
    nd, n, nb, K = mc._ndirs, mc.N, mc.nb, mc._K
    plan = mc.time_displaced_plan()
    assert (plan["rows"], plan["every"], plan["what"]) == (3, 5, 3)
    want = dict(greens=2 * nb * n * n + nb * n + 1, correlations=4 * nd + 3 * n + 1, pairing=nd * K * K + 1,
                susceptibilities=4 * nd + nd * K * K + nd * mc._Kcc + 1, time_displaced=(2 * nb + 4) * 3 * nd + 1)
    for sec in SECTIONS:
        cnt = size(gpu, mc, sec)
        assert cnt == want[sec], sec
        rc, host = host_get(gpu, mc, sec, cnt)
        assert rc == 0 and np.isnan(host[cnt]) and not np.isnan(host[:cnt]).any(), sec  # fills exactly `size` doubles
        assert host[cnt - 1] == 2 * mc.n_walkers, sec                                  # two samples of every walker
        assert np.array_equal(host[:cnt], local(gpu, mc, sec)), sec
        rc, dev = device_export(gpu, mc, sec, cnt)
        assert rc == 0 and np.isnan(dev[cnt]), sec
        assert np.array_equal(dev[:cnt], host[:cnt]), sec
        assert mc.binner_size(sec)[2] == 2, sec


def test_reduction_of_one_handle_equals_the_local_sums(gpu, done):
    mc = done
    packed = 0
    for sec in SECTIONS[:4]:
        loc = local(gpu, mc, sec)
        assert np.array_equal(mc.reduced(sec), loc), sec
        packed += loc.size
    td, sus = mc.time_displaced_raw(), local(gpu, mc, "susceptibilities")
    assert np.array_equal(mc.reduced("time_displaced"), np.concatenate([td[:-1], sus[-1:]]))
    packed += td.size - 1  # the time-displaced count is not packed
    assert mc.reduce_size() == packed + 6 + 4
    buf = mc.reduce_export()
    assert buf.size == packed + 10
    off = 0
    for sec in SECTIONS:  # the sections in DQMC_RED_* order, back to back
        loc = local(gpu, mc, sec)[:None if sec != "time_displaced" else -1]
        assert np.array_equal(buf[off:off + loc.size], loc), sec
        off += loc.size


@pytest.mark.parametrize("kind", KINDS)
def test_reset_zeroes_every_section_and_binner(gpu, kind):
    mc = configured(gpu, kind)
    before = {sec: mc.binner_size(sec) for sec in SECTIONS}
    sizes = {sec: size(gpu, mc, sec) for sec in SECTIONS}
    mc.reset_accumulators()
    for sec in SECTIONS:
        assert size(gpu, mc, sec) == sizes[sec], sec
        loc = local(gpu, mc, sec)
        assert loc.size == sizes[sec] and not loc.any(), sec
        E, L, T = mc.binner_size(sec)
        assert (E, L) == before[sec][:2] and before[sec][2] == 2 and T == 0, sec
    accumulate_all(mc)  # and the sections take samples again
    for sec in SECTIONS:
        assert local(gpu, mc, sec)[-1] == mc.n_walkers and mc.binner_size(sec)[2] == 1, sec
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_retabling_voids_the_reduction_and_the_binners(gpu, kind):
    mc = configured(gpu, kind)
    mc.reduce(None)
    assert np.array_equal(mc.reduced("correlations"), mc.correlations_raw())
    fp = LT.fast_pairs(mc.model.l)
    nd = fp.ndirections() // 2
    mc.set_pair_directions(LT.Tables(fp.dir_of % nd, nd))  # another n_dirs: every layout that hangs on it changes
    assert size(gpu, mc, "correlations") == 4 * nd + 3 * mc.N + 1
    with pytest.raises(gpu.DQMCError) as e:
        mc.reduced("correlations")
    assert e.value.code == gpu._lib.ERR_STATE and "call dqmc_reduce first" in str(e.value)
    mc.reduce_import(np.zeros(mc.reduce_size()))  # a reduction packed elsewhere, for another layout
    with pytest.raises(gpu.DQMCError) as e:
        mc.reduced("correlations")
    assert e.value.code == gpu._lib.ERR_STATE and "reconfigured after the last reduction" in str(e.value)
    with pytest.raises(gpu.DQMCError) as e:  # refused before anything is accumulated
        mc.accumulate_correlations()
    assert e.value.code == gpu._lib.ERR_STATE and "layout has changed" in str(e.value)
    assert mc.binner_size("correlations")[2] == 2 and not mc.correlations_raw().any()
    mc.reduce(None)
    assert np.array_equal(mc.reduced("correlations"), mc.correlations_raw())
    assert np.array_equal(mc.reduced("greens"), mc.accumulators())
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_unconfigured_sections_refuse_get_and_export(gpu, kind):
    mc = fresh(gpu, kind)
    lib = gpu.lib()
    for sec in SECTIONS[1:]:
        for rc, out in (host_get(gpu, mc, sec, 1), device_export(gpu, mc, sec, 1)):
            assert rc == gpu._lib.ERR_STATE and lib.dqmc_last_error(mc._h).decode() == NEED[sec], sec
            assert np.isnan(out).all(), sec
    for sec in ("correlations", "pairing", "time_displaced"):
        assert size(gpu, mc, sec) == 0
    assert size(gpu, mc, "greens") == 2 * mc.nb * 256 + mc.nb * 16 + 1 and not mc.accumulators().any()
    mc.close()


@pytest.mark.parametrize("kind", KINDS)
def test_retabling_gives_device_memory_back(gpu, kind):
    """20 calls of dqmc_set_pair_directions, each of which rebuilds the correlations section, the current-current plan and
    the time-displaced section: free device memory (hipMemGetInfo) after the 20th is not below that after the 2nd, less one
    allocation granule, taken as what the first call - the one that allocates for the first time - costs"""
    free = lambda: torch.cuda.mem_get_info()[0]  # noqa: E731
    mc = fresh(gpu, kind)
    fp = LT.fast_pairs(mc.model.l)
    nd = fp.ndirections()
    tabs = [fp, LT.Tables((fp.dir_of + 1) % nd, nd)]  # the same n_dirs, so that the targets below stay valid
    f0 = free()
    mc.set_pair_directions(tabs[0])
    granule = max(f0 - free(), 0)
    mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))
    mc.set_current_targets(gpu.EachLocalQuadBySyncedDistance(mc.model.l))
    mc.set_time_displaced(5, ("greens", "density"))
    mc.set_pair_directions(tabs[1])
    f2 = free()
    for i in range(2, 20):
        mc.set_pair_directions(tabs[i % 2])
    f20 = free()
    print("free before %d, first call took %d, after 2nd %d, after 20th %d" % (f0, granule, f2, f20))
    assert f20 >= f2 - granule
    mc.close()
