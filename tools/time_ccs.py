"""One accumulate_susceptibilities pass at the config-3 shape (16x16 attractive, beta = 8, 32 walkers,
K_pc = K_cc = 5) with and without current targets; run under `rocprofv3 --kernel-trace --stats -- python
tools/time_ccs.py` for the per-kernel times (cc_lds_kernel, cc_fold_kernel, sus_pairing_kernel, ...)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

mc_amd = g.load_package()


def one(with_cc, reps=2):
    model = mc_amd.HubbardModelAttractive(16, 2)
    mc = mc_amd.DQMC(model, beta=8.0, n_walkers=32, seed=5)
    mc.set_local_targets(mc_amd.EachLocalQuadByDistance(model.l, 5))
    if with_cc:
        mc.set_current_targets(mc_amd.EachLocalQuadBySyncedDistance(model.l, 5))
        assert mc.current_targets_fast_path()
    mc.prepare()
    mc.update_until_measure()
    mc.accumulate_susceptibilities()  # (warm-up: stacks built, code loaded)
    mc.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mc.accumulate_susceptibilities()
        mc.synchronize()
        ts.append(time.perf_counter() - t0)
    res = mc.susceptibilities()
    mc.close()
    return min(ts), res


t_off, _ = one(False)
t_on, res = one(True)
print("pass without current targets: %.2f ms, with: %.2f ms (slices 80)" % (1e3 * t_off, 1e3 * t_on))
print("CCS[0:3, :] =", res["CCS"][:3])
