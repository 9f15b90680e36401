"""Wall time of one accumulate_susceptibilities pass at the bench config-3 shape (16x16 attractive, beta = 8, 80 slices,
32 walkers) with time-displaced recording off and on, in one process:

  off        recording off
  greens     GREENS, the one-lane-per-direction kernel
  general    GREENS under DQMC_TDM_GENERAL=1 (the pair-list kernel), on a second handle in the same state
  both       GREENS | DENSITY

Every repetition visits the four variants, in an order that rotates and reverses from one repetition to the next; a
pass is timed from the call to the end of the handle's stream.  Prints median and range per variant and the added time
over "off".  --every sets the row stride, --reps the repetitions (at least 5), --json adds one machine-readable line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

mc_amd = g.load_package()


def make(general):
    if general:
        os.environ["DQMC_TDM_GENERAL"] = "1"
    try:
        model = mc_amd.HubbardModelAttractive(16, 2)
        mc = mc_amd.DQMC(model, beta=8.0, n_walkers=32, seed=5)
    finally:
        os.environ.pop("DQMC_TDM_GENERAL", None)
    mc.set_pair_directions(mc_amd.EachSitePairByDistance(model.l))
    mc.prepare()
    mc.update_until_measure()
    return mc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    a, b = make(False), make(True)
    variants = {"off": (a, 0, 0), "greens": (a, args.every, 1), "general": (b, args.every, 1), "both": (a, args.every, 3)}
    for mc, every, what in variants.values():  # warm-up: stacks built, code loaded, buffers allocated once
        mc.set_time_displaced(every, what)
        mc.accumulate_susceptibilities()
    a.set_time_displaced(args.every, 1)
    assert a.time_displaced_plan()["fast"] == 1 and b.time_displaced_plan()["fast"] == 0
    names = list(variants)
    times = {k: [] for k in names}
    for rep in range(args.reps):
        order = names[rep % 4:] + names[:rep % 4]
        for k in (order[::-1] if rep % 2 else order):
            mc, every, what = variants[k]
            mc.set_time_displaced(every, what)
            mc.synchronize()
            t0 = time.perf_counter()
            mc.accumulate_susceptibilities()
            mc.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in times.items()}
    print("one accumulate_susceptibilities pass, 16x16 attractive, 80 slices, 32 walkers, every = %d, %d repetitions, "
          "library %s" % (args.every, args.reps, mc_amd.lib().dqmc_build_commit().decode()))
    for k in names:
        print("  %-8s median %8.2f ms  range %8.2f .. %8.2f ms  added over off %+8.2f ms (%+.1f %%)"
              % (k, med[k], min(times[k]), max(times[k]), med[k] - med["off"], 100.0 * (med[k] / med["off"] - 1.0)))
    if args.json:
        print(json.dumps({"every": args.every, "reps": args.reps, "times_ms": times, "median_ms": med}))
    a.close()
    b.close()


if __name__ == "__main__":
    main()
