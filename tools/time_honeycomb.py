"""Wall time of the measurement passes on HoneycombLattice(12) (n = 288, 432 directions; attractive, beta = 8, 80 slices,
32 walkers) next to SquareLattice(17) (n = 289, the yardstick for the cost per pair visited), in one process:

  honeycomb   the Green's rows in the injective form (tdm_greens_inj_kernel)
  general     the same lattice under DQMC_TDM_GENERAL=1 (the pair lists), on a second handle in the same state
  square17    SquareLattice(17), the Latin square form

Timed per case: one accumulate_correlations pass, one accumulate_susceptibilities pass with GREENS | DENSITY recorded at
every = 1, and that pass with GREENS alone and with recording off (their difference is what the Green's rows cost: the
only launches that differ between the forms).  Every repetition visits the cases in an order that rotates and reverses;
a pass is timed from the call to the end of the handle's stream.  Prints median and range.  --reps repetitions (at least
7), --L / --square the sizes, --json adds one machine-readable line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import honeycomb_ref as HR  # noqa: E402  (the vectorised direction tables: the package's are a Python double loop)
import lattice_tables as LT  # noqa: E402

mc_amd = g.load_package()


def make(lattice, pairs, general, walkers):
    if general:
        os.environ["DQMC_TDM_GENERAL"] = "1"
    try:
        mc = mc_amd.DQMC(mc_amd.HubbardModelAttractive(l=lattice), beta=8.0, n_walkers=walkers, seed=5)
    finally:
        os.environ.pop("DQMC_TDM_GENERAL", None)
    mc.set_pair_directions(pairs)
    mc.prepare()
    mc.update_until_measure()
    return mc


def timed(fn, mc):
    mc.synchronize()
    t0 = time.perf_counter()
    fn()
    mc.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--L", type=int, default=12)
    ap.add_argument("--square", type=int, default=17)
    ap.add_argument("--walkers", type=int, default=32)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    hc, sq = mc_amd.HoneycombLattice(args.L), mc_amd.SquareLattice(args.square)
    hp, sp = HR.fast_pairs(args.L), LT.fast_pairs(sq)
    handles = {"honeycomb": make(hc, hp, False, args.walkers), "general": make(hc, hp, True, args.walkers),
               "square17": make(sq, sp, False, args.walkers)}
    want = {"honeycomb": 2, "general": 0, "square17": 1}
    passes = {"correlations": None, "sus_both": 3, "sus_greens": 1, "sus_off": 0}
    for name, mc in handles.items():  # warm-up: stacks built, code loaded, buffers allocated once
        mc.accumulate_correlations()
        for what in (3, 1, 0):
            mc.set_time_displaced(1 if what else 0, what or 1)
            mc.accumulate_susceptibilities()
            if what:
                assert mc.time_displaced_plan()["fast"] == want[name], (name, mc.time_displaced_plan())
    cases = [(h, p) for p in passes for h in handles]
    times = {c: [] for c in cases}
    for rep in range(args.reps):
        k = rep % len(cases)
        order = cases[k:] + cases[:k]
        for h, p in (order[::-1] if rep % 2 else order):
            mc = handles[h]
            if p == "correlations":
                times[(h, p)].append(timed(mc.accumulate_correlations, mc))
            else:
                what = passes[p]
                mc.set_time_displaced(1 if what else 0, what or 1)
                times[(h, p)].append(timed(mc.accumulate_susceptibilities, mc))
    med = {c: statistics.median(v) for c, v in times.items()}
    print("HoneycombLattice(%d) n = %d, %d directions; SquareLattice(%d) n = %d; attractive, 80 slices, %d walkers, "
          "every = 1, %d repetitions, library %s" % (args.L, hc.sites, hp.ndirections(), args.square, sq.sites, args.walkers,
                                                     args.reps, mc_amd.lib().dqmc_build_commit().decode()))
    for p in passes:
        for h in handles:
            v = times[(h, p)]
            print("  %-12s %-10s median %8.2f ms  range %8.2f .. %8.2f ms" % (p, h, med[(h, p)], min(v), max(v)))
    rows = {h: med[(h, "sus_greens")] - med[(h, "sus_off")] for h in handles}
    pairs = {"honeycomb": hc.sites ** 2, "general": hc.sites ** 2, "square17": sq.sites ** 2}
    for h in handles:
        print("  Green's rows (sus_greens - sus_off) %-10s %+8.2f ms  = %.3f ns per pair, matrix, walker and row"
              % (h, rows[h], 1e6 * rows[h] / (pairs[h] * 2 * 81 * args.walkers)))
    print("  sus_both honeycomb / square17, scaled by the pairs visited: %.3f; honeycomb / general: %.3f"
          % (med[("honeycomb", "sus_both")] / med[("square17", "sus_both")] * pairs["square17"] / pairs["honeycomb"],
             med[("honeycomb", "sus_both")] / med[("general", "sus_both")]))
    if args.json:
        print(json.dumps({"reps": args.reps, "times_ms": {"%s/%s" % c: v for c, v in times.items()},
                          "median_ms": {"%s/%s" % c: v for c, v in med.items()}}))
    for mc in handles.values():
        mc.close()


if __name__ == "__main__":
    main()
