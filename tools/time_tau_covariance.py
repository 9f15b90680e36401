"""Cost of the tau-tau' covariance accumulator (csrc/taucov.hip: a gather per pass and one streamed rank-1 update of every
series' S2 per closed bin), one JSON line per case.  Config 3's shape: attractive Hubbard 16 x 16, beta = 8, dtau = 0.1 (80
slices), 32 walkers, n_q = 8 momenta, recording at every = 1 (81 rows) and every = 2 (41 rows), GREENS | DENSITY (40
series).  One pass, accumulate_susceptibilities with the recorded rows, is timed as the median over `--repeats` turns of one
synchronous call at the same measurement point, the cases alternated turn by turn in one process:

    none    momenta set, no binner, accumulator off
    binner  the momentum time-displaced binner on (what the accumulator's cost is set against: binner - none)
    cov1    binner and accumulator, bin_size = 1: every pass closes a bin, the worst case
    cov16   binner and accumulator, bin_size = 16: the timed pass closes no bin and writes the open-bin sums only

With `--parent-lib PATH` (another build of the library, such as the parent commit's) the "binner" case is also timed on
that build, loaded next to this one and alternated with the others, and the ratio this / parent is printed: with the
accumulator off the pass must run at the parent's rate.

    python tools/time_tau_covariance.py [--out FILE] [--repeats R] [--parent-lib PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_momentum import on, other_build  # noqa: E402

L, BETA, DTAU, W, NQ, CAPACITY = 16, 8.0, 0.1, 32, 8, 7


def make(mc_amd, case, every):
    m = mc_amd.HubbardModelAttractive(L, 2)
    mc = mc_amd.DQMC(m, beta=BETA, delta_tau=DTAU, n_walkers=W, seed=11)
    mc.set_pair_directions(mc_amd.EachSitePairByDistance(m.l))
    mc.set_momenta(mc_amd.momentum_grid(m.l)[0][:NQ])
    mc.set_time_displaced(every)
    mc.prepare()
    mc.update_until_measure()
    if case != "none":
        mc.enable_binning(("momentum_time_displaced",), capacity=CAPACITY)
    if case.startswith("cov"):
        mc.set_tau_covariance(int(case[3:]))
    return mc


def one(mc):
    mc.reset_accumulators()  # (the binner has a capacity; the open bin starts empty, so cov16 never closes one)
    mc.synchronize()
    t0 = time.perf_counter()
    mc.accumulate_susceptibilities()
    mc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    cases = ["none", "binner", "cov1", "cov16"] + (["parent"] if a.parent_lib else [])
    libs = {c: None for c in cases}
    if a.parent_lib:
        libs["parent"] = other_build(a.parent_lib)
    lines = []
    for every in (1, 2):
        hs, t, plan = {}, {c: [] for c in cases}, {}
        try:
            for c in cases:
                with on(libs[c]):
                    hs[c] = make(mc_amd, "binner" if c == "parent" else c, every)
            for c in ("cov1", "cov16"):
                plan[c] = hs[c].tau_covariance_plan()
            for turn in range(a.repeats + 1):  # turn 0 warms up: the unequal-time stack, first launches
                for c in cases:
                    with on(libs[c]):
                        ms = one(hs[c])
                    if turn:
                        t[c].append(ms)
        finally:
            for c, h in hs.items():
                with on(libs[c]):
                    h.close()
        med = {c: float(np.median(t[c])) for c in cases}
        for c in cases:
            d = dict(what="time_tau_covariance", every=every, case=c, median_ms=med[c], min_ms=min(t[c]), max_ms=max(t[c]))
            if c == "parent":
                d["this_over_parent"] = med["binner"] / med[c]
            else:
                d["added_ms"] = med[c] - med["none"]
            if c in plan:
                d.update(series=plan[c]["series"], rows=plan[c]["rows"], bytes=plan[c]["bytes"],
                         added_over_binner_ms=med[c] - med["binner"])
            lines.append(d)
    text = "\n".join(json.dumps(d) for d in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
