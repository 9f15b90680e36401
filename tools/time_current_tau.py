"""Cost of the imaginary-time current recording (csrc/current_tau.hip, current_tau.inl) inside the susceptibility pass,
one JSON line per case.  Config 3's shape: attractive Hubbard 16 x 16, beta = 8, dtau = 0.1 (80 slices), 32 walkers,
current targets set, n_q = 8 momenta (q = 0 among them).  accumulate_susceptibilities is timed as the median over
`--repeats` turns of one synchronous call at the same measurement point, the cases alternated turn by turn in one
process:

    off      momenta set, recording off          every1   a row per slice (81 rows)          every8   11 rows

With `--parent-lib PATH` (another build of the library, such as the parent commit's) the pass is also timed on that
build, loaded next to this one and alternated with the other cases: with the recording off the pass must sit inside the
parent's own run-to-run spread, and both ranges are printed.

    python tools/time_current_tau.py [--out FILE] [--repeats R] [--parent-lib PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_momentum import on, other_build  # noqa: E402

L, BETA, DTAU, W, N_Q = 16, 8.0, 0.1, 32, 8
EVERY = {"off": 0, "every1": 1, "every8": 8, "parent": 0}


def make(mc_amd, case):
    """a handle at its measurement point"""
    m = mc_amd.HubbardModelAttractive(L, 2)
    mc = mc_amd.DQMC(m, beta=BETA, delta_tau=DTAU, n_walkers=W, seed=11)
    mc.set_current_targets(mc_amd.EachLocalQuadBySyncedDistance(m.l))
    if case != "parent":
        mc.set_momenta(mc_amd.momentum_grid(m.l)[0][:N_Q])
    mc.prepare()
    mc.update_until_measure()
    if EVERY[case]:
        mc.set_current_time_displaced(EVERY[case])
    return mc


def one(mc):
    mc.reset_accumulators()
    mc.synchronize()
    t0 = time.perf_counter()
    mc.accumulate_susceptibilities()
    mc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    cases = ["off", "every1", "every8"] + (["parent"] if a.parent_lib else [])
    libs = {c: None for c in cases}
    if a.parent_lib:
        libs["parent"] = other_build(a.parent_lib)
    hs, t = {}, {c: [] for c in cases}
    try:
        for c in cases:
            with on(libs[c]):
                hs[c] = make(mc_amd, c)
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
    res = {c: dict(median_ms=float(np.median(t[c])), min_ms=min(t[c]), max_ms=max(t[c])) for c in cases}
    lines = []
    for c in cases:
        d = dict(res[c], what="time_current_tau", case=c, rows=0 if not EVERY[c] else 1 + int(round(BETA / DTAU)) // EVERY[c])
        if c == "parent":
            d["off_over_parent"] = res["off"]["median_ms"] / res[c]["median_ms"]
            d["off_within_parent_spread"] = bool(res["off"]["median_ms"] <= res[c]["max_ms"])
        elif c != "off":
            d["added_ms"] = res[c]["median_ms"] - res["off"]["median_ms"]
            d["added_us_per_row"] = 1e3 * d["added_ms"] / d["rows"]
        lines.append(d)
    text = "\n".join(json.dumps(d) for d in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
