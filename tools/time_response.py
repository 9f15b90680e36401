"""Cost of the response binners (csrc/response.hip: the channel contraction of every walker's pairing sample and the bond
kinetic energy, then momentum.hip's transform with both tables and the ordinary binner push), one JSON line per case.
Config 3's shape: attractive Hubbard 16 x 16, beta = 8, dtau = 0.1 (80 slices), 32 walkers, local and current targets set.
Two passes are timed, each as the median over `--repeats` turns of one synchronous call at the same measurement point,
the cases alternated turn by turn in one process:

    accumulate_pairing        and        accumulate_susceptibilities

each with the response binners off ("off": channels and momenta set, nothing enabled) and on ("on": n_ch = 3, n_q = 8,
the three binners, no real-space binner next to them).  With `--parent-lib PATH` (another build of the library, such as
the parent commit's) the passes are also timed on that build, loaded next to this one and alternated with the other
cases, and the ratio off / parent is printed: with the binners off the passes must run at the parent's rate.

    python tools/time_response.py [--out FILE] [--repeats R] [--parent-lib PATH]"""
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

L, BETA, DTAU, W, N_Q, CAPACITY = 16, 8.0, 0.1, 32, 8, 7
RESP = ("response_pairing", "response_pairing_susceptibility", "response_current")


def make(mc_amd, case):
    """case: "off", "on", "parent" -> a handle at its measurement point"""
    m = mc_amd.HubbardModelAttractive(L, 2)
    mc = mc_amd.DQMC(m, beta=BETA, delta_tau=DTAU, n_walkers=W, seed=11)
    pairs = mc_amd.EachSitePairByDistance(m.l)
    mc.set_local_targets(mc_amd.EachLocalQuadByDistance(m.l, pairs=pairs))
    mc._set_current_targets(mc_amd.EachLocalQuadBySyncedDistance(m.l, pairs=pairs).trg_of, mc._K, None)
    if case != "parent":
        mc.set_momenta(mc_amd.momentum_grid(m.l)[0][1:1 + N_Q])
        mc.set_pair_channels("default")
    mc.prepare()
    mc.update_until_measure()
    if case == "on":
        mc.enable_binning(RESP, capacity=CAPACITY)
    return mc


def one(mc, which):
    mc.reset_accumulators()  # (the binners have a capacity)
    mc.synchronize()
    t0 = time.perf_counter()
    if which == "pairing":
        mc.accumulate_pairing()
    else:
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
    cases = ["off", "on"] + (["parent"] if a.parent_lib else [])
    libs = {c: None for c in cases}
    if a.parent_lib:
        libs["parent"] = other_build(a.parent_lib)
    hs, res = {}, {}
    try:
        for c in cases:
            with on(libs[c]):
                hs[c] = make(mc_amd, c)
        for which in ("pairing", "susceptibilities"):
            t = {c: [] for c in cases}
            for turn in range(a.repeats + 1):  # turn 0 warms up: the unequal-time stack, first launches
                for c in cases:
                    with on(libs[c]):
                        ms = one(hs[c], which)
                    if turn:
                        t[c].append(ms)
            for c in cases:
                res[(which, c)] = dict(median_ms=float(np.median(t[c])), min_ms=min(t[c]), max_ms=max(t[c]))
    finally:
        for c, h in hs.items():
            with on(libs[c]):
                h.close()
    lines = []
    for (which, c), v in res.items():
        d = dict(v, what="time_response", pass_=which, case=c)
        if c == "parent":
            d["off_over_parent"] = res[(which, "off")]["median_ms"] / v["median_ms"]
        else:
            d["added_ms"] = v["median_ms"] - res[(which, "off")]["median_ms"]
        lines.append(d)
    text = "\n".join(json.dumps(d) for d in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
