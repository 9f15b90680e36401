"""Cost of the momentum-space binners (csrc/momentum.hip: one MFMA GEMM per segment of every walker's sample, then the
ordinary binner push), one JSON line per case.  Config 3's shape: attractive Hubbard 16 x 16, beta = 8, dtau = 0.1 (80
slices), 32 walkers, recording at every = 1 (81 rows).  Two passes are timed, each as the median over `--repeats` turns
of one synchronous call at the same measurement point, the cases alternated turn by turn in one process:

    accumulate_correlations        and        accumulate_susceptibilities (with the time-displaced rows)

each with no binner, with the real-space binner of its sections, and with the momentum binner at n_q = 8 and n_q = 256
(no real-space binner next to it).  With `--parent-lib PATH` (another build of the library, such as the parent commit's)
the no-binner passes are also timed on that build, loaded next to this one and alternated with the other cases, and the
ratio this / parent is printed: with momenta off the passes must run at the parent's rate.

    python tools/time_momentum.py [--out FILE] [--repeats R] [--parent-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, BETA, DTAU, W, EVERY, CAPACITY = 16, 8.0, 0.1, 32, 1, 7


class on:
    """the package's calls go to `library` inside the block (None: this build)"""

    def __init__(self, library):
        self.library = library

    def __enter__(self):
        from montecarlo_jl_amd import _lib
        self.mine, _lib._lib = _lib._lib, (self.library or _lib._lib)

    def __exit__(self, *exc):
        from montecarlo_jl_amd import _lib
        _lib._lib = self.mine


def other_build(path):
    """another build of the library with the prototypes of the entry points it has"""
    from montecarlo_jl_amd import _lib
    P = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(P, name):
            f = getattr(P, name)
            f.restype, f.argtypes = res, args
    return P


def make(mc_amd, case):
    """case: "none", "parent" (no binner), "real", "q8", "q256" -> a handle at its measurement point"""
    m = mc_amd.HubbardModelAttractive(L, 2)
    mc = mc_amd.DQMC(m, beta=BETA, delta_tau=DTAU, n_walkers=W, seed=11)
    mc.set_pair_directions(mc_amd.EachSitePairByDistance(m.l))
    if case.startswith("q"):
        mc.set_momenta(mc_amd.momentum_grid(m.l)[0][:int(case[1:])])
    mc.set_time_displaced(EVERY)
    mc.prepare()
    mc.update_until_measure()
    if case == "real":
        mc.enable_binning(("correlations", "susceptibilities", "time_displaced"), capacity=CAPACITY)
    elif case.startswith("q"):
        mc.enable_binning(("momentum_correlations", "momentum_susceptibilities", "momentum_time_displaced"), capacity=CAPACITY)
    return mc


def one(mc, which):
    mc.reset_accumulators()  # (the binners have a capacity)
    mc.synchronize()
    t0 = time.perf_counter()
    if which == "correlations":
        mc.accumulate_correlations()
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
    cases = ["none", "real", "q8", "q256"] + (["parent"] if a.parent_lib else [])
    libs = {c: None for c in cases}
    if a.parent_lib:
        libs["parent"] = other_build(a.parent_lib)
    hs, res = {}, {}
    try:
        for c in cases:
            with on(libs[c]):
                hs[c] = make(mc_amd, c)
        for which in ("correlations", "susceptibilities"):
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
        d = dict(v, what="time_momentum", pass_=which, case=c)
        if c == "parent":
            d["this_over_parent"] = res[(which, "none")]["median_ms"] / v["median_ms"]
        else:
            d["added_ms"] = v["median_ms"] - res[(which, "none")]["median_ms"]
        lines.append(d)
    text = "\n".join(json.dumps(d) for d in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
