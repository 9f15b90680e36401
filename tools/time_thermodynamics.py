"""Cost of the thermodynamics pass (csrc/thermo.hip: one workgroup per walker streams G once, then a one-workgroup
reduce), one JSON line per case.  Config 3's shape: Hubbard 16 x 16, beta = 8, dtau = 0.1 (80 slices), 32 walkers.  Timed,
each as the median over `--repeats` turns of one synchronous call at the same measurement point, the cases alternated turn
by turn in one process:

    accumulate_thermodynamics   attractive model: no binner / with its binner / with sign weighting (s = +1, no chain)
                                repulsive model at mu = 0.4 with sign weighting (one slice chain per measurement point)
    accumulate_greens           the same true-G products (eTinv G eT) and one streaming pass over G: what the pass costs
                                without the new kernel
    accumulate_correlations     the pass the thermodynamics one is put next to
    sweep(1)                    one full sweep of the same handle

    python tools/time_thermodynamics.py [--out FILE] [--repeats R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, BETA, DTAU, W, CAPACITY = 16, 8.0, 0.1, 32, 7


def make(mc_amd, case):
    rep = case == "repulsive_sign"
    m = mc_amd.HubbardModelRepulsive(L, 2, mu=0.4) if rep else mc_amd.HubbardModelAttractive(L, 2)
    mc = mc_amd.DQMC(m, beta=BETA, delta_tau=DTAU, n_walkers=W, seed=11, sign_weighting=case.endswith("sign"))
    mc.set_pair_directions(mc_amd.EachSitePairByDistance(m.l))
    mc.set_thermodynamics()
    if case == "binner":
        mc.enable_binning("thermodynamics", capacity=CAPACITY)
    mc.prepare()
    mc.update_until_measure()
    return mc


def one(mc, call):
    mc.reset_accumulators()  # (the binner has a capacity)
    mc.synchronize()
    t0 = time.perf_counter()
    call()
    mc.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    cases = ["none", "binner", "sign", "repulsive_sign"]
    hs = {c: make(mc_amd, c) for c in cases}
    calls = [("thermodynamics", c, hs[c].accumulate_thermodynamics) for c in cases]
    calls += [("greens", "none", hs["none"].accumulate_greens), ("correlations", "none", hs["none"].accumulate_correlations),
              ("greens", "repulsive_sign", hs["repulsive_sign"].accumulate_greens)]
    t = {(p, c): [] for p, c, _ in calls}
    sweeps = {c: [] for c in ("none", "repulsive_sign")}
    try:
        for turn in range(a.repeats + 1):  # turn 0 warms up
            for p, c, call in calls:
                ms = one(hs[c], call)
                if turn:
                    t[(p, c)].append(ms)
        for turn in range(4):
            for c in sweeps:
                hs[c].synchronize()
                t0 = time.perf_counter()
                hs[c].sweep(1)
                hs[c].synchronize()
                if turn:
                    sweeps[c].append((time.perf_counter() - t0) * 1e3)
    finally:
        for h in hs.values():
            h.close()
    lines = [dict(what="time_thermodynamics", pass_=p, case=c, median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v))
             for (p, c), v in t.items()]
    for d in lines:
        if d["pass_"] == "thermodynamics":  # what the new kernels add to the true-G products and the sign chain
            base = "repulsive_sign" if d["case"] == "repulsive_sign" else "none"
            d["minus_greens_pass_ms"] = d["median_ms"] - float(np.median(t[("greens", base)]))
    lines += [dict(what="time_thermodynamics", pass_="sweep", case=c, median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v))
              for c, v in sweeps.items()]
    text = "\n".join(json.dumps(d) for d in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
