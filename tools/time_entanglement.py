"""Cost of the Renyi-2 entanglement measurement (csrc/entangle.hip) on the MI355X: 16 x 16 attractive Hubbard, beta = 8,
32 walkers = 496 pairs; one strip of N_A = 16, 64 and 128 sites each, and the eight strips of width 1 .. 8 together.

Per case: ms per accumulate_entanglement (wall clock over `--reps` calls behind a synchronize), the share of it that the
two GEMMs of true_greens take (HIP events per kernel family: "gemm" is launched by nothing else in the call), and the
time of one sweep in the same process.  One JSON line per case.

    python tools/time_entanglement.py [--reps 20] [--walkers 32] [--beta 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--walkers", type=int, default=32)
    ap.add_argument("--beta", type=float, default=8.0)
    a = ap.parse_args()
    P = g.load_package()
    l = P.SquareLattice(16)
    strip = lambda w: P.lattices.strip_subsystem(l, w).tolist()
    cases = [("N_A=16", [strip(1)]), ("N_A=64", [strip(4)]), ("N_A=128", [strip(8)]),
             ("strips 1..8", [strip(w) for w in range(1, 9)])]
    mc = P.DQMC(P.HubbardModelAttractive(l=l, U=1.0, mu=0.3), beta=a.beta, n_walkers=a.walkers, seed=5)
    mc.prepare()
    mc.sweep(1)
    t0 = time.perf_counter()
    mc.sweep(1)
    sweep_ms = (time.perf_counter() - t0) * 1e3
    for name, subs in cases:
        mc.set_entanglement(subs)
        mc.accumulate_entanglement()  # (warm-up: the first launch of a kernel form loads its code object)
        mc.synchronize()
        mc.timing_enable(True)
        before = mc.timing()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            mc.accumulate_entanglement()
        mc.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.reps
        after = mc.timing()
        mc.timing_enable(False)
        fam = {k: (after[k][0] - before[k][0]) / a.reps for k in after}
        res = mc.entanglement()
        print(json.dumps({"case": name, "walkers": a.walkers, "pairs": a.walkers * (a.walkers - 1) // 2, "beta": a.beta,
                          "ms_per_accumulate": round(wall, 4), "ms_true_greens": round(fam["gemm"], 4),
                          "ms_entanglement_kernels": round(fam["misc"], 4),
                          "true_greens_share": round(fam["gemm"] / wall, 4), "ms_per_sweep": round(sweep_ms, 3),
                          "S2": [round(float(x), 6) for x in res["S2"]], "failures": res["failures"]}), flush=True)
    mc.close()


if __name__ == "__main__":
    main()
