"""Rates of the Ising kernel (csrc/ising.hip): site updates per second and sweeps per second, one JSON line per shape.

Shapes: the temperature scan of the reference's example (example/ising2d/Ising2D.jl: L = 8, 16, 32, 64 with 256
chains each, here one handle per L with per-walker beta spread around T_c), and 8 x 8 with 16384 walkers.  The device
time is the wall time of MC.sweep (one synchronising C call that runs the sweeps in bounded launches) after a warm-up.
The CPU comparison is orc_ising_run (the oracle's sequential restatement, one host core) on one chain of the same
shape in the same process; `cpu_16_cores_extrapolated` is that rate times 16, not a measurement.

    python tools/time_ising.py [--sweeps N] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=0, help="timed sweeps per shape (0: sized per shape)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    O = g.load_oracle()
    src_hash = mc_amd.lib().dqmc_build_source_hash().decode()
    shapes = [(8, 256), (16, 256), (32, 256), (64, 256), (8, 16384)]
    lines = []
    for L, W in shapes:
        N = L * L
        T = mc_amd.IsingTc * np.linspace(0.8, 1.2, W)
        mc = mc_amd.MC(mc_amd.IsingModel(dims=2, L=L), T=T, n_walkers=W, seed=1, thermalization=10 ** 9)
        warm = max(2, int(2e5 / N))
        t0 = time.perf_counter()
        mc.sweep(warm)  # warm-up (also leaves the random start behind); sizes the timed run to about half a second
        per_sweep = (time.perf_counter() - t0) / warm
        sweeps = args.sweeps or int(min(10 ** 6, max(10, 0.5 / per_sweep)))
        t0 = time.perf_counter()
        mc.sweep(sweeps)
        dt = time.perf_counter() - t0
        acc = np.mean([mc.analysis(w)["acc_rate"] for w in (0, W // 2, W - 1)])
        mc.close()
        cpu_sweeps = max(5, int(2e6 / N))
        t0 = time.perf_counter()
        O.ising_run(L, 1.0 / mc_amd.IsingTc, 0, cpu_sweeps, 1)
        cdt = time.perf_counter() - t0
        cpu_rate = cpu_sweeps * N / cdt
        line = {"shape": "square L=%d" % L, "n_sites": N, "n_walkers": W, "sweeps_timed": sweeps,
                "seconds": round(dt, 4), "site_updates_per_s": W * N * sweeps / dt,
                "walker_sweeps_per_s": W * sweeps / dt, "sweeps_per_s_per_walker": sweeps / dt,
                "acc_rate_sampled": round(float(acc), 4),
                "cpu_1_core_site_updates_per_s": cpu_rate, "cpu_16_cores_extrapolated_site_updates_per_s": 16 * cpu_rate,
                "speedup_vs_1_core": W * N * sweeps / dt / cpu_rate, "source_hash": src_hash}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
