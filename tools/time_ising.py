"""Rates of the Ising kernel (csrc/ising.hip): site updates per second and sweeps per second, one JSON line per shape.

Shapes: the temperature scan of the reference's example (example/ising2d/Ising2D.jl: L = 8, 16, 32, 64 with 256
chains each, here one handle per L with per-walker beta spread around T_c), and 8 x 8 with 16384 walkers.  The device
time is the wall time of MC.sweep (one synchronising C call that runs the sweeps in bounded launches) after a warm-up.
The CPU comparison is orc_ising_run (the oracle's sequential restatement, one host core) on one chain of the same
shape in the same process; `cpu_16_cores_extrapolated` is that rate times 16, not a measurement.

`--binning` times the per-walker binner instead (include/dqmc_hip.h, "error bars of the MC flavor"): L = 8, 16, 64 with
256 chains at T_c, every sweep measured, with and without a cluster move per sweep; handles with the binner off and on
take turns in one process (two turns each, the spread is in the line), and the binner's pooled tau of |M| gives the
effective samples per second.

    python tools/time_ising.py [--sweeps N] [--binning] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_binning(mc_amd, args, src_hash):
    """binner off against on, alternated: sweeps/s per walker of both and what a measured sweep costs more"""
    lines = []
    for L in (8, 16, 64):
        for cluster in (False, True):
            N, W = L * L, 256
            warm = max(2, int(2e5 / N))
            sweeps = args.sweeps or max(10, int(1.5e6 / N))
            kw = dict(T=mc_amd.IsingTc, n_walkers=W, seed=1, thermalization=warm, cluster_moves=cluster, global_rate=1)
            mcs = {"off": mc_amd.MC(mc_amd.IsingModel(dims=2, L=L), **kw),
                   "on": mc_amd.MC(mc_amd.IsingModel(dims=2, L=L), binning=True, binning_capacity=2 * sweeps, **kw)}
            for mc in mcs.values():
                mc.sweep(warm)
            dt = {"off": [], "on": []}
            for _ in range(2):
                for k, mc in mcs.items():
                    t0 = time.perf_counter()
                    mc.sweep(sweeps)
                    dt[k].append(time.perf_counter() - t0)
            b = mcs["on"].binned(walkers=range(W))
            assert mcs["on"].stats(0).sum_E == mcs["off"].stats(0).sum_E and b["count"] == (2 * sweeps) >> b["level"]
            for mc in mcs.values():
                mc.close()
            off, on = min(dt["off"]), min(dt["on"])
            tau = b["Magn"]["M"]["tau"]
            line = {"shape": "square L=%d" % L, "n_sites": N, "n_walkers": W, "cluster_moves": cluster,
                    "sweeps_timed": sweeps, "seconds_off": [round(t, 4) for t in dt["off"]],
                    "seconds_on": [round(t, 4) for t in dt["on"]], "sweeps_per_s_per_walker_off": sweeps / off,
                    "sweeps_per_s_per_walker_on": sweeps / on, "binner_cost_per_measured_sweep_us": (on - off) / sweeps * 1e6,
                    "binner_cost_percent": 100.0 * (on / off - 1.0), "level": b["level"], "tau_absM": tau,
                    "tau_E": b["Energy"]["E"]["tau"], "absM": b["Magn"]["M"],
                    "effective_absM_samples_per_s_per_walker": sweeps / on / (2.0 * max(tau, 0.0) + 1.0),
                    "source_hash": src_hash}
            print(json.dumps(line), flush=True)
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=0, help="timed sweeps per shape (0: sized per shape)")
    ap.add_argument("--binning", action="store_true", help="time the binner on against off instead of the shapes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    src_hash = mc_amd.lib().dqmc_build_source_hash().decode()
    if args.binning:
        lines = time_binning(mc_amd, args, src_hash)
        if args.out:
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
        return
    O = g.load_oracle()
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
