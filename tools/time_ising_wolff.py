"""Rates and decorrelation of the Ising flavor's Wolff cluster move (csrc/ising.hip ising_wolff_kernel), one JSON line per
shape: 2D square L = 16, 32, 64 at beta_c with 256 walkers (the example's temperature-scan batch, example/ising2d).

Per shape:
- Wolff moves/s: wall time of `--moves` calls of dqmc_mc_global_move for every walker (one launch and one synchronise
  each), and the walker-sweeps/s of MC.sweep local-only and with a move after every sweep (r = 1);
- the mean cluster size (sum of cluster sizes / moves);
- the integrated autocorrelation time of |M| and E in sweeps, local-only and with r = 1: every walker is first brought
  to equilibrium with r = 1, then a series of one measurement per sweep is recorded; tau_int = 1/2 + sum_t rho(t) over
  Sokal's automatic window (the first W >= 6 tau_int(W)), rho pooled over the walkers;
- effective samples per second: walker-sweeps/s / (2 tau_int).

    python tools/time_ising_wolff.py [--out FILE] [--scale S]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BETA_C = 0.5 * np.log(1.0 + np.sqrt(2.0))


def tau_int(series):
    """integrated autocorrelation time of per-walker series (rows) with Sokal's window (c = 6), rho pooled over rows"""
    x = np.asarray(series, dtype=float)
    x = x - x.mean()
    n = x.shape[1]
    f = np.fft.rfft(x, 2 * n, axis=1)
    acf = np.fft.irfft(f * np.conj(f), axis=1)[:, :n].sum(axis=0) / (x.shape[0] * np.arange(n, 0, -1))
    rho = acf / acf[0]
    tau = 0.5
    for t in range(1, n):
        tau += rho[t]
        if t >= 6.0 * tau:
            return float(tau), t
    return float(tau), n  # no window found: the series is too short for this tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every series length")
    ap.add_argument("--moves", type=int, default=200)
    args = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    L_ = mc_amd.lib()
    src_hash = L_.dqmc_build_source_hash().decode()
    W = 256
    # series lengths (sweeps): local-only tau_int grows about as L^2.2, so its series grows with L
    shapes = [(16, 20000, 4000), (32, 40000, 4000), (64, 80000, 4000)]
    lines = []
    for L, n_local, n_cluster in shapes:
        n_local, n_cluster = int(n_local * args.scale), int(n_cluster * args.scale)
        N = L * L
        cap = max(n_local, n_cluster)
        model = mc_amd.IsingModel(dims=2, L=L)
        mc = mc_amd.MC(model, beta=BETA_C, n_walkers=W, seed=L, thermalization=10 ** 9, series_capacity=cap,
                       cluster_moves=True, global_rate=1)
        rate = lambda r: mc._c(L_.dqmc_mc_set_global_rate(mc._h, r))  # noqa: E731
        line = {"shape": "square L=%d" % L, "n_sites": N, "n_walkers": W, "beta": BETA_C}
        # equilibrium: 1000 sweeps with a move after each
        mc.sweep(1000)
        # rates: one global_move launch per call
        mc.global_move(-1)
        g0 = mc.global_stats(0)
        t0 = time.perf_counter()
        for _ in range(args.moves):
            mc.global_move(-1)
        dt = time.perf_counter() - t0
        line["wolff_moves_per_s"] = W * args.moves / dt
        line["wolff_move_launch_us"] = 1e6 * dt / args.moves
        sizes = [mc.global_stats(w) for w in range(W)]
        g1 = mc.global_stats(0)
        line["mean_cluster_size"] = float(np.sum([s.sum_cluster_size for s in sizes]) /
                                          np.sum([s.prop_global for s in sizes]))
        line["mean_cluster_fraction"] = line["mean_cluster_size"] / N
        assert g1.prop_global - g0.prop_global == args.moves
        for label, r in (("local", 0), ("r1", 1)):
            rate(r)
            n = n_local if r == 0 else n_cluster
            mc.reset_accumulators()
            mc.thermalization = mc.last_sweep  # measure every sweep from here
            t0 = time.perf_counter()
            mc.sweep(n)
            dt = time.perf_counter() - t0
            ws = W * n / dt
            line["walker_sweeps_per_s_" + label] = ws
            line["series_sweeps_" + label] = n
            E = np.array([mc.series(w)[0] for w in range(W)])
            M = np.array([mc.series(w)[1] for w in range(W)])
            for obs, s in (("absM", M), ("E", E)):
                tau, win = tau_int(s)
                line["tau_int_%s_%s" % (obs, label)] = round(tau, 2)
                line["tau_window_%s_%s" % (obs, label)] = win
                line["eff_samples_per_s_%s_%s" % (obs, label)] = ws / (2.0 * tau)
            line["local_sweep_plus_move_us" if r else "local_sweep_us"] = 1e6 * dt / n
        line["move_over_local_sweep"] = line["local_sweep_plus_move_us"] / line["local_sweep_us"] - 1.0
        line["eff_samples_gain_absM"] = line["eff_samples_per_s_absM_r1"] / line["eff_samples_per_s_absM_local"]
        line["source_hash"] = src_hash
        mc.close()
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
