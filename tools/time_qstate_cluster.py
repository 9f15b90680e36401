#!/usr/bin/env python3
"""What the reflection cluster move of the q-state engine costs and what it buys, at the couplings where local sweeps slow
down: Potts q = 3 at beta_c = ln(1 + sqrt 3) and clock q = 6 at beta = 1.1, near its upper (disordering) transition, on
SquareLattice(L), L = 16, 32, 64, 64 walkers each.

    python tools/time_qstate_cluster.py [--out FILE.json] [--quick]

Per case two handles run the same number of sweeps behind a thermalization, one with local sweeps only and one with
cluster_rate = 1, every `measure_rate`-th sweep recorded in the series.  Reported:
  us_per_move           (t(rate 1) - t(rate 0)) / sweeps: the host clock around sweep() calls that end in a device
                        synchronise, the whole handle's 64 moves side by side
  cluster_size_over_N   sum_cluster_size / prop_global / N, averaged over the walkers
  tau_int_M2            the integrated autocorrelation time of M^2 = Mx^2 + My^2 in sweeps, 1/2 + sum of the normalised
                        autocorrelation up to Sokal's automatic window (the first W >= 6 tau), the function averaged over
                        the walkers; `tau_window_ok` is false where the series is shorter than 50 tau (then a lower bound)
  eff_samples_per_s     walkers * sweeps per second / (2 tau_int_M2)
for both handles.  Prints one JSON line per case."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def tau_int(series):
    """series [walkers][n]: (tau in records, whether n >= 50 tau)"""
    x = np.asarray(series, dtype=np.float64)
    x = x - x.mean(axis=1, keepdims=True)
    n = x.shape[1]
    f = np.fft.rfft(x, 2 * n, axis=1)
    acf = np.fft.irfft(f * np.conj(f), axis=1)[:, :n] / np.arange(n, 0, -1)
    rho = acf.mean(axis=0)
    if rho[0] <= 0.0:
        return 0.5, True
    rho = rho / rho[0]
    tau = 0.5
    for w in range(1, n):
        tau += rho[w]
        if w >= 6.0 * tau:
            break
    return float(tau), bool(n >= 50.0 * tau)


def run(g, model, beta, W, therm, sweeps, rate, cluster_rate):
    mc = g.MC(model, beta=beta, n_walkers=W, seed=1, thermalization=therm, measure_rate=rate,
              series_capacity=sweeps // rate, cluster_rate=cluster_rate)
    mc.sweep(therm)
    t0 = time.perf_counter()
    mc.sweep(sweeps)
    dt = time.perf_counter() - t0
    m2 = []
    for w in range(W):
        _, mx, my = mc.series(w)
        m2.append((mx.astype(np.float64) ** 2 + my.astype(np.float64) ** 2) / 2.0 ** 60)
    cl = [mc.cluster_stats(w) for w in range(W)]
    size = float(np.mean([c.sum_cluster_size / c.prop_global for c in cl])) if cluster_rate else None
    mc.close()
    tau, ok = tau_int(m2)
    return dt, tau * rate, ok, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short runs (a rehearsal, not a measurement)")
    args = ap.parse_args()
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_qstate_cluster: no HIP device visible (there is no CPU fallback)")
    W = 64
    results = []
    for kind, q, beta in (("potts", 3, math.log(1.0 + math.sqrt(3.0))), ("clock", 6, 1.1)):
        for L, sweeps, rate in ((16, 65536, 1), (32, 65536, 1), (64, 131072, 4)):
            if args.quick:
                sweeps //= 64
            therm = sweeps // 8
            l = g.SquareLattice(L)
            N = L * L
            model = g.PottsModel(q, l=l) if kind == "potts" else g.ClockModel(q, l=l)
            t_loc, tau_loc, ok_loc, _ = run(g, model, beta, W, therm, sweeps, rate, 0)
            t_cl, tau_cl, ok_cl, size = run(g, model, beta, W, therm, sweeps, rate, 1)
            r = {"model": kind, "q": q, "L": L, "beta": beta, "walkers": W, "sweeps": sweeps, "measure_rate": rate,
                 "seconds_local": t_loc, "seconds_cluster": t_cl, "us_per_move": (t_cl - t_loc) / sweeps * 1e6,
                 "us_per_sweep_local": t_loc / sweeps * 1e6, "cluster_size_over_N": size / N,
                 "tau_int_M2_local": tau_loc, "tau_int_M2_cluster": tau_cl, "tau_window_ok_local": ok_loc,
                 "tau_window_ok_cluster": ok_cl, "eff_samples_per_s_local": W * sweeps / t_loc / (2.0 * tau_loc),
                 "eff_samples_per_s_cluster": W * sweeps / t_cl / (2.0 * tau_cl),
                 "source_hash": g.lib().dqmc_build_source_hash().decode()}
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
