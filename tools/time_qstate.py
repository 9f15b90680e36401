#!/usr/bin/env python3
"""Site updates per second of the q-state (Potts, clock) engine on the device, beside the numpy restatement of
tests/qstate_ref.py on one host core and, for q = 2, beside the Ising checkerboard kernel at the same size.

    python tools/time_qstate.py [--out FILE.json] [--quick] [--cluster-rate K] [--binner] [--case KIND:Q:L:W]

Cases: Potts q = 3, clock q = 8 and Potts q = 2 on SquareLattice(L), L = 32 and 128, with 64 and 1024 walkers, at
beta = 1.0, every tenth sweep measured.  A device time is the host clock around sweep() calls that end in a device
synchronise, after a warm-up of the same shape; the best of three windows is reported.  The restatement runs 8 walkers
(its time per site update does not depend on the count beyond that) for a few sweeps.  With --cluster-rate K > 0 the device
runs one cluster move per walker behind every K-th sweep (the sweeps then cost more than their site updates; the
restatement column stays the local sweep's).  With --binner every sweep is measured and each case runs twice, without and
with the device binner: us_per_binned_measurement is the difference of the two windows per sweep (the push of all walkers,
which run side by side).  --case runs one case only, e.g. potts:3:32:1024.  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402


def timed(mc, sweeps, windows=3):
    mc.sweep(sweeps)  # warm-up of the same shape
    best = float("inf")
    for _ in range(windows):
        t0 = time.perf_counter()
        mc.sweep(sweeps)
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sweep counts (a rehearsal, not a measurement)")
    ap.add_argument("--cluster-rate", type=int, default=0, help="a cluster move behind every K-th sweep (0: none)")
    ap.add_argument("--binner", action="store_true", help="every sweep measured; time the binner's push")
    ap.add_argument("--case", default=None, help="KIND:Q:L:W, one case only")
    args = ap.parse_args()
    only = tuple(args.case.split(":")) if args.case else None
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_qstate: no HIP device visible (there is no CPU fallback)")
    import qstate_ref as ref
    beta, rate = 1.0, (1 if args.binner else 10)
    results = []
    for kind, q in (("potts", 3), ("clock", 8), ("potts", 2)):
        for L in (32, 128):
            if only and (kind, str(q), str(L)) != only[:3]:
                continue
            l = g.SquareLattice(L)
            N = L * L
            table = ref.potts_table(q) if kind == "potts" else ref.clock_table(q)
            # the restatement on one host core
            wk = ref.Walkers(l, q, table, [beta] * 8, range(8))
            n_ref = 2 if L == 128 else 10
            wk.run(1, 1, 0, rate)
            t0 = time.perf_counter()
            wk.run(2, n_ref, 0, rate)
            host_rate = 8 * N * n_ref / (time.perf_counter() - t0)
            for W in (64, 1024):
                if only and str(W) != only[3]:
                    continue
                target = 5e7 * W if not args.quick else 2e6  # site updates per window: a few tenths of a second
                sweeps = max(10, int(target / (N * W)) // 10 * 10)
                model = g.PottsModel(q, l=l) if kind == "potts" else g.ClockModel(q, l=l)
                extra = {"cluster_rate": args.cluster_rate} if args.cluster_rate else {}
                mc = g.MC(model, beta=beta, n_walkers=W, seed=1, measure_rate=rate, **extra)
                dt = timed(mc, sweeps)
                acc = mc.analysis(0)["acc_rate"]
                mc.close()
                r = {"model": kind, "q": q, "L": L, "walkers": W, "sweeps": sweeps, "seconds": dt,
                     "site_updates_per_s": N * W * sweeps / dt, "acc_rate": acc, "host_site_updates_per_s": host_rate}
                if args.cluster_rate:
                    r["cluster_rate"] = args.cluster_rate
                if args.binner:
                    mc = g.MC(model, beta=beta, n_walkers=W, seed=1, measure_rate=rate, binner=5 * sweeps, **extra)
                    dtb = timed(mc, sweeps)
                    mc.close()
                    r["seconds_binner"] = dtb
                    r["us_per_binned_measurement"] = (dtb - dt) / sweeps * 1e6
                if q == 2:  # the yardstick: the Ising checkerboard kernel at the same L and walker count
                    im = g.MC(g.IsingModel(l=l), beta=beta / 2.0, n_walkers=W, seed=1, measure_rate=rate,
                              update="checkerboard")  # (the same physics: J_potts = 2 J_ising)
                    dti = timed(im, sweeps)
                    im.close()
                    r["ising_site_updates_per_s"] = N * W * sweeps / dti
                    r["ising_over_qstate"] = dt / dti
                results.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
