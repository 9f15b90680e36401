#!/usr/bin/env python3
"""What the scaling measurement of the q-state engine (S(k), csrc/qs_scaling.inl) costs on the device, beside the
sweep it follows.

    python tools/time_qstate_scaling.py [--out FILE.json] [--quick] [--case KIND:Q:L:W]

Cases: Potts q = 3 and clock q = 8 on SquareLattice(L), L = 16, 32, 64 and 128, with 64 and 1024 walkers, n_k = 2 (the
reciprocal vectors), at beta = 1.0, measuring every sweep and every tenth.  Each case times four handles in the same
call, with the same seeds and so the same chains: without and with the measurement, each without and with the device
binner.  A time is the host clock around sweep() calls that end in a device synchronise, after a warm-up of the same
shape; the best of three windows is reported.  us_per_sweep is the handle without the measurement; us_per_measurement is
the difference of the two windows per measured sweep: the measurement kernel of the whole handle (all walkers side by
side), the launch that now ends at the measured sweep and, with the binner, the push of the second section.
--case runs one case only, e.g. potts:3:64:64.  Prints one JSON line per case and measure rate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--case", default=None, help="KIND:Q:L:W, one case only")
    args = ap.parse_args()
    only = tuple(args.case.split(":")) if args.case else None
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_qstate_scaling: no HIP device visible (there is no CPU fallback)")
    beta = 1.0
    results = []
    for kind, q in (("potts", 3), ("clock", 8)):
        for L in (16, 32, 64, 128):
            for W in (64, 1024):
                if only and (kind, str(q), str(L), str(W)) != only:
                    continue
                l = g.SquareLattice(L)
                N = L * L
                target = 2e8 if not args.quick else 2e6  # site updates per window
                sweeps = min(2000, max(20, int(target / (N * W)) // 10 * 10))
                model = g.PottsModel(q, l=l) if kind == "potts" else g.ClockModel(q, l=l)
                for rate in (1, 10):
                    n_meas = sweeps // rate
                    dt = {}
                    for scaling in (False, True):
                        for binner in (False, True):
                            mc = g.MC(model, beta=beta, n_walkers=W, seed=1, measure_rate=rate, scaling=scaling,
                                      binner=5 * n_meas if binner else False)
                            dt[scaling, binner] = timed(mc, sweeps)
                            mc.close()
                    r = {"model": kind, "q": q, "L": L, "walkers": W, "n_k": 2, "measure_rate": rate, "sweeps": sweeps,
                         "us_per_sweep": dt[False, False] / sweeps * 1e6,
                         "us_per_measurement": (dt[True, False] - dt[False, False]) / n_meas * 1e6,
                         "us_per_sweep_binner": dt[False, True] / sweeps * 1e6,
                         "us_per_measurement_binner": (dt[True, True] - dt[False, True]) / n_meas * 1e6}
                    results.append(r)
                    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
