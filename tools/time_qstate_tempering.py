#!/usr/bin/env python3
"""What replica exchange costs in the q-state engine, and what it gives: microseconds per exchange round (a launch of its
own behind the sweep kernel), swap rates and replica round trips.

    python tools/time_qstate_tempering.py [--out FILE.json] [--quick] [--case Q:L:W]

Cases: Potts q = 3 and q = 8 on SquareLattice(L), L = 16, 32 and 64, with 64 and 1024 walkers in ladders of R = 8 betas
spread by +-4 % around beta_c = ln(1 + sqrt q), a round after every sweep (k = 1) and after every tenth (k = 10), every
tenth sweep measured.  A time is the host clock around sweep() calls that end in a device synchronise, after a warm-up of
the same shape, best of three windows; us_per_round is the difference to the same run without exchange, per round.  Round
trips are counted on the first ladder over a further 200 rounds: a replica that has visited slot 0 and then slot R - 1 and
comes back to slot 0 has made one.  Prints one JSON line per case."""
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

R = 8


def timed(mc, sweeps, windows=3):
    mc.sweep(sweeps)
    best = float("inf")
    for _ in range(windows):
        t0 = time.perf_counter()
        mc.sweep(sweeps)
        best = min(best, time.perf_counter() - t0)
    return best


def round_trips(mc, k, polls):
    """round trips of the replicas of ladder 0 over `polls` rounds"""
    state = {}  # label -> 0: last end visited was slot 0, 1: slot R - 1
    trips = 0
    for _ in range(polls):
        mc.sweep(k)
        labels = [mc.exchange_stats(w).replica for w in range(R)]
        for slot, end in ((0, 0), (R - 1, 1)):
            lab = labels[slot]
            if state.get(lab) is not None and state[lab] != end and end == 0:
                trips += 1
            state[lab] = end
    return trips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sweep counts (a rehearsal, not a measurement)")
    ap.add_argument("--case", default=None, help="Q:L:W, one case only")
    args = ap.parse_args()
    only = tuple(int(x) for x in args.case.split(":")) if args.case else None
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_qstate_tempering: no HIP device visible (there is no CPU fallback)")
    results = []
    for q in (3, 8):
        beta_c = math.log(1.0 + math.sqrt(q))
        betas = list(beta_c * np.linspace(0.96, 1.04, R))
        for L in (16, 32, 64):
            l = g.SquareLattice(L)
            N = L * L
            for W in (64, 1024):
                if only and (q, L, W) != only:
                    continue
                target = 2e7 * W if not args.quick else 2e6
                sweeps = max(10, int(target / (N * W)) // 10 * 10)
                kw = dict(beta=betas, n_walkers=W, seed=1, measure_rate=10)
                mc = g.MC(g.PottsModel(q, l=l), tempering=(R, 0), **kw)  # the ladder's betas, no rounds
                base = timed(mc, sweeps)
                mc.close()
                for k in (1, 10):
                    mc = g.MC(g.PottsModel(q, l=l), tempering=(R, k), **kw)
                    dt = timed(mc, sweeps)
                    rounds = sweeps // k
                    x = [mc.exchange_stats(w) for w in range(R - 1)]
                    trips = round_trips(mc, k, 20 if args.quick else 200)
                    mc.close()
                    r = {"q": q, "L": L, "walkers": W, "R": R, "k": k, "sweeps": sweeps, "seconds": dt,
                         "seconds_without_rounds": base, "us_per_sweep_without_rounds": base / sweeps * 1e6,
                         "us_per_round": (dt - base) / rounds * 1e6,
                         "swap_rates": [s.acc_exchange / max(s.prop_exchange, 1) for s in x],
                         "round_trips_ladder0_in_200_rounds": trips}
                    results.append(r)
                    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
