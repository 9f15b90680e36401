#!/usr/bin/env python3
"""Bytes of the classical MC flavor's state blob and the times of state() / set_state() on the device, next to the time
of one sweep in the same call.

    python tools/time_mc_checkpoint.py [--out FILE.json] [--quick]

Cases: Potts q = 3 on SquareLattice(L), L = 32 and 64, with 64 and 1024 walkers, and the Ising model (sequential sweep) at
L = 64 with 256 walkers, at beta = 1.0 (Ising: 0.44), every sweep measured; each case without a binner and with the binner
at its default capacity (100000 measurements).  A time is the host clock around the call, which ends in a device
synchronise, after one call of the same shape; the best of five is reported (sweeps: the best of three windows, per
sweep).  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def best(f, n):
    f()
    t = float("inf")
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t = min(t, time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="few sweeps (a rehearsal, not a measurement)")
    args = ap.parse_args()
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_mc_checkpoint: no HIP device visible (there is no CPU fallback)")
    cases = [("potts3", L, W) for L in (32, 64) for W in (64, 1024)] + [("ising", 64, 256)]
    results = []
    for kind, L, W in cases:
        l = g.SquareLattice(L)
        for binner in (False, True):
            if kind == "ising":
                mc = g.MC(g.IsingModel(l=l), beta=0.44, n_walkers=W, seed=1, binning=binner)
            else:
                mc = g.MC(g.PottsModel(3, l=l), beta=1.0, n_walkers=W, seed=1, binner=binner)
            sweeps = 4 if args.quick else max(4, int(2e7 / (L * L * max(W, 512) / 512)) // (L * L))
            t_sweep = best(lambda: mc.sweep(sweeps), 3) / sweeps
            blob = mc.state()
            t_state = best(mc.state, 5)
            t_set = best(lambda: mc.set_state(blob), 5)
            assert mc.state().tobytes() == blob.tobytes()
            r = {"model": kind, "L": L, "walkers": W, "binner": binner, "blob_bytes": int(blob.size),
                 "ms_state": 1e3 * t_state, "ms_set_state": 1e3 * t_set, "ms_sweep": 1e3 * t_sweep, "sweeps_timed": sweeps}
            mc.close()
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
