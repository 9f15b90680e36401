#!/usr/bin/env python3
"""What the stiffness measurement of the q-state engine (the helicity modulus, csrc/qs_stiffness.inl) costs on the
device, beside the sweep it follows, and that a handle without it runs as fast as the parent commit's.

    python tools/time_qstate_stiffness.py [--out FILE.json] [--quick] [--case L:W] [--parent DIR [--rounds 3]]

Cases: clock q = 6 on SquareLattice(L), L = 16, 32, 64 and 128, with 64 and 1024 walkers, n_dir = 2 (the cartesian axes),
at beta = 1.0, every sweep measured.  Each case times four handles in the same call, with the same seeds and so the same
chains: without and with the measurement, each without and with the device binner.  A time is the host clock around
sweep() calls that end in a device synchronise, after a warm-up of the same shape; the best of three windows is
reported.  us_per_sweep is the handle without the measurement; us_per_measurement is the difference of the two windows
per measured sweep: the measurement kernel of the whole handle (all walkers side by side), the launch that now ends at
the measured sweep and, with the binner, the push of the third section.  --case runs one case only, e.g. 64:64.

--parent DIR: a built tree of the parent commit.  tools/time_qstate.py (the feature off: no handle there has the
measurement) then runs as a child process in this tree and in DIR in turn, --rounds times each, and the site updates per
second of every case are reported as (min, max) per tree: overlapping ranges are the condition.  Prints one JSON line per
case."""
import argparse
import json
import os
import subprocess
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


def feature_off(parent, rounds, quick):
    """time_qstate.py in this tree and in `parent`, alternated: {case: {"this" | "parent": [site updates per s ..]}}"""
    rates = {}
    for r in range(rounds):
        trees = (("this", ROOT), ("parent", os.path.abspath(parent)))
        for name, tree in (trees if r % 2 == 0 else trees[::-1]):  # (the order of the two reversed from round to round)
            cmd = [sys.executable, os.path.join(tree, "tools", "time_qstate.py")] + (["--quick"] if quick else [])
            out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("time_qstate.py failed in %s:\n%s" % (tree, out.stderr[-2000:]))
            print("round %d, %s tree: done" % (r + 1, name), file=sys.stderr, flush=True)
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    c = json.loads(line)
                    key = "%s:%d:%d:%d" % (c["model"], c["q"], c["L"], c["walkers"])
                    rates.setdefault(key, {"this": [], "parent": []})[name].append(c["site_updates_per_s"])
    rows = []
    for key, v in rates.items():
        row = {"feature_off_case": key, "this_min": min(v["this"]), "this_max": max(v["this"]),
               "parent_min": min(v["parent"]), "parent_max": max(v["parent"]), "rounds": rounds}
        row["ranges_overlap"] = row["this_max"] >= row["parent_min"] and row["parent_max"] >= row["this_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sweep counts (a rehearsal, not a measurement)")
    ap.add_argument("--case", default=None, help="L:W, one case only")
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: compare time_qstate.py's rates")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    only = tuple(args.case.split(":")) if args.case else None
    g = entry.load_package()
    if g.device_count() < 1:
        raise SystemExit("time_qstate_stiffness: no HIP device visible (there is no CPU fallback)")
    beta, q = 1.0, 6
    results = []
    for L in (16, 32, 64, 128):
        for W in (64, 1024):
            if only and (str(L), str(W)) != only:
                continue
            l = g.SquareLattice(L)
            N = L * L
            target = 2e8 if not args.quick else 2e6  # site updates per window
            sweeps = min(2000, max(20, int(target / (N * W)) // 10 * 10))
            model = g.ClockModel(q, l=l)
            dt = {}
            for stiffness in (False, True):
                for binner in (False, True):
                    mc = g.MC(model, beta=beta, n_walkers=W, seed=1, measure_rate=1, stiffness=stiffness,
                              binner=5 * sweeps if binner else False)
                    dt[stiffness, binner] = timed(mc, sweeps)
                    mc.close()
            r = {"model": "clock", "q": q, "L": L, "walkers": W, "n_dir": 2, "measure_rate": 1, "sweeps": sweeps,
                 "us_per_sweep": dt[False, False] / sweeps * 1e6,
                 "us_per_measurement": (dt[True, False] - dt[False, False]) / sweeps * 1e6,
                 "us_per_sweep_binner": dt[False, True] / sweeps * 1e6,
                 "us_per_measurement_binner": (dt[True, True] - dt[False, True]) / sweeps * 1e6}
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.parent:
        results += feature_off(args.parent, args.rounds, args.quick)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
