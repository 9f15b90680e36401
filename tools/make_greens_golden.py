"""Writes tests/golden/greens_graded.json and greens_graded.npy: extended-precision expected values of
calculate_greens_AVX! on the chain-graded inputs of tests/greens_ref.py, for tests/test_gpu_greens_graded.py and
tests/test_greens_golden.py.  CPU only; needs the CPU oracle.

    python tools/make_greens_golden.py [--jobs 8] [--cache FILE]

Per (n, unit) the inputs are graded_udt_inputs(n, g, SEED0 + n, ...)[unit]; G comes from greens_mp at 80 digits (minutes
at n >= 256).  Kept, rounded to float64: the two probes G V and G' V (n x 4 each) and diag(G) - 9 n numbers per case, all
cases one after the other in the .npy (binary: as text they are 700 KB), each case's "offset" in the .json - and, in
the .json, the generator's arguments and the float64 oracle's own error against them under the reference's pivot rule (orc_set_udt_presort(0)) and with every call site
pre-sorted (orc_set_udt_presort(7), what the device's one-launch UDT does at n = 256), in the measure of
greens_ref.probe_err / diag_err; up to n = 64 also the oracle's relerr over every entry of G.

Choice of g.  Per n the largest g of 40, 30, 20, 10 at which the reference-rule oracle is within 1e-11 of the extended-
precision values in both measures, for every unit kept; the errors at the rejected g are recorded under "sizes".
--cache keeps the extended-precision values between runs of this tool."""
import argparse
import json
import multiprocessing as mproc
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import greens_ref as ref  # noqa: E402

SEED0 = 1000
G_CANDIDATES = [40, 30, 20, 10]
BOUND = 1e-11
UNITS = {16: [0, 1, 2], 36: [0], 64: [0, 1, 2], 100: [0, 1], 256: [0, 1, 2, 8, 32, 64], 257: [0, 1], 292: [0, 1],
         324: [0, 1]}
FULL_UP_TO = 64


def seed_of(n):
    return SEED0 + n


def inputs(n, g, unit):
    return ref.graded_unit(n, g, seed_of(n) + unit)


def expected(job):
    """extended precision -> probes and diagonal rounded to float64 (and G itself up to n = 64, for the oracle's full error)"""
    n, g, unit = job
    import mpmath as mp
    a = inputs(n, g, unit)
    G = ref.greens_mp(a)
    with mp.workdps(ref.DIGITS):
        pr = [ref.to_float(p) for p in ref.probe(G, ref.probe_matrix(n, seed_of(n)))]
        out = dict(probe=[p.tolist() for p in pr], diag=ref.to_float(np.diag(G)).tolist())
    if n <= FULL_UP_TO:
        from oracle import oracle as O
        out["oracle_full"] = [ref.full_err(ref.oracle_greens(O, a, m), G) for m in (0, ref.PRESORT_ALL_SITES)]
    return out


def oracle_errors(n, g, unit, exp):
    from oracle import oracle as O
    a = inputs(n, g, unit)
    V = ref.probe_matrix(n, seed_of(n))
    out = {}
    for name, mask in (("reference", 0), ("presorted", ref.PRESORT_ALL_SITES)):
        G = ref.oracle_greens(O, a, mask)
        out[name] = dict(probe=ref.probe_err(G, V, exp["probe"]), diag=ref.diag_err(G, exp["diag"]))
    if "oracle_full" in exp:
        out["reference"]["full"], out["presorted"]["full"] = exp["oracle_full"]
    return out


class Runner:
    def __init__(self, jobs, cache):
        self.pool = mproc.Pool(jobs)
        self.cache_path = cache
        self.cache = pickle.load(open(cache, "rb")) if cache and os.path.exists(cache) else {}

    def run(self, jobs):
        todo = sorted((j for j in jobs if j not in self.cache), key=lambda j: -j[0])
        for j, r in zip(todo, self.pool.imap(expected, todo, chunksize=1)):
            self.cache[j] = r
            print("done", j, flush=True)
            if self.cache_path:
                pickle.dump(self.cache, open(self.cache_path, "wb"))
        return [self.cache[j] for j in jobs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=ref.GOLDEN_PATH)
    args = ap.parse_args()
    from oracle import oracle as O
    O.build()
    run = Runner(args.jobs, args.cache)
    sizes = {n: dict(seed=seed_of(n), g=None, rejected={}) for n in UNITS}
    cases = {}
    for g in G_CANDIDATES:
        open_n = [n for n in UNITS if sizes[n]["g"] is None]
        jobs = [(n, g, u) for n in open_n for u in UNITS[n]]
        for j, exp in zip(jobs, run.run(jobs)):
            cases[j] = dict(n=j[0], g=g, seed=seed_of(j[0]), unit=j[2], oracle_err=oracle_errors(*j, exp), probe=exp["probe"],
                            diag=exp["diag"])
        for n in open_n:
            worst = max(max(cases[(n, g, u)]["oracle_err"]["reference"][k] for k in ("probe", "diag")) for u in UNITS[n])
            print("n = %d, g = %d: reference-rule oracle %.3e" % (n, g, worst), flush=True)
            if worst <= BOUND:
                sizes[n]["g"] = g
                sizes[n]["oracle_reference_rule"] = worst
            else:
                sizes[n]["rejected"][str(g)] = worst
    for n in UNITS:
        if sizes[n]["g"] is None:
            raise SystemExit("n = %d: the oracle misses %g at every g" % (n, BOUND))
    kept = [cases[(n, sizes[n]["g"], u)] for n in UNITS for u in UNITS[n]]
    values, offset = [], 0
    for c in kept:  # the numbers go to the .npy: probe G V, probe G' V (row-major n x 4 each), diag
        v = np.concatenate([np.asarray(c.pop(k), dtype=np.float64).reshape(-1) for k in ("probe", "diag")])
        assert v.size == 9 * c["n"]
        c["offset"] = offset
        offset += v.size
        values.append(v)
    values_path = os.path.splitext(args.out)[0] + ".npy"
    np.save(values_path, np.concatenate(values).astype("<f8"))
    head = dict(digits=ref.DIGITS, probe_columns=ref.PROBE_COLUMNS, presort_mask=ref.PRESORT_ALL_SITES, bound=BOUND,
                g_candidates=G_CANDIDATES, other_units_g=3, sizes={str(n): sizes[n] for n in UNITS})
    with open(args.out, "w") as f:  # one case per line: the arrays would otherwise take a line per number
        f.write("{\n")
        for k, v in head.items():
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(v)))
        f.write(' "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c) for c in kept))
        f.write("\n ]\n}\n")
    for path in (args.out, values_path):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
