"""Writes tests/golden/logdet_sizes.json: the expected log|det(I + B_M ... B_1)| and signs of the logdet tests at every
size-selected kernel form (tests/test_gpu_logdet_sizes.py, tests/test_logdet_golden.py) and of the global moves away
from 4 x 4 (tests/test_gpu_global_move.py).  CPU only; needs the built package for the lattices and the CPU oracle.

    python tools/make_logdet_golden.py [--jobs 8] [--cache FILE]

Seeds.  Per repulsive case with n >= 64 the float64 oracle (global_move_ref.oracle_logdet) scans the fields
field(seed, n, M) from the case's first seed on and four seeds are kept: the first two whose product of signs is negative,
the first with both blocks negative (else a third negative product) and the first with both positive; where fewer than
two negative products turn up, the first four seeds of the scan (a positive-sign case).  The counts of
the scan go into the file ("search").  Every kept field is then confirmed:
  n <= 100  slogdet_mp at 60 digits is the expected value; the oracle's signs must equal its signs.
  n = 256   oracle_logdet is the expected value, accepted only if second_route_logdet (forward chain, pivoted QR every 5
            slices, Loh's splitting of D) gives the same signs and logabsdet within 1e-9; both are stored.
The moves: TriangularLattice(8) with the proposals of FLIP_ALL and FLIP_SITE (sites chosen so that one walker's
proposal has p < 0), and 4 x 4 attractive at dtau = 0.01, beta = 3 (300 slices) with FLIP_SITE.  --cache keeps the
extended-precision values between runs of this tool."""
import argparse
import json
import multiprocessing as mproc
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as entry  # noqa: E402
import global_move_ref as ref  # noqa: E402

DTAU, SAFE_MULT, SECOND_SAFE_MULT = 0.1, 10, 5
CASES = [
    dict(name="square6", lattice=["square", 6], model="repulsive", U=8.0, mu=0.0, beta=2.0, first_seed=100, scan=0),
    dict(name="triangular8", lattice=["triangular", 8], model="repulsive", U=8.0, mu=0.0, beta=4.0, first_seed=2, scan=60),
    dict(name="triangular10", lattice=["triangular", 10], model="repulsive", U=8.0, mu=0.0, beta=4.0, first_seed=0,
         scan=60),
    dict(name="cubic4", lattice=["cubic", 4], model="repulsive", U=8.0, mu=0.0, beta=2.0, first_seed=0, scan=200),
    dict(name="triangular16", lattice=["triangular", 16], model="repulsive", U=8.0, mu=0.0, beta=2.0, first_seed=0,
         scan=200),
    dict(name="square16_attractive", lattice=["square", 16], model="attractive", U=4.0, mu=0.5, beta=1.0, first_seed=200,
         scan=0),
]
SLICES300 = dict(name="slices300", lattice=["square", 4], model="attractive", U=4.0, mu=0.5, beta=3.0, dtau=0.01)


def _model(case):
    return ref.golden_model(entry.load_package(), case)


def _slices(case):
    return int(round(case["beta"] / case.get("dtau", DTAU)))


def _conf(case, seed, flip):
    """the field of a seed, or its proposal: flip = None, "all" or a site"""
    m = _model(case)
    c = ref.field(seed, m.hopping_matrix()[0].shape[0], _slices(case))
    if flip is None:
        return m, c
    return m, ref.apply_flip(c, ref.FLIP_ALL) if flip == "all" else ref.apply_flip(c, ref.FLIP_SITE, int(flip))


def _oracle(args):
    case, seed, flip = args
    m, c = _conf(case, seed, flip)
    lad, sg, _ = ref.oracle_logdet(entry.load_oracle(), m, case.get("dtau", DTAU), SAFE_MULT, c)
    return lad, sg


def _second(args):
    case, seed, flip = args
    m, c = _conf(case, seed, flip)
    return ref.second_route_logdet(entry.load_oracle(), m, case.get("dtau", DTAU), SECOND_SAFE_MULT, c)


def _mp(args):
    case, seed, flip = args
    m, c = _conf(case, seed, flip)
    lad, sg = ref.slogdet_mp(m, case.get("dtau", DTAU), c)
    return [ref.mp.nstr(x, 30) for x in lad], sg


class Runner:
    def __init__(self, jobs, cache):
        self.pool = mproc.Pool(jobs)
        self.cache_path = cache
        self.cache = pickle.load(open(cache, "rb")) if cache and os.path.exists(cache) else {}

    def mp(self, jobs):
        key = lambda j: json.dumps([{k: v for k, v in j[0].items() if k not in ("first_seed", "scan")}, j[1], j[2]],
                                   sort_keys=True)
        todo = [j for j in jobs if key(j) not in self.cache]
        for j, r in zip(todo, self.pool.map(_mp, todo, chunksize=1)):
            self.cache[key(j)] = r
            if self.cache_path:
                pickle.dump(self.cache, open(self.cache_path, "wb"))
        return [self.cache[key(j)] for j in jobs]


def pick_seeds(run, case):
    """-> (four seeds, search record)"""
    first, scan = case["first_seed"], case["scan"]
    if not scan:
        return [first + i for i in range(4)], None
    seeds = list(range(first, first + scan))
    signs = [sg for _, sg in run.pool.map(_oracle, [(case, s, None) for s in seeds])]
    negprod = [s for s, g in zip(seeds, signs) if g[0] * g[1] < 0]
    both = [s for s, g in zip(seeds, signs) if g[0] < 0 and g[1] < 0]
    plus = [s for s, g in zip(seeds, signs) if g[0] > 0 and g[1] > 0]
    rec = dict(first_seed=first, seeds_tried=scan, seeds_with_a_negative_block=len(negprod) + len(both),
               seeds_with_a_negative_product=len(negprod))
    if len(negprod) < 2:  # (a bipartite lattice at half filling: the product is positive for every field)
        return seeds[:4], rec
    third = both[:1] or negprod[2:3]
    return sorted(negprod[:2] + third + plus[:4 - 2 - len(third)]), rec


def expected(run, case, jobs):
    """the expected values of a list of (case, seed, flip): -> dict(sign, logabsdet, oracle_sign, oracle_logabsdet, ...)"""
    orc = run.pool.map(_oracle, jobs, chunksize=1)
    out = dict(oracle_sign=[o[1] for o in orc], oracle_logabsdet=[[repr(x) for x in o[0]] for o in orc])
    n = _conf(*jobs[0])[1].shape[0]
    if n <= 100:
        gold = run.mp(jobs)
        out.update(reference="mpmath, 60 digits", sign=[g[1] for g in gold], logabsdet=[g[0] for g in gold])
    else:
        sec = run.pool.map(_second, jobs, chunksize=1)
        out.update(reference="oracle_logdet, confirmed by second_route_logdet", sign=out["oracle_sign"],
                   logabsdet=out["oracle_logabsdet"], second_logabsdet=[[repr(x) for x in s[0]] for s in sec])
        for j, o, s in zip(jobs, orc, sec):
            if o[1] != s[1] or max(abs(a - b) for a, b in zip(o[0], s[0])) > 1e-9:
                raise SystemExit("the two float64 routes disagree at %r: %r %r" % (j[1:], o, s))
    if out["sign"] != out["oracle_sign"]:
        raise SystemExit("oracle and reference signs differ in %s: %r %r" % (case["name"], out["sign"], out["oracle_sign"]))
    return out


def spec(case):
    d = {k: case[k] for k in ("lattice", "model", "U", "mu", "beta")}
    d["slices"] = _slices(case)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=ref.GOLDEN_PATH)
    args = ap.parse_args()
    entry.load_oracle().build()
    run = Runner(args.jobs, args.cache)
    gold = dict(delta_tau=DTAU, safe_mult=SAFE_MULT, logdet={}, moves={})
    for case in CASES:
        seeds, rec = pick_seeds(run, case)
        e = dict(spec(case), seeds=seeds, search=rec)
        e["n"] = int(_conf(case, seeds[0], None)[1].shape[0])
        e.update(expected(run, case, [(case, s, None) for s in seeds]))
        gold["logdet"][case["name"]] = e
        print(case["name"], seeds, e["sign"], rec, flush=True)

    # the moves at TriangularLattice(8): the fields of the logdet case; FLIP_SITE sites (5 seed + 3) % 64, but walker 0's
    # the first site whose proposal has a negative weight; FLIP_ALL needs a walker with a negative weight as it stands
    case = CASES[1]
    cur = gold["logdet"]["triangular8"]
    seeds, n = cur["seeds"], cur["n"]
    sites = [(5 * s + 3) % n for s in seeds]
    s0 = cur["sign"][0][0] * cur["sign"][0][1]
    scan = run.pool.map(_oracle, [(case, seeds[0], i) for i in range(n)])
    neg = [i for i, (_, g) in enumerate(scan) if g[0] * g[1] * s0 < 0]
    if not neg:
        raise SystemExit("no FLIP_SITE proposal of walker 0 has p < 0")
    sites[0] = neg[0]
    mv = dict(case="triangular8", seeds=seeds, sites=sites, sites_with_negative_p_for_walker_0=len(neg))
    mv["all"] = expected(run, case, [(case, s, "all") for s in seeds])
    mv["site"] = expected(run, case, [(case, s, i) for s, i in zip(seeds, sites)])
    for kind in ("all", "site"):
        p = [a[0] * a[1] * b[0] * b[1] for a, b in zip(cur["sign"], mv[kind]["sign"])]
        print("moves triangular8", kind, "signs of p", p, flush=True)
        if kind == "site" and min(p) > 0:
            raise SystemExit("no negative p among the FLIP_SITE proposals")
        mv[kind]["sign_of_p"] = p
    gold["moves"]["triangular8"] = mv

    # FLIP_SITE over 300 slices, 4 x 4 attractive
    case = SLICES300
    seeds = [400, 401, 402, 403]
    sites = [(5 * s + 3) % 16 for s in seeds]
    e = dict(spec(case), delta_tau=case["dtau"], seeds=seeds, sites=sites, n=16)
    e["cur"] = expected(run, case, [(case, s, None) for s in seeds])
    e["site"] = expected(run, case, [(case, s, i) for s, i in zip(seeds, sites)])
    gold["moves"]["slices300"] = e
    with open(args.out, "w") as f:
        json.dump(gold, f, indent=1)
        f.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
