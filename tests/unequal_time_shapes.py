"""Shapes, reference chains and reference-error figures shared by tests/test_gpu_unequal_time_sizes.py.
TEST INFRASTRUCTURE ONLY (a plain module: pytest does not collect it).

Run as a script it needs no GPU: `python tests/unequal_time_shapes.py` prints, for the shapes of ROWS, the two kinds of
figures that the tests' bounds are derived from:
  * the oracle's stabilised G(k,l) against `brute_force_greens` (ANCHOR_PAIRS, after prepare);
  * the oracle's iterators against the oracle's own greens(k,l), per shape and `recalculate`, after one
    update_until_measure (the CombinedGreensIterator needs current_slice == 1).
All distances use the expression of the suite's bar: |a - ref|.max() / max(1, |ref|.max()).
"""
import os
import sys
import time

import numpy as np

BETA, DELTA_TAU, SAFE_MULT, SLICES, SEED = 1.0, 0.1, 5, 10, 31
M, S = SLICES, SAFE_MULT

# (id, n, lattice, environment set around handle creation, what the row reaches)
ROWS = [
    ("n64", 64, ("chain", 64), {}, "FULL GEMM forms, one tile; LDS-resident QR"),
    ("n100", 100, ("square", 10), {}, "partial tiles on both edges at n <= 256"),
    ("n128", 128, ("chain", 128), {}, "FULL, 2 x 2 tiles; misc kernels stride"),
    ("n256", 256, ("square", 16), {}, "one-launch UDT mixed with pivoted UDT + rdivp; Kronecker hopping"),
    ("n256-refpivot", 256, ("square", 16), {"DQMC_QR_NOBLOCKED": "1"}, "the reference's pivot rule at 256"),
    ("n257", 257, ("chain", 257), {}, "panel QR, TRSM panels 256 + 1, one-element partial tile"),
    ("n320", 320, ("chain", 320), {}, "FULL forms above 256, TRSM panels 160 + 160"),
]
ROW = {r[0]: r for r in ROWS}

# slice pairs (k, l) that walk every branch of compute_inverse_udt_block, full1 and full2 with M = 10, s = 5
PAIRS = [(0, 0), (M, M), (3, 3), (M, 0), (0, M), (7, 2), (2, 7), (10, 5), (5, 10), (4, 6), (6, 4), (9, 1), (1, 9)]
ANCHOR_PAIRS = [(0, 0), (7, 2), (2, 7), (M, 0)]


def walkers_of(n, kind):
    """one walker for the attractive model; two for the repulsive one up to n = 128, one above"""
    return 2 if kind == "repulsive" and n <= 128 else 1


def lattice(pkg, spec):
    return pkg.Chain(spec[1]) if spec[0] == "chain" else pkg.SquareLattice(spec[1])


def model(pkg, kind, spec):
    cls = pkg.HubbardModelAttractive if kind == "attractive" else pkg.HubbardModelRepulsive
    return cls(l=lattice(pkg, spec))


def dist(a, ref):
    return np.abs(np.asarray(a) - ref).max() / max(1.0, np.abs(ref).max())


class Reference:
    """The oracle chains of one shape and model (one per walker: the lattice's hopping matrix, the walker's HS field and
    seed, as tests/test_gpu_sizes.py::_oracles builds them), advanced by prepare and `sweeps` update_until_measure, with
    one UnequalTimeOracle per walker and block and the effective G(k,l) computed once per pair."""

    def __init__(self, O, UT, mdl, kind, confs, seeds, sweeps=0):
        T = mdl.hopping_matrix()[0]
        self.UT, self.kind = UT, kind
        self.oracles = []
        for conf, seed in zip(confs, seeds):
            o = O.OracleDQMC(mdl.l.sites, kind, beta=BETA, delta_tau=DELTA_TAU, safe_mult=SAFE_MULT, U=mdl.U, hopping=T)
            o.set_conf(conf)
            o.seed(seed)
            o.prepare()
            for _ in range(sweeps):
                o.update_until_measure()
            self.oracles.append(o)
        self.nb = self.oracles[0].nb
        self.ut = [[UT.UnequalTimeOracle(o, b) for b in range(o.nb)] for o in self.oracles]
        self._g = {}

    def greens_eff(self, w, b, k, l):
        key = (w, b, k, l)
        if key not in self._g:
            g = self.ut[w][b].calculate_greens(k, l)
            g.setflags(write=False)
            self._g[key] = g
        return self._g[key]

    def greens(self, w, b, k, l):
        return self.ut[w][b].to_true(self.greens_eff(w, b, k, l))

    def fresh_ut(self, w, b):
        """a stack of its own (for a build under another pivot rule)"""
        return self.UT.UnequalTimeOracle(self.oracles[w], b)


def initial_confs(pkg, n, walkers, seed=SEED):
    """the HS fields and seeds that DQMC(..., seed=seed) gives its walkers"""
    seeds = [seed + w for w in range(walkers)]
    return [pkg.rand_conf(np.random.Generator(np.random.Philox(key=s)), n, SLICES) for s in seeds], seeds


# ---- what the bounds are derived from (CPU only) ----------------------------------------------------------------------
def anchor_error(ref, brute_force_greens, w=0):
    """worst distance of the oracle's stabilised G(k,l) from the dense evaluation of the definition"""
    worst = 0.0
    for b in range(ref.nb):
        for k, l in ANCHOR_PAIRS:
            worst = max(worst, dist(ref.greens_eff(w, b, k, l), brute_force_greens(ref.oracles[w], b, k, l)))
    return worst


def iterator_errors(ref, w=0):
    """{recalculate: worst distance of the oracle's iterators from the oracle's own greens(k, l)} for GreensIterator(0,
    recalculate) and CombinedGreensIterator(recalculate) with recalculate = s and 4 s; key "l3": GreensIterator(3, s)"""
    out = {}
    o = ref.oracles[w]
    for recalc in (S, 4 * S):
        worst = 0.0
        for b in range(ref.nb):
            ut = ref.ut[w][b]
            for k, g in enumerate(ut.greens_iterator(0, recalc)):
                worst = max(worst, dist(g, ref.greens(w, b, k, 0)))
            for i, (g0l, gl0, gll) in enumerate(ut.combined_greens_iterator(o.greens_eff()[b], recalc)):
                l = i + 1
                worst = max(worst, dist(g0l, ref.greens(w, b, 0, l)), dist(gl0, ref.greens(w, b, l, 0)),
                            dist(gll, ref.greens(w, b, l, l)))
        out[recalc] = worst
    worst = 0.0
    for b in range(ref.nb):
        for i, g in enumerate(ref.ut[w][b].greens_iterator(3, S)):
            worst = max(worst, dist(g, ref.greens(w, b, 3 + i, 3)))
    out["l3"] = worst
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    from oracle import oracle as O, unequal_time_oracle as UT
    pkg = g.load_package()
    O.build()
    for rid in ("n64", "n256"):
        _, n, spec, _, _ = ROW[rid]
        for kind in ("attractive", "repulsive"):
            t0 = time.time()
            confs, seeds = initial_confs(pkg, n, 1)
            ref = Reference(O, UT, model(pkg, kind, spec), kind, confs, seeds)
            print("anchor    %-5s %-10s oracle vs brute force: %.3g   (%.1f s)"
                  % (rid, kind, anchor_error(ref, UT.brute_force_greens), time.time() - t0), flush=True)
    for rid in ("n64", "n128", "n256"):
        _, n, spec, _, _ = ROW[rid]
        for kind in ("attractive", "repulsive"):
            t0 = time.time()
            confs, seeds = initial_confs(pkg, n, 1)
            ref = Reference(O, UT, model(pkg, kind, spec), kind, confs, seeds, sweeps=1)
            e = iterator_errors(ref)
            print("iterators %-5s %-10s oracle iterator vs oracle greens: recalculate = s %.3g, 4 s %.3g, (3, s) %.3g   "
                  "(%.1f s)" % (rid, kind, e[S], e[4 * S], e["l3"], time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
