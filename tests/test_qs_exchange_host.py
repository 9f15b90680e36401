"""The host arithmetic of the q-state engine's replica exchange (csrc/mc_tables.h: J, the pair tables, the product rule,
the cut of a dqmc_qs_sweep call into launches) without a GPU: tests/qs_exchange_check.cpp under the host sanitizers,
every line it prints restated here from the inputs it prints beside them (tests/qstate_tempering_ref.py)."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_tempering_ref as tref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """g++ -fsanitize=address,undefined, run once as a child process on the CPU (the sanitizer runtimes are linked into
    the program); -ffp-contract=off: a product is a product"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host code"
    exe = str(tmp_path_factory.mktemp("qs_exchange") / "qs_exchange_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "qs_exchange_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and "FAILED" not in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    return out.stdout


def test_bits(printed):
    """J is the smallest integer with 2^J > 2 n_bonds max |e_q30|: 50 at the create-time limits, 0 where no energy
    difference exists, above 62 where a handle must be refused"""
    rows = re.findall(r"^bits (\d+) (\d+) :((?: -?\d+)+)$", printed, re.M)
    assert len(rows) == 9
    got, tables = {}, {}
    for nb, J, e in rows:
        e = [int(x) for x in e.split()]
        assert int(J) == tref.exchange_bits(int(nb), e), (nb, e)
        got[int(nb)] = int(J)
        tables[int(nb)] = e
    assert got[65536] == 50 and got[0] == 0 and got[7] == 0 and got[1] == 2 and got[18] == 36 and got[2147483647] > 62
    # the inclusive table limit |e_q30| = 2^32 on 324 bonds (CubicLattice(4, 3)) and 80 bonds (BilayerSquareLattice(4);
    # tests/test_qstate_models_host.py checks these counts against the lattices): 2^42 > 648 2^32 >= 2^41, 2^40 > 160 2^32
    assert tables[324] == ref.tables(7, ref.clock_table(7), 4.0)[0].tolist() and tables[324][0] == 2 ** 32
    assert tables[80] == ref.tables(3, ref.potts_table(3), -4.0)[0].tolist() and tables[80][0] == -2 ** 32
    assert got[324] == 42 and got[80] == 40


def test_the_beta_domain_of_the_acceptance_product(printed):
    """qs_beta_in_domain accepts iff fl(fl(beta z) range) <= 700, range = (max e_q30 - min e_q30) 2^-30: restated for
    nine neighbouring doubles around 700 / (z range), which lie on both sides, for the clock table at z = 4 and the
    |J e| = 4 tables at z = 8.  The refusal names beta, z, the range and the bound.  At the largest accepted beta every
    partial product of z table entries is finite and non-zero: 10^4 random index tuples (seed 20261) and the two extreme
    tuples, whose last partial product is e^(+-700) to rounding."""
    lines = printed.splitlines()
    heads = [i for i, s in enumerate(lines) if s.startswith("domain ")]
    assert len(heads) == 4
    seen = set()
    for h in heads:
        m = re.match(r"^domain (\d+) (\S+) :((?: -?\d+)+)$", lines[h])
        z, rng, e = int(m.group(1)), float.fromhex(m.group(2)), [int(x) for x in m.group(3).split()]
        assert rng == (max(e) - min(e)) / 2.0 ** 30
        seen.add((z, rng))
        verdicts = []
        for s in lines[h + 1:]:
            v = re.match(r"^verdict (\d+) (\S+) ([01])$", s)
            if v:
                beta = float.fromhex(v.group(2))
                assert int(v.group(1)) == z and bool(int(v.group(3))) == (beta * float(z) * rng <= 700.0), (z, beta)
                verdicts.append((beta, bool(int(v.group(3)))))
            elif s.startswith("refusal "):
                for word in ("fn: beta = ", "z = %d" % z, "%.17g" % rng, "bound of 700"):
                    assert word in s, (word, s)
            else:
                break
        assert len(verdicts) == 13
        near = verdicts[:9]
        assert [b for b, _ in near] == sorted(b for b, _ in near) and near[0][1] and not near[-1][1]
        assert [ok for _, ok in near] == sorted((ok for _, ok in near), reverse=True)  # one edge, accepted below it
        assert [ok for _, ok in verdicts[9:]] == [True, True, 50.0 * z * rng <= 700.0, False]
        top = max(b for b, ok in near if ok)
        assert abs(top * z * rng / 700.0 - 1.0) < 2e-15
        w = ref.weights(e, top)  # math.exp raises on overflow: it does not here
        assert np.all(np.isfinite(w)) and np.all(w > 0.0)
        q = len(e)
        g = np.random.default_rng(20261)
        a, b = g.integers(0, q, (10000, z)), g.integers(0, q, (10000, z))
        hi, lo = int(np.argmax(e)), int(np.argmin(e))
        a = np.concatenate([a, np.full((1, z), lo), np.full((1, z), hi)])
        b = np.concatenate([b, np.full((1, z), hi), np.full((1, z), lo)])
        with np.errstate(all="raise"):
            p = np.cumprod(w[a, b], axis=1)  # the partial products in the device's order
        assert np.all(np.isfinite(p)) and np.all(p >= sys.float_info.min), (z, p.min(), p.max())
        assert abs(math.log(p[-2, -1]) - 700.0) < 1e-9 and abs(math.log(p[-1, -1]) + 700.0) < 1e-9
    assert (4, 2.0) in seen and (8, 8.0) in seen


def test_tables_and_products(printed):
    """t[j] = exp(-(|db| 2^(j - 30))) through the C library's exp, and the product over the set bits in ascending order,
    bit for bit"""
    tables = {}
    for db, J, v in re.findall(r"^table (\S+) (\d+)((?: \S+)+)$", printed, re.M):
        t = [float.fromhex(x) for x in v.split()]
        assert len(t) == int(J) and t == tref.pair_table(float.fromhex(db), int(J)), db
        tables[db] = t
    assert len(tables) == 6 and all(x == 1.0 for x in tables["0x0p+0"])
    rows = re.findall(r"^product (\S+) (\d+) (\S+)$", printed, re.M)
    assert len(rows) == 60
    for db, d, p in rows:
        assert float.fromhex(p) == tref.product(tables[db], int(d)), (db, d)
    # the product is exp(-|db| |d| 2^-30) to the header's bound of about 2 J ulp
    import math
    for db, d, p in rows:
        x = abs(float.fromhex(db)) * int(d) / 2.0 ** 30
        if x < 700.0:
            assert abs(float.fromhex(p) * math.exp(x) - 1.0) <= (2 * 50 + 4) * 2.0 ** -53 * max(1.0, x), (db, d)


def test_decisions(printed):
    rows = re.findall(r"^swaps (\S+) (-?\d+) (\S+) ([01])$", printed, re.M)
    assert len(rows) == 6 * 5 * 4
    seen = set()
    for db, d, u, swap in rows:
        db, d, u = float.fromhex(db), int(d), float.fromhex(u)
        if tref.rule(db, d) == "swap":
            want = True
        else:
            want = u < tref.product(tref.pair_table(db, 50), abs(d))
        assert bool(int(swap)) == want, (db, d, u)
        seen.add((tref.rule(db, d), want))
    assert seen == {("swap", True), ("decide", True), ("decide", False)}


def test_launch_cut(printed):
    """entry by entry against the restatement, which walks the sweeps one at a time"""
    rows = re.findall(r"^cut((?: -?\d+){7}) :(.*)$", printed, re.M)
    assert len(rows) == 10
    for args, v in rows:
        n, first, therm, rate, k, chunk, T0 = (int(x) for x in args.split())
        got = [tuple(int(x) for x in e.split(",")) for e in v.split()]
        want = [(a, b, int(c), d) for a, b, c, d in tref.launch_cut(n, first, therm, rate, k, chunk, T0)]
        assert got == want, (args, got, want)
        assert sum(e[0] for e in got) == n
        for m, f, defer, T in got:  # a launch holds at most one round, at its end
            last = f + m - 1
            assert m <= chunk and (k == 0 or all(i % k for i in range(f, last)))
            assert defer == int(k > 0 and last % k == 0 and last > therm and last % rate == 0)
    cuts = {a.strip(): v for a, v in rows}
    assert len(cuts["7 1 0 1 1 100 0"].split()) == 7 and len(cuts["5 1 0 1 9 100 0"].split()) == 1
    assert cuts["0 1 0 1 2 4 0"].strip() == "" and len(cuts["1100 1 0 1 0 976 0"].split()) == 2
