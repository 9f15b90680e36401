"""The host tables of the classical MC flavor (csrc/mc_tables.h: the lattice tables of a create, the colour-sorted tables
of a checkerboard sweep, the arithmetic of the logarithmic binner) without a GPU: tests/mc_tables_check.cpp under the
host sanitizers, every line it prints restated here in numpy from the inputs it prints beside them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")
CASES = ["square4", "square3", "triangular4", "chain5", "chain300", "chain700"]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """g++ -fsanitize=address,undefined, run once as a child process on the CPU (the sanitizer runtimes are linked into
    the program); -ffp-contract=off: the finish is the header's formula operation by operation"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host code"
    exe = str(tmp_path_factory.mktemp("mc_tables") / "mc_tables_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "mc_tables_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and "FAILED" not in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    return out.stdout


def _case(printed, name):
    rows = re.findall(r"^case %s (\S+)((?: -?\d+)*)$" % re.escape(name), printed, re.M)
    return {k: np.array(v.split(), dtype=np.int64) for k, v in rows}


@pytest.mark.parametrize("name", CASES)
def test_lattice_and_colour_tables(printed, name):
    """nbr = neighs - 1, pairs = the column-major bonds row by row, rows padded to 8 with a spare row; then, for both
    lengths of `off` (n_colours + 1 as the Ising engine uploads it, 17 as the q-state engine does): site = the stable
    argsort of the colouring, rows = nbr[site] padded to 8, off = the cumulative bincount, largest = the largest class,
    threads = whole waves for it, 64 at least and 256 at most"""
    c = _case(printed, name)
    N, z, nb = (int(v) for v in c["shape"])
    neighs, bonds, colour = c["neighs"].reshape(N, z), c["bonds"].reshape(2, nb), c["colour"]
    nbr = neighs - 1
    assert np.array_equal(c["nbr"].reshape(N, z), nbr)
    assert np.array_equal(c["pairs"].reshape(nb, 2), bonds.T - 1)
    padded = np.zeros((N + 1, 8), dtype=np.int64)
    padded[:N, :z] = nbr
    assert np.array_equal(c["padded"].reshape(N + 1, 8), padded)
    # the colouring the program made is one (an input, checked so that the tables below mean something)
    nc = int(colour.max()) + 1
    assert colour.min() == 0 and np.all(colour[nbr] != colour[:, None])
    assert nc == 2 if name in ("square4", "chain300", "chain700") else nc > 2  # the odd and triangular ones need more
    site = np.argsort(colour, kind="stable")
    rows = np.zeros((N, 8), dtype=np.int64)
    rows[:, :z] = nbr[site]
    counts = np.bincount(colour, minlength=nc)
    largest = int(counts.max())
    threads = min(256, max(64, -(-largest // 64) * 64))
    for tag, n_off in (("off0.", nc + 1), ("off17.", 17)):
        off = np.concatenate(([0], np.cumsum(np.bincount(colour, minlength=n_off - 1))))
        assert np.array_equal(c[tag + "site"], site)
        assert np.array_equal(c[tag + "rows"].reshape(N, 8), rows)
        assert np.array_equal(c[tag + "off"], off) and len(off) == n_off and off[-1] == N
        assert list(c[tag + "largest_threads"]) == [largest, threads]
    assert threads == {"chain300": 192, "chain700": 256}.get(name, 64)  # 150 -> 3 waves, 350 -> the cap


def test_refusals(printed):
    """what must not become tables, each with the caller's function name in front"""
    got = dict(re.findall(r"^refused (\S+): (.*)$", printed, re.M))
    want = {"colour_high": "the colour of site 5 is out of range 0..n_colours-1",
            "colour_negative": "the colour of site 0 is out of range 0..n_colours-1",
            "n_colours_0": "n_colours must be in 1..16", "n_colours_17": "n_colours must be in 1..16",
            "shared": "the neighbours 0 and 1 (0-based sites) share colour 0", "null": "null colouring",
            "self": "site 0 lists itself as a neighbour (0-based): no colouring",
            "neighbour_0": "neighbour index out of range 1..n_sites",
            "neighbour_N1": "neighbour index out of range 1..n_sites", "bond_N1": "bond index out of range 1..n_sites",
            "no_bonds_table": "neighbour or bonds table missing",
            "series_negative": "n_bonds and series_capacity must be >= 0"}
    assert got == {k: "dqmc_fn: " + v for k, v in want.items()}


def test_binner_counts(printed):
    """levels = ceil(log2(capacity + 1)); the level a push stops at = the trailing 1-bits of the pushes before it (at or
    past the levels: no room); the reliable level = the last one with count = T >> level >= 32, else 0"""
    caps = [1, 2, 3, 100000, 2 ** 40]
    levels = {int(c): int(L) for c, L in re.findall(r"^levels (\d+) (\d+)$", printed, re.M)}
    assert levels == {c: next(L for L in range(1, 64) if 2 ** L >= c + 1) for c in caps}
    assert levels == {1: 1, 2: 2, 3: 2, 100000: 17, 2 ** 40: 41}
    for key, want in (("lmax", lambda T, L: next(l for l in range(64) if not (T >> l) & 1)),
                      ("reliable", lambda T, L: max([l for l in range(L) if (T >> l) >= 32], default=0))):
        rows = {int(c): [int(x) for x in v.split()] for c, v in re.findall(r"^%s (\d+)((?: \d+)+)$" % key, printed, re.M)}
        assert sorted(rows) == caps
        for c in caps:
            assert rows[c] == [want(T, levels[c]) for T in range(71)], (key, c)
    # capacity 3 has two levels: the fourth push (T = 3 before it) finds no room
    lmax3 = [int(x) for x in re.search(r"^lmax 3((?: \d+)+)$", printed, re.M).group(1).split()]
    assert [l >= 2 for l in lmax3[:4]] == [False, False, False, True]
    rows = re.findall(r"^measurements_in (\d+) (\d+) (\d+)((?: \d+)+)$", printed, re.M)
    assert len(rows) == 36
    for therm, rate, first, v in rows:
        therm, rate, first = int(therm), int(rate), int(first)
        want = [sum(1 for i in range(first, last + 1) if i > therm and i % rate == 0) for last in range(first - 1, 13)]
        assert [int(x) for x in v.split()] == want


def _covN(a, b, q, n):
    """the header's varN / covN, operation by operation"""
    if n < 2.0:
        return float("nan")
    return (q / (n - 1.0) - a * b / (n * (n - 1.0))) / n


@pytest.mark.parametrize("name", ["ising", "fss3", "fss0", "ising_short", "fss_single"])
def test_binner_finish(printed, name):
    """both element layouts, bit for bit (IEEE doubles on both sides, no contraction): Ising's pairs (2p, 2p + 1), the
    FSS section's (0, 1 + p); NaN below two samples"""
    rows = dict(re.findall(r"^finish %s (\S+) (.*)$" % name, printed, re.M))
    ne, npairs, from_first, T, level = (int(x) for x in rows["shape"].split())
    v = {k: [float.fromhex(x) for x in rows[k].split()] for k in rows if k != "shape"}
    n0, nl = float(T), float(T >> level)
    want = {"mean": [v["xs0"][k] / n0 for k in range(ne)],
            "varN": [_covN(v["xs"][k], v["xs"][k], v["x2"][k], nl) for k in range(ne)],
            "varN0": [_covN(v["xs0"][k], v["xs0"][k], v["x20"][k], n0) for k in range(ne)]}
    want["tau"] = [0.5 * (np.float64(want["varN"][k]) / np.float64(want["varN0"][k]) - 1.0) for k in range(ne)]
    want["covN"] = [_covN(v["xs"][0], v["xs"][1 + p], v["xy"][p], nl) if from_first
                    else _covN(v["xs"][2 * p], v["xs"][2 * p + 1], v["xy"][p], nl) for p in range(npairs)]
    for key, w in want.items():
        assert len(v[key]) == len(w)
        assert np.array_equal(np.array(v[key]), np.array(w, dtype=np.float64), equal_nan=True), key
    if nl < 2:
        assert all(np.isnan(v["varN"])) and all(np.isnan(v["covN"])) and all(np.isnan(v["tau"]))
    if n0 < 2:
        assert all(np.isnan(v["varN0"])) and not any(np.isnan(v["mean"]))
    if nl >= 2:
        assert not any(np.isnan(v["varN"])) and not any(np.isnan(v["covN"]))


def test_mc_tables_header_has_no_hip_in_it():
    txt = open(os.path.join(CSRC, "mc_tables.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()
