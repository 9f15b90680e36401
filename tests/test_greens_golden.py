"""tests/golden/greens_graded.json and .npy (tools/make_greens_golden.py) checked on the CPU: the n = 36 entry recomputed with
mpmath, the conditions its choice of g has to meet, and every stored oracle error against a fresh run of the float64
oracle.  No GPU.

The oracle is plain C without a BLAS, but its compiler may contract and vectorise differently on another host, so a
recomputed oracle is one more float64 evaluation: like the device in test_gpu_greens_graded.py it is held to ten times
the stored error (or 64 eps), and both are printed."""
import mpmath as mp
import numpy as np
import pytest

import greens_ref as ref

FLOOR = 64 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _inputs(case):
    return ref.graded_unit(case["n"], case["g"], case["seed"] + case["unit"])


def test_the_36_site_entry_is_what_mpmath_gives(golden):
    (case,) = [c for c in golden["cases"] if c["n"] == 36]
    G = ref.greens_mp(_inputs(case), golden["digits"])
    with mp.workdps(golden["digits"]):
        pr = [ref.to_float(p) for p in ref.probe(G, ref.probe_matrix(36, case["seed"]))]
        dg = ref.to_float(np.diag(G))
    # the stored numbers are these, rounded to float64 (eps / 2); the inputs come out of LAPACK's QR, whose last bits may
    # differ between hosts, and an input moved by an ulp moves G like one float64 evaluation does (the oracle is at 3e-15
    # here): 64 eps, the floor of the device's bound
    worst = max(ref.rel(pr[0], case["probe"][0]), ref.rel(pr[1], case["probe"][1]), ref.rel(dg, case["diag"]))
    print("n = 36: recomputed against stored %.3e" % worst)
    assert worst <= FLOOR


def test_the_choice_of_g(golden):
    """every size reaches g >= 20, the reference-rule oracle is within the bound at the chosen g in both measures, every
    larger candidate was rejected on a measured error, and D straddles 1 with a quarter of its entries on each side"""
    assert golden["bound"] == 1e-11 and golden["g_candidates"] == [40, 30, 20, 10]
    for n, size in golden["sizes"].items():
        assert size["g"] >= 20, n
        assert sorted(int(g) for g in size["rejected"]) == sorted(g for g in golden["g_candidates"] if g > size["g"])
        assert all(e > golden["bound"] for e in size["rejected"].values())
        mine = [c for c in golden["cases"] if c["n"] == int(n)]
        assert mine and all(c["g"] == size["g"] and c["seed"] == size["seed"] for c in mine)
        worst = max(c["oracle_err"]["reference"][k] for c in mine for k in ("probe", "diag"))
        assert worst == size["oracle_reference_rule"] <= golden["bound"]
        a = _inputs(mine[0])
        assert ref.straddles_one(a[1]) and ref.straddles_one(a[4])
        print("n = %s: g = %d, reference-rule oracle %.3e, pre-sorted %.3e" % (
            n, size["g"], worst, max(c["oracle_err"]["presorted"][k] for c in mine for k in ("probe", "diag"))))


def test_stored_oracle_errors_against_a_fresh_oracle(O, golden):
    fails = []
    for case in golden["cases"]:
        a = _inputs(case)
        V = ref.probe_matrix(case["n"], case["seed"])
        for rule, mask in (("reference", 0), ("presorted", golden["presort_mask"])):
            G = ref.oracle_greens(O, a, mask)
            for name, err in (("probe", ref.probe_err(G, V, case["probe"])), ("diag", ref.diag_err(G, case["diag"]))):
                stored = case["oracle_err"][rule][name]
                print("n = %d unit %d %s %s: stored %.3e, this host %.3e" % (case["n"], case["unit"], rule, name, stored, err))
                if not err <= max(10 * stored, FLOOR):
                    fails.append((case["n"], case["unit"], rule, name, stored, err))
    assert not fails, fails
