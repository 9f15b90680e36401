"""tests/golden/logdet_sizes.json (tools/make_logdet_golden.py) checked on the CPU: the n = 36 entry recomputed with
mpmath, and the float64 oracle against every entry, which is where the tolerance bases of test_gpu_logdet_sizes.py and of
the moves away from 4 x 4 in test_gpu_global_move.py are measured.  No GPU.

The bases are the distances measured where the file was written (the oracle's own values are stored in it, and the
stored distance is asserted to be within the basis).  The oracle's matrix products go through the host's BLAS, whose
summation order differs between CPUs, so a recomputed oracle is one more float64 evaluation with reordered sums: like the
device it is held to ten times the basis, and its distance is printed next to the basis."""
import mpmath as mp
import numpy as np
import pytest

import global_move_ref as ref
from test_gpu_logdet_sizes import BASIS, NEGATIVE, TOL

MOVE_BASIS = {"triangular8": 4.7e-10, "slices300": 1.5e-14}  # over the current and the proposed fields


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def test_the_36_site_entry_is_what_mpmath_gives(mc_amd, golden):
    case = golden["logdet"]["square6"]
    model = ref.golden_model(mc_amd, case)
    for w, s in enumerate(case["seeds"][:2]):
        lad, sg = ref.slogdet_mp(model, golden["delta_tau"], ref.field(s, case["n"], case["slices"]))
        assert sg == case["sign"][w]
        with mp.workdps(ref.DPS):
            assert all(abs(a - mp.mpf(b)) < mp.mpf(10) ** -25 for a, b in zip(lad, case["logabsdet"][w]))


def _stored_distance(entry):
    """the largest |oracle - golden| as the file records it"""
    with mp.workdps(40):
        return max(float(abs(mp.mpf(float(a)) - mp.mpf(b))) for x, y in zip(entry["oracle_logabsdet"], entry["logabsdet"])
                   for a, b in zip(x, y))


def _oracle_distance(O, pkg, golden, case, entry, flips):
    model = ref.golden_model(pkg, case)
    worst = 0.0
    for w, s in enumerate(case["seeds"]):
        c = ref.field(s, case["n"], case["slices"])
        if flips is not None:
            c = ref.apply_flip(c, ref.FLIP_ALL) if flips == "all" else ref.apply_flip(c, ref.FLIP_SITE, flips[w])
        lad, sg, _ = ref.oracle_logdet(O, model, case.get("delta_tau", golden["delta_tau"]), golden["safe_mult"], c)
        assert sg == entry["sign"][w], (s, sg, entry["sign"][w])
        with mp.workdps(40):
            worst = max(worst, max(float(abs(mp.mpf(a) - mp.mpf(b))) for a, b in zip(lad, entry["logabsdet"][w])))
    return worst


@pytest.mark.parametrize("name", sorted(BASIS))
def test_oracle_logdet_against_the_golden_values(mc_amd, O, golden, name):
    """signs equal; the stored |oracle - golden| is within the basis test_gpu_logdet_sizes.py multiplies by ten, the
    recomputed one within ten times the basis.  At n = 256 the golden value is the oracle's own, and the basis is the
    stored difference of the two float64 routes, or 1.45e-13 where that is larger."""
    case = golden["logdet"][name]
    worst = _oracle_distance(O, mc_amd, golden, case, case, None)
    stored = _stored_distance(case)
    if case["n"] == 256:
        stored = max(abs(float(a) - float(b)) for x, y in zip(case["logabsdet"], case["second_logabsdet"])
                     for a, b in zip(x, y))
        assert stored <= 1e-9
        stored = max(stored, 1.45e-13)
    print("logdet %s: basis stored %.3e, used %.3e; this host's oracle %.3e, tolerance %.3e"
          % (name, stored, BASIS[name], worst, TOL[name]))
    assert stored <= BASIS[name]
    assert worst <= TOL[name]
    sg = np.array(case["sign"])
    if name in NEGATIVE:
        assert (sg < 0).sum() >= 2 and (sg.prod(axis=1) < 0).any()


@pytest.mark.parametrize("name,kind", [("triangular8", "all"), ("triangular8", "site"), ("slices300", "site")])
def test_oracle_logdet_against_the_golden_proposals(mc_amd, O, golden, name, kind):
    mv = golden["moves"][name]
    case = golden["logdet"][mv["case"]] if "case" in mv else mv
    case = dict(case, seeds=mv["seeds"])
    worst = _oracle_distance(O, mc_amd, golden, case, mv[kind], "all" if kind == "all" else mv["sites"])
    stored = _stored_distance(mv[kind])
    if "cur" in mv:
        worst = max(worst, _oracle_distance(O, mc_amd, golden, case, mv["cur"], None))
        stored = max(stored, _stored_distance(mv["cur"]))
    print("moves %s %s: basis stored %.3e, used %.3e; this host's oracle %.3e" % (name, kind, stored, MOVE_BASIS[name], worst))
    assert stored <= MOVE_BASIS[name]
    assert worst <= 10 * MOVE_BASIS[name]
