"""mc.pool_walkers, no GPU: the one place where MC.binned, MC.binned_fss, QStateMC.binned, binned_scaling and
binned_stiffness turn per-walker binner results into {mean, std_error, tau, std_error_walkers}.  Hand-made per-walker
tuples (obs, count, level) with entry = (mean, variance of the mean at the level, the same at level 0 or None), against
the formulas of MC.binned's docstring with the numbers written out here:

    mean = sum_w mean_w / W,  std_error = sqrt(max(sum_w var_w, 0)) / W,  tau = (sum_w var_w / sum_w var0_w - 1) / 2,
    std_error_walkers = sqrt(sum_w (mean_w - mean)^2 / (W (W - 1)))

The variances are dyadic, so sums, quotients and the square roots of 1, 4 and 9 are exact and compared with ==; the other
square roots are one correctly rounded operation on each side and compared to 1e-15."""
import importlib
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pool(mc_amd):
    return importlib.import_module(mc_amd.__name__ + ".mc").pool_walkers


def per_walker(tuples):
    return lambda w: tuples[w]


BETAS = np.array([0.5, 0.5, 0.5, 0.25])
THREE = [({"x": (1.0, 0.25, 0.125), "S": [(2.0, 1.0, 0.5), (0.0, 0.0, 1.0)]}, 64, 3),
         ({"x": (2.0, 0.5, 0.0625), "S": [(4.0, 1.0, 0.25), (0.0, 0.0, 1.0)]}, 64, 3),
         ({"x": (6.0, 0.25, 0.0625), "S": [(6.0, 2.0, 0.25), (3.0, 9.0, 1.0)]}, 64, 3)]


def test_one_walker_unpooled(pool):
    out = pool("binned", BETAS, 1, None, per_walker(THREE))
    assert out == {"count": 64, "level": 3, "x": {"mean": 2.0, "std_error": math.sqrt(0.5), "tau": 3.5},
                   "S": [{"mean": 4.0, "std_error": 1.0, "tau": 1.5}, {"mean": 0.0, "std_error": 0.0, "tau": -0.5}]}
    assert "n_walkers" not in out and "std_error_walkers" not in out["x"] and "std_error_walkers" not in out["S"][0]


def test_three_walkers_pooled_scalar_and_list_entries(pool):
    out = pool("binned", BETAS, 0, [0, 1, 2], per_walker(THREE))
    assert out["count"] == 64 and out["level"] == 3 and out["n_walkers"] == 3
    assert set(out) == {"count", "level", "n_walkers", "x", "S"} and len(out["S"]) == 2
    x = out["x"]  # means 1, 2, 6; variances sum to 1; level-0 variances sum to 1/4
    assert x["mean"] == 3.0 and x["std_error"] == 1.0 / 3.0 and x["tau"] == 1.5
    assert x["std_error_walkers"] == pytest.approx(math.sqrt(14.0 / 6.0), rel=1e-15)
    s0, s1 = out["S"]  # means 2, 4, 6 and 0, 0, 3; variances sum to 4 and 9; level-0 variances to 1 and 3
    assert s0["mean"] == 4.0 and s0["std_error"] == 2.0 / 3.0 and s0["tau"] == 1.5
    assert s0["std_error_walkers"] == pytest.approx(math.sqrt(8.0 / 6.0), rel=1e-15)
    assert s1 == {"mean": 1.0, "std_error": 1.0, "tau": 1.0, "std_error_walkers": 1.0}
    for o in (x, s0, s1):
        assert list(o) == ["mean", "std_error", "tau", "std_error_walkers"]


def test_derived_entry_under_both_tau_conventions(pool):
    per = [({"E": (1.0, 1.0, 0.5), "C": (10.0, 4.0, None), "xi": [(3.0, 1.0, None)]}, 8, 0),
           ({"E": (3.0, 3.0, 0.5), "C": (20.0, 12.0, None), "xi": [(5.0, 3.0, None)]}, 8, 0)]
    absent = pool("binned_fss", BETAS, 0, [0, 1], per_walker(per))
    assert absent["C"] == {"mean": 15.0, "std_error": 2.0, "std_error_walkers": 5.0}
    assert absent["xi"] == [{"mean": 4.0, "std_error": 1.0, "std_error_walkers": 1.0}]
    assert absent["E"]["tau"] == 1.5
    nan = pool("binned", BETAS, 0, [0, 1], per_walker(per), derived_tau=float("nan"))
    assert list(nan["C"]) == ["mean", "std_error", "tau", "std_error_walkers"]
    assert math.isnan(nan["C"]["tau"]) and math.isnan(nan["xi"][0]["tau"]) and nan["E"]["tau"] == 1.5
    assert {k: v for k, v in nan["C"].items() if k != "tau"} == absent["C"]
    one = pool("binned", BETAS, 1, None, per_walker(per), derived_tau=float("nan"))
    assert math.isnan(one["C"]["tau"]) and one["C"]["mean"] == 20.0 and one["C"]["std_error"] == math.sqrt(12.0)


def test_negative_summed_variance_clamps_and_nan_stays(pool):
    per = [({"neg": (1.0, -1.0, 1.0), "nan": (1.0, float("nan"), 1.0), "mean_nan": (float("nan"), 1.0, 1.0)}, 4, 1),
           ({"neg": (1.0, 0.25, 1.0), "nan": (1.0, 1.0, 1.0), "mean_nan": (1.0, 3.0, 1.0)}, 4, 1)]
    out = pool("binned", BETAS, 0, [0, 1], per_walker(per))
    assert out["neg"]["std_error"] == 0.0 and out["neg"]["tau"] == 0.5 * (-0.75 / 2.0 - 1.0)
    assert math.isnan(out["nan"]["std_error"]) and math.isnan(out["nan"]["tau"]) and out["nan"]["mean"] == 1.0
    assert math.isnan(out["mean_nan"]["mean"]) and math.isnan(out["mean_nan"]["std_error_walkers"])
    assert out["mean_nan"]["std_error"] == 1.0


def test_one_walker_pooled_has_no_scatter(pool):
    out = pool("binned_stiffness", BETAS, 0, [2], per_walker(THREE))
    assert out["n_walkers"] == 1 and out["x"]["mean"] == 6.0 and out["x"]["std_error"] == 0.5
    assert math.isnan(out["x"]["std_error_walkers"]) and all(math.isnan(o["std_error_walkers"]) for o in out["S"])


@pytest.mark.parametrize("method", ["binned", "binned_fss", "binned_scaling", "binned_stiffness"])
def test_unequal_betas_and_no_walker_are_refused_under_the_callers_name(pool, method):
    def never(w):
        raise AssertionError("the per-walker results are asked for only after the checks")

    with pytest.raises(ValueError, match="^%s: the pooled walkers must share one beta$" % method):
        pool(method, BETAS, 0, [0, 3], never)
    with pytest.raises(ValueError, match="^%s: no walker given$" % method):
        pool(method, BETAS, 0, [], never)
