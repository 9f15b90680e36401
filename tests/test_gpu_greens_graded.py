"""calculate_greens_AVX! (stack.jl:337-393) on chain-graded inputs, one call per case, at every size-selected kernel form,
against extended precision (tests/greens_ref.py; expected values of n >= 100 in tests/golden/greens_graded.json / .npy, written by
tools/make_greens_golden.py and checked on the CPU by test_greens_golden.py).

Inputs: D = exp(linspace(+g, -g, n)) on both sides, g per size the largest of 40, 30, 20, 10 at which the float64 oracle
under the reference's pivot rule stays within 1e-11 of the extended-precision values (recorded in the golden file), so
that the matrix of the first UDT, Dl (Tl Tr') Dr, is graded by rows and by columns over dozens of decades.

Measure: err = max |probe - probe_ref| / max |probe_ref| for the probes G V and G' V, V in {-1, +1}^(n x 4) (the larger
of the two), and the same on diag(G); up to n = 64, where mpmath is cheap enough at test time, relerr over every entry.
Bound: err <= max(10 e_oracle, 64 eps), e_oracle the stored error of the oracle run under the pivot rule of the device
form (every call site pre-sorted for the one-launch UDT of n = 256 up to 32 units, the reference's rule elsewhere), in the
same measure; the factor 10 is the project's margin over a measured value (ANCHOR_BOUND, test_gpu_unequal_time_sizes.py).
Cap: err < TOL = 1e-10 whatever the oracle does."""
import os

import numpy as np
import pytest

import greens_ref as ref
import launch_rules as R
from test_gpu_dqmc import TOL

pytestmark = pytest.mark.gpu

FLOOR = 64 * np.finfo(np.float64).eps
MARGIN = 10
OTHER_UNITS_G = 3


@pytest.fixture(scope="module")
def golden():
    g = ref.load_golden()
    assert g["other_units_g"] == OTHER_UNITS_G
    return dict(sizes={int(n): s for n, s in g["sizes"].items()}, cases={(c["n"], c["unit"]): c for c in g["cases"]})


@pytest.fixture(scope="module")
def caps(gpu):
    return R.capacities(gpu)


def _inputs(golden, n, batch, checked):
    """the batch: the checked units at the size's g, the others at g = 3 (no expected values are kept for them)"""
    size = golden["sizes"][n]
    assert size["g"] >= 20, "n = %d: the inputs do not reach g = 20" % n
    gs = [size["g"] if u in checked else OTHER_UNITS_G for u in range(batch)]
    args = ref.graded_udt_inputs(n, gs, size["seed"], batch)
    for u in checked:  # not vacuous: both sides of 1 are populated
        assert ref.straddles_one(args[1][u]) and ref.straddles_one(args[4][u])
    return args


def _device(gpu, args, env=None):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return gpu.calculate_greens_AVX(*args)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _bound(e_oracle):
    return max(MARGIN * e_oracle, FLOOR)


def _check(label, G, case, rule):
    """one unit against its stored expected values, under the stored oracle error of `rule`; -> list of failures"""
    V = ref.probe_matrix(case["n"], case["seed"])
    fails = []
    for name, err in (("probe", ref.probe_err(G, V, case["probe"])), ("diag", ref.diag_err(G, case["diag"]))):
        e_orc = case["oracle_err"][rule][name]
        print("%s unit %d %s: device %.3e, %s-rule oracle %.3e, bound %.3e"
              % (label, case["unit"], name, err, rule, e_orc, _bound(e_orc)))
        if not (err <= _bound(e_orc) and err < TOL):
            fails.append((label, case["unit"], name, err, _bound(e_orc)))
    return fails


_small = {}


@pytest.mark.parametrize("unit", [0, 1, 2])
@pytest.mark.parametrize("n", [16, 64])
def test_lds_qr_every_entry(gpu, golden, n, unit):
    """case a: n <= 64 (LDS QR, small TRSM), three units in one call; every entry of G against mpmath at test time"""
    if n not in _small:
        args = _inputs(golden, n, 3, (0, 1, 2))
        _small[n] = (args, _device(gpu, args))
    args, G = _small[n]
    case = golden["cases"][(n, unit)]
    Gmp = ref.greens_mp(ref.unit(args, unit))
    err = ref.full_err(G[unit], Gmp)
    e_orc = case["oracle_err"]["reference"]["full"]
    print("n = %d unit %d: device %.3e, oracle %.3e, bound %.3e (g = %d)" % (n, unit, err, e_orc, _bound(e_orc), case["g"]))
    assert err <= _bound(e_orc) and err < TOL
    assert not _check("n = %d" % n, G[unit], case, "reference")


CASES = {
    "b_n100": (100, 2, (0, 1), None),
    "c_n256_one_launch": (256, 3, (0, 1, 2), "one_launch"),
    "d_n256_33_units_cooperative": (256, 33, (0, 8, 32), "coop"),
    "e_n256_65_units_single_workgroup": (256, 65, (0, 64), "tile"),
    "f_n257": (257, 2, (0, 1), None),
    "f_n292": (292, 2, (0, 1), None),
    "f_n324": (324, 2, (0, 1), None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_graded_greens_at_every_form(gpu, golden, caps, name):
    """cases b-f: off every tile grid; n = 256 at 3 units (one-launch pre-pivoted UDT, MFMA TRSM), at 33 (cooperative QR +
    tail, a partial later group of eight) and at 65 (single-workgroup QR); panel QR and panelled TRSM on both sides of the
    slab-height switch at 291 / 292.  The one-launch case is run a second time under DQMC_QRB_SITES=0, the reference's
    pivot rule on the device, and held to the reference-rule oracle's error."""
    n, batch, checked, form = CASES[name]
    one_launch = R.udt_one_launch(n, batch, caps)
    if form is not None:
        reached = "one_launch" if one_launch else ("coop" if R.qr_coop(n, batch, caps) else "tile")
        assert reached == form, "%d units at n = %d take the %s form on this device" % (batch, n, reached)
    args = _inputs(golden, n, batch, checked)
    G = _device(gpu, args)
    assert np.all(np.isfinite(G))
    fails = []
    for u in checked:
        fails += _check(name, G[u], golden["cases"][(n, u)], "presorted" if one_launch else "reference")
    if one_launch:
        G0 = _device(gpu, args, {"DQMC_QRB_SITES": "0"})
        for u in checked:
            fails += _check(name + " DQMC_QRB_SITES=0", G0[u], golden["cases"][(n, u)], "reference")
            print("%s unit %d: pre-pivoted against reference rule on the device %.3e"
                  % (name, u, np.abs(G[u] - G0[u]).max() / np.abs(G0[u]).max()))
    assert not fails, fails
