"""dqmc_logdet through the engine at every size-selected kernel form, with negative determinants, against
tests/golden/logdet_sizes.json (tools/make_logdet_golden.py; checked on the CPU by test_logdet_golden.py).

Cases (dtau = 0.1, four walkers with the fields global_move_ref.field(seed, n, M)):
  square6              SquareLattice(6), U = 8, beta = 2        n = 36   LDS LU off the lane grid, two blocks
  triangular8          TriangularLattice(8), U = 8, beta = 4    n = 64   the last LDS size
  cubic4               cubic L = 4, U = 8, beta = 2             n = 64   kron3's lattice at the small size
  triangular10         TriangularLattice(10), U = 8, beta = 4   n = 100  in-memory LU off every stride
  triangular16         TriangularLattice(16), U = 8, beta = 2   n = 256  one-launch UDT, three-factor hopping, in-memory LU
  square16_attractive  16 x 16, U = 4, mu = 0.5, beta = 1       n = 256  the +1 control

Negative signs, as the float64 oracle's scan found them (the kept seeds confirmed as below): triangular8 25 of the
seeds 2 .. 61 with a negative block (17 with a negative product), triangular10 28 of 0 .. 59 (24), triangular16 4 of
0 .. 199 (4).  cubic4: of the seeds 0 .. 199 one has both blocks negative and none a negative product - the lattice is
bipartite and half filled, det_up det_dn > 0 - so it stays a positive-sign case, like square6.

Expected values: 60-digit mpmath for n <= 100; at n = 256 the float64 oracle, accepted only where a second float64 route
with another stabilisation agrees in both signs and within 1e-9.

Tolerances on logabsdet, by the rule of test_gpu_global_move.py: ten times the largest |oracle_logdet - golden| on
exactly these inputs, measured on the CPU (test_logdet_golden.py asserts the bases):
  square6 5.07e-13 -> 5.1e-12      triangular8 4.69e-10 -> 4.7e-9      cubic4 2.12e-12 -> 2.2e-11
  triangular10 3.49e-9 -> 3.5e-8      (the measured figure rounded up to two digits, times ten)
  n = 256: the basis is the larger of the two float64 routes' difference and the 1.45e-13 of test_gpu_global_move.py:
  triangular16 2.12e-11 -> 2.2e-10      square16_attractive 1.14e-13 < 1.45e-13 -> 1.45e-12
Signs must be equal."""
import mpmath as mp
import numpy as np
import pytest

import global_move_ref as ref

pytestmark = pytest.mark.gpu

BASIS = {"square6": 5.1e-13, "triangular8": 4.7e-10, "cubic4": 2.2e-12, "triangular10": 3.5e-9,
         "triangular16": 2.2e-11, "square16_attractive": 1.45e-13}
TOL = {k: 10 * v for k, v in BASIS.items()}
NEGATIVE = ("triangular8", "triangular10", "triangular16")  # the cases that must present negative determinants


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def worst_difference(lad, expected):
    """max |lad - expected| with the expected decimal strings taken at 40 digits"""
    with mp.workdps(40):
        return max(float(abs(mp.mpf(float(lad[w, b])) - mp.mpf(expected[w][b])))
                   for w in range(lad.shape[0]) for b in range(lad.shape[1]))


@pytest.mark.parametrize("name", sorted(BASIS))
def test_logdet_against_the_golden_values(gpu, golden, name):
    case = golden["logdet"][name]
    model = ref.golden_model(gpu, case)
    mc = gpu.DQMC(model, n_walkers=4, beta=case["beta"], delta_tau=golden["delta_tau"], safe_mult=golden["safe_mult"])
    try:
        n, M = case["n"], case["slices"]
        assert (mc.N, mc.p.slices) == (n, M)
        assert (mc.udt_one_launch_sites() != 0) == (n == 256)
        for w, s in enumerate(case["seeds"]):
            mc.set_conf(w, ref.field(s, n, M))
        lad, sg = mc.logdet()
        want = np.array(case["sign"])
        negative = int((want < 0).sum())
        print("logdet %s: %d negative blocks of %d, %d walkers with a negative product"
              % (name, negative, want.size, int((want.prod(axis=1) < 0).sum())))
        if name in NEGATIVE:
            assert negative >= 2 and (want.prod(axis=1) < 0).any()
        assert np.array_equal(sg, want), (name, sg.tolist(), want.tolist())
        worst = worst_difference(lad, case["logabsdet"])
        print("logdet %s: max |device - golden| = %.3e, tolerance %.3e" % (name, worst, TOL[name]))
        assert worst <= TOL[name]
        lad2, sg2 = mc.logdet()
        assert lad2.tobytes() == lad.tobytes() and np.array_equal(sg, sg2)
    finally:
        mc.close()
