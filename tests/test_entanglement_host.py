"""Host side of the Renyi-2 entanglement measurement, no GPU: the purity / S2 / jackknife arithmetic of
dqmc.entanglement_from_pair_sums against the brute-force delete-one-walker jackknife, lattices.strip_subsystem on the three
lattices that have one, and the float64 reference of tests/entanglement_ref.py against extended precision, which gives the
reference's own error e_ref(N_A) that the GPU tolerances (tests/test_gpu_entanglement.py) are built on."""
import mpmath
import numpy as np
import pytest

import entanglement_ref as ER


@pytest.mark.parametrize("W", [3, 4, 7])
def test_pair_sums_arithmetic_equals_the_brute_force_jackknife(mc_amd, W):
    """seeded random symmetric pair sums (only the strictly upper triangle is read), two subsystems, count 5"""
    from montecarlo_jl_amd.dqmc import entanglement_from_pair_sums
    rng = np.random.default_rng(100 + W)
    count = 5
    ps = rng.uniform(0.05, 0.9, (2, W, W)) * count
    ps = 0.5 * (ps + ps.transpose(0, 2, 1))
    res = entanglement_from_pair_sums(ps, count)
    upper = entanglement_from_pair_sums(np.triu(ps, 1), count)
    for s in range(2):
        purity, s2, err = ER.jackknife_brute(ps[s], count)
        assert abs(res["purity"][s] - purity) <= 4e-16 * W * W * purity
        assert abs(res["S2"][s] - s2) <= 1e-14
        assert abs(res["S2_std_error"][s] - err) <= 1e-13 * max(err, 1.0)
        assert err > 0
    for k in res:
        assert np.array_equal(res[k], upper[k]), k
    one = entanglement_from_pair_sums(ps[1], count)  # a single [W, W] matrix gives scalars
    assert one["purity"] == res["purity"][1] and one["S2_std_error"] == res["S2_std_error"][1]


def test_two_walkers_have_no_error_bar_and_bad_input_is_refused(mc_amd):
    from montecarlo_jl_amd.dqmc import entanglement_from_pair_sums
    ps = np.zeros((1, 2, 2))
    ps[0, 0, 1] = 0.5
    res = entanglement_from_pair_sums(ps, 2)
    assert "S2_std_error" not in res and res["purity"][0] == 0.25 and res["S2"][0] == -np.log(0.25)
    with pytest.raises(ValueError):
        entanglement_from_pair_sums(ps, 0)
    with pytest.raises(ValueError):
        entanglement_from_pair_sums(np.zeros((1, 1, 1)), 1)
    with pytest.raises(ValueError):
        entanglement_from_pair_sums(np.zeros((2, 3, 4)), 1)


def test_strip_subsystem_on_the_three_lattices(mc_amd):
    strip = mc_amd.lattices.strip_subsystem
    sq = mc_amd.SquareLattice(4)       # site x + 4 y
    assert strip(sq, 2).tolist() == [0, 1, 4, 5, 8, 9, 12, 13]
    assert strip(sq, 1, axis=1).tolist() == [0, 1, 2, 3]
    assert strip(sq, 4).tolist() == list(range(16))
    cu = mc_amd.CubicLattice(3, 3)     # site x + 3 y + 9 z
    assert strip(cu, 1).tolist() == [3 * k for k in range(9)]
    assert strip(cu, 2, axis=2).tolist() == list(range(18))
    assert strip(cu, 1, axis=1).tolist() == [0, 1, 2, 9, 10, 11, 18, 19, 20]
    tr = mc_amd.TriangularLattice(4, Lx=4, Ly=3)  # site i + 4 j
    assert strip(tr, 3).tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    assert strip(tr, 2, axis=1).tolist() == list(range(8))
    for l, axis in ((sq, 0), (cu, 2), (tr, 1)):  # the coordinate read back from the lattice's own array
        for width in (1, 2):
            sites = strip(l, width, axis)
            coords = np.argwhere(np.isin(l.lattice, sites + 1))[:, axis]
            assert len(sites) == width * l.sites // l.lattice.shape[axis] and coords.max() == width - 1
    with pytest.raises(ValueError):
        strip(sq, 0)
    with pytest.raises(ValueError):
        strip(sq, 5)
    with pytest.raises(ValueError):
        strip(sq, 1, axis=2)
    with pytest.raises(TypeError):
        strip(mc_amd.Chain(8), 2)


@pytest.mark.parametrize("na", [1, 17, 64])
def test_float64_reference_against_extended_precision(na):
    """seeded random G (symmetric, spectrum in (0, 1)), three walkers, one and two blocks.  e_ref(N_A), the float64
    reference's own relative error, stays below 2^-52 N_A (N_A + 8) (N_A pivots, each behind a sum of N_A rounded products
    and the handful of roundings of I - G - G' + 2 G G' itself, which is all there is at N_A = 1; twice for the square); the
    two extended-precision routes (mpmath.det, the 240-bit fixed-point elimination) agree to 40 digits."""
    rng = np.random.default_rng(7 + na)
    sites = list(rng.permutation(na))
    for nb in (1, 2):
        greens = [[ER.random_greens(rng, na) for _ in range(nb)] for _ in range(3)]
        x = ER.pair_sample(greens, sites)
        with mpmath.workdps(ER.MP_DIGITS):
            direct = ER.pair_value_mp(greens[0], greens[1], sites, direct=True)
            fixed = ER.pair_value_mp(greens[0], greens[1], sites, direct=False)
            assert abs(fixed - direct) <= abs(direct) * mpmath.mpf(10) ** -40
            e01 = float(abs(mpmath.mpf(float(x[0, 1])) - direct) / abs(direct))
        x2, e_ref = ER.reference_error(greens, sites)
        assert np.array_equal(x, x2) and e_ref >= e01 * (1 - 1e-12)
        assert e_ref <= 2.0 ** -52 * na * (na + 8), (na, nb, e_ref)
        assert np.all(np.tril(x) == 0.0) and np.all(x[np.triu_indices(3, 1)] > 0.0)
