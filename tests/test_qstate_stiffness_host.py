"""The q-state engine's stiffness measurement (the helicity modulus) on the host, no GPU: lattices.bond_classes on every
lattice, the twist tables, the restatement of tests/qstate_stiffness_ref.py against the second derivative of the free
energy by enumeration and on configurations with known sums, the argument check of dqmc_qs_set_stiffness
(csrc/mc_tables.h, qs_stiffness_check) under the host sanitizers, and the keywords that are refused before a device is
touched."""
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_stiffness_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")
S3 = 0.8660254037844386

# name: (lattice, classes, the second moment sum_k (e_mu . d_k)^2 of a site's z slots per default direction)
LATTICES = {
    "chain5": (lambda g: g.Chain(5), 1, [2.0]),
    "square3": (lambda g: g.SquareLattice(3), 2, [2.0, 2.0]),
    "rect4x3": (lambda g: g.RectangularLattice(4, 3), 2, [2.0, 2.0]),
    # rows (1/2, s), (3/2, s), (1, 0) and their inverses, s = sqrt(3) / 2: 2 (1/4 + 9/4 + 1) and 2 (3/4 + 3/4)
    "triangular4": (lambda g: g.TriangularLattice(4), 3, [7.0, 3.0]),
    # three bonds of length 1 / sqrt(3) at 120 degrees: (3 / 2) (1 / 3) per axis
    "honeycomb3": (lambda g: g.HoneycombLattice(3), 3, [0.5, 0.5]),
    "bilayer3": (lambda g: g.BilayerSquareLattice(3), 3, [2.0, 2.0]),  # (True: the two in-plane axes)
    "cubic3x3": (lambda g: g.CubicLattice(3, 3), 3, [2.0, 2.0, 2.0]),
    "cubic4x3": (lambda g: g.CubicLattice(4, 3), 4, [2.0, 2.0, 2.0, 2.0]),
}


def _pairs(l):
    """{(i, j), i < j} -> the directed slots (k, src) between the two sites"""
    nb = np.asarray(l.neighs) - 1
    out = {}
    for k, i in itertools.product(range(nb.shape[0]), range(nb.shape[1])):
        j = int(nb[k, i])
        out.setdefault((min(i, j), max(i, j)), []).append((k, i))
    return out


@pytest.mark.parametrize("name", list(LATTICES))
def test_bond_classes(mc_amd, name):
    make, n_c, moment = LATTICES[name]
    l = make(mc_amd)
    cls, vec, x = mc_amd.bond_classes(l, True)
    nb = np.asarray(l.neighs) - 1
    z, N = nb.shape
    assert cls.shape == (z, N) and cls.dtype == np.int8 and vec.shape[0] == n_c == x.shape[1] and x.shape[0] == len(moment)
    assert cls.min() >= -1 and set(np.unique(cls[cls >= 0])) == set(range(n_c))
    # every undirected neighbour pair once, and with both of its slots the same class vector up to the sign
    pairs = _pairs(l)
    disp = np.zeros((z, N, vec.shape[1]))
    for (i, j), slots in pairs.items():
        assert len(slots) == 2 and sum(cls[k, s] >= 0 for k, s in slots) == 1, (name, i, j, slots)
        (kc, sc), = [(k, s) for k, s in slots if cls[k, s] >= 0]
        (ku, su), = [(k, s) for k, s in slots if cls[k, s] < 0]
        assert su != sc
        disp[kc, sc] = vec[cls[kc, sc]]
        disp[ku, su] = -vec[cls[kc, sc]]
    assert int((cls >= 0).sum()) == len(pairs) == z * N // 2
    # canonical orientation: the first non-zero component of a class vector is positive
    for v in vec:
        assert next(c for c in v if abs(c) > 1e-9) > 0
    assert np.array_equal(x, np.eye(vec.shape[1])[:len(moment)] @ vec.T)
    # the second moment of a site's slots along every direction
    m = np.einsum("md,kid->mki", np.eye(vec.shape[1])[:len(moment)], disp) ** 2
    np.testing.assert_allclose(m.sum(axis=1), np.array(moment)[:, None] * np.ones(N), rtol=0, atol=1e-12)
    if name != "cubic4x3":  # against the positions: the minimum image of r_j - r_i of every slot
        from montecarlo_jl_amd import lattices
        pos = np.array(lattices._positions(l))
        A = lattices._lattice_vectors(l)
        shifts = [sum(c * a for c, a in zip(cs, A)) for cs in itertools.product((-1, 0, 1), repeat=len(A))]
        for k, i in itertools.product(range(z), range(N)):
            raw = pos[nb[k, i]] - pos[i]
            best = min(np.linalg.norm(raw + s) for s in shifts)
            assert np.linalg.norm(disp[k, i]) == pytest.approx(best, abs=1e-12)
            if name != "bilayer3" or k < 4:  # (the interlayer bond is its own inverse: +z and -z are both images)
                assert any(np.linalg.norm(raw + s - disp[k, i]) < 1e-9 for s in shifts), (name, k, i)


def test_bond_classes_directions_and_refusals(mc_amd):
    l = mc_amd.TriangularLattice(4)
    a1 = np.array([0.5, S3])
    cls, vec, x = mc_amd.bond_classes(l, [a1, [1.0, 0.0]])
    np.testing.assert_allclose(vec, [[0.5, S3], [1.5, S3], [1.0, 0.0]], atol=1e-12)
    np.testing.assert_allclose(x, [[1.0, 1.5, 0.5], [0.5, 1.5, 1.0]], atol=1e-12)
    # honeycomb: the class of a slot depends on the sublattice of its source
    h = mc_amd.HoneycombLattice(3)
    cls, vec, _ = mc_amd.bond_classes(h, True)
    assert np.all(cls[0, 0::2] >= 0) and np.all(cls[0, 1::2] == -1)      # b = (1/sqrt(3), 0) from A to B
    assert np.all(cls[1:, 0::2] == -1) and np.all(cls[1:, 1::2] >= 0)    # the other two are canonical from B to A
    # a period of 2 along a requested direction
    with pytest.raises(ValueError, match="ambiguous"):
        mc_amd.bond_classes(mc_amd.SquareLattice(2), [[1.0, 0.0]])
    with pytest.raises(ValueError, match="ambiguous"):
        mc_amd.bond_classes(mc_amd.BilayerSquareLattice(3), [[0.0, 0.0, 1.0]])
    cls, vec, x = mc_amd.bond_classes(mc_amd.RectangularLattice(2, 3), [[0.0, 1.0]])  # x is not asked for: fine
    assert x.shape == (1, 2) and sorted(x[0].tolist()) == [0.0, 1.0]
    with pytest.raises(ValueError, match="unit vectors"):
        mc_amd.bond_classes(l, [[2.0, 0.0]])
    with pytest.raises(ValueError, match="direction vectors"):
        mc_amd.bond_classes(l, [[1.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="direction vectors"):
        mc_amd.bond_classes(l, np.zeros((5, 2)))


@pytest.mark.parametrize("q", [2, 5, 6, 64])
def test_twist_tables(mc_amd, q):
    m = mc_amd.ClockModel(q, dims=1, L=4)
    d1, d2 = m.twist_q30
    assert d1.dtype == np.int64 and d2.dtype == np.int64 and len(d1) == len(d2) == q
    for d in range(q):
        assert d1[(q - d) % q] == -d1[d] and d2[(q - d) % q] == d2[d], d
    assert d1[0] == 0 and (q % 2 or d1[q // 2] == 0)
    assert np.array_equal(d2, m.e_q30) and d2[0] == 2 ** 30
    if q == 2:
        assert not d1.any()
    else:
        assert d1[1] == ref.llround(np.sin(2.0 * np.pi / q) * 2.0 ** 30) > 0
    r1, r2 = ref.twist_q30(q, *ref.clock_twist(q))
    assert np.array_equal(d1, r1) and np.array_equal(d2, r2)
    # J scales and signs both
    mj = mc_amd.ClockModel(q, dims=1, L=4, J=-2.0)
    assert np.array_equal(mj.twist_q30[1], mj.e_q30) and mj.twist_q30[1][0] == -2 ** 31
    assert np.array_equal(mj.twist_q30[0], ref.twist_q30(q, *ref.clock_twist(q), J=-2.0)[0])


def test_twist_argument(mc_amd):
    e = [1.0, -0.5, 0.25, 0.25, -0.5]
    ok = ([0.0, 0.7, -0.1, 0.1, -0.7], [1.0, 0.5, -2.0, -2.0, 0.5])
    m = mc_amd.QStateModel(5, e, dims=1, L=4, J=-2.0, twist=ok)
    assert m.twist_q30[0].tolist() == [0] + [int(ref.llround(-2.0 * v * 2.0 ** 30)) for v in ok[0][1:]]
    assert m.twist_q30[1][2] == 2 ** 32
    assert mc_amd.QStateModel(5, e, dims=1, L=4).twist_q30 is None and mc_amd.PottsModel(3, dims=1, L=4).twist_q30 is None
    with pytest.raises(ValueError, match="antisymmetric"):
        mc_amd.QStateModel(5, e, dims=1, L=4, twist=([0.0, 0.7, -0.1, 0.1, 0.7], ok[1]))
    with pytest.raises(ValueError, match="antisymmetric"):
        mc_amd.QStateModel(5, e, dims=1, L=4, twist=([0.1, 0.7, -0.1, 0.1, -0.7], ok[1]))
    with pytest.raises(ValueError, match="symmetric"):
        mc_amd.QStateModel(5, e, dims=1, L=4, twist=(ok[0], [1.0, 0.5, -2.0, -2.0, 0.6]))
    with pytest.raises(ValueError, match="at most 4"):
        mc_amd.QStateModel(5, e, dims=1, L=4, J=-2.0, twist=(ok[0], [1.0, 0.5, -2.5, -2.5, 0.5]))
    with pytest.raises(ValueError, match="finite values"):
        mc_amd.QStateModel(5, e, dims=1, L=4, twist=(ok[0][:4], ok[1]))
    with pytest.raises(ValueError, match="pair"):
        mc_amd.QStateModel(5, e, dims=1, L=4, twist=3.0)


ENUM = {"chain4_q4": (lambda g: g.Chain(4), 4), "chain4_q5": (lambda g: g.Chain(4), 5),
        "square3_q3": (lambda g: g.SquareLattice(3), 3)}


@pytest.mark.parametrize("beta", [0.5, 1.5])
@pytest.mark.parametrize("name", list(ENUM))
def test_identity_by_enumeration(mc_amd, name, beta):
    """Upsilon_mu = (<T_mu> - beta <J_mu^2>) / N over all q^N states against the central second difference of
    F(phi) = -ln Z(phi) / beta at h = 1e-3, 1e-6 relative.  The three-point difference has the truncation error
    h^2 F'''' / 12, about 1e-7 of an O(1) derivative, and that is what it shows: 8.4e-8 absolute on Chain(4), q = 4 at
    beta = 0.5, where Upsilon is only 0.065 and the relative error is therefore 1.3e-6.  So the difference is taken with
    the five-point central stencil at the same h (the three-point differences at h and 2 h, extrapolated), whose
    truncation error is h^4 F'''''' / 90, below 1e-12; the round-off, eps ln Z / h^2, is about 1e-9.  The three-point
    value is printed beside it."""
    make, q = ENUM[name]
    l = make(mc_amd)
    cls, vec, x = mc_amd.bond_classes(l, True)
    got = ref.upsilon_exact(l, q, cls, x, beta)
    h = 1e-3
    for mu in range(len(x)):
        f = {m: ref.twisted_lnZ(l, q, cls, x[mu], beta, m * h) for m in (-2, -1, 0, 1, 2)}
        three = -(f[-1] - 2.0 * f[0] + f[1]) / (h * h) / beta / len(l)
        want = -(-f[-2] + 16.0 * f[-1] - 30.0 * f[0] + 16.0 * f[1] - f[2]) / (12.0 * h * h) / beta / len(l)
        print(name, beta, mu, got[mu], want, abs(got[mu] - want) / abs(want), "three-point:", three)
        assert got[mu] == pytest.approx(want, rel=1e-6), (name, beta, mu)
    if len(x) == 2:
        assert got[0] == pytest.approx(got[1], rel=1e-12)


def test_uniform_configuration(mc_amd):
    """all sites equal: every difference is 0, so J_mu = 0 and T_mu = d2[0] (bonds along mu), exactly"""
    for name, (make, n_c, _) in LATTICES.items():
        l = make(mc_amd)
        cls, vec, x = mc_amd.bond_classes(l, True)
        q = 6
        d1, d2 = ref.twist_q30(q, *ref.clock_twist(q))
        for s in (0, 4):
            I, K = ref.class_sums(np.full(len(l), s), l.neighs, cls, q, d1, d2, n_c)
            assert not I.any() and np.array_equal(K, [(cls == c).sum() * d2[0] for c in range(n_c)]), name
            T, J, J2 = ref.contract(I, K, x)
            assert not J.any() and not J2.any() and not np.signbit(J).any()
            if name in ("chain5", "square3", "rect4x3", "cubic3x3", "cubic4x3", "bilayer3"):
                assert np.array_equal(T, np.full(len(x), float(len(l)))), (name, T)  # one bond per site along every axis


def test_winding_configuration(mc_amd):
    """s_i = x_i mod q on RectangularLattice(2 q, 3), q = 5: every bond along x has s_i - s_j = -1 in its counted
    orientation (the neighbour at x + 1), every bond along y has 0"""
    q = 5
    l = mc_amd.RectangularLattice(2 * q, 3)
    N = len(l)
    cls, vec, x = mc_amd.bond_classes(l, True)
    assert vec.tolist() == [[1.0, 0.0], [0.0, 1.0]]
    conf = (np.arange(N) % (2 * q)) % q
    d1, d2 = ref.twist_q30(q, *ref.clock_twist(q))
    I, K = ref.class_sums(conf, l.neighs, cls, q, d1, d2, 2)
    assert I.tolist() == [N * int(d1[q - 1]), 0] and d1[q - 1] == -d1[1] < 0
    assert K.tolist() == [N * int(d2[1]), N * int(d2[0])]
    T, J, J2 = ref.contract(I, K, x)
    assert J[0] == float(N * int(d1[q - 1])) / 2.0 ** 30 and J[1] == 0.0 and T[1] == float(N)
    assert J[0] == pytest.approx(-N * np.sin(2 * np.pi / q), rel=1e-9) and J2[0] == J[0] * J[0]


def test_argument_check_under_the_sanitizers(tmp_path):
    """g++ -fsanitize=address,undefined, run once as a child process on the CPU"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host code"
    exe = str(tmp_path / "qs_stiffness_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "qs_stiffness_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and out.stdout.count("\n") == 19
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    for name, word in (("class_high", "outside -1..2"), ("d1_symmetry", "not antisymmetric"), ("d1_zero", "not antisymmetric"),
                       ("d2_symmetry", "not symmetric"), ("d1_magnitude", "2^32"), ("x_nan", "not finite")):
        assert re.search(r"^%s 0 f: .*%s" % (name, re.escape(word)), out.stdout, re.M), (name, out.stdout)


def test_keywords(mc_amd):
    """refused before any device is touched"""
    with pytest.raises(ValueError, match="twist="):
        mc_amd.MC(mc_amd.PottsModel(3, dims=2, L=4), beta=0.5, stiffness=True)
    with pytest.raises(ValueError, match="ambiguous"):
        mc_amd.MC(mc_amd.ClockModel(6, dims=2, L=2), beta=0.5, stiffness=True)
    with pytest.raises(ValueError, match="direction vectors"):
        mc_amd.MC(mc_amd.ClockModel(6, dims=2, L=4), beta=0.5, stiffness=[[1.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="stiffness"):
        mc_amd.MC(mc_amd.IsingModel(dims=2, L=4), beta=0.5, stiffness=True)
    with pytest.raises(NotImplementedError, match="stiffness=True"):  # the text that lists the q-state keywords
        mc_amd.MC(mc_amd.ClockModel(6, dims=2, L=4), beta=0.5, fss=True)


def test_abi_is_declared(mc_amd):
    from montecarlo_jl_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqmc_hip.h")).read()
    for name in ("dqmc_qs_set_stiffness", "dqmc_qs_get_stiffness", "dqmc_qs_get_stiffness_sample",
                 "dqmc_qs_stiffness_binner_get_level", "dqmc_qs_stiffness_binner_finish"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(_lib.lib(), name), name
    assert C_sizes(_lib) == (8 + 8 + 12 * 8, 36 * 8 + 8 + 4 + 4)


def C_sizes(_lib):
    import ctypes
    return ctypes.sizeof(_lib.QsStiffness), ctypes.sizeof(_lib.QsStiffnessBinned)


def test_restatement_in_the_ordered_phase(mc_amd):
    """the physics reference of the device test, the restatement alone: clock q = 6 on SquareLattice(8) at beta = 2.0,
    8 walkers, 500 + 2000 local sweeps.  Upsilon_x = 0.945995 +- 0.000862, Upsilon_y = 0.946128 +- 0.000896: the two
    axes agree within 4 combined standard errors, and the value lies between the 2 T / pi = 0.318 of the jump and the
    ground state's 1."""
    ux, ex, uy, ey = ref.physics_reference(2.0)
    print("Upsilon", ux, ex, uy, ey)
    assert ex > 0 and ey > 0 and abs(ux - uy) <= 4.0 * np.hypot(ex, ey)
    assert 2.0 * 0.5 / np.pi < ux < 1.0 and 2.0 * 0.5 / np.pi < uy < 1.0
