"""The inputs of test_gpu_factored_generic.py, checked without a GPU: every matrix the GPU cases use passes the acceptance
gate of its own kernel family (restated here from the comments of include/dqmc_hip.h and engine.cpp) with a wide margin,
fails the gate the engine tries before it, and has the properties the physical exponentials lack: it is not symmetric, its
factors are not circulant, and the two spin blocks differ."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factored_exps as FE  # noqa: E402

EPS = np.finfo(np.float64).eps
GATE_ULP = 256.0    # the engine's limit
MARGIN_ULP = 16.0   # what a matrix may measure to go to the GPU: one that only just passes does not


# ---- the gates.  Each returns the residual max|E - form| / (eps max|E|), inf where E[0, 0] > 0 fails
def kron_gate(E, dims):
    """kron_factor (16, 16), rect_factor (32, 8), kron3_factor (8, 8, 8), bilayer_factor (16, 16, 2): the factor of an
    axis is read from the entries whose other coordinates are 0 (Ex = E[0:mx, 0:mx]; Ey = E[0::mx, 0::mx][0:my, 0:my] /
    E[0, 0]; Ez = E[0::mx my, 0::mx my] / E[0, 0]), and the product is formed as fz * fy * fx"""
    if not E[0, 0] > 0.0 or E.shape[0] != int(np.prod(dims)):
        return np.inf
    fs, stride = [], 1
    for a, m in enumerate(dims):
        f = E[0:stride * m:stride, 0:stride * m:stride]
        fs.append(f if a == 0 else f / E[0, 0])
        stride *= m
    P = fs[-1]
    for f in fs[-2::-1]:
        P = np.kron(P, f)
    return np.abs(E - P).max() / (EPS * np.abs(E).max())


def _ops(factors):
    I = np.eye(FE.L)
    ops = [np.kron(I, factors[0]), np.kron(factors[1], I), FE._diagonal_operator(factors[2], -1)]
    if len(factors) == 4:
        ops.append(FE._diagonal_operator(factors[3], +1))
    return ops


def commuting_gate(E, factors):
    """tri_factor_ok: the claimed form (Fy (x) Fx) Ed and the orders Fx Ed Fy, Fy Ed Fx; ttp_factor_ok: the five orders of
    its table (first entry applied first), 0: Fx, 1: Fy, 2: Ed, 3: Ea.  The largest residual over the orders."""
    if not E[0, 0] > 0.0:
        return np.inf
    ops = _ops(factors)
    if len(factors) == 3:
        orders = [(2, 0, 1), (1, 2, 0), (0, 2, 1)]
    else:
        orders = [(3, 2, 0, 1), (1, 2, 3, 0), (0, 2, 3, 1), (0, 3, 2, 1), (1, 3, 2, 0)]
    worst = 0.0
    for order in orders:
        M = np.eye(FE.L * FE.L)
        for k in order:
            M = ops[k] @ M
        worst = max(worst, np.abs(E - M).max())
    return worst / (EPS * np.abs(E).max())


def _split(farr, nb, parts):
    """[block][eT2 | eTinv2][part] -> 16 x 16 factor, from the layout of triangular_factors / square_tp_factors"""
    f = farr.reshape(nb, 2, parts, FE.L, FE.L)
    return [[[f[b, m, k].T for k in range(parts)] for m in range(2)] for b in range(nb)]  # (column-major)


# the gate of each family, and the one the engine tries first at that n (which must refuse the matrices)
OWN = {"square16": (16, 16), "rect32x8": (32, 8), "cubic8": (8, 8, 8), "bilayer16": (16, 16, 2)}
TRIED_FIRST = {"rect32x8": [(16, 16)], "bilayer16": [(8, 8, 8)], "tri16": [(16, 16), (32, 8)], "ttp16": [(16, 16), (32, 8)]}


@pytest.fixture(scope="module", params=FE.ALL_CASES, ids=["%s-%s" % fc for fc in FE.ALL_CASES])
def case(request):
    family, name = request.param
    exps, farr = FE.case_inputs(family, name)
    return family, name, exps, farr


def test_own_gate_passes_with_margin(case):
    family, name, exps, farr = case
    worst = 0.0
    for b, e in enumerate(exps):
        for m, E in enumerate((e[2], e[3])):  # the gates read eT2 and eTinv2
            if family in OWN:
                r = kron_gate(E, OWN[family])
            else:
                r = commuting_gate(E, _split(farr, len(exps), len(FE.SCALES[family]))[b][m])
            worst = max(worst, r)
    print("%s %s: gate residual %.2f ulp (limit %g)" % (family, name, worst, GATE_ULP))
    assert worst <= MARGIN_ULP


def test_gates_tried_first_refuse(case):
    """the engine tries the 16 x 16 gate before the 32 x 8 one and the 8 x 8 x 8 gate before the two-layer one; a handle
    that has taken either never asks for the triangular or t-t' factors"""
    family, name, exps, farr = case
    for dims in TRIED_FIRST.get(family, []):
        for e in exps:
            assert kron_gate(e[2], dims) > 100 * GATE_ULP and kron_gate(e[3], dims) > 100 * GATE_ULP, dims


def test_products_are_consistent(case):
    family, name, exps, farr = case
    for eT, eTinv, eT2, eTinv2 in exps:
        I = np.eye(eT.shape[0])
        assert np.abs(eT2 @ eTinv2 - I).max() < 1e-13
        assert np.abs(eT @ eTinv - I).max() < 1e-13
        assert np.abs(eT @ eT - eT2).max() < 1e-13
        assert np.abs(eTinv @ eTinv - eTinv2).max() < 1e-13
        assert 1.0 < np.linalg.cond(eT2) < 4.0  # (the physical exponentials: about 2.2)


def test_asymmetry(case):
    family, name, exps, farr = case
    for e in exps:
        for E in e:
            asym = np.abs(E - E.T).max() / np.abs(E).max()
            if name == "symmetric":
                assert asym < 1e-14
            else:
                assert asym > 1e-2, asym


def _shift(F):
    return np.roll(F, (1, 1), axis=(0, 1))


def test_generic_factors_are_far_from_circulant():
    for family in FE.KRONECKER:
        for name, seeds in FE.CASES.items():
            base = 1000 * (1 + list(FE.FAMILIES).index(family))
            for s in seeds:
                gens = FE.generators(FE.FAMILIES[family], base + s, symmetric=name == "symmetric")
                for fs in FE.axis_exponentials(gens, FE.DELTA_TAU):
                    for F in fs:
                        assert np.abs(F - _shift(F)).max() > 1e-2 * np.abs(F).max(), (family, name, F.shape)
                        if name == "symmetric":
                            assert np.abs(F - F.T).max() < 1e-15


def test_commuting_factors_are_circulant_and_asymmetric():
    for family in ("tri16", "ttp16"):
        for name in ("attractive", "repulsive"):
            exps, farr = FE.case_inputs(family, name)
            parts = len(FE.SCALES[family])
            assert farr.shape == (len(exps) * 2 * parts * 256,)
            for per_block in _split(farr, len(exps), parts):
                for fs in per_block:
                    for F in fs:
                        assert np.abs(F - _shift(F)).max() < 1e-15
                        assert np.abs(F - F.T).max() > 1e-2 * np.abs(F).max()


def test_spin_blocks_differ():
    for family in FE.FAMILIES:
        exps, farr = FE.case_inputs(family, "repulsive")
        assert len(exps) == 2
        for E0, E1 in zip(*exps):
            assert np.abs(E0 - E1).max() > 1e-2 * np.abs(E0).max()
        assert all(len(FE.case_inputs(family, c)[0]) == 1 for c in FE.CASES if (family, c) in FE.ALL_CASES and c != "repulsive")


def test_builder_is_seeded():
    a, fa = FE.case_inputs("ttp16", "repulsive")
    b, fb = FE.case_inputs("ttp16", "repulsive")
    assert all(np.array_equal(x, y) for ea, eb in zip(a, b) for x, y in zip(ea, eb)) and np.array_equal(fa, fb)
    c, _ = FE.case_inputs("rect32x8", "attractive")
    d, _ = FE.case_inputs("rect32x8", "symmetric")
    assert c[0][0].shape == (256, 256) and np.abs(c[0][0] - d[0][0]).max() > 1e-2


def test_gate_restatements_on_the_physical_exponentials(mc_amd):
    """the restated gates accept what the engine is known to accept: the lattices' own exponentials, each by its own gate,
    and the model's own triangular and t-t' factors"""
    dtau = 0.1
    models = {"square16": mc_amd.HubbardModelAttractive(16, 2),
              "rect32x8": mc_amd.HubbardModelAttractive(l=mc_amd.RectangularLattice(32, 8)),
              "cubic8": mc_amd.HubbardModelAttractive(8, 3),
              "bilayer16": mc_amd.HubbardModelAttractive(l=mc_amd.BilayerSquareLattice(16), t_perp=1.3)}
    for family, model in models.items():
        e = mc_amd.hopping_exponentials(model.hopping_matrix()[0], dtau)
        assert kron_gate(e[2], OWN[family]) <= GATE_ULP and kron_gate(e[3], OWN[family]) <= GATE_ULP, family
        for dims in TRIED_FIRST.get(family, []):
            assert kron_gate(e[2], dims) > GATE_ULP
    for model, fn, parts in ((mc_amd.HubbardModelAttractive(l=mc_amd.TriangularLattice(16), mu=-0.3), mc_amd.triangular_factors, 3),
                             (mc_amd.HubbardModelAttractive(16, 2, tp=-0.25, mu=-0.3), mc_amd.square_tp_factors, 4)):
        e = mc_amd.hopping_exponentials(model.hopping_matrix()[0], dtau)
        f = _split(fn(model, dtau), 1, parts)[0]
        assert commuting_gate(e[2], f[0]) <= GATE_ULP and commuting_gate(e[3], f[1]) <= GATE_ULP
        assert commuting_gate(e[2], [1.001 * f[0][0]] + f[0][1:]) > GATE_ULP  # (and refuse a factor that is off)
