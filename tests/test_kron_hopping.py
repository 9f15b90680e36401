"""The Kronecker form of the hopping exponentials that the n = 256 slice products use (kron.hip; the gate is
kron_split in hopping_forms.h (kron_factor before the form table), restated here in numpy, so no GPU is needed).  On the periodic 16 x 16 square lattice
(site x + 16 y) T is a Kronecker sum, so eT2 and eTinv2 are Ey (x) Ex up to rounding."""
import numpy as np
import pytest

GATE = 256 * np.finfo(float).eps


def factor(E):
    """engine.cpp kron_factor: Ex = E[0:16, 0:16], Ey = E[0::16, 0::16] / E[0, 0]; (Ex, Ey, residual / max|E|)"""
    assert E[0, 0] > 0
    ex = E[:16, :16].copy()
    ey = E[::16, ::16] / E[0, 0]
    return ex, ey, np.abs(E - np.kron(ey, ex)).max() / np.abs(E).max()


def exps(mc_amd, model, dtau):
    return [mc_amd.dqmc.hopping_exponentials(T, dtau) for T in model.hopping_matrix()]


@pytest.mark.parametrize("kind,mu", [("attractive", 0.0), ("attractive", 0.5), ("repulsive", 0.0)])
@pytest.mark.parametrize("dtau", [0.1, 0.05])
def test_square_lattice_exponentials_pass_the_gate(mc_amd, kind, mu, dtau):
    if kind == "attractive":
        model = mc_amd.HubbardModelAttractive(16, 2, mu=mu)
    else:
        model = mc_amd.HubbardModelRepulsive(16, 2)
    for eT, eTinv, eT2, eTinv2 in exps(mc_amd, model, dtau):
        for E in (eT2, eTinv2):
            ex, ey, res = factor(E)
            assert res <= GATE, res
            # the transposed factors of the daggered products: (Ey (x) Ex)' = Ey' (x) Ex', the same residual
            assert np.abs(E.T - np.kron(ey.T, ex.T)).max() / np.abs(E).max() <= GATE


def test_one_perturbed_bond_fails_the_gate(mc_amd):
    model = mc_amd.HubbardModelAttractive(16, 2)
    T = model.hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2                      # one bond with t != 1
    for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
        assert factor(E)[2] > 100 * GATE


def test_factored_product_is_two_16_contractions():
    """(Ay (x) Ax) vec(V) = vec(Ax V Ay'), V[x, y] = v[x + 16 y]: what one step of kron_chain_kernel computes, in the
    order it computes it (the contraction over the register index first, then the lane index after the transpose)"""
    rng = np.random.default_rng(3)
    ax, ay, X = rng.standard_normal((16, 16)), rng.standard_normal((16, 16)), rng.standard_normal((256, 5))
    ref = np.kron(ay, ax) @ X
    for c in range(5):
        V = X[:, c].reshape(16, 16, order="F")     # V[x, y]
        P = ay @ V.T                               # parity 0: registers hold y, the lanes x; sum over y first
        Q = ax @ P.T                               # Q[x, y]: after the transpose, sum over x
        assert np.abs(Q.reshape(-1, order="F") - ref[:, c]).max() < 1e-12 * np.abs(ref).max()
