"""The three-factor Kronecker form of the hopping exponentials that the n = 512 slice products use (kron3.hip; the gate is
kron_split in hopping_forms.h (kron3_factor before the form table), restated here in numpy, so no GPU is needed).  On the periodic 8 x 8 x 8 cubic lattice
(site x + 8 y + 64 z) T is a Kronecker sum, so eT2 and eTinv2 are Ez (x) Ey (x) Ex up to rounding."""
import numpy as np
import pytest

EPS = np.finfo(float).eps
GATE = 256 * EPS


def factor3(E):
    """engine.cpp kron3_factor: Ex = E[0:8, 0:8], Ey = E[0::8, 0::8][:8, :8] / E00, Ez = E[0::64, 0::64] / E00;
    (Ex, Ey, Ez, residual / max|E|)"""
    assert E.shape == (512, 512) and E[0, 0] > 0
    ex = E[:8, :8].copy()
    ey = E[0::8, 0::8][:8, :8] / E[0, 0]
    ez = E[0::64, 0::64] / E[0, 0]
    return ex, ey, ez, np.abs(E - np.kron(ez, np.kron(ey, ex))).max() / np.abs(E).max()


def exps(mc_amd, model, dtau):
    return [mc_amd.dqmc.hopping_exponentials(T, dtau) for T in model.hopping_matrix()]


@pytest.mark.parametrize("kind,mu", [("attractive", 0.0), ("attractive", 0.5), ("repulsive", 0.0)])
@pytest.mark.parametrize("dtau", [0.1, 0.05])
def test_cubic_lattice_exponentials_pass_the_gate(mc_amd, kind, mu, dtau):
    if kind == "attractive":
        model = mc_amd.HubbardModelAttractive(8, 3, mu=mu)
    else:
        model = mc_amd.HubbardModelRepulsive(8, 3)
    for eT, eTinv, eT2, eTinv2 in exps(mc_amd, model, dtau):
        for name, E in (("eT2", eT2), ("eTinv2", eTinv2)):
            ex, ey, ez, res = factor3(E)
            print("L = 8, mu = %.1f, dtau = %.2f, %s: %.1f ulp of max|E|" % (mu, dtau, name, res / EPS))
            assert res <= GATE, res
            # the transposed factors of the daggered products and the wrap's right products: the same residual
            assert np.abs(E.T - np.kron(ez.T, np.kron(ey.T, ex.T))).max() / np.abs(E).max() <= GATE


def test_one_perturbed_bond_fails_the_gate(mc_amd):
    T = mc_amd.HubbardModelAttractive(8, 3).hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2                      # one bond with t != 1
    for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
        assert factor3(E)[3] > 100 * GATE


def test_16_by_32_square_lattice_fails_the_gate(mc_amd):
    """n = 512 as well, but a two-factor product of 16 x 16 and 32 x 32 blocks: not Ez (x) Ey (x) Ex with 8 x 8 factors"""
    def ring(L):
        C = np.zeros((L, L))
        for i in range(L):
            C[(i + 1) % L, i] = C[(i - 1) % L, i] = 1.0
        return C
    T = -(np.kron(np.eye(32), ring(16)) + np.kron(ring(32), np.eye(16)))
    for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
        assert factor3(E)[3] > 100 * GATE


def operand_images(ex, ey, ez):
    """what engine.cpp kron3_images hands to the kernel: Exy = Ey (x) Ex as [mp][m][r][lane] A operands and
    I2 (x) Ez as [q][lane]"""
    exy = np.kron(ey, ex)
    img_xy = np.zeros((4, 4, 4, 64))
    for mp in range(4):
        for m in range(4):
            for r in range(4):
                for lane in range(64):
                    img_xy[mp, m, r, lane] = exy[16 * mp + (lane & 15), 16 * m + 4 * r + (lane >> 4)]
    bd = np.kron(np.eye(2), ez)
    img_z = np.array([[bd[lane & 15, 4 * q + (lane >> 4)] for lane in range(64)] for q in range(4)])
    return img_xy, img_z


def mfma(a, b, c):
    """v_mfma_f64_16x16x4_f64 over the 64 lanes: a, b one value per lane, c / result [lane][4]"""
    A = np.zeros((16, 4)); B = np.zeros((4, 16))
    for lane in range(64):
        A[lane & 15, lane >> 4] = a[lane]
        B[lane >> 4, lane & 15] = b[lane]
    D = A @ B
    out = c.copy()
    for lane in range(64):
        for r in range(4):
            out[lane, r] += D[(lane >> 4) + 4 * r, lane & 15]
    return out


def test_kernel_step_order_reproduces_the_product():
    """one wave's two columns through the two states of kron3_chain_kernel, in the order it works: state Z, the
    8-contraction, the transpose, the 64-contraction in state I; then the next step from state I back to Z"""
    rng = np.random.default_rng(5)
    ex, ey, ez = (rng.standard_normal((8, 8)) for _ in range(3))
    X = rng.standard_normal((512, 2))
    A = np.kron(ez, np.kron(ey, ex))
    img_xy, img_z = operand_images(ex, ey, ez)
    lanes = np.arange(64)
    g, c = lanes >> 4, lanes & 15

    def eidx(st, m, r):
        return 16 * m + g + 4 * r + 64 * (c & 7) if st else 16 * m + c + 64 * (g + 4 * (r & 1))

    def hcol(st, r):
        return c >> 3 if st else np.full(64, r >> 1)

    v = np.zeros((4, 64, 4))  # [tile m][lane][register r]
    for m in range(4):
        for r in range(4):
            v[m, :, r] = X[eidx(0, m, r), hcol(0, r)]

    def contract_z(v):
        out = np.zeros_like(v)
        for m in range(4):
            for q in range(4):
                out[m] = mfma(img_z[q], v[m, :, q], out[m])
        return out

    def contract_i(v):
        out = np.zeros_like(v)
        for m in range(4):
            for r in range(4):
                for mp in range(4):
                    out[mp] = mfma(img_xy[mp, m, r], v[m, :, r], out[mp])
        return out

    def transpose(v, st):
        T = np.zeros((16, 65))
        w = np.zeros_like(v)
        for m in range(4):
            for r in range(4):
                if st:
                    T[c, 16 * m + g + 4 * r] = v[m, :, r]
                else:
                    T[g + 4 * r, 16 * m + c] = v[m, :, r]
        for m in range(4):
            for r in range(4):
                w[m, :, r] = T[g + 4 * r, 16 * m + c] if st else T[c, 16 * m + g + 4 * r]
        return w

    v = contract_i(transpose(contract_z(v), 0))          # step 0: Z -> I
    got = np.zeros((512, 2))
    for m in range(4):
        for r in range(4):
            got[eidx(1, m, r), hcol(1, r)] = v[m, :, r]
    assert np.abs(got - A @ X).max() < 1e-12 * np.abs(A @ X).max()
    v = contract_z(transpose(contract_i(v), 1))          # step 1: I -> Z
    for m in range(4):
        for r in range(4):
            got[eidx(0, m, r), hcol(0, r)] = v[m, :, r]
    ref = A @ (A @ X)
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()
