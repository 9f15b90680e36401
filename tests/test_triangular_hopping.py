"""The three-factor form of the triangular 16 x 16 lattice's hopping exponentials that the n = 256 slice products use
(tri.hip): the factors triangular_factors() builds, the residual the engine's gate (tri_factor_ok in hopping_forms.h, restated
here in numpy) bounds, and a register-level replay of the kernel's step order.  No GPU is needed."""
import numpy as np
import pytest

EPS = np.finfo(float).eps
GATE = 256 * EPS
L = 16


def diag_op(fd):
    """Ed: (Ed v)(x, y) = sum_y' Fd[y, y'] v(x - y + y', y') in the site order x + 16 y"""
    Ed = np.zeros((256, 256))
    for y in range(L):
        for yp in range(L):
            for x in range(L):
                Ed[x + L * y, (x - y + yp) % L + L * yp] = fd[y, yp]
    return Ed


def factors(f):
    """[block][eT2 / eTinv2] -> (Fx, Fy, Fd) from the flat array dqmc_set_triangular_factors takes"""
    nb = f.size // 1536
    m = f.reshape(nb, 2, 3, 16, 16)
    return [[tuple(m[b, k, j].T for j in range(3)) for k in range(2)] for b in range(nb)]


def residuals(E, fx, fy, fd):
    """max|E - P| / max|E| for the claimed form (Fy (x) Fx) Ed and the two orders the kernel applies"""
    Ed, Kx, Ky = diag_op(fd), np.kron(np.eye(L), fx), np.kron(fy, np.eye(L))
    s = np.abs(E).max()
    return [np.abs(E - P).max() / s for P in (np.kron(fy, fx) @ Ed, Kx @ Ed @ Ky, Ky @ Ed @ Kx)]


def models(mc_amd, kind, mu):
    l = mc_amd.TriangularLattice(L)
    return mc_amd.HubbardModelAttractive(l=l, mu=mu) if kind == "attractive" else mc_amd.HubbardModelRepulsive(l=l)


@pytest.mark.parametrize("kind,mu", [("attractive", 0.0), ("attractive", 0.5), ("repulsive", 0.0)])
@pytest.mark.parametrize("dtau", [0.1, 0.05])
def test_factors_pass_the_gate(mc_amd, kind, mu, dtau):
    model = models(mc_amd, kind, mu)
    f = mc_amd.triangular_factors(model, dtau)
    assert f.shape == (1536 * model.flv,)
    for b, T in enumerate(model.hopping_matrix()):
        eT, eTinv, eT2, eTinv2 = mc_amd.hopping_exponentials(T, dtau)
        for k, (name, E) in enumerate((("eT2", eT2), ("eTinv2", eTinv2))):
            fx, fy, fd = factors(f)[b][k]
            assert E[0, 0] > 0
            res = residuals(E, fx, fy, fd)
            print("%s mu = %.1f dtau = %.2f %s: %s ulp" % (kind, mu, dtau, name, ", ".join("%.1f" % (r / EPS) for r in res)))
            assert max(res) <= GATE, res
            # the transposed factors of the daggered products and the wraps' right products
            Ed, Kx, Ky = diag_op(fd.T), np.kron(np.eye(L), fx.T), np.kron(fy.T, np.eye(L))
            for P in (Kx @ Ed @ Ky, Ky @ Ed @ Kx):
                assert np.abs(E.T - P).max() / np.abs(E).max() <= GATE


def test_one_perturbed_bond_fails_the_gate(mc_amd):
    model = models(mc_amd, "attractive", 0.0)
    T = model.hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2  # one bond with t != 1
    f = factors(mc_amd.triangular_factors(model, 0.1))[0]
    for k, E in enumerate(mc_amd.hopping_exponentials(T, 0.1)[2:]):
        assert min(residuals(E, *f[k])) > 100 * GATE


def test_square_lattice_exponentials_are_not_triangular(mc_amd):
    """the same sites without the diagonal hopping: the triangular factors do not reproduce it"""
    model = models(mc_amd, "attractive", 0.0)
    E = mc_amd.hopping_exponentials(mc_amd.HubbardModelAttractive(16, 2).hopping_matrix()[0], 0.1)[2]
    assert min(residuals(E, *factors(mc_amd.triangular_factors(model, 0.1))[0][0])) > 100 * GATE


def mfma(a, b, c):
    """v_mfma_f64_16x16x4_f64 over the 64 lanes: a, b one value per lane, c / result [lane][4]; D[(lane >> 4) + 4 r][lane & 15]"""
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


lanes = np.arange(64)
G, CI = lanes >> 4, lanes & 15


def idx(par, r):
    """entry index of register r in state A (par 0) or B (par 1), tri.hip idx()"""
    return (G + 4 * r) + 16 * CI if par else CI + 16 * (G + 4 * r)


def a_operands(F):
    """lane value of k-block q: F[row ci][k = 4 q + g]"""
    return [F[CI, 4 * q + G] for q in range(4)]


def product(F, v):
    p = np.zeros_like(v)
    for q, aq in enumerate(a_operands(F)):
        p = mfma(aq, v[:, q], p)
    return p


def step(v, par, fx, fy, fd):
    """one step of tri_chain_kernel on one column tile, as the kernel orders it: f1, the sheared pass, Fd, the second
    pass, f3"""
    f1, f3 = (fx, fy) if par else (fy, fx)
    t1 = np.zeros((16, 17))
    p = product(f1, v)
    for r in range(4):
        t1[G + 4 * r, CI] = p[:, r]
    w = np.zeros_like(v)
    for r in range(4):
        y = G + 4 * r
        x = (CI + y) & 15
        w[:, r] = t1[x, y] if par else t1[y, x]
    t2 = np.zeros((16, 17))
    p = product(fd, w)
    for r in range(4):
        t2[G + 4 * r, CI] = p[:, r]
    for r in range(4):
        k = G + 4 * r
        w[:, r] = t2[k, (CI - k) & 15] if par else t2[CI, (k - CI) & 15]
    return product(f3, w)


@pytest.mark.parametrize("transposed", [False, True])
def test_kernel_step_order_reproduces_the_product(transposed):
    """two steps (state A -> B -> A) on random factors that commute like the lattice's (circulants): E X and E' X"""
    rng = np.random.default_rng(7)

    def circulant():
        c = rng.standard_normal(L)
        return np.array([[c[(i - j) % L] for j in range(L)] for i in range(L)])
    fx, fy, fd = circulant(), circulant(), circulant()
    E = np.kron(fy, fx) @ diag_op(fd)
    if transposed:
        fx, fy, fd, E = fx.T, fy.T, fd.T, E.T
    X = rng.standard_normal(256)
    v = np.zeros((64, 4))
    for r in range(4):
        v[:, r] = X[idx(0, r)]
    v = step(v, 0, fx, fy, fd)
    got = np.zeros(256)
    for r in range(4):
        got[idx(1, r)] = v[:, r]
    ref = E @ X
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()
    v = step(v, 1, fx, fy, fd)
    for r in range(4):
        got[idx(0, r)] = v[:, r]
    ref = E @ ref
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()


def test_kernel_step_order_with_the_lattice_factors(mc_amd):
    """the same replay with the factors of eT2 of the attractive model at mu = 0.5: E X within the gate's rounding"""
    model = models(mc_amd, "attractive", 0.5)
    fx, fy, fd = factors(mc_amd.triangular_factors(model, 0.1))[0][0]
    E = mc_amd.hopping_exponentials(model.hopping_matrix()[0], 0.1)[2]
    X = np.random.default_rng(3).standard_normal(256)
    v = np.zeros((64, 4))
    for r in range(4):
        v[:, r] = X[idx(0, r)]
    v = step(v, 0, fx, fy, fd)
    got = np.zeros(256)
    for r in range(4):
        got[idx(1, r)] = v[:, r]
    assert np.abs(got - E @ X).max() < 1e-12 * np.abs(E @ X).max()
