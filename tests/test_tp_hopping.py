"""Next-nearest-neighbour hopping t' on the square lattice, host side: the hopping matrix, the lattices and decompositions
that refuse it, the four-factor form of the 16 x 16 lattice's hopping exponentials that the n = 256 slice products use
(ttp.hip) with the residual the engine's gate (ttp_factor_ok in hopping_forms.h, restated here in numpy) bounds, a
register-level replay of the kernel's step order, the checkpoint's model entry and the helpers that refuse tp != 0.
No GPU is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_triangular_hopping import CI, G, diag_op, idx, product  # noqa: E402

EPS = np.finfo(float).eps
GATE = 256 * EPS
L = 16
# (t, t', mu, delta_tau): the sets the four-factor form was measured at (29 - 44 ulp)
SETS = [(1.0, -0.25, 0.0, 0.1), (1.0, -0.25, -0.8, 0.1), (1.0, 0.3, 0.5, 0.05), (1.0, -0.4, -1.0, 0.125)]


# ---- the hopping matrix
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
@pytest.mark.parametrize("Ls", [4, 6, 16])
def test_hopping_matrix_with_tp(mc_amd, kind, Ls):
    t, tp, mu = 1.1, -0.3, 0.4
    cls = mc_amd.HubbardModelAttractive if kind == "attractive" else mc_amd.HubbardModelRepulsive
    m = cls(Ls, 2, t=t, tp=tp, mu=mu)
    assert m.tp == tp
    Ts = m.hopping_matrix()
    assert len(Ts) == m.flv
    k = 2.0 * np.pi * np.arange(Ls) / Ls
    band = np.sort((-2.0 * t * (np.cos(k)[:, None] + np.cos(k)[None, :])
                    - 4.0 * tp * np.cos(k)[:, None] * np.cos(k)[None, :] - mu).reshape(-1))
    for T in Ts:
        assert np.array_equal(T, T.T)
        assert np.abs(T.sum(axis=1) - (-4.0 * t - 4.0 * tp - mu)).max() < 1e-13
        assert np.abs(np.linalg.eigvalsh(T) - band).max() < 1e-12
        assert np.array_equal(np.diag(T), np.full(Ls * Ls, -mu))
        assert (np.count_nonzero(T - np.diag(np.diag(T)), axis=1) == 8).all()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_tp_zero_is_bit_identical(mc_amd, kind):
    cls = mc_amd.HubbardModelAttractive if kind == "attractive" else mc_amd.HubbardModelRepulsive
    for Ls, mu in ((4, 0.0), (6, 0.3)):
        a, b = cls(Ls, 2, t=0.9, mu=mu), cls(Ls, 2, t=0.9, mu=mu, tp=0.0)
        assert b.tp == 0.0
        for Ta, Tb in zip(a.hopping_matrix(), b.hopping_matrix()):
            assert Ta.tobytes() == Tb.tobytes()
    m = mc_amd.HubbardModel(4, 2, U=2.0, tp=-0.2)
    assert isinstance(m, mc_amd.HubbardModelRepulsive) and m.tp == -0.2
    m = mc_amd.HubbardModel(4, 2, U=-2.0, tp=-0.2)
    assert isinstance(m, mc_amd.HubbardModelAttractive) and m.tp == -0.2 and m.U == 2.0


def test_L2_counts_coinciding_diagonals_twice(mc_amd):
    """at L = 2 upright = downleft and downright = upleft (and the two coincide as well): the one diagonal neighbour of a
    site gets -tp from all four rows, as its nearest neighbours get -t from two rows each"""
    T = mc_amd.HubbardModelAttractive(2, 2, t=1.0, tp=0.25, mu=0.0).hopping_matrix()[0]
    ref = np.array([[0, -2, -2, -1], [-2, 0, -1, -2], [-2, -1, 0, -2], [-1, -2, -2, 0]], dtype=np.float64)
    assert np.array_equal(T, ref)


def test_nnn_table(mc_amd):
    l = mc_amd.SquareLattice(4)
    assert l.nnn.shape == (4, 16)
    site = lambda x, y: 1 + x % 4 + 4 * (y % 4)
    for y in range(4):
        for x in range(4):
            s = site(x, y) - 1
            assert list(l.nnn[:, s]) == [site(x + 1, y + 1), site(x - 1, y + 1), site(x - 1, y - 1), site(x + 1, y - 1)]
            # the rows are the sums of the rows of neighs they are named after: up = x + 1, right = y + 1
            assert l.nnn[0, s] == l.neighs[1, l.neighs[0, s] - 1] and l.nnn[2, s] == l.neighs[3, l.neighs[2, s] - 1]
            assert l.nnn[1, s] == l.neighs[1, l.neighs[2, s] - 1] and l.nnn[3, s] == l.neighs[3, l.neighs[0, s] - 1]
    d = l.next_neighbors(True)
    assert len(d) == 64 and d[:4] == [(1, int(v)) for v in l.nnn[:, 0]]
    u = l.next_neighbors(False)
    assert len(u) == 32 and len({frozenset(b) for b in u}) == 32
    assert {frozenset(b) for b in u} == {frozenset(b) for b in d}
    assert np.array_equal(mc_amd.SquareLattice(4).neighs, l.neighs)


def test_tp_is_refused_where_it_is_not_defined(mc_amd):
    for l in (mc_amd.Chain(8), mc_amd.CubicLattice(3, 4), mc_amd.TriangularLattice(4)):
        for cls in (mc_amd.HubbardModelAttractive, mc_amd.HubbardModelRepulsive):
            with pytest.raises(ValueError, match="SquareLattice"):
                cls(l=l, tp=-0.25)
            assert cls(l=l, tp=0.0).tp == 0.0
    with pytest.raises(ValueError):
        mc_amd.HubbardModelAttractive(8, 1, tp=0.1)
    with pytest.raises(ValueError):
        mc_amd.HubbardModelRepulsive(4, 3, tp=0.1)
    model = mc_amd.HubbardModelAttractive(4, 2, tp=-0.25)
    for cb in (True, "sparse", "dense"):  # (refused before a device is asked for)
        with pytest.raises(ValueError, match="diagonal"):
            mc_amd.DQMC(model, beta=1.0, checkerboard=cb)


# ---- the four factors and the gate
def anti_op(fa):
    """Ea: (Ea v)(x, y) = sum_y' Fa[y, y'] v(x + y - y', y') in the site order x + 16 y"""
    Ea = np.zeros((256, 256))
    for y in range(L):
        for yp in range(L):
            for x in range(L):
                Ea[x + L * y, (x + y - yp) % L + L * yp] = fa[y, yp]
    return Ea


def factors(f):
    """[block][eT2 / eTinv2] -> (Fx, Fy, Fd, Fa) from the flat array dqmc_set_square_tp_factors takes"""
    nb = f.size // 2048
    m = f.reshape(nb, 2, 4, 16, 16)
    return [[tuple(m[b, k, j].T for j in range(4)) for k in range(2)] for b in range(nb)]


def orders(fx, fy, fd, fa):
    """the claimed form (Fy (x) Fx) Ed Ea and the four orders the kernel applies (a step from state A, one from state B,
    and the transposes of what the transposed factors give in those two)"""
    Ed, Ea, Kx, Ky = diag_op(fd), anti_op(fa), np.kron(np.eye(L), fx), np.kron(fy, np.eye(L))
    return [np.kron(fy, fx) @ Ed @ Ea, Kx @ Ea @ Ed @ Ky, Ky @ Ea @ Ed @ Kx, Ky @ Ed @ Ea @ Kx, Kx @ Ed @ Ea @ Ky]


def residuals(E, fx, fy, fd, fa):
    s = np.abs(E).max()
    return [np.abs(E - P).max() / s for P in orders(fx, fy, fd, fa)]


def kron_gate_residual(E):
    """kron_factor of engine.cpp: max|E - Ey (x) Ex| / max|E| with Ex = E[0:16, 0:16], Ey = E[0::16, 0::16] / E[0, 0]"""
    return np.abs(E - np.kron(E[0::16, 0::16] / E[0, 0], E[0:16, 0:16])).max() / np.abs(E).max()


def model_of(mc_amd, t, tp, mu, kind="attractive"):
    cls = mc_amd.HubbardModelAttractive if kind == "attractive" else mc_amd.HubbardModelRepulsive
    return cls(16, 2, t=t, tp=tp, mu=mu)


@pytest.mark.parametrize("t,tp,mu,dtau", SETS)
def test_factors_pass_the_gate_and_the_kronecker_gate_fails(mc_amd, t, tp, mu, dtau):
    for kind in ("attractive", "repulsive"):
        model = model_of(mc_amd, t, tp, mu, kind)
        f = mc_amd.square_tp_factors(model, dtau)
        assert f.shape == (2048 * model.flv,) and f.flags.c_contiguous
        if kind == "repulsive":  # both spin blocks share T
            assert np.array_equal(f[:2048], f[2048:])
            continue
        E4 = mc_amd.hopping_exponentials(model.hopping_matrix()[0], dtau)
        for k, (name, E) in enumerate((("eT2", E4[2]), ("eTinv2", E4[3]))):
            fx, fy, fd, fa = factors(f)[0][k]
            assert E[0, 0] > 0
            res = residuals(E, fx, fy, fd, fa)
            kr = kron_gate_residual(E)
            print("t = %g tp = %g mu = %g dtau = %g %s: %s ulp; Kronecker gate %.3g ulp"
                  % (t, tp, mu, dtau, name, ", ".join("%.1f" % (r / EPS) for r in res), kr / EPS))
            assert max(res) <= GATE, res
            assert kr > GATE  # the two-factor path cannot take these matrices
            # the transposed factors of the daggered products and the wraps' right products, in the kernel's two orders
            for P in orders(fx.T, fy.T, fd.T, fa.T)[1:3]:
                assert np.abs(E.T - P).max() / np.abs(E).max() <= GATE


def test_tp_zero_matrices_pass_the_kronecker_gate(mc_amd):
    E = mc_amd.hopping_exponentials(model_of(mc_amd, 1.0, 0.0, -0.4).hopping_matrix()[0], 0.1)
    assert kron_gate_residual(E[2]) <= GATE and kron_gate_residual(E[3]) <= GATE


def test_one_perturbed_bond_and_another_tp_fail_the_gate(mc_amd):
    t, tp, mu, dtau = SETS[1]
    model = model_of(mc_amd, t, tp, mu)
    f = factors(mc_amd.square_tp_factors(model, dtau))[0]
    T = model.hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2  # one bond with t != 1
    for k, E in enumerate(mc_amd.hopping_exponentials(T, dtau)[2:]):
        assert min(residuals(E, *f[k])) > 100 * GATE
    wrong = factors(mc_amd.square_tp_factors(model_of(mc_amd, t, -0.3, mu), dtau))[0]
    for k, E in enumerate(mc_amd.hopping_exponentials(model.hopping_matrix()[0], dtau)[2:]):
        assert min(residuals(E, *wrong[k])) > 100 * GATE
    # and the triangular three-factor form (one diagonal only) is another matrix
    tri = mc_amd.HubbardModelAttractive(l=mc_amd.TriangularLattice(16), mu=mu)
    for k, E in enumerate(mc_amd.hopping_exponentials(tri.hopping_matrix()[0], dtau)[2:]):
        assert min(residuals(E, *f[k])) > 100 * GATE


# ---- register-level replay of ttp_chain_kernel (one wave, one column tile)
def tile_write(p):
    """product_to(): the accumulator tile as [row][lane], row stride 17"""
    t = np.zeros((16, 17))
    for r in range(4):
        t[G + 4 * r, CI] = p[:, r]
    return t


def step(v, par, fx, fy, fd, fa):
    """one step on one column tile, as the kernel orders it: f1, pass to S, Fd, pass to R, Fa, pass to B / A, f4"""
    f1, f4 = (fx, fy) if par else (fy, fx)
    t1 = tile_write(product(f1, v))
    w = np.zeros_like(v)
    for r in range(4):
        y = G + 4 * r
        x = (CI + y) & 15
        w[:, r] = t1[x, y] if par else t1[y, x]
    t2 = tile_write(product(fd, w))
    for r in range(4):
        y = G + 4 * r
        w[:, r] = t2[y, (CI - 2 * y) & 15]
    t1 = tile_write(product(fa, w))  # (the first pass's region again)
    for r in range(4):
        k = G + 4 * r
        w[:, r] = t1[k, (k + CI) & 15] if par else t1[CI, (k + CI) & 15]
    return product(f4, w)


def load(X, par=0):
    v = np.zeros((64, 4))
    for r in range(4):
        v[:, r] = X[idx(par, r)]
    return v


def store(v, par):
    out = np.zeros(256)
    for r in range(4):
        out[idx(par, r)] = v[:, r]
    return out


def circulant(rng):
    c = rng.standard_normal(L)
    return np.array([[c[(i - j) % L] for j in range(L)] for i in range(L)])


@pytest.mark.parametrize("transposed", [False, True])
def test_kernel_step_order_reproduces_the_product(transposed):
    """two steps (state A -> B -> A) on random factors that commute like the lattice's (circulants): E X and E' X"""
    rng = np.random.default_rng(11)
    fx, fy, fd, fa = (circulant(rng) for _ in range(4))
    E = np.kron(fy, fx) @ diag_op(fd) @ anti_op(fa)
    if transposed:
        fx, fy, fd, fa, E = fx.T, fy.T, fd.T, fa.T, E.T
    X = rng.standard_normal(256)
    v = step(load(X), 0, fx, fy, fd, fa)
    ref = E @ X
    assert np.abs(store(v, 1) - ref).max() < 1e-12 * np.abs(ref).max()
    v = step(v, 1, fx, fy, fd, fa)
    ref = E @ ref
    assert np.abs(store(v, 0) - ref).max() < 1e-12 * np.abs(ref).max()


def test_each_pass_lands_in_its_state():
    """pass by pass with non-commuting random factors: after each product the tile holds the partial product in the
    state the layout names (A: (y, x), S: (y, u), R: (y, w), B: (x, y))"""
    rng = np.random.default_rng(5)
    fx, fy, fd, fa = (rng.standard_normal((L, L)) for _ in range(4))
    Ed, Ea, Kx, Ky = diag_op(fd), anti_op(fa), np.kron(np.eye(L), fx), np.kron(fy, np.eye(L))
    X = rng.standard_normal(256)
    for par, (K1, K4) in enumerate(((Ky, Kx), (Kx, Ky))):
        f1, f4 = (fx, fy) if par else (fy, fx)
        v = load(X, par)
        p1 = product(f1, v)
        assert np.abs(store(p1, par) - K1 @ X).max() < 1e-12
        t1 = tile_write(p1)
        w = np.zeros_like(v)
        xs = np.zeros((64, 4), dtype=np.int64)
        for r in range(4):
            y = G + 4 * r
            xs[:, r] = (CI + y) & 15
            w[:, r] = t1[xs[:, r], y] if par else t1[y, xs[:, r]]
        ref = K1 @ X
        for r in range(4):  # state S: (y, u) at x = u + y
            assert np.abs(w[:, r] - ref[xs[:, r] + 16 * (G + 4 * r)]).max() < 1e-12
        p2 = product(fd, w)
        ref = Ed @ ref
        for r in range(4):
            assert np.abs(p2[:, r] - ref[xs[:, r] + 16 * (G + 4 * r)]).max() < 1e-12
        t2 = tile_write(p2)
        for r in range(4):  # state R: (y, w) at x = w - y
            y = G + 4 * r
            w[:, r] = t2[y, (CI - 2 * y) & 15]
            assert np.abs(w[:, r] - ref[((CI - y) & 15) + 16 * y]).max() < 1e-12
        p3 = product(fa, w)
        ref = Ea @ ref
        for r in range(4):
            y = G + 4 * r
            assert np.abs(p3[:, r] - ref[((CI - y) & 15) + 16 * y]).max() < 1e-11
        assert np.abs(store(step(load(X, par), par, fx, fy, fd, fa), par ^ 1) - K4 @ ref).max() < 1e-10


def conf_scale(c, sign, bn, epl, eml):
    """fk_conf() of factored_common.h"""
    return np.where(((c > 0) == (sign > 0)) != bn, epl, eml)


def chain(X0, nb, blk, ax, ay, steps, conf, epl, eml):
    """the kernel's step loop on one column of block blk: the operands of step s from the buffers ax / ay as request()
    indexes them (block b at + 256 b, Fd at ay + 256 (nb + b), Fa at ay + 256 (2 nb + b)), the scalings as fk_conf()"""
    mat = lambda buf, off: buf[off:off + 256].reshape(16, 16, order="F")
    v = load(X0)
    for s, (pre, post) in enumerate(steps):
        par = s & 1
        fx, fy = mat(ax, 256 * blk), mat(ay, 256 * blk)
        fd, fa = mat(ay, 256 * (nb + blk)), mat(ay, 256 * (2 * nb + blk))
        if pre is not None:
            for r in range(4):
                v[:, r] *= conf_scale(conf[pre[0]][idx(par, r)], pre[1], blk != 0, epl, eml)
        v = step(v, par, fx, fy, fd, fa)
        if post is not None:
            for r in range(4):
                v[:, r] *= conf_scale(conf[post[0]][idx(par ^ 1, r)], post[1], blk != 0, epl, eml)
    return store(v, len(steps) & 1)


@pytest.mark.parametrize("nb", [1, 2])
def test_two_step_chain_with_scalings_and_blocks(nb):
    """post_2 (.) E (pre_2 (.) (post_1 (.) E (pre_1 (.) X))) with the factors of every block at its offset"""
    rng = np.random.default_rng(23)
    F = [[circulant(rng) for _ in range(4)] for _ in range(nb)]  # [block] -> Fx, Fy, Fd, Fa
    ax = np.concatenate([F[b][0].reshape(-1, order="F") for b in range(nb)])
    ay = np.concatenate([F[b][j].reshape(-1, order="F") for j in (1, 2, 3) for b in range(nb)])
    conf = rng.integers(0, 2, size=(3, 256)) * 2 - 1
    lam = 0.37
    epl, eml = np.exp(lam), np.exp(-lam)
    steps = [((0, +1), (1, -1)), ((2, -1), (0, +1))]
    X = rng.standard_normal(256)
    for blk in range(nb):
        fx, fy, fd, fa = F[blk]
        E = np.kron(fy, fx) @ diag_op(fd) @ anti_op(fa)
        sg = -1.0 if blk else 1.0  # block 1 of the repulsive model sees the field with the other sign
        ref = X.copy()
        for pre, post in steps:
            ref = np.exp(sg * post[1] * lam * conf[post[0]]) * (E @ (np.exp(sg * pre[1] * lam * conf[pre[0]]) * ref))
        got = chain(X, nb, blk, ax, ay, steps, conf, epl, eml)
        assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()
    if nb == 2:  # the blocks' factors differ, so a wrong offset shows
        assert np.abs(chain(X, nb, 0, ax, ay, steps, conf, epl, eml) - chain(X, nb, 1, ax, ay, steps, conf, epl, eml)).max() > 1e-3


def test_kernel_step_order_with_the_lattice_factors(mc_amd):
    """the same replay with the factors of eT2 at t' = -0.25, mu = -0.8: E X and then E E X within the gate's rounding"""
    t, tp, mu, dtau = SETS[1]
    model = model_of(mc_amd, t, tp, mu)
    fx, fy, fd, fa = factors(mc_amd.square_tp_factors(model, dtau))[0][0]
    E = mc_amd.hopping_exponentials(model.hopping_matrix()[0], dtau)[2]
    X = np.random.default_rng(3).standard_normal(256)
    v = step(load(X), 0, fx, fy, fd, fa)
    assert np.abs(store(v, 1) - E @ X).max() < 1e-12 * np.abs(E @ X).max()
    v = step(v, 1, fx, fy, fd, fa)
    assert np.abs(store(v, 0) - E @ E @ X).max() < 1e-12 * np.abs(E @ E @ X).max()


# ---- checkpoint preamble and the helpers that refuse tp != 0 (host level: no handle is created)
def test_checkpoint_model_entry(mc_amd):
    D = mc_amd.DQMC
    m0 = mc_amd.HubbardModelRepulsive(4, 2, U=4.0, mu=-0.4)
    assert D._model_entry(m0) == {"class": "HubbardModelRepulsive", "U": 4.0, "t": 1.0, "mu": -0.4}
    assert "tp" not in D._model_entry(mc_amd.HubbardModelAttractive(4, 2, tp=0.0))
    assert D._model_entry(mc_amd.HubbardModelRepulsive(4, 2)) == {"class": "HubbardModelRepulsive", "U": 1.0, "t": 1.0}
    for cls in (mc_amd.HubbardModelAttractive, mc_amd.HubbardModelRepulsive):
        m = cls(4, 2, U=4.0, mu=-0.4, tp=-0.25)
        e = D._model_entry(m)
        assert e["tp"] == -0.25
        back = D._model_from_entry(e, mc_amd.SquareLattice(4))
        assert type(back) is cls and (back.U, back.t, back.mu, back.tp) == (4.0, 1.0, -0.4, -0.25)
        assert np.array_equal(back.hopping_matrix()[0], m.hopping_matrix()[0])
        assert e == D._model_entry(m)  # (the entry was not consumed)
    # an entry written before tp existed
    old = D._model_from_entry({"class": "HubbardModelAttractive", "U": 2.0, "t": 1.0, "mu": 0.5}, mc_amd.SquareLattice(4))
    assert old.tp == 0.0 and old.mu == 0.5


@pytest.mark.parametrize("call", [lambda mc: mc.superfluid_stiffness(), lambda mc: mc.superfluid_stiffness(axis=1),
                                  lambda mc: mc.drude_weight(), lambda mc: mc.dc_conductivity()])
def test_stiffness_helpers_refuse_tp(mc_amd, call):
    """the guard stands in front of everything that touches the device, so an object without a handle reaches it"""
    mc = object.__new__(mc_amd.DQMC)
    mc._h = None
    mc.model = mc_amd.HubbardModelRepulsive(4, 2, tp=-0.25)
    with pytest.raises(NotImplementedError, match="diagonal bonds"):
        call(mc)
    mc.model = mc_amd.HubbardModelRepulsive(4, 2)
    mc._dirs = mc._mom = None
    with pytest.raises(Exception) as ei:  # tp = 0: past the guard, to the first thing the helper needs
        call(mc)
    assert not isinstance(ei.value, NotImplementedError)
