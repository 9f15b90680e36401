"""BilayerSquareLattice(L) on the host: the tables against a brute-force construction from coordinates, the direction
folding on the torus Z_L x Z_L x Z_2, the quad iterators, the momentum grid with q_z = 0 / pi, the models' t_perp, the
pair channels, and the factored form Ez (x) Ey (x) Ex of the hopping exponentials at 16 x 16 x 2 that bilayer.hip applies
(the gate is kron_split in hopping_forms.h, restated here in numpy, and the kernel's step order, restated lane by lane: no
GPU is needed)."""
import itertools

import numpy as np
import pytest

EPS = np.finfo(float).eps
GATE = 256 * EPS


def site(x, y, z, L):
    return 1 + x % L + L * (y % L) + L * L * (z % 2)


def brute_tables(L):
    """neighs (5 rows) and bonds from the coordinates alone: up = x + 1, right = y + 1, down, left, perp = other layer"""
    n = 2 * L * L
    neighs = np.zeros((5, n), dtype=np.int64)
    bonds = []
    for z in range(2):
        for y in range(L):
            for x in range(L):
                s = site(x, y, z, L)
                neighs[:, s - 1] = (site(x + 1, y, z, L), site(x, y + 1, z, L), site(x - 1, y, z, L), site(x, y - 1, z, L),
                                    site(x, y, z + 1, L))
    for s in range(1, n + 1):
        bonds.append((s, neighs[0, s - 1], 0))
        bonds.append((s, neighs[1, s - 1], 0))
        if s <= L * L:
            bonds.append((s, neighs[4, s - 1], 0))
    return neighs, np.array(bonds, dtype=np.int64)


@pytest.mark.parametrize("L", [2, 3, 4])
def test_tables_match_the_brute_force_construction(mc_amd, L):
    l = mc_amd.BilayerSquareLattice(L)
    neighs, bonds = brute_tables(L)
    assert len(l) == l.sites == 2 * L * L and l.lattice.shape == (L, L, 2)
    assert l.lattice[1, L - 1, 1] == site(1, L - 1, 1, L)  # 1 + x + L y + L^2 z, column-major
    assert l.neighs.shape == (5, 2 * L * L) and np.array_equal(l.neighs, neighs)
    assert l.n_bonds == 5 * L * L and np.array_equal(l.bonds, bonds)
    # the in-plane rows are SquareLattice's, per layer
    sq = mc_amd.SquareLattice(L)
    for z in range(2):
        assert np.array_equal(l.neighs[:4, z * L * L:(z + 1) * L * L], sq.neighs + z * L * L)
    # every physical bond once: the undirected bonds, doubled, are the directed neighbour list (at L = 2 the periodic
    # in-plane bond pairs coincide, as on SquareLattice(2); the perp bonds never do)
    directed = l.neighbors(True)
    assert len(directed) == 5 * len(l)
    reduced = l.neighbors(False)
    assert sorted(reduced + [(t, s) for s, t in reduced]) == sorted(directed)
    perp = [(s, t) for s, t in reduced if abs(s - t) == L * L and (s - 1) // (L * L) != (t - 1) // (L * L)]
    assert len(perp) == L * L and len(set(perp)) == L * L
    assert not isinstance(l, mc_amd.SquareLattice)


@pytest.mark.parametrize("L", [2, 3, 4])
def test_directions_fold_to_one_per_site(mc_amd, L):
    """z = +1 and z = -1 are the same displacement on the two-layer torus: one direction per in-plane offset and layer
    difference, n_dirs == n_sites, every direction holding every source once"""
    l = mc_amd.BilayerSquareLattice(L)
    it = mc_amd.EachSitePairByDistance(l)
    assert it.ndirections() == l.sites
    assert all(len(p) == l.sites and len(set(s for s, _ in p)) == l.sites for p in it.pairs)
    zs = sorted(set(round(float(d[2])) for d in it.directions))
    assert len(zs) == 2 and zs[0] * zs[1] == 0 and abs(zs[0] + zs[1]) == 1  # one image of the interlayer step, not both
    norms = [np.linalg.norm(d) for d in it.directions]
    assert norms == sorted(norms) and norms[0] == 0
    lat = mc_amd.lattices
    assert [tuple(p) for p in lat._positions(l)] == [(i + 1.0, j + 1.0, k + 1.0) for k in range(2) for j in range(L)
                                                     for i in range(L)]
    assert [tuple(v) for v in lat._lattice_vectors(l)] == [(L, 0, 0), (0, L, 0), (0, 0, 2)]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_quad_iterators_build_with_the_default_k(mc_amd, L):
    l = mc_amd.BilayerSquareLattice(L)
    for cls in (mc_amd.EachLocalQuadByDistance, mc_amd.EachLocalQuadBySyncedDistance):
        q = cls(l)
        assert q.K == 6 and q.trg_of.shape == (l.sites, 6)
        assert (q.trg_of >= 0).all()  # no site without a target: a Bravais lattice
    if L > 2:  # the five nearest neighbours of site 1 are its targets in directions 1 .. 5
        q = mc_amd.EachLocalQuadByDistance(l)
        assert q.trg_of[0, 0] == 0 and set(q.trg_of[0, 1:]) == set(int(t) - 1 for t in l.neighs[:, 0])


def test_momentum_grid_has_bonding_and_antibonding_labels(mc_amd):
    L = 4
    l = mc_amd.BilayerSquareLattice(L)
    q, labels = mc_amd.momentum_grid(l)
    assert q.shape == (32, 3) and labels.shape == (32, 3)
    want = [(a, b, c) for c in range(2) for b in range(L) for a in range(L)]  # the first label fastest
    assert [tuple(m) for m in labels] == want
    assert np.allclose(q, np.array(want) * np.array([2 * np.pi / L, 2 * np.pi / L, np.pi]))
    assert any(np.allclose(v, [np.pi, np.pi, np.pi]) for v in q)
    # the plane waves of the grid are orthogonal characters of the torus
    pos = np.array(mc_amd.lattices._positions(l))
    F = np.exp(1j * pos @ q.T)
    assert np.allclose(F.conj().T @ F, 32 * np.eye(32))


def test_strip_subsystem_accepts_the_lattice(mc_amd):
    l = mc_amd.BilayerSquareLattice(4)
    strip = mc_amd.strip_subsystem
    assert strip(l, 1, axis=2).tolist() == list(range(16))  # one layer
    assert strip(l, 2, axis=0).tolist() == sorted(site(x, y, z, 4) - 1 for x in range(2) for y in range(4) for z in range(2))
    with pytest.raises(ValueError):
        strip(l, 3, axis=2)


def ring(L):
    C = np.zeros((L, L))
    for i in range(L):
        C[(i + 1) % L, i] += 1.0
        C[(i - 1) % L, i] += 1.0
    return C


def kron_sum_hopping(L, t, t_perp, mu):
    """T = -t (I2 (x) I (x) C + I2 (x) C (x) I) - t_perp (X (x) I (x) I) - mu, site x + L y + L^2 z"""
    I, C, X = np.eye(L), ring(L), np.array([[0.0, 1.0], [1.0, 0.0]])
    return (-t * (np.kron(np.eye(2), np.kron(I, C)) + np.kron(np.eye(2), np.kron(C, I))) - t_perp * np.kron(X, np.kron(I, I))
            - mu * np.eye(2 * L * L))


@pytest.mark.parametrize("L", [2, 3, 4])
def test_hopping_matrix_is_the_kronecker_sum(mc_amd, L):
    l = mc_amd.BilayerSquareLattice(L)
    m = mc_amd.HubbardModelAttractive(l=l, t=0.9, t_perp=2.5, mu=-0.3)
    assert m.t_perp == 2.5
    assert np.array_equal(m.hopping_matrix()[0], kron_sum_hopping(L, 0.9, 2.5, -0.3))
    r = mc_amd.HubbardModelRepulsive(l=l, t=1.1, mu=0.2)  # t_perp = None: t
    assert r.t_perp == 1.1
    Ts = r.hopping_matrix()
    assert len(Ts) == 2 and all(np.array_equal(T, kron_sum_hopping(L, 1.1, 1.1, 0.2)) for T in Ts)
    assert isinstance(mc_amd.HubbardModel(l=l, U=-2.0, t_perp=0.5), mc_amd.HubbardModelAttractive)
    assert mc_amd.HubbardModel(l=l, U=2.0, t_perp=0.5).t_perp == 0.5


def test_model_errors(mc_amd):
    for cls in (mc_amd.HubbardModelAttractive, mc_amd.HubbardModelRepulsive):
        with pytest.raises(ValueError, match="t_perp"):
            cls(4, 2, t_perp=1.0)
        with pytest.raises(ValueError, match="t_perp"):
            cls(l=mc_amd.CubicLattice(3, 2), t_perp=0.0)
        with pytest.raises(ValueError, match="tp"):
            cls(l=mc_amd.BilayerSquareLattice(4), tp=-0.2)
        assert cls(4, 2).t_perp is None  # every other lattice: no such hopping


def test_other_models_keep_their_matrices(mc_amd):
    """the matrices of the lattices that were there, restated as they were built before t_perp"""
    for model in (mc_amd.HubbardModelAttractive(4, 2, mu=0.3, t=0.7), mc_amd.HubbardModelRepulsive(3, 3, mu=-0.2),
                  mc_amd.HubbardModelAttractive(2, 2), mc_amd.HubbardModelRepulsive(l=mc_amd.TriangularLattice(4)),
                  mc_amd.HubbardModelAttractive(l=mc_amd.SquareLattice(4), tp=-0.25)):
        N = len(model.l)
        T = np.diag(np.full(N, -model.mu)) if model.flv == 1 else np.zeros((N, N))
        if model.flv == 2 and model.mu != 0.0:
            T[np.diag_indices(N)] = -model.mu
        for src, trg in model.l.neighbors(True):
            T[trg - 1, src - 1] += -model.t
        if model.tp != 0.0:
            for src, trg in model.l.next_neighbors(True):
                T[trg - 1, src - 1] += -model.tp
        for got in model.hopping_matrix():
            assert np.array_equal(got, T)


def test_default_pair_channels(mc_amd):
    l = mc_amd.BilayerSquareLattice(4)
    it = mc_amd.EachSitePairByDistance(l)
    ch = mc_amd.lattices.default_pair_channels(l, it.directions, 6)
    assert list(ch) == ["s", "s*", "d", "s_perp"]
    d = np.array(it.directions[:6])
    inplane = [k for k in range(1, 6) if d[k, 2] == 0]
    perp = [k for k in range(1, 6) if d[k, 2] != 0]
    assert len(inplane) == 4 and len(perp) == 1
    assert ch["s"].tolist() == [1, 0, 0, 0, 0, 0]
    assert all(ch["s*"][k] == 0.5 for k in inplane) and ch["s*"][perp[0]] == 0 and ch["s*"][0] == 0
    assert all(ch["d"][k] == (0.5 if d[k, 0] != 0 else -0.5) for k in inplane) and ch["d"][perp[0]] == 0
    assert ch["s_perp"].tolist() == [1.0 if k == perp[0] else 0.0 for k in range(6)]
    with pytest.raises(ValueError):
        mc_amd.lattices.default_pair_channels(l, it.directions, 5)


# ---- the factored form at 16 x 16 x 2
def bilayer_factor(E):
    """engine.cpp bilayer_factor: Ex = E[0:16, 0:16], Ey = E[0::16, 0::16][:16, :16] / E00, Ez = E[0::256, 0::256] / E00;
    (Ex, Ey, Ez, residual / max|E|)"""
    assert E.shape == (512, 512) and E[0, 0] > 0
    ex = E[:16, :16].copy()
    ey = E[0::16, 0::16][:16, :16] / E[0, 0]
    ez = E[0::256, 0::256] / E[0, 0]
    return ex, ey, ez, np.abs(E - np.kron(ez, np.kron(ey, ex))).max() / np.abs(E).max()


def test_bilayer_exponentials_pass_the_gate(mc_amd):
    """t_perp in {0.3, 1, 3.5} x mu in {0, -0.8} x dtau in {0.05, 0.1, 0.125}, eT2 and eTinv2: the residual of the engine's
    extraction rule in units of eps max|E|.  Measured worst value: 34.9: the 256-ulp rule of the other
    factored forms holds with the same margin."""
    l = mc_amd.BilayerSquareLattice(16)
    worst = 0.0
    for t_perp, mu, dtau in itertools.product((0.3, 1.0, 3.5), (0.0, -0.8), (0.05, 0.1, 0.125)):
        T = mc_amd.HubbardModelAttractive(l=l, t_perp=t_perp, mu=mu).hopping_matrix()[0]
        for name, E in zip(("eT2", "eTinv2"), mc_amd.dqmc.hopping_exponentials(T, dtau)[2:]):
            ex, ey, ez, res = bilayer_factor(E)
            assert ez.shape == (2, 2)
            worst = max(worst, res / EPS)
            assert res <= GATE, (t_perp, mu, dtau, name, res / EPS)
            # the transposed factors of the daggered products and the wrap's right products: the same residual
            assert np.abs(E.T - np.kron(ez.T, np.kron(ey.T, ex.T))).max() / np.abs(E).max() <= GATE
    print("worst max|E - Ez (x) Ey (x) Ex| / (eps max|E|) over the grid: %.1f" % worst)
    assert worst < 256


def test_other_n512_hoppings_fail_the_gate(mc_amd):
    """one bond at 1.2 t, and the 8 x 8 x 8 cubic lattice (which keeps kron3.hip: its own gate is tried first)"""
    l = mc_amd.BilayerSquareLattice(16)
    T = mc_amd.HubbardModelAttractive(l=l, t_perp=1.3).hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2
    for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
        assert bilayer_factor(E)[3] > 100 * GATE
    T = mc_amd.HubbardModelAttractive(8, 3).hopping_matrix()[0]
    for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
        assert bilayer_factor(E)[3] > 100 * GATE


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
    """one wave's two columns (four plane tiles) through two steps of bilayer_chain_kernel, in the order it works: the
    first scaling, the layer mix in registers, P = Fa V, the 16 x 17 LDS transpose, Q = Fb P^T, the second scaling; then
    the staging image of a transposed store with its padded stride"""
    rng = np.random.default_rng(7)
    ex, ey = rng.standard_normal((16, 16)), rng.standard_normal((16, 16))
    ez = rng.standard_normal((2, 2))
    pre, post = rng.standard_normal(512), rng.standard_normal(512)
    X = rng.standard_normal((512, 2))
    A = np.kron(ez, np.kron(ey, ex))
    lanes = np.arange(64)
    g, c = lanes >> 4, lanes & 15

    def idx(par, r):
        return (g + 4 * r) + 16 * c if par else c + 16 * (g + 4 * r)

    def operand(F):  # lane: F[row ci][k = 4 q + g] of the column-major factor
        return [F[c, 4 * q + g] for q in range(4)]

    v = np.zeros((4, 64, 4))  # [tile t = 2 h + z][lane][register r]
    for t in range(4):
        for r in range(4):
            v[t, :, r] = X[256 * (t & 1) + idx(0, r), t >> 1]

    def step(v, par):
        fa, fb = (ex, ey) if par else (ey, ex)
        v = v.copy()
        for t in range(4):
            for r in range(4):
                v[t, :, r] *= pre[256 * (t & 1) + idx(par, r)]
        for h in range(2):
            p0, p1 = v[2 * h].copy(), v[2 * h + 1].copy()
            v[2 * h] = ez[0, 0] * p0 + ez[0, 1] * p1
            v[2 * h + 1] = ez[1, 0] * p0 + ez[1, 1] * p1
        out = np.zeros_like(v)
        for t in range(4):
            p = np.zeros((64, 4))
            for q, a in enumerate(operand(fa)):
                p = mfma(a, v[t, :, q], p)
            tile = np.zeros((16, 17))
            for r in range(4):
                tile[g + 4 * r, c] = p[:, r]
            q4 = np.zeros((64, 4))
            for q, b in enumerate(operand(fb)):
                q4 = mfma(b, tile[c, 4 * q + g], q4)
            out[t] = q4
        for t in range(4):
            for r in range(4):
                out[t, :, r] *= post[256 * (t & 1) + idx(par ^ 1, r)]
        return out

    def unpack(v, par):
        got = np.zeros((512, 2))
        for t in range(4):
            for r in range(4):
                got[256 * (t & 1) + idx(par, r), t >> 1] = v[t, :, r]
        return got

    ref1 = post[:, None] * (A @ (pre[:, None] * X))
    v = step(v, 0)
    assert np.abs(unpack(v, 1) - ref1).max() < 1e-12 * np.abs(ref1).max()
    # the transposed staging image after an odd number of steps: entry e, column cl at 10 e + 2 (e >> 4) + cl, every
    # address written once, and read back as rows of 8 columns
    addr = set()
    img = np.full(512 * 10 + 32 * 2, np.nan)
    for t in range(4):
        for r in range(4):
            e = 256 * (t & 1) + idx(1, r)
            a = 10 * e + 2 * (e >> 4) + (t >> 1)
            assert not addr & set(a.tolist()) and a.max() < img.size
            addr |= set(a.tolist())
            img[a] = v[t, :, r]
    for e in range(512):
        assert np.array_equal(img[10 * e + 2 * (e >> 4):10 * e + 2 * (e >> 4) + 2], unpack(v, 1)[e])
    ref2 = post[:, None] * (A @ (pre[:, None] * ref1))
    v = step(v, 1)
    assert np.abs(unpack(v, 0) - ref2).max() < 1e-12 * np.abs(ref2).max()
