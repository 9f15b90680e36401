"""RectangularLattice(Lx, Ly) on the host: the tables against a construction from coordinates and against SquareLattice(L)
at Lx = Ly = L, the hopping matrix as a Kronecker sum (with mu and t'), the iterators, the momentum grid, the pair channels,
the errors, and the factored form Ey (x) Ex of unequal factors at 32 x 8 that rect.hip applies (the gate is kron_split in
hopping_forms.h, restated here in numpy, and the kernel's two step forms and staging addresses, restated lane by lane: no GPU is
needed)."""
import itertools

import numpy as np
import pytest

EPS = np.finfo(float).eps
GATE = 256 * EPS
SHAPES = [(2, 3), (3, 2), (4, 3), (5, 2), (6, 4)]


def site(x, y, Lx, Ly):
    return 1 + x % Lx + Lx * (y % Ly)


def brute_tables(Lx, Ly):
    """neighs, nnn and bonds from the coordinates alone: up = x + 1, right = y + 1, down, left; upright = (x + 1, y + 1),
    downright = (x - 1, y + 1), downleft, upleft"""
    n = Lx * Ly
    neighs, nnn = np.zeros((4, n), dtype=np.int64), np.zeros((4, n), dtype=np.int64)
    for y in range(Ly):
        for x in range(Lx):
            s = site(x, y, Lx, Ly) - 1
            neighs[:, s] = [site(x + dx, y + dy, Lx, Ly) for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1))]
            nnn[:, s] = [site(x + dx, y + dy, Lx, Ly) for dx, dy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    bonds = []
    for s in range(1, n + 1):
        bonds += [(s, neighs[0, s - 1], 0), (s, neighs[1, s - 1], 0)]
    return neighs, nnn, np.array(bonds, dtype=np.int64)


@pytest.mark.parametrize("Lx,Ly", SHAPES)
def test_tables_match_the_construction_from_coordinates(mc_amd, Lx, Ly):
    l = mc_amd.RectangularLattice(Lx, Ly)
    neighs, nnn, bonds = brute_tables(Lx, Ly)
    assert (l.Lx, l.Ly) == (Lx, Ly) and len(l) == l.sites == Lx * Ly and l.lattice.shape == (Lx, Ly)
    assert l.lattice[Lx - 1, 1] == site(Lx - 1, 1, Lx, Ly)  # 1 + x + Lx y, column-major
    assert np.array_equal(l.neighs, neighs) and np.array_equal(l.nnn, nnn)
    assert l.n_bonds == 2 * Lx * Ly and np.array_equal(l.bonds, bonds)
    directed, reduced = l.neighbors(True), l.neighbors(False)
    assert len(directed) == 4 * len(l)
    assert sorted(reduced + [(t, s) for s, t in reduced]) == sorted(directed)  # (a length-2 axis: the pair stands twice)
    assert l.next_neighbors(True) == [(s + 1, int(t)) for s in range(len(l)) for t in nnn[:, s]]
    assert l.next_neighbors(False) == [(s + 1, int(t)) for s in range(len(l)) for t in nnn[:2, s]]
    assert not isinstance(l, mc_amd.SquareLattice) and not hasattr(l, "L")


@pytest.mark.parametrize("L", [2, 3, 4])
def test_equal_lengths_give_the_square_lattice(mc_amd, L):
    lat = mc_amd.lattices
    r, s = mc_amd.RectangularLattice(L, L), mc_amd.SquareLattice(L)
    for name in ("neighs", "nnn", "bonds", "lattice"):
        assert np.array_equal(getattr(r, name), getattr(s, name)), name
    assert r.neighbors(True) == s.neighbors(True) and r.next_neighbors(False) == s.next_neighbors(False)
    assert np.array_equal(np.array(lat._positions(r)), np.array(lat._positions(s)))
    assert np.array_equal(np.array(lat._lattice_vectors(r)), np.array(lat._lattice_vectors(s)))
    ir, is_ = mc_amd.EachSitePairByDistance(r), mc_amd.EachSitePairByDistance(s)
    assert np.array_equal(np.array(ir.directions), np.array(is_.directions))
    assert ir.pairs == is_.pairs and np.array_equal(ir.dir_of, is_.dir_of)
    for cls in (mc_amd.EachLocalQuadByDistance, mc_amd.EachLocalQuadBySyncedDistance):
        if L > 2:
            qr, qs = cls(r, pairs=ir), cls(s, pairs=is_)
            assert qr.K == qs.K == 5 and np.array_equal(qr.trg_of, qs.trg_of) and len(qr) == len(qs)
    (qa, la), (qb, lb) = mc_amd.momentum_grid(r), mc_amd.momentum_grid(s)
    assert np.array_equal(qa, qb) and np.array_equal(la, lb)
    assert mc_amd.build_checkerboard(r)[2] == mc_amd.build_checkerboard(s)[2]
    assert np.array_equal(mc_amd.build_checkerboard(r)[0], mc_amd.build_checkerboard(s)[0])
    assert np.array_equal(mc_amd.greedy_colouring(r), mc_amd.greedy_colouring(s))
    if L > 2:  # (at L = 2 the four neighbours are two directions: no d channel on either class)
        cr, cs = lat.default_pair_channels(r, ir.directions, 5), lat.default_pair_channels(s, is_.directions, 5)
        assert list(cr) == list(cs) and all(np.array_equal(cr[k], cs[k]) for k in cr)


def ring(L):
    C = np.zeros((L, L))
    for i in range(L):
        C[(i + 1) % L, i] += 1.0
        C[(i - 1) % L, i] += 1.0
    return C


def kron_sum_hopping(Lx, Ly, t, mu, tp=0.0):
    """T = -mu I - t (I_Ly (x) Cx + Cy (x) I_Lx) - t' Cy (x) Cx, site x + Lx y"""
    Cx, Cy = ring(Lx), ring(Ly)
    return -mu * np.eye(Lx * Ly) - t * (np.kron(np.eye(Ly), Cx) + np.kron(Cy, np.eye(Lx))) - tp * np.kron(Cy, Cx)


@pytest.mark.parametrize("Lx,Ly", SHAPES)
def test_hopping_matrix_is_the_kronecker_sum(mc_amd, Lx, Ly):
    l = mc_amd.RectangularLattice(Lx, Ly)
    m = mc_amd.HubbardModelAttractive(l=l, t=0.9, mu=-0.3)
    assert np.array_equal(m.hopping_matrix()[0], kron_sum_hopping(Lx, Ly, 0.9, -0.3))
    r = mc_amd.HubbardModelRepulsive(l=l, t=1.1, mu=0.2, tp=-0.25)
    Ts = r.hopping_matrix()
    assert len(Ts) == 2 and all(np.allclose(T, kron_sum_hopping(Lx, Ly, 1.1, 0.2, -0.25), rtol=0, atol=1e-15) for T in Ts)
    a = mc_amd.HubbardModelAttractive(l=l, tp=0.3)
    assert a.tp == 0.3 and np.allclose(a.hopping_matrix()[0], kron_sum_hopping(Lx, Ly, 1.0, a.mu, 0.3), rtol=0, atol=1e-15)


@pytest.mark.parametrize("Lx,Ly", SHAPES)
def test_iterators_grid_and_helpers(mc_amd, Lx, Ly):
    lat = mc_amd.lattices
    l = mc_amd.RectangularLattice(Lx, Ly)
    n = Lx * Ly
    assert [tuple(p) for p in lat._positions(l)] == [(i + 1.0, j + 1.0) for j in range(Ly) for i in range(Lx)]
    assert [tuple(v) for v in lat._lattice_vectors(l)] == [(Lx, 0), (0, Ly)]
    it = mc_amd.EachSitePairByDistance(l)
    assert it.ndirections() == n  # one target per direction: the fast measurement forms apply
    assert all(len(p) == n and len(set(s for s, _ in p)) == n for p in it.pairs)
    assert lat._default_K(l) == 5
    if min(Lx, Ly) > 2:
        for cls in (mc_amd.EachLocalQuadByDistance, mc_amd.EachLocalQuadBySyncedDistance):
            q = cls(l, pairs=it)
            assert q.K == 5 and q.trg_of.shape == (n, 5) and (q.trg_of >= 0).all()
            assert q.trg_of[0, 0] == 0 and set(q.trg_of[0, 1:]) == set(int(t) - 1 for t in l.neighs[:, 0])
    q, labels = mc_amd.momentum_grid(l)
    want = [(a, b) for b in range(Ly) for a in range(Lx)]  # the first label fastest
    assert [tuple(m) for m in labels] == want
    assert np.allclose(q, np.array(want) * np.array([2 * np.pi / Lx, 2 * np.pi / Ly]), rtol=0, atol=1e-14)
    F = np.exp(1j * np.array(lat._positions(l)) @ q.T)
    assert np.allclose(F.conj().T @ F, n * np.eye(n))
    # strips: up to the length of the chosen axis
    strip = mc_amd.strip_subsystem
    assert strip(l, 1, axis=0).tolist() == sorted(site(0, y, Lx, Ly) - 1 for y in range(Ly))
    assert strip(l, Ly, axis=1).tolist() == list(range(n))
    assert strip(l, Lx, axis=0).tolist() == list(range(n))
    for bad in (dict(width=Lx + 1, axis=0), dict(width=Ly + 1, axis=1), dict(width=0), dict(width=1, axis=2)):
        with pytest.raises(ValueError):
            strip(l, **bad)
    # a proper colouring, and a checkerboard decomposition that uses every bond once
    col = mc_amd.greedy_colouring(l)
    assert all(col[s] != col[t - 1] for s in range(n) for t in l.neighs[:, s])
    if min(Lx, Ly) > 2:
        cb, groups, ng = mc_amd.build_checkerboard(l)
        assert sorted(cb[2]) == list(range(1, l.n_bonds + 1)) and ng == len(groups)
        for gs, ge in groups:
            used = cb[:2, gs - 1:ge].reshape(-1)
            assert len(set(used.tolist())) == used.size


def test_pair_channel_signs(mc_amd):
    """d = +1/2 on the bonds along x, -1/2 on those along y: an exchanged axis shows at Lx != Ly"""
    for Lx, Ly in ((6, 4), (4, 3), (3, 4)):
        l = mc_amd.RectangularLattice(Lx, Ly)
        it = mc_amd.EachSitePairByDistance(l)
        ch = mc_amd.lattices.default_pair_channels(l, it.directions, 5)
        assert list(ch) == ["s", "s*", "d"]
        d = np.array(it.directions[:5])
        assert ch["s"].tolist() == [1, 0, 0, 0, 0] and ch["s*"].tolist() == [0, 0.5, 0.5, 0.5, 0.5]
        for k in range(1, 5):
            assert abs(d[k]).sum() == 1
            assert ch["d"][k] == (0.5 if d[k, 0] != 0 else -0.5)
        assert ch["d"].sum() == 0


def test_errors(mc_amd):
    for bad in ((1, 4), (4, 1), (0, 0)):
        with pytest.raises(ValueError):
            mc_amd.RectangularLattice(*bad)
    l = mc_amd.RectangularLattice(4, 3)
    for cls in (mc_amd.HubbardModelAttractive, mc_amd.HubbardModelRepulsive):
        with pytest.raises(ValueError, match="t_perp"):
            cls(l=l, t_perp=1.0)
        assert cls(l=l).t_perp is None
        with pytest.raises(ValueError, match="tp"):  # the lattices without an nnn table still refuse t'
            cls(l=mc_amd.TriangularLattice(4), tp=-0.2)
    assert mc_amd.DQMC._lattice_args("RectangularLattice") == ("Lx", "Ly")
    assert mc_amd.DQMC._lattice_args("SquareLattice") == ("L",) and mc_amd.DQMC._lattice_args("Nope") is None


def test_ising_model_takes_the_lattice(mc_amd):
    l = mc_amd.RectangularLattice(6, 4)
    m = mc_amd.IsingModel(l=l)
    conf = np.ones(24, dtype=np.int64)
    assert m.energy(conf) == -48.0 and m.propose_local(5, conf) == 8.0


# ---- the factored form at 32 x 8
def rect_factor(E):
    """engine.cpp rect_factor: Ex = E[0:32, 0:32], Ey = E[0::32, 0::32][:8, :8] / E00; (Ex, Ey, residual / max|E|)"""
    assert E.shape == (256, 256) and E[0, 0] > 0
    ex = E[:32, :32].copy()
    ey = E[0::32, 0::32][:8, :8] / E[0, 0]
    return ex, ey, np.abs(E - np.kron(ey, ex)).max() / np.abs(E).max()


def test_rect_exponentials_pass_the_gate(mc_amd):
    """t in {1, 0.7} x mu in {0, -0.8, 0.5} x dtau in {0.05, 0.1, 0.125}, eT2 and eTinv2 of the model's own exponentials:
    the residual of the engine's extraction rule in units of eps max|E|.  Measured worst value: 31.4 (an eigh exponential of the same matrices
    gives 15.3, the model's own exponential differs from it by a few ulp)."""
    l = mc_amd.RectangularLattice(32, 8)
    worst = 0.0
    for t, mu, dtau in itertools.product((1.0, 0.7), (0.0, -0.8, 0.5), (0.05, 0.1, 0.125)):
        T = mc_amd.HubbardModelAttractive(l=l, t=t, mu=mu).hopping_matrix()[0]
        for name, E in zip(("eT2", "eTinv2"), mc_amd.dqmc.hopping_exponentials(T, dtau)[2:]):
            ex, ey, res = rect_factor(E)
            assert ex.shape == (32, 32) and ey.shape == (8, 8)
            worst = max(worst, res / EPS)
            assert res <= GATE, (t, mu, dtau, name, res / EPS)
            assert np.abs(E.T - np.kron(ey.T, ex.T)).max() / np.abs(E).max() <= GATE  # the transposed factors: the same
    print("worst max|E - Ey (x) Ex| / (eps max|E|) over the grid: %.1f" % worst)
    assert worst < 256


def test_other_n256_hoppings_fail_the_gate(mc_amd):
    """8 x 32, 64 x 4 and 16 x 16, 32 x 8 with t' = -0.25, and one changed bond keep the dense path"""
    Ts = [mc_amd.HubbardModelAttractive(l=mc_amd.RectangularLattice(8, 32)).hopping_matrix()[0],
          mc_amd.HubbardModelAttractive(l=mc_amd.RectangularLattice(64, 4)).hopping_matrix()[0],
          mc_amd.HubbardModelAttractive(l=mc_amd.SquareLattice(16)).hopping_matrix()[0],
          mc_amd.HubbardModelAttractive(l=mc_amd.RectangularLattice(32, 8), tp=-0.25).hopping_matrix()[0]]
    T = mc_amd.HubbardModelAttractive(l=mc_amd.RectangularLattice(32, 8)).hopping_matrix()[0]
    T[0, 1] = T[1, 0] = -1.2
    for T in Ts + [T]:
        for E in mc_amd.dqmc.hopping_exponentials(T, 0.1)[2:]:
            assert rect_factor(E)[2] > 100 * GATE


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
    """one wave's two columns (two tiles of the stacked 16 x 32 plane) through two steps of rect_chain_kernel, in the order
    it works.  Even step: the first scaling in layout R, P = Dy Z with Dy = diag(Ey, Ey), the 16 x 36 LDS image, Q^T = Ex
    P^T, the second scaling in layout C.  Odd step: P^T = Ex Z^T from the registers, the same LDS image written
    transposed, Q = Dy P, back in layout R.  Then the staging addresses of a transposed and a plain store.  12 MFMAs per
    column and step are counted."""
    rng = np.random.default_rng(11)
    ex, ey = rng.standard_normal((32, 32)), rng.standard_normal((8, 8))
    pre, post = rng.standard_normal(256), rng.standard_normal(256)
    X = rng.standard_normal((256, 2))
    A = np.kron(ey, ex)
    lanes = np.arange(64)
    g, c = lanes >> 4, lanes & 15
    TLD = 36
    count = [0]

    def idx(par, t, r):
        return (16 * t + g + 4 * r) + 32 * (c & 7) if par else (16 * t + c) + 32 * (g + 4 * (r & 1))

    def col(par, r):
        return c >> 3 if par else np.full(64, r >> 1)

    dy = [np.where((c >> 3) == ((4 * q + g) >> 3), ey[c & 7, (4 * q + g) & 7], 0.0) for q in range(4)]
    exo = [[ex[16 * t + c, 4 * q + g] for q in range(8)] for t in range(2)]

    def mm(a, b, acc):
        count[0] += 1
        return mfma(a, b, acc)

    v = np.zeros((2, 64, 4))  # [tile][lane][register]
    for t in range(2):
        for r in range(4):
            v[t, :, r] = X[idx(0, t, r), r >> 1]

    def step(v, par):
        v = v.copy()
        for t in range(2):
            for r in range(4):
                v[t, :, r] *= pre[idx(par, t, r)]
        tile = np.full(16 * TLD, np.nan)
        out = np.zeros_like(v)
        if not par:
            for t in range(2):
                p = np.zeros((64, 4))
                for q in range(4):
                    p = mm(dy[q], v[t, :, q], p)
                for r in range(4):
                    tile[(g + 4 * r) * TLD + 16 * t + c] = p[:, r]
            for t in range(2):
                q4 = np.zeros((64, 4))
                for q in range(8):
                    q4 = mm(exo[t][q], tile[c * TLD + 4 * q + g], q4)
                out[t] = q4
        else:
            for t in range(2):
                p = np.zeros((64, 4))
                for q in range(8):
                    p = mm(exo[t][q], v[q >> 2, :, q & 3], p)
                for r in range(4):
                    tile[c * TLD + 16 * t + g + 4 * r] = p[:, r]
            for t in range(2):
                q4 = np.zeros((64, 4))
                for q in range(4):
                    q4 = mm(dy[q], tile[(4 * q + g) * TLD + 16 * t + c], q4)
                out[t] = q4
        for t in range(2):
            for r in range(4):
                out[t, :, r] *= post[idx(par ^ 1, t, r)]
        return out

    def unpack(v, par):
        got = np.full((256, 2), np.nan)
        for t in range(2):
            for r in range(4):
                got[idx(par, t, r), col(par, r)] = v[t, :, r]
        return got

    assert np.array_equal(unpack(v, 0), X)  # layout R holds every entry of both columns once
    ref1 = post[:, None] * (A @ (pre[:, None] * X))
    v = step(v, 0)
    assert count[0] == 24  # 12 per column
    assert np.abs(unpack(v, 1) - ref1).max() < 1e-12 * np.abs(ref1).max()
    # the transposed staging image after an odd number of steps (wave w = 1 of 4: columns 2, 3 of the workgroup's 8): entry
    # e, column cl at 10 e + 2 (e >> 4) + cl, every address written once, inside the kernel's LDS, read back as column pairs
    size = 256 * 10 + 16 * 2
    addr, img = set(), np.full(size, np.nan)
    for t in range(2):
        for r in range(4):
            e = idx(1, t, r)
            a = 10 * e + 2 * (e >> 4) + 2 * 1 + col(1, r)
            assert not addr & set(a.tolist()) and a.max() < size
            addr |= set(a.tolist())
            img[a] = v[t, :, r]
    for e in range(256):
        assert np.array_equal(img[10 * e + 2 * (e >> 4) + 2:10 * e + 2 * (e >> 4) + 4], unpack(v, 1)[e])
    # every thread's 16-byte read of the transposed store lies in the image and is aligned
    for k in range(4):
        e2 = 2 * (np.arange(256) + 256 * k)
        a = (e2 >> 3) * 10 + ((e2 >> 3) >> 4) * 2 + (e2 & 7)
        assert (a % 2 == 0).all() and a.max() + 1 < size
    ref2 = post[:, None] * (A @ (pre[:, None] * ref1))
    v = step(v, 1)
    assert count[0] == 48
    assert np.abs(unpack(v, 0) - ref2).max() < 1e-12 * np.abs(ref2).max()
    # the plain staging image after an even number of steps: [column][entry], every address once
    addr = set()
    for t in range(2):
        for r in range(4):
            a = (2 * 1 + col(0, r)) * 256 + idx(0, t, r)
            assert not addr & set(a.tolist()) and a.max() < 8 * 256
            addr |= set(a.tolist())
    assert addr == set(range(2 * 256, 4 * 256))
