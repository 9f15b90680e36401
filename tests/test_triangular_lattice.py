"""TriangularLattice(L; Lx, Ly) (src/lattices/triangular.jl) and the Hubbard models built on it, on the host: a literal
restatement of its tables, the reference's lattice-iterator checks (test/lattices.jl:43-86 on TriangularLattice(0, Lx=2,
Ly=6)), the pair and local-quad iterators, the hopping spectrum and the checkerboard tables."""
import numpy as np
import pytest


def circshift(A, s):
    """Julia circshift: B[i, j] = A[i - s1, j - s2] (periodic)"""
    Lx, Ly = A.shape
    B = np.zeros_like(A)
    for i in range(Lx):
        for j in range(Ly):
            B[i, j] = A[(i - s[0]) % Lx, (j - s[1]) % Ly]
    return B


def tables(Lx, Ly):
    """build_neighbortable / build_ext_neighbortable (triangular.jl:60-99), rows up, upright, right, down, downleft,
    left, each as lattice[:]"""
    lat = np.arange(1, Lx * Ly + 1).reshape((Lx, Ly), order="F")
    out = []
    for k in (1, 2):
        shifts = [(-k, 0), (-k, -k), (0, -k), (k, 0), (k, k), (0, k)]
        out.append(np.array([circshift(lat, s).reshape(-1, order="F") for s in shifts]))
    return lat, out[0], out[1]


@pytest.mark.parametrize("L,Lx,Ly", [(4, 4, 4), (6, 6, 6), (16, 16, 16), (0, 2, 6), (5, 3, 5)])
def test_tables_match_the_literal_restatement(mc_amd, L, Lx, Ly):
    l = mc_amd.TriangularLattice(L, Lx=Lx, Ly=Ly)
    lat, neighs, ext = tables(Lx, Ly)
    assert (l.Lx, l.Ly, l.sites, len(l)) == (Lx, Ly, Lx * Ly, Lx * Ly)
    assert np.array_equal(l.lattice, lat)
    assert l.neighs.shape == (6, Lx * Ly) and np.array_equal(l.neighs, neighs)
    assert np.array_equal(l.ext_neighs, ext)
    assert np.array_equal(l.isAsite, [(i % 2) == 0 for j in range(1, Ly + 1) for i in range(1, Lx + 1)])
    assert l.n_bonds == 6 * Lx * Ly
    want = []
    for src in lat.reshape(-1, order="F"):
        want += [(src, t, 0) for t in neighs[:3, src - 1]] + [(src, t, 0) for t in ext[:3, src - 1]]
    assert np.array_equal(l.bonds, np.array(want))
    # site (i, j) 1-based is i + Lx (j - 1): up is i + 1, right j + 1, upright both
    i, j = 1, Ly
    s = i + Lx * (j - 1)
    site = lambda a, b: 1 + (a - 1) % Lx + Lx * ((b - 1) % Ly)
    assert l.neighs[0, s - 1] == site(i + 1, j)
    assert l.neighs[1, s - 1] == site(i + 1, j + 1)
    assert l.neighs[2, s - 1] == site(i, j + 1)
    assert l.neighs[4, s - 1] == site(i - 1, j - 1)
    assert l.ext_neighs[1, s - 1] == site(i + 2, j + 2)


@pytest.fixture(scope="module")
def ref_lattice(mc_amd):
    """TriangularLattice(0, Lx=2, Ly=6), the lattice of the reference's iterator tests"""
    return mc_amd.TriangularLattice(0, Lx=2, Ly=6)


def test_reference_iterator_checks(mc_amd, ref_lattice):
    l = ref_lattice
    assert len(l) == 12
    for m in (mc_amd.HubbardModelAttractive(l=l), mc_amd.HubbardModelRepulsive(l=l)):
        dirs = mc_amd.EachSitePairByDistance(m.l).directions
        for i in range(1, len(dirs)):
            assert np.linalg.norm(dirs[i - 1]) < np.linalg.norm(dirs[i]) + 1e-5
        # EachSite / EachSiteAndFlavor: 1:N and 1:N*flv (test/lattices.jl:65-86)
        assert len(m.l) == 12 and m.flv * len(m.l) == (12 if m.flv == 1 else 24)
    # Lx = 2: up and down are the same site, which counts twice in the hopping
    T = mc_amd.HubbardModelAttractive(l=l).hopping_matrix()[0]
    assert np.array_equal(l.neighs[0], l.neighs[3]) and not np.array_equal(l.neighs[1], l.neighs[4])
    s, up, ur = 0, l.neighs[0, 0] - 1, l.neighs[1, 0] - 1
    assert T[up, s] == -2.0 and T[ur, s] == -1.0 and np.array_equal(T, T.T)


@pytest.mark.parametrize("L", [4, 6])
def test_pair_directions_one_per_target(mc_amd, L):
    l = mc_amd.TriangularLattice(L)
    it = mc_amd.EachSitePairByDistance(l)
    n = L * L
    assert it.ndirections() == n and all(len(p) == n for p in it.pairs)
    assert len(it) == n * n and sum(1 for _ in it) == n * n
    norms = [np.linalg.norm(d) for d in it.directions]
    assert all(a < b + 1e-5 for a, b in zip(norms, norms[1:]))  # sorted by directed norm (rounding ties)


@pytest.mark.parametrize("L", [4, 6])
def test_local_quads_k7_are_the_geometric_neighbours(mc_amd, L):
    l = mc_amd.TriangularLattice(L)
    q = mc_amd.EachLocalQuadByDistance(l)
    assert q.K == 7 and q.trg_of.shape == (L * L, 7) and (q.trg_of >= 0).all()
    assert (q.trg_of[:, 0] == np.arange(L * L)).all()
    d = q.pairs_by_dir.directions
    assert np.linalg.norm(d[0]) == 0
    six = sorted(tuple(np.round(v, 6)) for v in d[1:7])
    want = sorted(tuple(np.round(s * np.array(v), 6)) for v in ((1, 0), (0.5, 0.8660254037844386),
                                                                   (-0.5, 0.8660254037844386)) for s in (1, -1))
    assert six == want
    s = mc_amd.EachLocalQuadBySyncedDistance(l)
    assert s.K == 7 and len(s) == 7 * (L * L) ** 2


def test_positions_and_neighbours_do_not_line_up(mc_amd):
    """the reference's quirk, kept: positions() puts upright (i+1, j+1) at sqrt(3), and the geometric nearest neighbour
    (i+1, j-1) carries no hopping; so the six shortest directions of the measurements are not the six bonds"""
    L = 6
    l = mc_amd.TriangularLattice(L)
    pos = mc_amd.lattices._positions(l)
    s = 0  # (i, j) = (1, 1)
    ur = l.neighs[1, s] - 1
    assert abs(np.linalg.norm(pos[ur] - pos[s]) - np.sqrt(3)) < 1e-12
    geo = 1 + L * (L - 1)  # (i + 1, j - 1) = (2, L), 0-based
    assert abs(np.linalg.norm(pos[s] - pos[geo] + np.array([float(L), 0.0])) - 1.0) < 1e-12
    T = mc_amd.HubbardModelAttractive(l=l).hopping_matrix()[0]
    assert T[geo, s] == 0.0 and T[ur, s] == -1.0
    q = mc_amd.EachLocalQuadByDistance(l)
    assert geo in q.trg_of[s, 1:] and ur not in q.trg_of[s, 1:]


@pytest.mark.parametrize("L,mu", [(4, 0.0), (6, 0.3), (16, 0.5)])
def test_hopping_spectrum(mc_amd, L, mu):
    T = mc_amd.HubbardModelAttractive(l=mc_amd.TriangularLattice(L), mu=mu).hopping_matrix()[0]
    k = 2 * np.pi * np.arange(L) / L
    kx, ky = np.meshgrid(k, k)
    want = np.sort((-mu - 2.0 * (np.cos(kx) + np.cos(ky) + np.cos(kx + ky))).ravel())
    assert np.abs(np.linalg.eigvalsh(T) - want).max() < 1e-12


@pytest.mark.parametrize("U", [1.0, -1.0])
def test_hubbard_models(mc_amd, U):
    l = mc_amd.TriangularLattice(4)
    m = mc_amd.HubbardModel(l=l, U=U)
    assert isinstance(m, mc_amd.HubbardModelRepulsive if U > 0 else mc_amd.HubbardModelAttractive)
    Ts = m.hopping_matrix()
    assert len(Ts) == m.flv and m.U == 1.0
    for T in Ts:
        assert np.array_equal(T, T.T)
        off = T - np.diag(np.diag(T))
        assert ((off != 0).sum(axis=0) == 6).all() and np.allclose(off.sum(axis=0), -6.0)


@pytest.mark.parametrize("L,groups", [(4, 14), (6, 16)])
def test_checkerboard_tables(mc_amd, L, groups):
    l = mc_amd.TriangularLattice(L)
    cb, grp, ng = mc_amd.build_checkerboard(l)
    assert ng == groups and cb.shape == (3, 6 * L * L) and grp[-1][1] == 6 * L * L
    T = mc_amd.HubbardModelAttractive(l=l).hopping_matrix()[0]
    tb = mc_amd.checkerboard_tables(T, l, 0.1)
    assert len(tb["seqs"]) == 7 and max(len(s) for s in tb["seqs"]) == 2 * ng - 1 <= 32
    # the ext bonds (every second triple of the bonds table) carry no hopping: T is zero on them, so their factors are
    # the identity on their sites
    ext = l.bonds.reshape(L * L, 2, 3, 3)[:, 1].reshape(-1, 3)
    assert all(T[t - 1, s - 1] == 0.0 for s, t, _ in ext)
    eT, eTinv, eT2, eTinv2 = mc_amd.checkerboard_exponentials(T, l, 0.1)
    assert np.abs(eT2 @ eTinv2 - np.eye(L * L)).max() < 1e-12
    seqs, lens = mc_amd.checkerboard_seqs(tb)
    assert seqs.shape == (7, 32) and list(lens) == [len(s) for s in tb["seqs"]]


def test_sparse_checkerboard_too_many_groups_is_refused(mc_amd, monkeypatch):
    """the engine takes factor sequences of up to 32 entries: more bond groups than 16 are refused with a clear error
    before any handle is touched (the dense checkerboard form stays available)"""
    from importlib import import_module
    dq = import_module(mc_amd.__name__ + ".dqmc")
    l = mc_amd.TriangularLattice(4)
    T = mc_amd.HubbardModelAttractive(l=l).hopping_matrix()[0]
    real = mc_amd.lattices.build_checkerboard

    def split(lat):  # the same bonds in one group each
        cb, _, _ = real(lat)
        return cb, [(i, i) for i in range(1, cb.shape[1] + 1)], cb.shape[1]
    monkeypatch.setattr(mc_amd.lattices, "build_checkerboard", split)
    with pytest.raises(ValueError, match="32"):
        mc_amd.checkerboard_seqs(dq.checkerboard_tables(T, l, 0.1))
