"""CubicLattice(D, L) (src/lattices/cubic.jl) and the 3D Hubbard models built on it, on the host: the reference's
lattice tests (test/lattices.jl:1-40, the "Lattice Iterators" testset on HubbardModelAttractive(3, 3)) and a literal
restatement of build_neighbortable(CubicLattice, ...)."""
import numpy as np
import pytest


def neighbortable(L, D):
    """build_neighbortable(CubicLattice, lattice, D) (cubic.jl:43-56): circshift by -1, then +1, along each dimension"""
    lat = np.arange(1, L ** D + 1).reshape((L,) * D, order="F")
    ups = [np.roll(lat, -1, axis=d).reshape(-1, order="F") for d in range(D)]
    downs = [np.roll(lat, 1, axis=d).reshape(-1, order="F") for d in range(D)]
    return np.array(ups + downs)


@pytest.mark.parametrize("L", [3, 4])
def test_reference_lattice_checks_in_3d(mc_amd, L):
    d = 3
    l = mc_amd.CubicLattice(d, L)
    assert len(l) == L ** d
    bonds = l.neighbors(True)
    assert len(bonds) == 2 * d * L ** d
    assert len(set(bonds)) == len(bonds)
    for i in range(len(l)):
        grp = bonds[2 * d * i:2 * d * (i + 1)]
        assert all(b[0] == grp[0][0] for b in grp)               # same source
        assert len(set(b[1] for b in grp)) == 2 * d              # different targets
    reduced = l.neighbors(False)
    assert len(reduced) == d * L ** d
    assert sorted(reduced + [(t, s) for s, t in reduced]) == sorted(bonds)


@pytest.mark.parametrize("D,L", [(3, 3), (3, 4), (3, 2), (4, 3)])
def test_tables_match_the_literal_restatement(mc_amd, D, L):
    l = mc_amd.CubicLattice(D, L)
    ref = neighbortable(L, D)
    assert l.neighs.shape == (2 * D, L ** D)
    assert np.array_equal(l.neighs, ref)
    assert l.n_bonds == D * L ** D
    want = [(src, ref[d, src - 1], 0) for src in range(1, L ** D + 1) for d in range(D)]
    assert np.array_equal(l.bonds, np.array(want))
    # site x + L y + L^2 z (1-based): its upright neighbour along x is x + 1 mod L
    if D == 3:
        x, y, z = 1, L - 1, 0
        s = 1 + x + L * y + L * L * z
        assert l.neighs[0, s - 1] == 1 + (x + 1) % L + L * y + L * L * z
        assert l.neighs[2, s - 1] == 1 + x + L * y + L * L * ((z + 1) % L)
        assert l.neighs[4, s - 1] == 1 + x + L * ((y - 1) % L) + L * L * z


def test_choose_lattice(mc_amd):
    from importlib import import_module
    models = import_module(mc_amd.__name__ + ".models")
    assert isinstance(models.choose_lattice(1, 5), mc_amd.Chain)
    assert isinstance(models.choose_lattice(2, 5), mc_amd.SquareLattice)
    c = models.choose_lattice(3, 5)
    assert isinstance(c, mc_amd.CubicLattice) and (c.dim, c.L, len(c)) == (3, 5, 125)
    c4 = models.choose_lattice(4, 3)
    assert isinstance(c4, mc_amd.CubicLattice) and len(c4) == 81


def test_pair_iterators_need_3d(mc_amd):
    """cubic.jl defines positions / lattice_vectors for D = 3 only: the model builds, the iterators refuse"""
    m = mc_amd.HubbardModelAttractive(3, 4)
    assert len(m.l) == 81 and m.hopping_matrix()[0].shape == (81, 81)
    with pytest.raises(NotImplementedError, match="D = 3 only"):
        mc_amd.EachSitePairByDistance(m.l)


@pytest.fixture(scope="module")
def pairs333(mc_amd):
    m = mc_amd.HubbardModelAttractive(3, 3)
    return m, mc_amd.EachSitePairByDistance(m.l)


def test_iterator_directions_sorted_and_minimal(mc_amd, pairs333):
    m, it = pairs333
    dirs = it.directions
    for i in range(1, len(dirs)):
        assert np.linalg.norm(dirs[i - 1]) < np.linalg.norm(dirs[i]) + 1e-5
    # every (dir, src, trg) has the minimal-image displacement of its direction
    L, n = 3, 27
    pos = lambda s: np.array([(s - 1) % L, ((s - 1) // L) % L, (s - 1) // (L * L)], dtype=float) + 1
    for d, s, t in it:
        delta = pos(s) - pos(t)
        best = min(np.linalg.norm(delta + L * np.array(k)) for k in np.ndindex(3, 3, 3) for k in [np.array(k) - 1])
        assert abs(np.linalg.norm(dirs[d - 1]) - best) < 1e-9
        assert np.allclose(np.mod(dirs[d - 1] - delta, L), 0)
    assert len(it) == n * n
    assert sum(1 for _ in it) == n * n
    # on 3 x 3 x 3 every displacement has one minimal image: 27 directions, one per target of each source
    assert it.ndirections() == 27 and all(len(p) == n for p in it.pairs)
    assert np.linalg.norm(dirs[0]) == 0 and all(abs(np.linalg.norm(dirs[k]) - 1) < 1e-12 for k in range(1, 7))


def test_ties_keep_discovery_order(mc_amd):
    """on 4 x 4 x 4 the direction (2, 0, 0) has two images of equal norm; the first in generate_combinations order wins,
    and directions of equal norm stay in the order they were found (a stable sort, like Julia's sortperm)"""
    l = mc_amd.CubicLattice(3, 4)
    it = mc_amd.EachSitePairByDistance(l)
    norms = [np.linalg.norm(d) for d in it.directions]
    assert norms == sorted(norms) and it.ndirections() == 64
    assert len(it) == 64 * 64
    # restated discovery order of the directions from origin 1
    lat = mc_amd.lattices
    pos, wrap = lat._positions(l), lat.generate_combinations(lat._lattice_vectors(l))
    found = []
    for trg, p in enumerate(pos):
        d = pos[0] - p + wrap[0]
        for v in wrap[1:]:
            if np.linalg.norm(pos[0] - p + v) + 1e-6 < np.linalg.norm(d):
                d = pos[0] - p + v
        found.append(d)
    order = sorted(range(64), key=lambda k: np.linalg.norm(found[k]))
    assert all(np.allclose(it.directions[i], found[k]) for i, k in enumerate(order))
    # the image of (2, 0, 0) from site 1 is the first in generate_combinations order: -2 (x - v), not +2
    assert any(np.allclose(d, [-2, 0, 0]) for d in it.directions)
    assert not any(np.allclose(d, [2, 0, 0]) for d in it.directions)


def test_local_quads_k7(mc_amd, pairs333):
    m, it = pairs333
    q = mc_amd.EachLocalQuadByDistance(m.l)
    assert q.K == 7 and q.trg_of.shape == (27, 7) and (q.trg_of >= 0).all()
    nb = set(int(t) - 1 for t in m.l.neighs[:, 0])
    assert set(q.trg_of[0, 1:]) == nb and q.trg_of[0, 0] == 0
    assert len(q) == (27 * 7) ** 2
    s = mc_amd.EachLocalQuadBySyncedDistance(m.l)
    assert s.K == 7 and len(s) == 7 * 27 * 27


@pytest.mark.parametrize("U", [1.0, -1.0])
def test_hubbard_model_3d(mc_amd, U):
    m = mc_amd.HubbardModel(L=4, dims=3, U=U)
    assert isinstance(m, mc_amd.HubbardModelRepulsive if U > 0 else mc_amd.HubbardModelAttractive)
    assert isinstance(m.l, mc_amd.CubicLattice) and len(m.l) == 64 and m.U == 1.0
    for T in m.hopping_matrix():
        assert np.array_equal(T, T.T)
        off = T - np.diag(np.diag(T))
        assert ((off != 0).sum(axis=0) == 6).all() and np.allclose(off.sum(axis=0), -6.0)
    # L = 2: up and down neighbour along a dimension are the same site: -2t per dimension
    T = mc_amd.HubbardModelAttractive(2, 3).hopping_matrix()[0]
    off = T - np.diag(np.diag(T))
    assert ((off != 0).sum(axis=0) == 3).all() and set(np.unique(off[off != 0])) == {-2.0}
    assert np.array_equal(T, T.T)


def test_checkerboard_tables_on_cubic(mc_amd):
    m = mc_amd.HubbardModelAttractive(4, 3)
    cb, groups, ng = mc_amd.build_checkerboard(m.l)
    assert cb.shape == (3, 3 * 64) and groups[-1][1] == 3 * 64
    T = m.hopping_matrix()[0]
    tb = mc_amd.checkerboard_tables(T, m.l, 0.1)
    assert max(len(s) for s in tb["seqs"]) <= 32 and len(tb["seqs"]) == 7
