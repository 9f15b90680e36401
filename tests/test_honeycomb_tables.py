"""HoneycombLattice(L) on the host: the tables against a construction from coordinates, the hopping spectrum against the
two graphene bands, the 3 L^2 directions of a lattice with a basis, the K = 7 quad tables, the sublattice signs, the pair
channels, strips, the checkpoint's lattice registry and the rule by which the device picks the form of its Green's rows
(tests/honeycomb_ref.py; no GPU is needed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import honeycomb_ref as HR  # noqa: E402
import lattice_tables as LT  # noqa: E402
import time_displaced_ref as TR  # noqa: E402

_cache = {}


def tables(mc_amd, L):
    if L not in _cache:
        l = mc_amd.HoneycombLattice(L)
        _cache[L] = (l, mc_amd.EachSitePairByDistance(l))
    return _cache[L]


@pytest.mark.parametrize("L", [2, 3, 4])
def test_tables_match_the_construction_from_coordinates(mc_amd, L):
    l = mc_amd.HoneycombLattice(L)
    n = 2 * L * L
    assert len(l) == l.sites == n and l.lattice.shape == (L, L, 2)
    assert all(l.lattice[x, y, o] == 1 + HR.site(x, y, o, L) for x in range(L) for y in range(L) for o in range(2))
    assert np.array_equal(l.neighs, HR.brute_neighs(L))
    assert np.array_equal(l.sublattice, np.arange(n) % 2) and np.array_equal(l.isAsite, l.sublattice == 0)
    pos = np.array(mc_amd.lattices._positions(l))
    assert np.array_equal(pos, HR.positions(L))
    assert np.allclose(mc_amd.lattices._lattice_vectors(l), [HR.V1 * L, HR.V2 * L])
    # the three neighbours are the three sites at distance 1 / sqrt(3) on the torus, on the other sublattice
    wrap = LT._images([HR.V1 * L, HR.V2 * L])
    for i in range(n):
        near = [j for j in range(n) if min(np.linalg.norm(pos[i] - pos[j] + v) for v in wrap) < 0.6 and j != i]
        assert sorted(near) == sorted(int(t) - 1 for t in l.neighs[:, i])
        assert all(l.sublattice[j] != l.sublattice[i] for j in near)
    # j in neighs(i) <=> i in neighs(j)
    adj = np.zeros((n, n), dtype=int)
    for s, t in l.neighbors(True):
        adj[s - 1, t - 1] += 1
    assert np.array_equal(adj, adj.T) and adj.sum() == 3 * n and adj.max() == 1
    # every physical bond once, the three rows of each A source
    assert l.n_bonds == 3 * L * L and l.bonds.shape == (3 * L * L, 3)
    want = [(s, int(t), 0) for s in range(1, n + 1, 2) for t in l.neighs[:, s - 1]]
    assert [tuple(b) for b in l.bonds] == want
    und = l.neighbors(False)
    assert len(set(und)) == 3 * L * L and sorted(und + [(t, s) for s, t in und]) == sorted(l.neighbors(True))
    cb, groups, n_groups = mc_amd.build_checkerboard(l)
    assert n_groups == 3 and [b - a + 1 for a, b in groups] == [L * L] * 3


def test_the_triple_bond_of_one_cell(mc_amd):
    l = mc_amd.HoneycombLattice(1)
    assert l.sites == 2 and l.neighs.tolist() == [[2, 1], [2, 1], [2, 1]]
    T = mc_amd.HubbardModelAttractive(l=l, t=0.7).hopping_matrix()[0]
    assert T[0, 1] == T[1, 0] == -3 * 0.7


@pytest.mark.parametrize("L", [3, 6])
def test_hopping_spectrum_is_the_two_bands(mc_amd, L):
    l = mc_amd.HoneycombLattice(L)
    q, labels = mc_amd.momentum_grid(l)
    assert q.shape == (L * L, 2) and [tuple(m) for m in labels] == [(a, b) for b in range(L) for a in range(L)]
    assert np.allclose(q @ (HR.V1 * L) / (2 * np.pi), labels[:, 0]) and np.allclose(q @ (HR.V2 * L) / (2 * np.pi), labels[:, 1])
    t, mu = 0.9, 0.3
    e = HR.band_energies(q, t)
    want = np.sort(np.concatenate([-mu - e, -mu + e]))
    assert (e < 1e-12).sum() == 2  # the two Dirac points are on the grid: zero modes
    for model in (mc_amd.HubbardModelAttractive(l=l, t=t, mu=mu), mc_amd.HubbardModelRepulsive(l=l, t=t, mu=mu),
                  mc_amd.HubbardModel(l=l, U=-1.0, t=t, mu=mu)):
        for T in model.hopping_matrix():
            assert np.array_equal(T, T.T)
            assert np.abs(np.linalg.eigvalsh(T) - want).max() < 1e-12


def test_model_errors(mc_amd):
    l = mc_amd.HoneycombLattice(2)
    for cls in (mc_amd.HubbardModelAttractive, mc_amd.HubbardModelRepulsive):
        with pytest.raises(ValueError, match="tp"):
            cls(l=l, tp=0.2)
        with pytest.raises(ValueError, match="t_perp"):
            cls(l=l, t_perp=1.0)
        assert cls(l=l).t_perp is None and cls(l=l).tp == 0.0


@pytest.mark.parametrize("L", [2, 3, 4])
def test_directions_of_a_lattice_with_a_basis(mc_amd, L):
    l, it = tables(mc_amd, L)
    n = l.sites
    assert it.ndirections() == 3 * L * L
    dir_of = it.dir_of
    # every source and every target meets a direction at most once
    assert all(len(set(dir_of[i])) == n for i in range(n)) and all(len(set(dir_of[:, j])) == n for j in range(n))
    sub = l.sublattice
    counts = {0: 0, 1: 0, 2: 0}
    for d, prs in enumerate(it.pairs):
        kinds = set((int(sub[s - 1]), int(sub[t - 1])) for s, t in prs)
        if kinds == {(0, 0), (1, 1)}:  # same-sublattice displacements from A and from B share a direction
            assert len(prs) == n
            counts[0] += 1
        else:
            assert kinds in ({(0, 1)}, {(1, 0)}) and len(prs) == n // 2
            counts[1 if kinds == {(0, 1)} else 2] += 1
    assert counts == {0: L * L, 1: L * L, 2: L * L}
    # the vectorised restatement gives the same table
    fp = HR.fast_pairs(L)
    assert fp.ndirections() == it.ndirections() and np.array_equal(fp.dir_of, dir_of)
    assert np.allclose(np.array(fp.directions), np.array(it.directions))
    # the sublattice signs
    sg = mc_amd.sublattice_sign(it, l)
    assert sg.shape == (3 * L * L,) and (sg == 1).sum() == L * L and (sg == -1).sum() == 2 * L * L
    assert np.array_equal(sg[dir_of], np.where(sub[:, None] == sub[None, :], 1.0, -1.0))
    assert sg[0] == 1.0 and np.all(sg[1:7] == -1.0)  # on-site, then the six bond directions
    with pytest.raises(TypeError):
        mc_amd.sublattice_sign(it, mc_amd.SquareLattice(2))


@pytest.mark.parametrize("L", [2, 3, 4])
def test_quad_tables_with_seven_directions(mc_amd, L):
    l, it = tables(mc_amd, L)
    for cls in (mc_amd.EachLocalQuadByDistance, mc_amd.EachLocalQuadBySyncedDistance):
        q = cls(l, pairs=it)
        assert q.K == 7 and q.trg_of.shape == (l.sites, 7)
        assert np.array_equal(q.trg_of[:, 0], np.arange(l.sites))
        for i in range(l.sites):
            t = q.trg_of[i, 1:]
            assert (t >= 0).sum() == 3 and sorted(t[t >= 0]) == sorted(int(x) - 1 for x in l.neighs[:, i])
        assert np.array_equal(q.trg_of, HR.quads(HR.fast_pairs(L), 7).trg_of)
    # the Bravais lattices keep their default K
    assert mc_amd.EachLocalQuadByDistance(mc_amd.SquareLattice(4)).K == 5
    assert mc_amd.EachLocalQuadBySyncedDistance(mc_amd.TriangularLattice(4)).K == 7
    assert mc_amd.EachLocalQuadByDistance(mc_amd.BilayerSquareLattice(3)).K == 6


def test_default_pair_channels(mc_amd):
    l, it = tables(mc_amd, 3)
    ch = mc_amd.lattices.default_pair_channels(l, it.directions, 7)
    assert list(ch) == ["s", "s*"]
    assert ch["s"].tolist() == [1, 0, 0, 0, 0, 0, 0] and ch["s*"].tolist() == [0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    q = mc_amd.EachLocalQuadByDistance(l, pairs=it)
    seen = np.where(q.trg_of >= 0, ch["s*"][None, :], 0.0)
    assert np.array_equal(np.sort(seen, axis=1)[:, -3:], np.full((l.sites, 3), 0.5)) and np.all(seen.sum(axis=1) == 1.5)


def test_strip_subsystem(mc_amd):
    L = 4
    l = mc_amd.HoneycombLattice(L)
    strip = mc_amd.strip_subsystem
    assert strip(l, 2, axis=0).tolist() == sorted(HR.site(x, y, o, L) for x in range(2) for y in range(L) for o in range(2))
    assert strip(l, 1, axis=1).tolist() == sorted(HR.site(x, 0, o, L) for x in range(L) for o in range(2))
    assert strip(l, L).tolist() == list(range(2 * L * L))
    for bad in (dict(width=0), dict(width=L + 1), dict(width=1, axis=2)):
        with pytest.raises(ValueError):
            strip(l, **bad)


def test_checkpoint_names_the_lattice(mc_amd, tmp_path):
    """the lattice registry of the checkpoint preamble and a write / read round trip of a preamble that names it"""
    reg = mc_amd.DQMC._LATTICES
    assert reg["HoneycombLattice"] == ("L",)
    l = mc_amd.HoneycombLattice(3)
    entry = {"class": type(l).__name__, "args": [int(getattr(l, a)) for a in reg[type(l).__name__]]}
    from importlib import import_module
    ckpt = import_module(mc_amd.__name__ + ".checkpoint")
    path = str(tmp_path / "pre.ckpt")
    ckpt.write(path, {"format": 1, "lattice": entry}, np.arange(16, dtype=np.uint8))
    pre, blob = ckpt.read(path)
    assert pre["lattice"] == {"class": "HoneycombLattice", "args": [3]} and bytes(blob) == bytes(range(16))
    back = getattr(mc_amd.lattices, pre["lattice"]["class"])(*pre["lattice"]["args"])
    assert np.array_equal(back.neighs, l.neighs)
    # the entries of the other lattices are as they were
    assert {k: v for k, v in reg.items() if k != "HoneycombLattice"} == {
        "SquareLattice": ("L",), "Chain": ("sites",), "CubicLattice": ("dim", "L"), "TriangularLattice": ("L", "Lx", "Ly"),
        "BilayerSquareLattice": ("L",)}


def test_form_of_the_greens_rows(mc_amd):
    """the selection rule of td_setup: honeycomb tables take the injective form, the Bravais lattices keep the Latin square
    form (where the old rule, time_displaced_ref.src_of_table, gave a table, the new one says 1), the ring table and a
    table with a repeated target keep the pair lists"""
    for L in (2, 3, 6):
        fp = HR.fast_pairs(L)
        n, nd = 2 * L * L, fp.ndirections()
        assert TR.src_of_table(fp.dir_of, nd) is None
        assert HR.greens_rows_form(fp.dir_of, nd) == 2
        assert HR.greens_rows_form(fp.dir_of, nd, general_switch=True) == 0
        so = HR.src_of_holes(fp.dir_of, nd)
        assert so.shape == (nd, n) and (so >= 0).sum() == n * n
        i, j = np.nonzero(np.ones((n, n), dtype=bool))
        assert np.array_equal(so[fp.dir_of[i, j], j], i)
    for l in (mc_amd.SquareLattice(4), mc_amd.SquareLattice(6), mc_amd.TriangularLattice(4), mc_amd.TriangularLattice(4, Lx=3, Ly=5),
              mc_amd.CubicLattice(3, 3), mc_amd.BilayerSquareLattice(3), mc_amd.Chain(9)):
        fp = LT.fast_pairs(l)
        assert TR.src_of_table(fp.dir_of, fp.ndirections()) is not None
        assert HR.greens_rows_form(fp.dir_of, fp.ndirections()) == 1
    n = 33  # the ring table: both senses of a distance share a direction
    d = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
    assert HR.greens_rows_form(np.minimum(d, n - d), n // 2 + 1) == 0
    assert HR.greens_rows_form(np.tile(np.arange(n), (n, 1)), n) == 0  # dir_of[i, j] = j: every target repeats
    # more than 2 n directions: every pair its own direction is injective, but the table would hold n^3 entries
    assert HR.greens_rows_form(np.arange(16).reshape(4, 4), 16) == 0
    assert HR.greens_rows_form(np.arange(4).reshape(2, 2), 4) == 2  # n_dirs == 2 n: the bound itself
