"""The helpers of the measurement-size tests, without a device: tests/lattice_tables.py against the package's own
iterators (exactly), tests/measurement_ref.py against the literal restatements the suite already trusts
(oracle/ref_test_oracle.py, tests/cc_reference.py) on a 4 x 4 lattice, and the launch plans of the current-current LDS
kernel that tests/test_gpu_measurement_sizes.py relies on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_reference as CC  # noqa: E402
import lattice_tables as LT  # noqa: E402
import measurement_ref as MR  # noqa: E402

LATTICES = {
    "square4": lambda m: m.SquareLattice(4),
    "square5": lambda m: m.SquareLattice(5),
    "square6": lambda m: m.SquareLattice(6),
    "chain10": lambda m: m.Chain(10),
    "chain33": lambda m: m.Chain(33),
    "triangular4": lambda m: m.TriangularLattice(4),
    "triangular5_4x6": lambda m: m.TriangularLattice(5, Lx=4, Ly=6),
    "cubic3": lambda m: m.CubicLattice(3, 3),
}


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_tables_equal_the_package_iterators(mc_amd, name):
    l = LATTICES[name](mc_amd)
    ref = mc_amd.EachSitePairByDistance(l)
    fp = LT.fast_pairs(l)
    assert fp.ndirections() == ref.ndirections()
    assert fp.dir_of.dtype == np.int32 and np.array_equal(fp.dir_of, ref.dir_of)
    assert np.abs(np.array(fp.directions) - np.array(ref.directions)).max() < 1e-12
    K = min(1 + l.neighs.shape[0], ref.ndirections())
    for Kq in sorted({K, min(9, ref.ndirections())}):
        q = mc_amd.EachLocalQuadByDistance(l, Kq, pairs=ref)
        s = mc_amd.EachLocalQuadBySyncedDistance(l, Kq, pairs=ref)
        fq, fs = LT.fast_quads(l, Kq, pairs=fp), LT.fast_quads(l, Kq, pairs=fp, synced=True)
        assert np.array_equal(fq.trg_of, q.trg_of) and np.array_equal(fs.trg_of, s.trg_of)
        assert fq.K == q.K and fq.ndirections() == q.ndirections() and fs.ndirections() == s.ndirections()
    with pytest.raises(ValueError):
        LT.fast_quads(l, ref.ndirections() + 1, pairs=fp)


def _random_blocks(rng, n, nb):
    # like a Green's function: diagonal around 1/2, off-diagonal entries of both signs
    return [0.5 * np.eye(n) + 0.3 * rng.standard_normal((n, n)) for _ in range(nb)]


def _close(val, ab, ref, what):
    ref = np.asarray(ref)
    assert val.shape == ref.shape, what
    assert np.all(np.abs(val - ref) <= 1e-13 * ab), (what, np.abs(val - ref).max())
    assert np.all(ab >= np.abs(val) * (1 - 1e-12)), what  # |sum| <= sum of |terms|


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_references_equal_the_literal_restatements(mc_amd, R, kind):
    L, n, K, dtau = 4, 16, 5, 0.1
    attractive = kind == "attractive"
    nb = 1 if attractive else 2
    rng = np.random.default_rng(20 + nb)
    l = mc_amd.SquareLattice(L)
    model = (mc_amd.HubbardModelAttractive if attractive else mc_amd.HubbardModelRepulsive)(l=l)
    T = model.hopping_matrix()
    fp = LT.fast_pairs(l)
    fq = LT.fast_quads(l, K, pairs=fp)
    nd = fp.ndirections()
    G = _random_blocks(rng, n, nb)
    # equal time
    ref = R.equal_time_correlations(G, L, attractive)
    got = MR.equal_time(G, fp.dir_of, nd)
    assert sorted(got) == sorted(ref)
    for k in ref:
        _close(got[k][0], got[k][1], ref[k], k)
    val, ab = MR.pairing(G, fp.dir_of, nd, fq.trg_of)
    _close(val, ab, R.pairing_correlation(G, L, attractive, K), "pairing")
    # time-displaced, three steps
    steps = [tuple(_random_blocks(rng, n, nb) for _ in range(3)) for _ in range(3)]
    it = mc_amd.EachLocalQuadBySyncedDistance(l, K)
    got = MR.susceptibilities(T, G, steps, fp.dir_of, nd, dtau, trg_loc=fq.trg_of, trg_cc=it.trg_of)
    ref = R.susceptibilities(G, steps, L, attractive, K, dtau)
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS"):
        _close(got[k][0], got[k][1], ref[k], k)
    _close(got["CCS"][0], got["CCS"][1], CC.current_current_susceptibility(G, steps, T, it, attractive, dtau), "CCS")
    # cc_kernel quad by quad over the package's iterator
    quad = np.zeros(nd * K)
    for g0l, gl0, gll in steps:
        if attractive:
            pg = (G[0], g0l[0], gl0[0], gll[0])
            for lin, s1, t1, s2, t2 in it:
                quad[lin - 1] += CC.cc_kernel_attractive(pg, T[0], s1 - 1, t1 - 1, s2 - 1, t2 - 1)
        else:
            pg = tuple(CC.blockdiag(x) for x in (G, g0l, gl0, gll))
            T2 = CC.blockdiag(T)
            for lin, s1, t1, s2, t2 in it:
                quad[lin - 1] += CC.cc_kernel(pg, T2, n, s1 - 1, t1 - 1, s2 - 1, t2 - 1)
    _close(got["CCS"][0], got["CCS"][1], quad.reshape((nd, K), order="F") * dtau / n, "CCS quad by quad")
    # accumulate_greens
    walkers = [_random_blocks(rng, n, nb) for _ in range(3)]
    s = MR.greens_sums(walkers)
    flat = lambda blocks: np.concatenate([b.reshape(-1, order="F") for b in blocks])
    _close(s["G"][0], s["G"][1], sum(flat(w) for w in walkers), "G")
    _close(s["G2"][0], s["G2"][1], sum(flat(w) ** 2 for w in walkers), "G2")
    _close(s["occupation"][0], s["occupation"][1],
           np.concatenate([sum(1 - np.diag(w[b]) for w in walkers) for b in range(nb)]), "occupation")


def test_references_honour_missing_targets(mc_amd):
    """a target table with holes: the masked sums equal the sum over the quads that exist"""
    rng = np.random.default_rng(5)
    l = mc_amd.SquareLattice(4)
    n, K = 16, 5
    fp = LT.fast_pairs(l)
    trg = LT.fast_quads(l, K, pairs=fp).trg_of.copy()
    trg[rng.random(trg.shape) < 0.2] = -1
    trg[3, :] = -1
    trg[:, 2] = -1
    T = mc_amd.HubbardModelRepulsive(l=l).hopping_matrix()
    G = _random_blocks(rng, n, 2)
    step = tuple(_random_blocks(rng, n, 2) for _ in range(3))
    val, ab = MR.cc_step(T, G, *step, fp.dir_of, n, trg)
    pg = tuple(CC.blockdiag(x) for x in (G,) + step)
    ref = np.zeros((n, K))
    for k in range(K):
        for s1 in range(n):
            for s2 in range(n):
                if trg[s1, k] >= 0 and trg[s2, k] >= 0:
                    ref[fp.dir_of[s1, s2], k] += CC.cc_kernel(pg, CC.blockdiag(T), n, s1, trg[s1, k], s2, trg[s2, k])
    _close(val, ab, ref / n, "CCS with holes")
    assert np.all(val[:, 2] == 0.0) and np.all(ab[:, 2] == 0.0)
    val, ab = MR.pairing(G, fp.dir_of, n, trg)
    ref = np.zeros((n, K, K))
    for s1 in range(n):
        for s2 in range(n):
            for k1 in range(K):
                for k2 in range(K):
                    if trg[s1, k1] >= 0 and trg[s2, k2] >= 0:
                        ref[fp.dir_of[s1, s2], k1, k2] += G[0][s1, s2] * G[1][trg[s1, k1], trg[s2, k2]]
    _close(val, ab, ref / n, "pairing with holes")


# (lattice, K, W) -> (C, chunks, chunks per workgroup, workgroups, threads), None: the general kernel
PLANS = [
    ("square", 24, 5, 1, (1, 576, 2, 288, 576)),
    ("square", 24, 5, 2, (1, 576, 3, 192, 576)),
    ("square", 24, 7, 1, None),
    ("square", 24, 8, 1, None),
    ("square", 6, 5, 2, (16, 3, 1, 3, 64)),
    ("square", 6, 8, 2, (16, 3, 1, 3, 64)),
    ("square", 6, 5, 256, (16, 3, 2, 2, 64)),
    ("square", 6, 9, 2, None),
    ("chain", 33, 5, 2, (16, 3, 1, 3, 64)),
    ("chain", 257, 5, 2, (8, 33, 1, 33, 320)),
    ("square", 10, 5, 3, (16, 7, 1, 7, 128)),     # E1 to E3: plans that no F case has
    ("chain", 257, 3, 2, (8, 33, 1, 33, 320)),
    ("square", 18, 5, 2, (2, 162, 1, 162, 384)),
]


_pairs_cache = {}


def _tables(mc_amd, kind, size, K):
    if (kind, size) not in _pairs_cache:
        l = mc_amd.SquareLattice(size) if kind == "square" else mc_amd.Chain(size)
        _pairs_cache[kind, size] = (l, LT.fast_pairs(l))
    l, fp = _pairs_cache[kind, size]
    return fp, LT.fast_quads(l, K, pairs=fp, synced=True)


@pytest.mark.parametrize("kind,size,K,W,expected", PLANS)
def test_cc_plan_table(mc_amd, kind, size, K, W, expected):
    fp, fq = _tables(mc_amd, kind, size, K)
    n = fp.dir_of.shape[0]
    p = LT.cc_plan(n, K, W, fq.trg_of, fp.dir_of, fp.ndirections())
    assert LT.plan_tuple(p) == expected
    if p is not None:
        last = n - (p["nchunks"] - 1) * p["C"]
        assert p["lds_bytes"] <= 80 * 1024 and 1 <= last <= p["C"]


def test_cc_plan_refuses_other_tables(mc_amd):
    fp, fq = _tables(mc_amd, "chain", 33, 3)
    hand = np.minimum(np.abs(np.subtract.outer(np.arange(33), np.arange(33))),
                      33 - np.abs(np.subtract.outer(np.arange(33), np.arange(33))))
    assert LT.cc_plan(33, 3, 2, fq.trg_of, hand, 17) is None          # n_dirs != n
    twice = fp.dir_of.copy()
    twice[4, 7] = twice[4, 8]
    assert LT.cc_plan(33, 3, 2, fq.trg_of, twice, 33) is None         # two s2 of one s1 share a direction
