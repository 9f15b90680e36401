"""The checkerboard sweep of the Ising flavor as include/dqmc_hip.h defines it (dqmc_mc_set_update), without a GPU: the
default colouring, exact invariance of the Boltzmann weight under one sweep, the restated chain against exact
enumeration on 4x4, and the ABI surface."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ising_checkerboard_ref as ref  # noqa: E402
import ising_wolff_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (lattice, colours, class sizes or None)
COLOURINGS = [
    ("chain10", lambda g: g.Chain(10), 2, (5, 5)),
    ("square2", lambda g: g.SquareLattice(2), 2, (2, 2)),
    ("square4", lambda g: g.SquareLattice(4), 2, (8, 8)),
    ("square8", lambda g: g.SquareLattice(8), 2, (32, 32)),
    ("square128", lambda g: g.SquareLattice(128), 2, (8192, 8192)),
    ("cubic4", lambda g: g.CubicLattice(3, 4), 2, (32, 32)),
    ("chain7", lambda g: g.Chain(7), 3, (3, 3, 1)),
    ("square5", lambda g: g.SquareLattice(5), 4, (9, 8, 4, 4)),
    ("cubic5", lambda g: g.CubicLattice(3, 5), 4, None),
    ("triangular4", lambda g: g.TriangularLattice(4), 4, None),
    ("triangular5", lambda g: g.TriangularLattice(5), 4, (7, 7, 7, 4)),
    ("triangular6", lambda g: g.TriangularLattice(6), 4, None),
]


@pytest.mark.parametrize("name,make,n_colours,sizes", COLOURINGS, ids=[c[0] for c in COLOURINGS])
def test_greedy_colouring(mc_amd, name, make, n_colours, sizes):
    l = make(mc_amd)
    col = mc_amd.greedy_colouring(l)
    assert col.dtype == np.int32 and col.shape == (len(l),)
    assert np.array_equal(col, ref.greedy_colouring(l))
    assert ref.is_valid(l, col)
    assert int(col.max()) + 1 == n_colours <= 16 and col.min() == 0
    if sizes is not None:
        assert tuple(np.bincount(col)) == sizes
    # the rule itself: every site has the smallest colour no earlier neighbour has
    nb = np.asarray(l.neighs) - 1
    for i in range(min(len(l), 200)):
        used = {int(col[j]) for j in nb[:, i] if j < i}
        assert col[i] == min(c for c in range(17) if c not in used)


def test_a_self_neighbour_is_refused(mc_amd):
    l = mc_amd.Chain(1)
    if 1 not in np.asarray(l.neighs)[:, 0]:
        return  # (Chain(1) builds without a self-neighbour: nothing to refuse)
    with pytest.raises(ValueError):
        mc_amd.greedy_colouring(l)
    with pytest.raises(ValueError):
        ref.greedy_colouring(l)


def _transition_matrix(l, beta):
    """P[a, b] of one checkerboard sweep over all 2^N states (bit i of a state = spin i up), by branching over the
    accept decisions: within a colour the sites decide independently from the state the colour began with"""
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    N = nb.shape[1]
    cls = ref.classes(ref.greedy_colouring(l))
    spins = lambda a: np.array([1 if (a >> i) & 1 else -1 for i in range(N)])  # noqa: E731
    P = np.eye(1 << N)
    for idx in cls:
        Pc = np.zeros((1 << N, 1 << N))
        for a in range(1 << N):
            s = spins(a)
            dE = [2.0 * s[i] * s[nb[:, i]].sum() for i in idx]
            p = [1.0 if d <= 0 else np.exp(-beta * d) for d in dE]
            for flips in itertools.product((0, 1), repeat=len(idx)):
                b, pr = a, 1.0
                for i, f, q in zip(idx, flips, p):
                    pr *= q if f else 1.0 - q
                    b ^= f << int(i)
                Pc[a, b] += pr
        P = P @ Pc
    E = np.array([-0.5 * sum(spins(a)[i] * spins(a)[nb[:, i]].sum() for i in range(N)) for a in range(1 << N)])
    return P, E


@pytest.mark.parametrize("beta", [0.3, 0.8])
@pytest.mark.parametrize("shape", ["chain4", "square2"])
def test_one_sweep_leaves_the_boltzmann_weight_invariant(mc_amd, shape, beta):
    """pi P = pi to 1e-13: pure fp64 rounding of a product of at most 16-state matrices (the double bonds of
    SquareLattice(2) count twice in dE and in E alike)"""
    l = mc_amd.Chain(4) if shape == "chain4" else mc_amd.SquareLattice(2)
    P, E = _transition_matrix(l, beta)
    np.testing.assert_allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    pi = np.exp(-beta * (E - E.min()))
    pi /= pi.sum()
    err = np.abs(pi @ P - pi).max()
    print(shape, beta, err)
    assert err <= 1e-13
    assert np.abs(P - np.eye(len(P))).max() > 0.1  # (the sweep does move)


def test_array_philox_is_the_scalar_one():
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 2 ** 63, 40, dtype=np.int64).astype(np.uint64)
    s = np.concatenate([rng.integers(0, 1000, 30), rng.integers(2 ** 32, 2 ** 40, 10)])
    i = rng.integers(0, 16384, 40)
    got = ref.u_cb_keys(keys, s, i)
    want = [float(ref.u_cb(int(k), int(x), int(j))) for k, x, j in zip(keys, s, i)]
    assert got.tolist() == want
    assert float(R.philox4_uniform(5, 7, 9, 3, 0)) == float(ref.u_cb(5, 9, 7))


def test_walker_and_ladders_restate_the_same_chain(mc_amd):
    l = mc_amd.SquareLattice(5)
    betas, keys = [0.2, 0.44, 0.6], [11, 12, 13]
    lad = ref.Ladders(l, betas, keys, series_capacity=10)
    lad.run(1, 12, 2, 3)
    for w in range(3):
        one = ref.Walker(l, betas[w], keys[w], series_capacity=10)
        one.run(1, 12, 2, 3, 0)
        assert np.array_equal(one.c, lad.c[w]) and one.s == lad.s[w] == 12
        st, lst = one.stats(), lad.stats(w)
        assert all(st[k] == lst[k] for k in st), (st, lst)
        assert st["uniforms_used"] == len(l) and st["prop_local"] == 12 * len(l)
        assert one.serE == lad.serE[w] and one.serM == lad.serM[w]


def test_4x4_against_exact_enumeration():
    """beta = 0.2, 0.44, 0.7, 512 walkers each, 200 + 2000 sweeps of the defined chain: means within 4.5 cross-walker
    standard errors (the seed is fixed in ising_checkerboard_ref: the device test reproduces these sums exactly)"""
    l, lad = ref.enum_run()
    assert lad.n_meas == ref.ENUM_SWEEPS and np.all(lad.s == ref.ENUM_THERM + ref.ENUM_SWEEPS)
    assert np.all(lad.draw == 16)  # the local stream gave the initial configuration and nothing else
    ref.check_enum(lad.sums, lad.n_meas, l)


def test_abi_surface(mc_amd):
    from montecarlo_jl_amd import _lib
    src = open(_lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for fn in ("dqmc_mc_set_update", "dqmc_mc_get_update"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, code), fn
        assert hasattr(L, fn), fn
        assert fn in _lib.SIGNATURES, fn
    assert re.search(r"#define\s+DQMC_MC_UPDATE_SEQUENTIAL\s+0\b", code)
    assert re.search(r"#define\s+DQMC_MC_UPDATE_CHECKERBOARD\s+1\b", code)
    assert "dqmc_mc_update_stats" in code
    assert _lib.SIGNATURES["dqmc_mc_set_update"][1] == [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    assert [f[0] for f in _lib.McUpdateStats._fields_] == ["kind", "n_colours", "sweeps_drawn"]
    assert C.sizeof(_lib.McUpdateStats) == 16
    # the colouring is validated before the device is asked for: a null handle is an argument error, not a crash
    assert L.dqmc_mc_set_update(None, 1, None, 2) == _lib.ERR_INVALID
