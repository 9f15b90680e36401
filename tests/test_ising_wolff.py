"""The Ising flavor's Wolff cluster move without a device: the four-word Philox restatement against the oracle's stream,
the restated move against a literal stack-based growth in the reference's shape, exact detailed balance of the move
as defined (transition matrices built by branching over the bond tests it makes), and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import ising_wolff_ref as R


def test_philox4_equals_the_oracle_stream_when_c2_c3_are_zero(O):
    for key in (0, 1, 123, 2 ** 32 + 7, 0xDEADBEEFCAFEF00D):
        idx = np.array([0, 1, 2, 31, 4095, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3], dtype=np.uint64)
        ours = R.local_uniform(key, idx)
        ref = np.array([O.philox_uniform(key, int(i)) for i in idx])
        assert np.array_equal(ours, ref), key
    # the cluster domain (c2 = 1) is another stream
    a = R.philox4_uniform(5, np.arange(64), 0, 1, 0)
    b = R.philox4_uniform(5, np.arange(64), 0, 0, 0)
    assert not np.any(a == b)
    assert np.all((a >= 0) & (a < 1))


def _stack_growth(conf, neighs0, key, m, p):
    """the reference's loop (IsingModel.jl:113-131): a stack, a membership test, and a draw only for an aligned
    neighbour not yet in the cluster, from the slot's own counter"""
    N = len(conf)
    seed = R.wolff_seed(key, m, N)
    cluster, tocheck = {seed}, [seed]
    while tocheck:
        cur = tocheck.pop()
        for k in range(neighs0.shape[0]):
            n = int(neighs0[k, cur])
            if conf[cur] == conf[n] and n not in cluster:
                if R.philox4_uniform(key, 1 + 8 * cur + k, m & 0xFFFFFFFF, 1, m >> 32) < p:
                    tocheck.append(n)
                    cluster.add(n)
    return np.array(sorted(cluster))


@pytest.mark.parametrize("name,make,beta", [
    ("square6", lambda g: g.SquareLattice(6), 0.44),
    ("square6_cold", lambda g: g.SquareLattice(6), 1.5),
    ("chain9", lambda g: g.Chain(9), 0.8),
    ("cubic3", lambda g: g.CubicLattice(3, 3), 0.25),
    ("triangular4", lambda g: g.TriangularLattice(4), 0.3),
])
def test_the_cluster_does_not_depend_on_the_growth_order(mc_amd, name, make, beta):
    l = make(mc_amd)
    neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
    rng = np.random.default_rng(11)
    p = R.wolff_p(beta)
    sizes = []
    for m in range(40):
        conf = rng.choice([-1, 1], len(l)).astype(np.int64)
        a = R.wolff_cluster(conf, neighs0, 77, m, p)
        assert np.array_equal(a, _stack_growth(conf, neighs0, 77, m, p)), (name, m)
        assert np.all(conf[a] == conf[a[0]])
        sizes.append(len(a))
    assert max(sizes) > 1


def _transition_matrix(neighs0, beta):
    """P[s, s'] of the move as defined, the seed uniform over the N sites and every bond test the growth makes an
    independent branch (p = 1 - exp(-2 beta)); states are bit patterns, bit i = 1 <=> s_i = +1"""
    z, N = neighs0.shape
    p = R.wolff_p(beta)
    P = np.zeros((1 << N, 1 << N))

    def grow(conf, cluster, slots, prob, out):
        # slots: directed slots (i, k) still to be looked at, in order
        while slots:
            i, k = slots[0]
            j = int(neighs0[k, i])
            if conf[j] == conf[i] and j not in cluster:
                rest = slots[1:]
                grow(conf, cluster | {j}, rest + [(j, q) for q in range(z)], prob * p, out)
                grow(conf, cluster, rest, prob * (1.0 - p), out)
                return
            slots = slots[1:]
        out.append((cluster, prob))

    for s in range(1 << N):
        conf = [1 if (s >> i) & 1 else -1 for i in range(N)]
        for seed in range(N):
            out = []
            grow(conf, frozenset([seed]), [(seed, q) for q in range(z)], 1.0 / N, out)
            for cluster, prob in out:
                t = s
                for i in cluster:
                    t ^= 1 << i
                P[s, t] += prob
    return P


@pytest.mark.parametrize("name,make", [
    ("chain4", lambda g: g.Chain(4)),
    ("chain5", lambda g: g.Chain(5)),
    ("square2_duplicate_slots", lambda g: g.SquareLattice(2)),
])
@pytest.mark.parametrize("beta", [0.0, 0.1, 0.44, 1.0, 3.0])
def test_detailed_balance_is_exact(mc_amd, name, make, beta):
    """pi(s) P(s -> s') = pi(s') P(s' -> s) with pi ~ exp(-beta E), E = -1/2 sum over the directed slots (the energy
    whose differences propose_local computes; on these lattices it equals the bonds table's); rows sum to 1"""
    l = make(mc_amd)
    neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
    bonds0 = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
    N = len(l)
    P = _transition_matrix(neighs0, beta)
    assert np.allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    E = np.zeros(1 << N)
    for s in range(1 << N):
        c = np.array([1 if (s >> i) & 1 else -1 for i in range(N)])
        E[s] = -0.5 * sum(c[i] * c[neighs0[k, i]] for i in range(N) for k in range(neighs0.shape[0]))
        assert E[s] == R.energy(c, bonds0)
    pi = np.exp(-beta * (E - E.min()))
    pi /= pi.sum()
    flow = pi[:, None] * P
    assert np.max(np.abs(flow - flow.T)) <= 1e-12, (name, beta)
    if beta > 0:  # the move connects every pair of states that differ by one cluster: not the identity
        assert np.count_nonzero(P - np.diag(np.diag(P))) > 0


def test_limits_of_p():
    """beta = 0: no slot is active (the seed alone flips); beta = 50: p rounds to 1.0 and every uniform is below it"""
    assert R.wolff_p(0.0) == 0.0
    assert R.wolff_p(50.0) == 1.0
    u = R.philox4_uniform(3, np.arange(1 << 16), 0, 1, 0)
    assert u.max() < 1.0


def test_argument_checks_without_a_device(mc_amd):
    from montecarlo_jl_amd import _lib
    L = _lib.lib()
    st = _lib.McGlobalStats()
    assert L.dqmc_mc_set_global_rate(None, 1) == _lib.ERR_INVALID
    assert b"null handle" in L.dqmc_mc_last_error(None)
    assert L.dqmc_mc_global_move(None, -1) == _lib.ERR_INVALID
    assert b"dqmc_mc_global_move" in L.dqmc_mc_last_error(None)
    assert L.dqmc_mc_get_global_stats(None, 0, C.byref(st)) == _lib.ERR_INVALID
    model = mc_amd.IsingModel(dims=2, L=4)
    for rate in (0, -1, 2.5):
        with pytest.raises(ValueError, match="global_rate"):
            mc_amd.MC(model, beta=0.4, cluster_moves=True, global_rate=rate)
    with pytest.raises(NotImplementedError, match="global_move"):
        mc_amd.MC(model, beta=0.4, global_moves=True)


def test_struct_mirrors_the_header(mc_amd):
    from montecarlo_jl_amd import _lib
    assert C.sizeof(_lib.McGlobalStats) == 32
    assert [f for f, _ in _lib.McGlobalStats._fields_] == ["prop_global", "acc_global", "sum_cluster_size",
                                                            "moves_drawn"]
    src = open(_lib.HEADER_PATH).read()
    assert "int64_t prop_global, acc_global, sum_cluster_size;" in src and "uint64_t moves_drawn;" in src
