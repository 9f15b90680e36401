"""The reference of the DQMC global moves against what the reference code base itself pins: propose_local's closed
forms for one flipped spin, and the particle-hole symmetry of the repulsive model at half filling.  No GPU."""
import mpmath as mp
import numpy as np
import pytest

import global_move_ref as ref


def _conf(seed, n, M):
    rng = np.random.Generator(np.random.Philox(key=seed))
    return np.asfortranarray((2 * rng.integers(0, 2, size=(n, M)) - 1).astype(np.int8))


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_single_flip_ratio_equals_propose_local(mc_amd, kind):
    """det(I + B_M ... B_1' )/det(I + B_M ... B_1) for one spin flipped in slice 1 equals (1 + gamma (1 - G_ii))^2 resp.
    R_up R_dn with G = (I + B_M ... B_1)^-1, gamma = exp(-2 lambda s) - 1 (HubbardModelAttractive.jl:119-123,
    HubbardModelRepulsive.jl:138-151), to 1e-25 relative, all in 60-digit arithmetic; the full p also carries the
    attractive model's bosonic factor exp(2 lambda s)"""
    if kind == "attractive":
        model = mc_amd.HubbardModelAttractive(4, 2, U=4.0, mu=0.5)
    else:
        model = mc_amd.HubbardModelRepulsive(4, 2, U=8.0)
    dtau, M, site = 0.1, 10, 5
    conf = _conf(21, 16, M)
    new = conf.copy()
    new[site, 0] = -new[site, 0]
    _, _, G = ref.slogdet_mp(model, dtau, conf, exact=True, with_greens=True)
    p = ref.weight_ratio(model, dtau, conf, new, exact=True)
    with mp.workdps(ref.DPS):
        lam = mp.acosh(mp.exp(mp.mpf(model.U) * mp.mpf(dtau) / 2))
        s = int(conf[site, 0])
        dE = -2 * lam * s
        if kind == "attractive":
            closed = (1 + (mp.exp(dE) - 1) * (1 - G[0][site, site])) ** 2 * mp.exp(-dE)
        else:
            closed = (1 + (mp.exp(dE) - 1) * (1 - G[0][site, site])) * (1 + (mp.exp(-dE) - 1) * (1 - G[1][site, site]))
        assert abs(p - closed) <= mp.mpf(10) ** -25 * abs(closed), (p, closed)


def test_flip_all_is_exact_at_half_filling(mc_amd):
    """repulsive square lattice at half filling: det_up(-s) = det_dn(s), so conf -> -conf has p = 1 (to the working
    precision) whatever the field, and the per-block values are exchanged"""
    model = mc_amd.HubbardModelRepulsive(4, 2, U=8.0)
    conf = _conf(22, 16, 10)
    l0, s0 = ref.slogdet_mp(model, 0.1, conf, exact=True)
    l1, s1 = ref.slogdet_mp(model, 0.1, -conf, exact=True)
    with mp.workdps(ref.DPS):
        assert abs(l0[0] - l1[1]) < mp.mpf(10) ** -40 and abs(l0[1] - l1[0]) < mp.mpf(10) ** -40
        assert (s0[0], s0[1]) == (s1[1], s1[0])
        p = ref.weight_ratio(model, 0.1, conf, -conf, exact=True)
        assert abs(p - 1) < mp.mpf(10) ** -40


def test_oracle_logdet_agrees_with_mpmath(mc_amd, O):
    """the float64 restatement of the reference's algorithm (sum log D2, sign det A2) against mpmath on the engine's
    own inputs: the figure the GPU tolerances are ten times of (test_gpu_global_move.LOGDET_TOL)"""
    model = mc_amd.HubbardModelRepulsive(4, 2, U=8.0)
    conf = _conf(23, 16, 20)
    lad, sg, _ = ref.oracle_logdet(O, model, 0.1, 10, conf)
    l0, s0 = ref.slogdet_mp(model, 0.1, conf)
    assert sg == s0
    assert max(abs(float(a - b)) for a, b in zip(lad, l0)) < 1e-11


def test_move_uniform_is_the_ising_domain():
    """u(m, t): counter words (t, low32(m), 1, high32(m)) - never the local stream, whose words 2 and 3 are zero"""
    from ising_wolff_ref import local_uniform
    u = [ref.move_uniform(123, m, t) for m in (0, 1, 2 ** 32 + 5) for t in (0, 1)]
    assert len(set(u)) == len(u) and all(0.0 <= x < 1.0 for x in u)
    assert ref.move_uniform(123, 0, 0) != float(local_uniform(123, 0))
    assert ref.pick_site(0.999999999, 16) == 15 and ref.pick_site(0.0, 16) == 0 and ref.pick_site(1.0, 16) == 15
