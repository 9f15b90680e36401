"""The hand-over between pivot waves of the four-wave elimination (sweep_lu.hip, lu4_wave), against the oracle one
propagate / sweep_spatial at a time: HS field bit for bit, uniforms consumed and acceptance counters equal, G within 1e-10.

Site 15 of a block of 16 sites changes no row of the block: it has no payload in the step ring and no strip / inverse
update, the helpers publish the strip rows of the last panel (sites 12..15) before its flag arrives, and all the wave that
pivots next takes from it is x (0 for a rejected site).  The cases are the smallest shapes that reach each branch:
  Chain(64)      one full chunk, stand-alone elimination: three full hand-overs (both models)
  Chain(33)      blocks 16 / 16 / 1: a hand-over into a one-site block
  Chain(47)      blocks 16 / 16 / 15: the last block ends at c = 14 (no site 15, strip rows published at the panel end)
  6 x 6          blocks 16 / 16 / 4
  16 x 16        four chunks in fused launches (elimination beside the previous chunk's flush): the early prologue of the
                 attractive model, the two-barrier prologue of the repulsive one; 3 slices, up and back
  recorded uniforms               u = 1 - 2^-53 (only proposals with p > 1 are accepted: acceptance 0.17 in the oracle
                                  against 0.91 with the seeded stream) and u = 0 (every proposal accepted): last panels
                                  with all four sites rejected / mixed / all four accepted
Every case states which last-panel patterns it has seen (from the oracle's HS field before and after each sweep_spatial)."""
import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def last_panels(n):
    """first site of every last panel (sites 12..15 of a block of 16) behind which the same chunk of 64 has another block,
    with the number of sites of that next block"""
    out = []
    for s0 in range(12, n, 16):
        nxt = s0 + 4
        if nxt % 64 != 0 and nxt < n:
            out.append((s0, min(16, n - nxt, 64 - nxt % 64)))
    return out


def panel_patterns(before, after, n):
    """(all four accepted, all four rejected, mixed) last panels of one sweep_spatial, from the HS field around it"""
    flipped = before != after
    cols = np.nonzero(flipped.any(axis=0))[0]
    assert len(cols) <= 1
    if len(cols) == 0:
        return 0, len(last_panels(n)), 0
    f = flipped[:, cols[0]]
    acc = rej = mix = 0
    for s0, _ in last_panels(n):
        k = int(f[s0:s0 + 4].sum())
        acc, rej, mix = acc + (k == 4), rej + (k == 0), mix + (0 < k < 4)
    return acc, rej, mix


def sweep_fused_rule(n, walkers, nb, cus):
    """dqmc_create's choice of the fused chunk loop (restated in tests/test_gpu_sizes.py)"""
    if n % 64 != 0 or n < 128:
        return False
    ncp = 2 if n % 256 == 0 else 1
    nt = 8 if n % 128 == 0 else 4
    flush_blocks = ((walkers * nb + 7) // 8) * 8 * (n // 64) * (n // (16 * nt * ncp))
    return walkers + flush_blocks <= cus


def make_model(pkg, shape, kind, U=1.0):
    l = pkg.SquareLattice(shape[1]) if shape[0] == "square" else pkg.Chain(shape[1])
    cls = pkg.HubbardModelAttractive if kind == "attractive" else pkg.HubbardModelRepulsive
    return cls(l=l, U=U)


def make_oracle(O, model, kind, conf, beta, delta_tau, safe_mult, seed=None, uniforms=None):
    o = O.OracleDQMC(model.l.sites, kind, beta=beta, delta_tau=delta_tau, safe_mult=safe_mult, U=model.U,
                     hopping=model.hopping_matrix()[0])
    o.set_conf(conf)
    if uniforms is not None:
        o.set_uniforms(uniforms)
    else:
        o.seed(seed)
    return o


def run_case(gpu, O, shape, kind, walkers, nupd, beta=1.0, delta_tau=0.1, safe_mult=5, U=1.0, uniforms=None, fused=None):
    """prepare, then nupd x (propagate, sweep_spatial) compared after every call; returns the worst G error, the
    oracle's acceptance and the last-panel patterns seen"""
    model = make_model(gpu, shape, kind, U)
    mc = gpu.DQMC(model, beta=beta, delta_tau=delta_tau, safe_mult=safe_mult, n_walkers=walkers, seed=31)
    n = mc.N
    if fused is not None:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert sweep_fused_rule(n, walkers, mc.nb, cus) == fused
    if uniforms is not None:
        for w in range(walkers):
            mc.set_uniforms(w, uniforms)
    refs = [make_oracle(O, model, kind, mc.conf(w), beta, delta_tau, safe_mult, mc.seeds[w], uniforms)
            for w in range(walkers)]
    worst = 0.0

    def compare(conf=True):
        nonlocal worst
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                e = relerr(g, g0)
                worst = max(worst, e)
                assert e < TOL, e
    mc.prepare()
    for o in refs:
        o.prepare()
    compare()
    pat = np.zeros(3, dtype=int)
    for _ in range(nupd):
        mc.propagate()
        for o in refs:
            o.propagate()
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        compare(conf=False)
        before = [o.conf() for o in refs]
        mc.sweep_spatial()
        for o, b in zip(refs, before):
            o.sweep_spatial()
            pat += panel_patterns(b, o.conf(), n)
        compare()
        for w, o in enumerate(refs):  # (also between the calls: a draw counter that runs ahead shows at once)
            assert mc.uniforms_used(w) == o.uniforms_used()
    prop = acc = 0
    for w, o in enumerate(refs):
        a, st = mc.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
        assert mc.uniforms_used(w) == o.uniforms_used()
        prop, acc = prop + st.prop_local, acc + st.acc_local
    mc.close()
    rate = acc / prop
    print("%s %s, %d walkers, %d updates: worst rel |G - G_oracle| = %.3g, acceptance %.3f, last panels all accepted / "
          "all rejected / mixed = %d / %d / %d" % (shape, kind, walkers, nupd, worst, rate, pat[0], pat[1], pat[2]))
    return worst, rate, pat


CASES = [
    pytest.param(("chain", 64), "attractive", id="chain64-attractive-three_full_handovers"),
    pytest.param(("chain", 64), "repulsive", id="chain64-repulsive-three_full_handovers"),
    pytest.param(("chain", 33), "attractive", id="chain33-attractive-into_one_site_block"),
    pytest.param(("chain", 33), "repulsive", id="chain33-repulsive-into_one_site_block"),
    pytest.param(("chain", 47), "attractive", id="chain47-attractive-block_ends_at_c14"),
    pytest.param(("chain", 47), "repulsive", id="chain47-repulsive-block_ends_at_c14"),
    pytest.param(("square", 6), "attractive", id="square6-attractive-blocks_16_16_4"),
]


@pytest.mark.parametrize("shape,kind", CASES)
def test_standalone_elimination_matches_oracle(gpu, O, shape, kind):
    """beta = 1, safe_mult = 5, 2 walkers: prepare + 2 x slices + 3 updates (both directions, both wraps)"""
    _, _, pat = run_case(gpu, O, shape, kind, 2, 23, fused=False)
    assert pat.sum() == 2 * 23 * len(last_panels(shape[1] if shape[0] == "chain" else shape[1] ** 2))


def test_last_panel_tables():
    """the blocks the cases are named after (no GPU involved, but kept beside the cases it describes)"""
    assert last_panels(64) == [(12, 16), (28, 16), (44, 16)]
    assert last_panels(33) == [(12, 16), (28, 1)]
    assert last_panels(47) == [(12, 16), (28, 15)]   # the third block has sites c = 0..14: no site 15, no hand-over out
    assert last_panels(36) == [(12, 16), (28, 4)]
    assert len(last_panels(256)) == 12


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_fused_launches_match_oracle(gpu, O, kind):
    """16 x 16, 2 walkers, beta = 0.3 (3 slices, safe_mult = 3): up and back, 8 updates; chunks 1..3 of every slice are
    eliminated inside the fused launch, with the previous chunk pending"""
    _, _, pat = run_case(gpu, O, ("square", 16), kind, 2, 8, beta=0.3, safe_mult=3, fused=True)
    assert pat.sum() == 2 * 8 * 12


def test_mostly_rejected_last_panels(gpu, O):
    """Chain(64) attractive, U = 1, every walker fed uniforms just below 1: only the proposals with p > 1 (which consume
    no uniform) are accepted, 17.0 % in the oracle, so the x = 0 stream runs in every last panel: of the 138, 84 are
    rejected whole, 54 mixed, none accepted whole (the oracle's figures; the HS field is compared bit for bit, so they are
    exact).  Strong coupling lowers the acceptance of the seeded stream as well (U = 8, dtau = 0.2: 0.29; small U raises
    it: 0.99 at U = 0.1), but there G already differs from the oracle by 1.45e-10 after the first sweep_spatial, in this
    build and in its parent alike (the same figure), which is not the hand-over's doing: the case stays at U = 1."""
    uni = np.full(64 * 30, 1.0 - 2.0 ** -53)
    _, rate, pat = run_case(gpu, O, ("chain", 64), "attractive", 2, 23, uniforms=uni)
    assert 0.16 < rate < 0.18
    assert tuple(pat) == (0, 84, 54)


def test_all_accepted_last_panels(gpu, O):
    """recorded uniforms u = 0: every proposal is accepted, all 69 last panels whole (Chain(64), attractive, 1 walker)"""
    _, rate, pat = run_case(gpu, O, ("chain", 64), "attractive", 1, 23, uniforms=np.zeros(64 * 30))
    assert rate == 1.0 and tuple(pat) == (69, 0, 0)
