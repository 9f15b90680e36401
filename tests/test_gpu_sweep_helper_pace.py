"""The helper waves of the four-wave elimination (sweep_lu.hip, lu4_wave) take the x of a panel's four sites in ONE read
of sm.xs behind the flag of the panel's last site (lane group g: site g of the panel; 0 for a rejected site) instead of a
read and a select per site.  Every case goes through the engine and is compared with the CPU oracle one propagate /
sweep_spatial at a time: HS field bit for bit, uniforms consumed and acceptance counters equal, G within 1e-10.

  Chain(128)   the fused form at its smallest admitted size (two chunks per slice), both models, one full sweep at beta = 1
  16 x 16      four chunks per slice, hence all three hand-overs and every panel-end read in fused launches, both models,
               two slices up and back
  Chain(128)   acceptance patterns, on the same field and the same recorded uniforms as the oracle: panels rejected whole
               (u just below 1), a block of which only site 15 is accepted (one uniform of that stream set to 0: found
               with the oracle alone), every site accepted (U = 0.1 and u = 0)
  10 x 10      n = 100 is no multiple of 64: split form, second chunk of 36 sites (FULL == false: the x are read at the
               panel end), both models and the mostly rejected stream
The launch form of every case is asserted from mc.launch_plan(), restated by tests/launch_rules.py."""
import numpy as np
import pytest
import torch  # (at import time, before the library opens the device: imported later it reports no HIP device)

import launch_rules
from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10
U_REJECT = 1.0 - 2.0 ** -53


def make_model(pkg, shape, kind, U):
    l = pkg.SquareLattice(shape[1]) if shape[0] == "square" else pkg.Chain(shape[1])
    cls = pkg.HubbardModelAttractive if kind == "attractive" else pkg.HubbardModelRepulsive
    return cls(l=l, U=U)


def make_oracle(O, model, kind, conf, par, seed=None, uniforms=None):
    o = O.OracleDQMC(model.l.sites, kind, beta=par["beta"], delta_tau=par["delta_tau"], safe_mult=par["safe_mult"],
                     U=model.U, hopping=model.hopping_matrix()[0])
    o.set_conf(conf)
    if uniforms is not None:
        o.set_uniforms(uniforms)
    else:
        o.seed(seed)
    return o


def panel_counts(before, after):
    """(panels of four sites accepted whole, rejected whole, mixed; blocks of 16 of which exactly site 15 flipped) of one
    sweep_spatial, from the HS field around it"""
    flipped = before != after
    cols = np.nonzero(flipped.any(axis=0))[0]
    assert len(cols) <= 1
    n = before.shape[0]
    f = flipped[:, cols[0]] if len(cols) else np.zeros(n, dtype=bool)
    k = np.array([int(f[s:s + 4].sum()) for s in range(0, n - n % 4, 4)])
    only15 = sum(1 for s in range(0, n - 15, 16) if f[s + 15] and not f[s:s + 15].any())
    return np.array([(k == 4).sum(), (k == 0).sum(), ((k > 0) & (k < 4)).sum(), only15])


def crafted_conf(walker, n, slices):
    """the HS field the crafted case starts from (fixed, so that the search below finds the same block on every run)"""
    return np.random.default_rng(1000 + walker).choice(np.array([-1, 1], dtype=np.int8), size=(n, slices))


def only_site_15_stream(O, model, kind, conf, par, nupd, length):
    """A stream of uniforms just below 1 (every proposal that draws is rejected) with ONE entry set to 0: the draw of
    site 15 of the first block of 16 sites in which no proposal has p > 1, among blocks 0..2 of a chunk of 64: block 3
    is the last wave's own and has no helper, so it would not reach the panel read.  That site is then accepted and the
    15 before it are rejected; what was decided before that draw does not depend on it.  Found with the oracle alone.
    Returns the stream and (update, first site of the block)."""
    u = np.full(length, U_REJECT)
    o = make_oracle(O, model, kind, conf, par, uniforms=u)
    o.prepare()
    for k in range(nupd):
        o.propagate()
        used, before = o.uniforms_used(), o.conf()
        o.sweep_spatial()
        flipped = before != o.conf()
        cols = np.nonzero(flipped.any(axis=0))[0]
        f = flipped[:, cols[0]] if len(cols) else np.zeros(before.shape[0], dtype=bool)
        for s0 in range(0, before.shape[0] - 15, 16):
            if (s0 % 64) // 16 < 3 and not f[s0:s0 + 16].any():
                u[used + int((~f[:s0 + 15]).sum())] = 0.0  # every site that did not flip drew once, in site order
                return u, (k, s0)
    raise AssertionError("no block of 16 drawn proposals with helper waves in %d updates" % nupd)


def run_case(gpu, O, shape, kind, nupd, fused, walkers=2, beta=1.0, delta_tau=0.1, safe_mult=5, U=1.0, uniforms=None,
             craft=False):
    """prepare, then nupd x (propagate, sweep_spatial), compared after every call.  Returns the oracle's acceptance, the
    panel counts, the directions seen and per update the counts of walker 0"""
    par = dict(beta=beta, delta_tau=delta_tau, safe_mult=safe_mult)
    model = make_model(gpu, shape, kind, U)
    mc = gpu.DQMC(model, n_walkers=walkers, seed=31, **par)
    n = mc.N
    plan = mc.launch_plan()
    caps = dict(cus=plan["cus"])
    assert bool(plan["sweep_fused"]) == launch_rules.sweep_fused(n, walkers, mc.nb, caps) == fused, plan
    streams = [uniforms] * walkers
    crafted = None
    if craft:
        streams, crafted = [], []
        for w in range(walkers):
            mc.set_conf(w, crafted_conf(w, n, mc.p.slices))
            u, where = only_site_15_stream(O, model, kind, mc.conf(w), par, nupd, n * (nupd + 2))
            streams.append(u)
            crafted.append(where)
    refs = []
    for w in range(walkers):
        if streams[w] is not None:
            mc.set_uniforms(w, streams[w])
        refs.append(make_oracle(O, model, kind, mc.conf(w), par, mc.seeds[w], streams[w]))
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
    pat = np.zeros(4, dtype=int)
    per_update = [[] for _ in range(walkers)]
    directions = set()
    for _ in range(nupd):
        mc.propagate()
        for o in refs:
            o.propagate()
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        directions.add(mc.direction)
        compare(conf=False)
        before = [o.conf() for o in refs]
        mc.sweep_spatial()
        for w, (o, b) in enumerate(zip(refs, before)):
            o.sweep_spatial()
            c = panel_counts(b, o.conf())
            per_update[w].append((b != o.conf()).any(axis=1))
            pat += c
        compare()
        for w, o in enumerate(refs):
            assert mc.uniforms_used(w) == o.uniforms_used()
    prop = acc = 0
    for w, o in enumerate(refs):
        a, st = mc.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
        prop, acc = prop + st.prop_local, acc + st.acc_local
    assert mc.device_errors() == 0
    mc.close()
    print("%s %s, %d walkers, %d updates, %s: worst rel |G - G_oracle| = %.3g, acceptance %.3f, panels accepted whole / "
          "rejected whole / mixed = %d / %d / %d, blocks with only site 15 accepted %d" % (
              shape, kind, walkers, nupd, "fused" if fused else "split", worst, acc / prop, pat[0], pat[1], pat[2], pat[3]))
    return acc / prop, pat, directions, per_update, crafted


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_fused_form_at_its_smallest_size(gpu, O, kind):
    """Chain(128), 2 walkers, beta = 1: one full sweep (10 slices up and back); chunk 1 of every slice is eliminated in
    the fused launch beside the flush of chunk 0"""
    _, pat, directions, _, _ = run_case(gpu, O, ("chain", 128), kind, 20, fused=True)
    assert len(directions) == 2
    assert pat[:3].sum() == 2 * 20 * 32


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_four_chunks_up_and_down(gpu, O, kind):
    """16 x 16, 2 walkers, beta = 0.2 (2 slices, safe_mult = 2): 4 updates, a slice in each direction at least; four
    chunks per slice: three hand-overs and sixteen panel ends per chunk, three of the chunks in fused launches"""
    _, pat, directions, _, _ = run_case(gpu, O, ("square", 16), kind, 4, fused=True, beta=0.2, safe_mult=2)
    assert len(directions) == 2
    assert pat[:3].sum() == 2 * 4 * 64


def test_panels_rejected_whole(gpu, O):
    """uniforms just below 1: only proposals with p > 1 (which draw nothing) are accepted, so most panels bring x = 0 for
    all four sites, and a panel with one accepted site brings three zeros"""
    _, pat, _, _, _ = run_case(gpu, O, ("chain", 128), "attractive", 10, fused=True,
                               uniforms=np.full(128 * 12, U_REJECT))
    assert pat[0] < pat[:3].sum() and pat[1] > 0 and pat[2] > 0  # (the oracle's counts: the patterns were there)


def test_only_site_15_of_a_block_accepted(gpu, O):
    """the x of site 15 comes with the last panel's read (the site has no payload); the three sites before it bring 0"""
    _, pat, _, per_update, crafted = run_case(gpu, O, ("chain", 128), "attractive", 12, fused=True, craft=True)
    for w, (k, s0) in enumerate(crafted):
        f = per_update[w][k]
        assert (s0 % 64) // 16 < 3, (w, k, s0)  # a block that has helper waves: its last panel's read brings the x
        assert f[s0 + 15] and not f[s0:s0 + 15].any(), (w, k, s0)
    assert pat[3] >= 1


def test_every_site_accepted(gpu, O):
    """U = 0.1: nearly every proposal has p > 1 and draws nothing; the rest draw u = 0 and are accepted as well"""
    rate, pat, _, _, _ = run_case(gpu, O, ("chain", 128), "attractive", 6, fused=True, U=0.1,
                                  uniforms=np.zeros(128 * 8))
    assert rate == 1.0
    assert tuple(pat[:3]) == (2 * 6 * 32, 0, 0)


@pytest.mark.parametrize("kind,uniforms", [("attractive", None), ("repulsive", None),
                                           ("attractive", np.full(100 * 10, U_REJECT))],
                         ids=["attractive", "repulsive", "attractive-mostly_rejected"])
def test_short_last_chunk(gpu, O, kind, uniforms):
    """10 x 10: chunks of 64 and 36 sites (blocks 16 / 16 / 4), stand-alone eliminations; beta = 0.3 (3 slices), up and
    back"""
    _, pat, directions, _, _ = run_case(gpu, O, ("square", 10), kind, 8, fused=False, beta=0.3, safe_mult=3,
                                        uniforms=uniforms)
    assert len(directions) == 2
    assert pat[:3].sum() == 2 * 8 * 25
