"""Checkpoint and resume on the device (include/dqmc_hip.h "checkpoint and resume"; csrc/checkpoint.inl, state_blob.cpp;
dqmc.py: state / set_state / save / load / run(checkpoint=...)).

What "resumed" means: the import rebuilds the stack and G from the HS field, so a resumed chain agrees with the
uninterrupted one as device and oracle agree in test_gpu_dqmc.py (TOL, taken from there), not to the bit.  Exact are
(a) the payload through export and import, (b) the exporting chain's future, (c) the futures of two imports of one blob.

The chains are moved from measurement point to measurement point (prepare, update_until_measure, then whole sweeps), the
one place where the engine exports.  Shapes: SquareLattice(4) attractive and repulsive at beta = 1, delta_tau = 0.1,
safe_mult = 5, 2 walkers; TriangularLattice(4) repulsive at U = 12, beta = 2 with seed 2, where the two walkers' fields have
opposite signs over the sweeps the tests run (found by a scan over U, beta and seeds; test_round_trip_is_exact asserts it); SquareLattice(16) attractive with slices = 10: the pending sweep
chunk, the one-launch wrap and the one-launch UDT exist only at n = 256."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_tables as LT  # noqa: E402  (the package's iterators over all pairs at once: affordable at 16 x 16)
from test_gpu_dqmc import TOL  # noqa: E402  (the device-against-oracle bound on G)

pytestmark = pytest.mark.gpu

SHAPES = {"sq4_attractive": ("attractive", "square", 4), "sq4_repulsive": ("repulsive", "square", 4),
          "tri4_repulsive": ("repulsive", "triangular", 4), "sq16_attractive": ("attractive", "square", 16)}
SMALL = ["sq4_attractive", "sq4_repulsive", "tri4_repulsive"]
SECTIONS = ("greens", "correlations", "pairing", "susceptibilities", "time_displaced")
CAPACITY = 7  # three levels; no test pushes more than six samples


def model_of(gpu, shape, U=None):
    kind, lat, L = SHAPES[shape]
    l = gpu.SquareLattice(L) if lat == "square" else gpu.TriangularLattice(L)
    if kind == "attractive":
        return gpu.HubbardModelAttractive(l=l, U=1.0 if U is None else U, mu=0.3)
    return gpu.HubbardModelRepulsive(l=l, U=(12.0 if lat == "triangular" else 4.0) if U is None else U)


_tables = {}


def tables(l):
    """(pair directions, local quads, synced quads) of a lattice, built once"""
    key = (type(l).__name__, l.sites)
    if key not in _tables:
        pairs = LT.fast_pairs(l)
        _tables[key] = (pairs, LT.fast_quads(l, pairs=pairs), LT.fast_quads(l, pairs=pairs, synced=True))
    return _tables[key]


def make(gpu, shape, full=True, n_walkers=2, beta=None, capacity=CAPACITY, pairing=True, sign=None, model=None, **kw):
    """a prepared object at its measurement point; full: every measurement, binner, global moves at rate 1, sign weighting
    on the repulsive model; else Green's function, correlations and pairing with the Green's binner"""
    m = model_of(gpu, shape) if model is None else model
    sign = (m.kind == 1) if sign is None else sign
    tri = SHAPES[shape][1] == "triangular"
    beta = (2.0 if tri else 1.0) if beta is None else beta
    kw.setdefault("seed", 2 if tri else 4242)
    mc = gpu.DQMC(m, n_walkers=n_walkers, beta=beta, delta_tau=0.1, safe_mult=5, global_moves=full, global_rate=1,
                  sign_weighting=sign, thermalization=0, sweeps=0, measure_rate=1, **kw)
    try:
        pairs, local, synced = tables(m.l)
        if pairing:
            mc.set_local_targets(local)
        else:
            mc.set_pair_directions(pairs)
        if full:
            mc.set_current_targets(synced)
            mc.set_time_displaced(5, ("greens", "density"))
        mc.prepare()
        if full:
            mc._section_size("susceptibilities")  # lays the section out, as its first accumulate call would
        mc.enable_binning(SECTIONS if full else ("greens",), capacity=capacity)
        mc.update_until_measure()
        assert (mc.current_slice, mc.direction) == (1, 1)
    except BaseException:
        mc.close()
        raise
    mc._test_full, mc._test_pairing = full, pairing
    return mc


def advance(mc, sweeps):
    """whole sweeps from measurement point to measurement point, every configured measurement taken at each"""
    for _ in range(sweeps):
        mc.sweep(1)
        assert (mc.current_slice, mc.direction) == (1, 1)
        mc.accumulate_greens()
        mc.accumulate_correlations()
        if mc._test_pairing:
            mc.accumulate_pairing()
        if mc._test_full:
            mc.accumulate_susceptibilities(recalculate=mc.p.safe_mult)  # feeds the time-displaced rows as well


def sections_of(mc):
    secs = ["greens", "correlations"] + (["pairing"] if mc._test_pairing else [])
    return secs + (["susceptibilities", "time_displaced"] if mc._test_full else [])


def snapshot(mc, greens_eff=False):
    """everything the payload carries, read back through the public getters"""
    from montecarlo_jl_amd import _lib
    import ctypes as C
    s = {}
    for w in range(mc.n_walkers):
        s["conf%d" % w] = mc.conf(w)
        s["uniforms_used%d" % w] = np.array(mc.uniforms_used(w))
        a = mc.analysis(w)
        s["analysis%d" % w] = np.array([a.prop_local, a.acc_local, a.prop_global, a.acc_global] +
                                       [getattr(getattr(a, f), k) for f in ("negative_probability", "propagation_error")
                                        for k in ("max", "min", "sum", "count")], dtype=np.float64)
        g, last = mc.global_stats(w), mc.global_last(w)
        s["global%d" % w] = np.array([g["prop_global"], g["acc_global"], g["moves_drawn"], last["p"], last["accepted"],
                                      last["site"]], dtype=np.float64)
        if greens_eff:
            s["greens_eff%d" % w] = np.stack(mc.greens_eff(w))
    s["sign_failures"] = mc.sign_failures()
    secs = sections_of(mc)
    for sec in secs + ["sign"]:
        s["sums:" + sec] = mc._section(sec)
    binned = secs if mc._test_full else ["greens"]
    for sec in binned:
        ids = [(sec, mc._bin(sec))]
        if mc.sign_weighting():
            ids.append(("sign:" + sec, _lib.BIN_SIGN + SECTIONS.index(sec)))
        for name, bid in ids:
            n, L, T = C.c_size_t(), C.c_int32(), C.c_int64()
            mc._c(_lib.lib().dqmc_binner_size(mc._h, bid, C.byref(n), C.byref(L), C.byref(T)))
            s["pushes:" + name] = np.array(T.value)
            for w in range(mc.n_walkers):
                for lv in range(L.value):
                    xs, x2, cnt = np.zeros(n.value), np.zeros(n.value), C.c_int64()
                    mc._c(_lib.lib().dqmc_binner_get_level(mc._h, bid, w, lv, _lib.dptr(xs), _lib.dptr(x2), C.byref(cnt)))
                    s["bin:%s:w%d:l%d" % (name, w, lv)] = np.concatenate([xs, x2, [cnt.value]])
    return s


def assert_identical(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k], equal_nan=k.startswith("global")), "%s differs" % k


def closing(*mcs):
    for mc in mcs:
        if mc is not None:
            mc.close()


# ---- 1. round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_round_trip_is_exact(gpu, shape):
    a = b = None
    try:
        a = make(gpu, shape)
        advance(a, 3)
        blob = a.state()
        assert blob.dtype == np.uint8 and blob.size == a.state_size()
        want = snapshot(a)
        # the field part of the payload is what dqmc_get_conf_bits hands out, walker by walker, right behind the header
        # (whose size is the u32 at byte 12)
        head = int.from_bytes(bytes(blob[12:16]), "little")
        bits = np.concatenate([a.conf_bits(w).chunks for w in range(a.n_walkers)]).astype("<u8")
        assert head == 560 and np.array_equal(blob[head:head + 8 * bits.size], bits.view(np.uint8))
        if a.model.kind == 1:
            print("%s: sums of signs %s over %g samples" % (shape, want["sums:sign"].tolist(), want["sums:greens"][-1]))
        if shape == "tri4_repulsive":  # signs of both values are in the sums and the sign binners
            assert np.all(np.abs(want["sums:sign"]) < want["sums:greens"][-1])
        assert want["sums:greens"][-1] + a.sign_failures().sum() == 3 * a.n_walkers and want["pushes:greens"] == 3
        assert all(a.global_stats(w)["prop_global"] == 3 for w in range(2))
        b = make(gpu, shape, seed=99)  # other fields, other cursors: all of it is replaced
        b.set_state(blob)
        assert (b.current_slice, b.direction) == (1, 1)
        assert_identical(want, snapshot(b))
        assert np.array_equal(b.state(), blob)  # and it exports the same bytes again
        # G is the rebuilt one: the propagated G of the exporting chain within the parity bound
        for w in range(2):
            for ga, gb in zip(a.greens(w), b.greens(w)):
                assert np.abs(ga - gb).max() / np.abs(ga).max() < TOL
    finally:
        closing(a, b)


# ---- 2. export is read-only ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sq4_attractive", "sq4_repulsive", "sq16_attractive"])
def test_export_leaves_the_chain_alone(gpu, shape):
    a = b = None
    try:
        a, b = make(gpu, shape), make(gpu, shape)
        if shape == "sq16_attractive":  # the forms an export that wrote something would disturb
            plan = b.launch_plan()
            assert b.kron_hopping() and plan["sweep_fused"] and plan["udt_sites"] and any(plan["wrap_one_launch"])
        advance(a, 2)
        advance(a, 2)
        advance(b, 2)
        blob = b.state()
        blob2 = b.state()
        assert np.array_equal(blob, blob2)
        advance(b, 2)
        assert_identical(snapshot(a, greens_eff=True), snapshot(b, greens_eff=True))
    finally:
        closing(a, b)


# ---- 3. determinism of import ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sq4_repulsive", "sq16_attractive"])
def test_two_imports_have_one_future(gpu, shape):
    a = b = c = None
    try:
        a = make(gpu, shape)
        advance(a, 2)
        blob = a.state()
        b, c = make(gpu, shape, seed=1), make(gpu, shape, seed=2)
        b.set_state(blob)
        c.set_state(blob)
        assert_identical(snapshot(b, greens_eff=True), snapshot(c, greens_eff=True))
        advance(b, 2)
        advance(c, 2)
        assert_identical(snapshot(b, greens_eff=True), snapshot(c, greens_eff=True))
    finally:
        closing(a, b, c)


# ---- 4. against the uninterrupted run -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
def test_resumed_run_against_the_uninterrupted_one(gpu, shape):
    """A: 2 + 2 sweeps; B: A's blob at sweep 2, 2 sweeps.  The fields are the same, G at the last measurement point within
    TOL (test_gpu_dqmc.py), the sample counts equal, and the sums within TOL per sample: |sum_A - sum_B| <= TOL count
    max(1, max|sum_A| / count), the samples being sums of products of at most two entries of G over the sites, divided by
    the sites, of the size of the section's mean or of order one where the signed mean cancels."""
    a = b = None
    try:
        a = make(gpu, shape)
        advance(a, 2)
        blob = a.state()
        advance(a, 2)
        b = make(gpu, shape, seed=7)
        b.set_state(blob)
        advance(b, 2)
        for w in range(2):
            assert np.array_equal(a.conf(w), b.conf(w))
            assert a.uniforms_used(w) == b.uniforms_used(w)
            for ga, gb in zip(a.greens(w), b.greens(w)):
                err = np.abs(ga - gb).max() / np.abs(ga).max()
                print("%s walker %d: G resumed against uninterrupted %.3g" % (shape, w, err))
                assert err < TOL
        for sec in SECTIONS:
            sa, sb = a._section(sec), b._section(sec)
            cnt = sa[-1]
            assert cnt == sb[-1] and cnt > 0
            err, scale = np.abs(sa[:-1] - sb[:-1]).max(), max(1.0, np.abs(sa[:-1]).max() / cnt)
            print("%s %s: sums differ by %.3g over %g samples (scale %.3g)" % (shape, sec, err, cnt, scale))
            assert err <= TOL * cnt * scale
        assert np.array_equal(a._section("sign"), b._section("sign"))
    finally:
        closing(a, b)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def light_blob(gpu):
    a = make(gpu, "sq4_attractive", full=False)
    try:
        advance(a, 1)
        return a.state()
    finally:
        a.close()


def flipped_magic(blob):
    bad = blob.copy()
    bad[0] ^= 0x20
    return bad


def next_version(blob):
    bad = blob.copy()
    v = int.from_bytes(bytes(bad[8:12]), "little") + 1
    bad[8:12] = np.frombuffer(v.to_bytes(4, "little"), dtype=np.uint8)
    return bad


def site_out_of_range(blob):
    """the site of walker 0's latest global move (header, 2 x 3 field chunks, 2 x 16 cursor bytes, 2 x 80 counter bytes, then
    44 bytes into the walker's 56) set to n_sites"""
    bad = blob.copy()
    at = 560 + 2 * 3 * 8 + 2 * 16 + 2 * 80 + 44
    assert int.from_bytes(bytes(bad[at:at + 4]), "little") == 0  # (no global move was made)
    bad[at:at + 4] = np.frombuffer((16).to_bytes(4, "little"), dtype=np.uint8)
    return bad


REFUSALS = {
    "n_walkers": (dict(n_walkers=3), None, "n_walkers"),
    "slices": (dict(beta=2.0), None, "slices"),
    "model_kind": (dict(model="repulsive", sign=False), None, "model_kind"),
    "binner_capacity": (dict(capacity=15), None, "binner greens"),
    "section_on_one_side": (dict(pairing=False), None, "section pairing"),
    "sign_weighting_on_one_side": (dict(sign=True), None, "sign_on"),
    "truncated": ({}, lambda blob: blob[:-1], "n_bytes"),
    "trailing_byte": ({}, lambda blob: np.concatenate([blob, np.zeros(1, dtype=np.uint8)]), "n_bytes"),
    "magic": ({}, flipped_magic, "magic"),
    "version": ({}, next_version, "version"),
    "payload_site": ({}, site_out_of_range, "site"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_import_refusals_leave_the_handle_unchanged(gpu, light_blob, case):
    from montecarlo_jl_amd import _lib
    kw, damage, field = REFUSALS[case]
    kw = dict(kw)
    if kw.get("model") == "repulsive":
        kw["model"] = gpu.HubbardModelRepulsive(l=gpu.SquareLattice(4), U=1.0)
    y = z = None
    try:
        y, z = make(gpu, "sq4_attractive", full=False, **kw), make(gpu, "sq4_attractive", full=False, **kw)
        advance(y, 1)
        advance(z, 1)
        blob = light_blob if damage is None else damage(light_blob)
        with pytest.raises(_lib.DQMCError) as e:
            y.set_state(blob)
        print("%s: %s" % (case, e.value))
        assert e.value.code == _lib.ERR_INVALID and field in str(e.value)
        advance(y, 1)
        advance(z, 1)
        assert_identical(snapshot(y, greens_eff=True), snapshot(z, greens_eff=True))
    finally:
        closing(y, z)


# ---- 6. export state errors ------------------------------------------------------------------------------------------
def test_export_away_from_the_measurement_point(gpu):
    from montecarlo_jl_amd import _lib
    a = make(gpu, "sq4_attractive", full=False)
    try:
        a.state()
        a.update()
        assert (a.current_slice, a.direction) != (1, 1)
        with pytest.raises(_lib.DQMCError) as e:
            a.state()
        assert e.value.code == _lib.ERR_STATE and "measurement point" in str(e.value)
        a.close()
        a = gpu.DQMC(model_of(gpu, "sq4_attractive"), beta=1.0, safe_mult=5)
        with pytest.raises(_lib.DQMCError) as e:  # never prepared
            a.state()
        assert e.value.code == _lib.ERR_STATE
    finally:
        a.close()


def test_export_with_host_uniforms(gpu):
    from montecarlo_jl_amd import _lib
    a = gpu.DQMC(model_of(gpu, "sq4_attractive"), n_walkers=2, beta=1.0, safe_mult=5)
    try:
        a.set_uniforms(1, np.random.Generator(np.random.Philox(key=3)).random(16 * 10 * 4))
        a.prepare()
        a.update_until_measure()
        with pytest.raises(_lib.DQMCError) as e:
            a.state()
        assert e.value.code == _lib.ERR_STATE and "uniform" in str(e.value) and "walker 1" in str(e.value)
        a.seed(1, 5)  # back on its Philox stream
        a.state()
    finally:
        a.close()


# ---- 7. the Python level ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sq4_repulsive", "sq16_attractive"])
def test_save_and_load_round_trip(gpu, shape, tmp_path):
    from montecarlo_jl_amd import checkpoint
    a = b = None
    try:
        a = make(gpu, shape, seed=77, first_walker=5)
        advance(a, 3)
        p = tmp_path / "walkers5.ckpt"
        a.save(p)
        assert os.listdir(tmp_path) == ["walkers5.ckpt"]
        pre, blob = checkpoint.read(p)
        assert np.array_equal(blob, a.state()) and pre["last_sweep"] == 0 and not pre["mid_sweep"]
        assert pre["dqmc"]["first_walker"] == 5 and pre["dqmc"]["seed"] == 77
        b = gpu.DQMC.load(p)
        b._test_full, b._test_pairing = True, True
        assert type(b.model) is type(a.model) and type(b.model.l) is type(a.model.l) and b.N == a.N
        assert (b.model.U, b.model.t, b.model.mu) == (a.model.U, a.model.t, a.model.mu)
        assert b.seeds == a.seeds == [82, 83] and b._ctor == a._ctor and b.p == a.p
        assert b.sign_weighting() == a.sign_weighting() and b.time_displaced_plan() == a.time_displaced_plan()
        assert (b.current_slice, b.direction) == (1, 1)
        assert_identical(snapshot(a), snapshot(b))
        advance(b, 1)  # and it runs on, every measurement configured
    finally:
        closing(a, b)


def test_ranks_save_distinct_walkers(gpu, tmp_path):
    objs = []
    try:
        for rank in range(2):
            mc = make(gpu, "sq4_attractive", full=False, seed=11, first_walker=2 * rank)
            objs.append(mc)
            advance(mc, 1)
            mc.save(tmp_path / ("rank%d.ckpt" % rank))
        back = [gpu.DQMC.load(tmp_path / ("rank%d.ckpt" % rank)) for rank in range(2)]
        objs += back
        assert [b.seeds for b in back] == [[11, 12], [13, 14]]
        for rank in range(2):
            for w in range(2):
                assert np.array_equal(back[rank].conf(w), objs[rank].conf(w))
                assert back[rank].uniforms_used(w) == objs[rank].uniforms_used(w)
        assert not np.array_equal(back[0].conf(0), back[1].conf(0))
    finally:
        closing(*objs)


def test_global_rate_set_after_construction_is_saved(gpu, tmp_path):
    a = b = None
    try:
        a = make(gpu, "sq4_attractive", full=False)  # constructed without global moves
        a.set_global_rate(1, "all")
        advance(a, 2)
        assert a.global_stats(0)["prop_global"] == 2
        a.save(tmp_path / "gm.ckpt")
        b = gpu.DQMC.load(tmp_path / "gm.ckpt")
        b._test_full, b._test_pairing = False, True
        assert b.global_stats(0) == a.global_stats(0)
        advance(b, 1)
        assert b.global_stats(0)["prop_global"] == 3 and b.global_last(0)["site"] == 0  # a move of kind "all"
    finally:
        closing(a, b)


def run_object(gpu, **kw):
    m = gpu.HubbardModelAttractive(l=gpu.SquareLattice(4), U=1.0, mu=0.3)
    mc = gpu.DQMC(m, n_walkers=2, beta=1.0, delta_tau=0.1, safe_mult=5, seed=31, thermalization=2, sweeps=4, measure_rate=1,
                  global_moves=True, global_rate=2, **kw)
    mc.set_pair_directions(tables(m.l)[0])
    return mc


def test_run_with_checkpoints_and_resume(gpu, tmp_path):
    """run(checkpoint=p, checkpoint_every=2) over 6 sweeps: the file is whole whenever it is looked at, ends at sweep 6 and
    no temporary stays; the copy taken while it held sweep 4 resumes into exactly the rest: the up pass of sweep 4 and
    sweeps 5 and 6, i.e. (1 + 2 * 2) * slices updates of n_sites proposals each"""
    from montecarlo_jl_amd import checkpoint
    p, p4 = tmp_path / "run.ckpt", tmp_path / "at4.ckpt"
    seen = []
    a = b = None

    def look(mc, i):
        if os.path.exists(p):
            pre, blob = checkpoint.read(p)  # raises on a partial file
            seen.append((i, pre["last_sweep"]))
            if i == 5:
                shutil.copy(p, p4)
        assert [f for f in os.listdir(tmp_path) if f.endswith(".tmp")] == []
    try:
        a = run_object(gpu)
        a.run(measurements=("greens", "correlations"), binning=True, on_measure=look, checkpoint=p, checkpoint_every=2)
        assert seen == [(3, 2), (4, 2), (5, 4), (6, 4)]
        assert sorted(os.listdir(tmp_path)) == ["at4.ckpt", "run.ckpt"]
        pre, _ = checkpoint.read(p)
        assert pre["last_sweep"] == 6 and pre["mid_sweep"] and a.last_sweep == 6
        assert pre["binning"]["sections"] == {"greens": 0, "correlations": 0}

        b = gpu.DQMC.load(p4)
        assert b.last_sweep == 4 and (b.current_slice, b.direction) == (1, 1)
        assert b.accumulators()[-1] == 2 * 2 and b.binner_size("greens")[2] == 2  # sweeps 3 and 4 measured
        before = [b.analysis(w).prop_local for w in range(2)]
        b.run(measurements=("greens", "correlations"), binning=True)
        assert b.last_sweep == 6
        for w in range(2):
            assert b.analysis(w).prop_local - before[w] == (1 + 2 * 2) * b.p.slices * b.N
            assert b.analysis(w).prop_local == a.analysis(w).prop_local
            assert b.global_stats(w) == a.global_stats(w) and b.global_stats(w)["prop_global"] == 3  # sweeps 2, 4, 6
            assert np.array_equal(b.conf(w), a.conf(w)) and b.uniforms_used(w) == a.uniforms_used(w)
        for sec in ("greens", "correlations"):
            sa, sb = a._section(sec), b._section(sec)
            assert sa[-1] == sb[-1] == 4 * 2
            assert np.abs(sa - sb).max() <= TOL * sa[-1] * max(1.0, np.abs(sa[:-1]).max() / sa[-1])
        assert b.binner_size("greens")[2] == a.binner_size("greens")[2] == 4
        # an object whose run() has returned stands at (slices, -1): no export there
        from montecarlo_jl_amd import _lib
        assert (a.current_slice, a.direction) == (a.p.slices, -1)
        with pytest.raises(_lib.DQMCError) as e:
            a.save(tmp_path / "late.ckpt")
        assert e.value.code == _lib.ERR_STATE and not os.path.exists(tmp_path / "late.ckpt")
        # a loaded object saved again before it runs is still inside sweep 4: the copy resumes like the original
        b.close()
        b = gpu.DQMC.load(p4)
        b.save(tmp_path / "again.ckpt")
        pre, _ = checkpoint.read(tmp_path / "again.ckpt")
        assert pre["last_sweep"] == 4 and pre["mid_sweep"]
        b.close()
        b = gpu.DQMC.load(tmp_path / "again.ckpt")
        b.run(measurements=("greens", "correlations"), binning=True)
        for w in range(2):
            assert b.last_sweep == 6 and b.analysis(w).prop_local == a.analysis(w).prop_local
            assert b.global_stats(w) == a.global_stats(w) and np.array_equal(b.conf(w), a.conf(w))
        # a file of the last sweep resumes into the rest of that sweep and nothing else
        b.close()
        b = gpu.DQMC.load(p)
        before = b.analysis(0).prop_local
        b.run(measurements=("greens", "correlations"), binning=True)
        assert b.last_sweep == 6 and b.analysis(0).prop_local - before == b.p.slices * b.N
        assert b.accumulators()[-1] == 4 * 2
    finally:
        closing(a, b)
