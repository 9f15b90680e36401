"""Checkpoint and resume of the q-state engine on the device (dqmc_qs_state_*, QStateMC.save / load / run(checkpoint=...)).

The same seeds go into two objects: A runs 2n sweeps; B runs n sweeps, is saved, closed, loaded into a fresh object and
runs the rest.  Everything is compared with ==: the state blobs byte for byte, the series, measurements and binned dicts.
The split sweep is no multiple of the cluster or exchange rate, and the binner stands at T = 7 there (low three bits set:
three pending compressor values travel), or between two measurements with measure_rate 3.  The all-on case is also
compared with the numpy restatements run straight through."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref as ref  # noqa: E402
import qstate_cluster_ref as cref  # noqa: E402,F401  (the cluster move under the tempering restatement)
import qstate_tempering_ref as tref  # noqa: E402

pytestmark = pytest.mark.gpu

SIGNED = [1.0, -0.5, 0.25, -0.5]  # a signed pair-energy table, q = 4


def _make(g, case, **over):
    """a fresh object of a named case; `over` replaces constructor keywords"""
    if case == "potts3_rect35":  # N = 15: a padding byte in the last word; odd extents: more than 2 colours
        model, kw = g.PottsModel(3, l=g.RectangularLattice(3, 5)), dict(beta=[0.9, 1.0, 1.1], n_walkers=3, binner=64)
    elif case in ("clock6_all_on", "clock6_all_on_rate3"):
        model = g.ClockModel(6, l=g.SquareLattice(4))
        kw = dict(beta=[0.9, 1.0, 1.1] * 2, n_walkers=6, cluster_rate=2, tempering=(3, 2), binner=64, scaling=True,
                  stiffness=True, measure_rate=3 if case.endswith("rate3") else 1)
    elif case == "clock6_all_off":
        model, kw = g.ClockModel(6, l=g.SquareLattice(4)), dict(beta=[0.9, 1.1], n_walkers=2, series_capacity=0)
    elif case == "signed_triangular3":  # the running E is not the bonds energy of the configuration
        model = g.QStateModel(4, SIGNED, l=g.TriangularLattice(3), J=0.75)
        kw = dict(beta=[0.3, 0.5], n_walkers=2, binner=64, cluster_rate=3)
    else:
        raise KeyError(case)
    kw = dict(dict(seed=300, thermalization=4, sweeps=18, series_capacity=32), **kw)
    kw.update(over)
    mc = g.MC(model, **kw)
    assert type(mc) is g.QStateMC
    return mc


def _results(mc):
    out = {"state": mc.state().tobytes(), "last_sweep": mc.last_sweep, "replicas": mc.replicas().tolist()}
    for w in range(mc.n_walkers):
        out["series", w] = [a.tolist() for a in mc.series(w)]
        out["conf", w] = mc.conf(w).tolist()
        out["meas", w] = mc.measurements(w)
        if mc._binning is not None:
            out["binned", w] = mc.binned(w)
            if mc.k_vectors is not None:
                out["binned_scaling", w] = repr(mc.binned_scaling(w))
            if mc.stiffness_directions is not None:
                out["binned_stiffness", w] = repr(mc.binned_stiffness(w))
        if mc.k_vectors is not None:
            out["scaling", w] = repr(mc.scaling(w))
        if mc.stiffness_directions is not None:
            out["stiffness", w] = repr(mc.stiffness(w))
            out["sample", w] = [a.tolist() for a in mc.stiffness_sample(w)]
    return out


def _same(a, b, label):
    assert a.keys() == b.keys(), label
    for k in a:
        assert repr(a[k]) == repr(b[k]) if k != "state" else a[k] == b[k], (label, k)  # (repr: NaN taus compare equal)


SPLIT, TOTAL = 11, 22  # thermalization 4, measure_rate 1: T = 7 at the split; 11 is no multiple of 2 or 3


@pytest.mark.parametrize("case", ["potts3_rect35", "clock6_all_on", "clock6_all_on_rate3", "clock6_all_off",
                                  "signed_triangular3"])
def test_a_saved_and_loaded_run_continues_byte_for_byte(gpu, tmp_path, case):
    A = _make(gpu, case)
    A.sweep(TOTAL)
    B = _make(gpu, case)
    B.sweep(SPLIT)
    if B._binning is not None:
        want_T = 7 if B.measure_rate == 1 else 2  # rate 3: sweeps 6 and 9 measured, 12 is next
        assert B.binner_size()[1] == want_T, case
    if case == "potts3_rect35":
        assert int(B.colouring.max()) + 1 > 2 and B.N % 4 != 0
    mid = B.state()
    E_mid = [B.stats(w).energy_q30 for w in range(B.n_walkers)]
    path = tmp_path / "b.ckpt"
    B.save(path)
    assert np.array_equal(B.state(), mid), "export changed the handle"
    B.close()
    C2 = gpu.QStateMC.load(path)
    assert type(C2) is gpu.QStateMC and C2.last_sweep == SPLIT and C2.seeds == [300 + w for w in range(C2.n_walkers)]
    assert C2.state().tobytes() == mid.tobytes(), "the loaded object does not stand where the saved one stood"
    assert [C2.stats(w).energy_q30 for w in range(C2.n_walkers)] == E_mid  # restored, not recomputed
    if case == "signed_triangular3":
        # (the bonds table of this lattice also lists two-step bonds: a recomputed E would differ from the running one)
        assert any(C2.stats(w).energy_q30 != C2.model.energy_q30(C2.conf(w)) for w in range(2))
    C2.sweep(TOTAL - SPLIT)
    _same(_results(A), _results(C2), case)
    assert A.stats(0).n_meas > 0 and (case == "clock6_all_off" or len(A.series(0)[0]) == A.stats(0).n_meas)
    A.close()
    C2.close()


def test_the_resumed_all_on_run_matches_the_restatements_run_straight_through(gpu, tmp_path):
    """configurations, E_int, Mx, My, labels, counters, cursors, exact sums and series of the resumed run against
    qstate_tempering_ref (over qstate_cluster_ref and qstate_ref) run from sweep 1 to the end without a cut: ==."""
    B = _make(gpu, "clock6_all_on")
    B.sweep(SPLIT)
    path = tmp_path / "b.ckpt"
    B.save(path)
    B.close()
    mc = gpu.QStateMC.load(path)
    mc.sweep(TOTAL - SPLIT)
    betas = [0.9, 1.0, 1.1] * 2
    wk = tref.TemperingWalkers(gpu.SquareLattice(4), 6, ref.clock_table(6), betas, [300 + w for w in range(6)],
                               series_capacity=32, binner=64)
    wk.set_exchange(3, 2)
    wk.run(1, TOTAL, 4, 1, cluster_rate=2)
    assert wk.decided["acc"] + wk.decided["rej"] + wk.decided["free"] > 0
    for w in range(6):
        want, want_absM = wk.stats(w)
        st = mc.stats(w)
        assert {k: getattr(st, k) for k in want} == want, w
        assert abs(st.sum_absM - want_absM) <= 1e-13 * abs(want_absM)  # (the device's sqrt: the rule of test_gpu_qstate.py)
        cl, want_cl = mc.cluster_stats(w), wk.cluster_stats(w)
        assert {k: getattr(cl, k) for k in want_cl} == want_cl, w
        x, want_x = mc.exchange_stats(w), wk.exchange_stats(w)
        assert {k: getattr(x, k) for k in want_x} == want_x, w
        assert np.array_equal(mc.conf(w), wk.c[w]), w
        e, mx, my = mc.series(w)
        assert list(zip(e.tolist(), mx.tolist(), my.tolist())) == wk.ser[w], w
    assert np.array_equal(mc.replicas(), wk.replica)
    assert mc.binner_size() == (wk.bin.L, wk.bin.T)
    mc.close()


def test_run_with_checkpoints_changes_no_bit_and_its_file_finishes_the_run(gpu, tmp_path):
    kw = dict(thermalization=4, sweeps=14)
    A = _make(gpu, "clock6_all_on", **kw)
    A.run()
    path = tmp_path / "run.ckpt"
    B = _make(gpu, "clock6_all_on", **kw)
    B.run(checkpoint=path, checkpoint_every=4)
    assert B.last_sweep == 18 and B.state().tobytes() == A.state().tobytes()
    F = gpu.QStateMC.load(path)  # the file of the last sweep
    assert F.last_sweep == 18 and F.state().tobytes() == A.state().tobytes()
    F.close()
    B.close()
    # the first object dropped after sweep 8: its file loads and finishes to the same bytes
    D = _make(gpu, "clock6_all_on", **kw)
    D.run(checkpoint=path, checkpoint_every=4, sweeps=4)  # thermalization 4 + 4 sweeps: stops after sweep 8, saved there
    assert D.last_sweep == 8
    D.close()
    del D
    E = gpu.QStateMC.load(path)
    assert E.last_sweep == 8 and E.sweeps == 4
    E.run(sweeps=14, checkpoint=path, checkpoint_every=4)
    assert E.last_sweep == 18
    _same(_results(A), _results(E), "resumed run()")
    with pytest.raises(ValueError):
        E.run(checkpoint=path)
    A.close()
    E.close()


def _refused(gpu, target, blob, field):
    before = target.state()
    with pytest.raises(gpu.DQMCError) as e:
        target.set_state(blob)
    assert e.value.code == -1 and field in str(e.value), (field, str(e.value))
    assert target.state().tobytes() == before.tobytes(), "a refused import changed the handle (%s)" % field


def test_refusals_name_the_field_and_leave_the_handle_as_it_was(gpu):
    src = _make(gpu, "clock6_all_on")
    src.sweep(SPLIT)
    blob = src.state()
    src.close()
    col = ref.greedy_colouring(gpu.SquareLattice(4))
    others = {
        "n_walkers": dict(n_walkers=3, beta=[0.9, 1.0, 1.1]),
        "binner main capacity": dict(binner=128),
        "colouring": dict(colouring=(np.asarray(col) + 1) % (int(np.max(col)) + 1)),  # the classes renamed
        "betas": dict(beta=[0.9, 1.0, 1.1, 0.9, 1.0, 1.1000000000000003]),
        "exchange n_replicas": dict(tempering=None),
        "cluster rate": dict(cluster_rate=3),
        "n_k": dict(scaling=False),
        "stiffness n_dir": dict(stiffness=False),
        "series_capacity": dict(series_capacity=16),
    }
    for field, over in others.items():
        t = _make(gpu, "clock6_all_on", **over)
        t.sweep(3)
        _refused(gpu, t, blob, field)
        t.close()
    t = gpu.MC(gpu.ClockModel(5, l=gpu.SquareLattice(4)), beta=[0.9, 1.0, 1.1] * 2, n_walkers=6, seed=300, thermalization=4,
               series_capacity=32, cluster_rate=2, tempering=(3, 2), binner=64, scaling=True, stiffness=True)
    _refused(gpu, t, blob, "q: the blob has 6, the handle 5")
    t.close()
    # the other engine
    ising = gpu.MC(gpu.IsingModel(l=gpu.SquareLattice(4)), beta=[0.3] * 6, n_walkers=6, seed=300)
    ising.sweep(2)
    t = _make(gpu, "clock6_all_on")
    _refused(gpu, t, ising.state(), "engine kind")
    _refused(gpu, ising, blob, "engine kind")
    ising.close()
    # a blob cut by one byte; one payload byte flipped
    _refused(gpu, t, blob[:-1], "the header implies")
    bad = blob.copy()
    bad[len(bad) // 2] ^= 0x10
    _refused(gpu, t, bad, "checksum")
    t.set_state(blob)  # and the whole blob is taken
    assert t.state().tobytes() == blob.tobytes()
    t.close()
