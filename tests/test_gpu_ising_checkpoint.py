"""Checkpoint and resume of the Ising engine on the device (dqmc_mc_state_*, MC.save / load / run(checkpoint=...)).

The same seeds go into two objects: A runs 2n sweeps; B runs n sweeps, is saved, closed, loaded into a fresh object and
runs the rest.  Everything is compared with ==: the state blobs byte for byte, the series, measurements and binned dicts.
The split sweep is no multiple of the global or exchange rate, and the binner stands at T = 7 there (three pending
compressor values travel), or between two measurements with measure_rate 3.  One case is also compared with the numpy
restatements (ising_checkerboard_ref over ising_wolff_ref) run straight through."""
import numpy as np
import pytest

import ising_checkerboard_ref as CB
import ising_wolff_ref as R  # noqa: F401  (the sweep, the Wolff move and run!'s rule under ising_checkerboard_ref.Walker)

pytestmark = pytest.mark.gpu

SEED = 4321
BETAS8 = [0.30, 0.36, 0.42, 0.48] * 2
CASES = {
    # sequential sweep, W = 5: not a multiple of the 64-lane chain layout
    "sequential_w5": (lambda g: g.SquareLattice(6), dict(beta=[0.2, 0.3, 0.44, 0.5, 0.7], n_walkers=5)),
    "wolff_rate3": (lambda g: g.SquareLattice(6), dict(beta=[0.3, 0.44, 0.6], n_walkers=3, cluster_moves=True, global_rate=3)),
    # R = 4 divides 64: the rounds run inside the sweep kernel; R = 3: each round is a launch
    "exchange_fused": (lambda g: g.SquareLattice(6), dict(beta=BETAS8, n_walkers=8, n_replicas=4, exchange_rate=3)),
    "exchange_launch": (lambda g: g.SquareLattice(6), dict(beta=[0.35, 0.40, 0.45] * 2, n_walkers=6, n_replicas=3,
                                                           exchange_rate=3)),
    "checkerboard5": (lambda g: g.SquareLattice(5), dict(beta=[0.3, 0.44, 0.6], n_walkers=3, update="checkerboard")),
    "binning_fss": (lambda g: g.SquareLattice(6), dict(beta=[0.3, 0.44, 0.6], n_walkers=3, binning=True, binning_capacity=64,
                                                       fss=True)),
    "binning_fss_rate3": (lambda g: g.SquareLattice(6), dict(beta=[0.3, 0.44, 0.6], n_walkers=3, binning=True,
                                                             binning_capacity=64, fss=True, measure_rate=3)),
    "everything": (lambda g: g.SquareLattice(5), dict(beta=[0.35, 0.40, 0.45] * 2, n_walkers=6, n_replicas=3, exchange_rate=3,
                                                      cluster_moves=True, global_rate=4, update="checkerboard", binning=True,
                                                      binning_capacity=64, fss=True)),
    "all_off": (lambda g: g.SquareLattice(6), dict(beta=[0.44], n_walkers=1, series_capacity=0)),
}
SPLIT, TOTAL = 10, 20  # thermalization 3, measure_rate 1: T = 7 at the split; 10 is no multiple of 3 or 4


def _make(g, case, **over):
    make, kw = CASES[case]
    kw = dict(dict(seed=SEED, thermalization=3, sweeps=17, series_capacity=32), **kw)
    kw.update(over)
    mc = g.MC(g.IsingModel(l=make(g)), **kw)
    assert type(mc) is g.MC
    return mc


def _results(mc):
    out = {"state": mc.state().tobytes(), "last_sweep": mc.last_sweep, "replicas": mc.replicas().tolist()}
    for w in range(mc.n_walkers):
        out["series", w] = [a.tolist() for a in mc.series(w)]
        out["conf", w] = mc.conf(w).tolist()
        out["meas", w] = mc.measurements(w)
        out["update", w] = mc.update_stats(w).sweeps_drawn
        if mc._binning is not None:
            out["binned", w] = mc.binned(w)
            if mc.k_vectors is not None:
                out["binned_fss", w] = repr(mc.binned_fss(w))
        if mc.k_vectors is not None:
            out["fss", w] = repr(mc.fss(w))
    return out


def _same(a, b, label):
    assert a.keys() == b.keys(), label
    for k in a:
        assert repr(a[k]) == repr(b[k]) if k != "state" else a[k] == b[k], (label, k)  # (repr: NaN compares equal)


@pytest.mark.parametrize("case", list(CASES))
def test_a_saved_and_loaded_run_continues_byte_for_byte(gpu, tmp_path, case):
    A = _make(gpu, case)
    A.sweep(TOTAL)
    B = _make(gpu, case)
    B.sweep(SPLIT)
    if B._binning is not None:
        assert B.binner_size()[1] == (7 if B.measure_rate == 1 else 2), case  # rate 3: sweeps 6 and 9, 12 is next
    if case == "exchange_fused":
        assert B.exchange_fused()
    if case == "exchange_launch":
        assert not B.exchange_fused()
    if case in ("checkerboard5", "everything"):
        assert int(B.colouring.max()) + 1 >= 3
    mid = B.state()
    path = tmp_path / "b.ckpt"
    B.save(path)
    assert np.array_equal(B.state(), mid), "export changed the handle"
    B.close()
    C2 = gpu.MC.load(path)
    assert type(C2) is gpu.MC and C2.last_sweep == SPLIT and C2.seeds == [SEED + w for w in range(C2.n_walkers)]
    assert C2.state().tobytes() == mid.tobytes(), "the loaded object does not stand where the saved one stood"
    C2.sweep(TOTAL - SPLIT)
    _same(_results(A), _results(C2), case)
    assert A.stats(0).n_meas == TOTAL - 3 if A.measure_rate == 1 else A.stats(0).n_meas > 0
    A.close()
    C2.close()


def test_the_resumed_run_matches_the_restatements_run_straight_through(gpu, tmp_path):
    """checkerboard sweeps on the 5 x 5 lattice with a Wolff move behind every third: the resumed run against
    ising_checkerboard_ref.Walker (over ising_wolff_ref.Walker) run from sweep 1 to the end without a cut: =="""
    l = gpu.SquareLattice(5)
    betas = [0.3, 0.44, 0.6]
    kw = dict(beta=betas, n_walkers=3, seed=SEED, thermalization=3, sweeps=17, series_capacity=32, cluster_moves=True,
              global_rate=3, update="checkerboard")
    B = gpu.MC(gpu.IsingModel(l=l), **kw)
    B.sweep(SPLIT)
    path = tmp_path / "b.ckpt"
    B.save(path)
    B.close()
    mc = gpu.MC.load(path)
    mc.sweep(TOTAL - SPLIT)
    fields = ("sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "acc_local", "prop_local", "uniforms_used", "energy",
              "magnetization")
    for w, b in enumerate(betas):
        ref = CB.Walker(l, b, SEED + w, series_capacity=32)
        ref.run(1, TOTAL, 3, 1, 3)
        st, g = mc.stats(w), mc.global_stats(w)
        assert {f: getattr(st, f) for f in fields} == ref.stats(), w
        assert {f: getattr(g, f) for f in ref.gs} == ref.gs, w
        assert np.array_equal(mc.conf(w), ref.c), w
        e, m = mc.series(w)
        assert list(e) == ref.serE and list(m) == ref.serM, w
        assert mc.update_stats(w).sweeps_drawn == ref.s == TOTAL
    mc.close()


def test_run_with_checkpoints_changes_no_bit_and_its_file_finishes_the_run(gpu, tmp_path):
    A = _make(gpu, "everything")
    A.run()
    path = tmp_path / "run.ckpt"
    B = _make(gpu, "everything")
    B.run(checkpoint=path, checkpoint_every=4)
    assert B.last_sweep == 20 and B.state().tobytes() == A.state().tobytes()
    B.close()
    D = _make(gpu, "everything")
    D.run(checkpoint=path, checkpoint_every=4, sweeps=5)  # stops after sweep 8, saved there
    assert D.last_sweep == 8
    D.close()
    E = gpu.MC.load(path)
    assert E.last_sweep == 8
    E.run(sweeps=17)
    _same(_results(A), _results(E), "resumed run()")
    A.close()
    E.close()


def _refused(gpu, target, blob, field):
    before = target.state()
    with pytest.raises(gpu.DQMCError) as e:
        target.set_state(blob)
    assert e.value.code == -1 and field in str(e.value), (field, str(e.value))
    assert target.state().tobytes() == before.tobytes(), "a refused import changed the handle (%s)" % field


def test_refusals_name_the_field_and_leave_the_handle_as_it_was(gpu):
    src = _make(gpu, "everything")
    src.sweep(SPLIT)
    blob = src.state()
    col = np.asarray(src.colouring)
    src.close()
    others = {
        "n_walkers": dict(n_walkers=3, beta=[0.35, 0.40, 0.45]),
        "binner main capacity": dict(binning_capacity=128),
        "colouring": dict(colouring=(col + 1) % (int(col.max()) + 1)),  # the classes renamed
        "betas": dict(beta=[0.35, 0.40, 0.45, 0.35, 0.40, 0.45000000000000007]),
        "exchange n_replicas": dict(n_replicas=0, exchange_rate=0),
        "cluster rate": dict(global_rate=5),
        "update kind": dict(update="sequential"),
        "n_k": dict(fss=False),
    }
    for field, over in others.items():
        t = _make(gpu, "everything", **over)
        t.sweep(3)
        _refused(gpu, t, blob, field)
        t.close()
    # the other engine (a q = 2 Potts model on the same lattice)
    qs = gpu.MC(gpu.PottsModel(2, l=gpu.SquareLattice(5)), beta=[0.35, 0.40, 0.45] * 2, n_walkers=6, seed=SEED)
    qs.sweep(2)
    t = _make(gpu, "everything")
    _refused(gpu, t, qs.state(), "engine kind")
    _refused(gpu, qs, blob, "engine kind")
    qs.close()
    # a blob cut by one byte; one payload byte flipped
    _refused(gpu, t, blob[:-1], "the header implies")
    bad = blob.copy()
    bad[len(bad) // 2] ^= 0x10
    _refused(gpu, t, bad, "checksum")
    t.set_state(blob)  # and the whole blob is taken
    assert t.state().tobytes() == blob.tobytes()
    t.close()
