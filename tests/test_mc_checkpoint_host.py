"""Checkpoint and resume of the classical MC flavor, the parts that need no GPU: the six ABI symbols, null handles, the
preamble of each flavor through the file container, models that come back bit-equal, and files of another flavor."""
import ctypes as C
import inspect
import json
import math
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def ckpt(mc_amd):
    from montecarlo_jl_amd import checkpoint
    return checkpoint


def test_state_symbols_and_signatures(mc_amd):
    from montecarlo_jl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split())
            for m in re.finditer(r"\bint (dqmc_(?:mc|qs)_state_\w+)\s*\(([^)]*)\)\s*;", src)}
    want = {}
    for fam in ("mc", "qs"):
        want["dqmc_%s_state_size" % fam] = "dqmc_%s_handle *h, size_t *n_bytes" % fam
        want["dqmc_%s_state_export" % fam] = "dqmc_%s_handle *h, void *host_out, size_t n_bytes" % fam
        want["dqmc_%s_state_import" % fam] = "dqmc_%s_handle *h, const void *host_in, size_t n_bytes" % fam
    assert decl == want
    L = C.CDLL(_lib.LIB_PATH)
    S = _lib.SIGNATURES
    for name in want:
        assert hasattr(L, name)
        args = [C.c_void_p, C.POINTER(C.c_size_t)] if name.endswith("size") else [C.c_void_p, C.c_void_p, C.c_size_t]
        assert S[name] == (C.c_int, args)


def test_null_handles_are_invalid(mc_amd):
    from montecarlo_jl_amd import _lib
    lib = _lib.lib()
    for fam in ("mc", "qs"):
        n = C.c_size_t(7)
        buf = np.zeros(16, dtype=np.uint8)
        assert getattr(lib, "dqmc_%s_state_size" % fam)(None, C.byref(n)) == _lib.ERR_INVALID and n.value == 7
        assert getattr(lib, "dqmc_%s_state_export" % fam)(None, buf.ctypes.data, buf.size) == _lib.ERR_INVALID
        assert getattr(lib, "dqmc_%s_state_import" % fam)(None, buf.ctypes.data, buf.size) == _lib.ERR_INVALID
        assert b"null handle" in getattr(lib, "dqmc_%s_last_error" % fam)(None)
        assert not buf.any()


def test_objects_have_the_entry_points(mc_amd):
    for cls in (mc_amd.MC, mc_amd.QStateMC):
        for name in ("state", "set_state", "save", "load", "state_size"):
            assert callable(getattr(cls, name)), (cls, name)
        sig = inspect.signature(cls.run)
        assert "checkpoint" in sig.parameters and "checkpoint_every" in sig.parameters
        assert list(inspect.signature(cls.load).parameters) == ["path", "device_id"]
    assert mc_amd.MC._flavor == "mc_ising" and mc_amd.QStateMC._flavor == "mc_qstate"


def _through_the_container(ckpt, pre):
    blob = np.arange(40, dtype=np.uint8)
    back, b = ckpt.split(b"".join(bytes(p) for p in ckpt.join(pre, blob)))
    assert np.array_equal(b, blob)
    return back


def test_qstate_model_with_an_irrational_table_comes_back_bit_equal(mc_amd, ckpt):
    """pair_energy, J and twist travel as JSON floats, which round-trip doubles exactly: the model built from the entry has
    the same doubles and the same fixed-point tables"""
    Q = mc_amd.QStateMC
    a, b = math.sqrt(2.0) / 3.0, -math.pi / 7.0
    e = [1.0 / 3.0, a, b, b, a]
    d1 = [0.0, math.e / 5.0, -math.sqrt(3.0) / 2.0, math.sqrt(3.0) / 2.0, -math.e / 5.0]
    m = mc_amd.QStateModel(5, e, l=mc_amd.TriangularLattice(3), J=1.0 / 7.0, twist=(d1, e))
    entry = _through_the_container(ckpt, {"flavor": "mc_qstate", "model": Q._model_entry(m),
                                          "lattice": Q._lattice_entry(m.l)})
    l = Q._lattice_from_entry(entry["lattice"])
    assert type(l) is mc_amd.TriangularLattice and np.array_equal(l.neighs, m.l.neighs)
    m2 = Q._model_from_entry(entry["model"], l)
    assert type(m2) is mc_amd.QStateModel and m2.q == 5 and m2.J == m.J
    assert m2.pair_energy.tobytes() == m.pair_energy.tobytes()
    assert m2.twist[0].tobytes() == m.twist[0].tobytes() and m2.twist[1].tobytes() == m.twist[1].tobytes()
    for x, y in zip((m.e_q30, m.c_q30, m.s_q30) + m.twist_q30, (m2.e_q30, m2.c_q30, m2.s_q30) + m2.twist_q30):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert (m2.dims, m2.L) == (m.dims, m.L)
    # Potts and clock models come back as their own classes with the same tables
    for m in (mc_amd.PottsModel(3, l=mc_amd.RectangularLattice(3, 5), J=0.7), mc_amd.ClockModel(6, dims=2, L=4)):
        entry = _through_the_container(ckpt, {"model": Q._model_entry(m), "lattice": Q._lattice_entry(m.l)})
        m2 = Q._model_from_entry(entry["model"], Q._lattice_from_entry(entry["lattice"]))
        assert type(m2) is type(m) and np.array_equal(m2.e_q30, m.e_q30) and m2.J == m.J
        assert (m.twist_q30 is None) == (m2.twist_q30 is None)
        if m.twist_q30 is not None:
            assert all(np.array_equal(x, y) for x, y in zip(m.twist_q30, m2.twist_q30))


def test_ising_model_entry(mc_amd, ckpt):
    M = mc_amd.MC
    for m in (mc_amd.IsingModel(dims=2, L=6), mc_amd.IsingModel(l=mc_amd.RectangularLattice(3, 5)),
              mc_amd.IsingModel(dims=3, L=3), mc_amd.IsingModel(dims=1, L=7)):
        entry = _through_the_container(ckpt, {"model": M._model_entry(m), "lattice": M._lattice_entry(m.l)})
        m2 = M._model_from_entry(entry["model"], M._lattice_from_entry(entry["lattice"]))
        assert type(m2.l) is type(m.l) and np.array_equal(m2.l.neighs, m.l.neighs) and np.array_equal(m2.l.bonds, m.l.bonds)
        assert (m2.dims, m2.L) == (m.dims, m.L)
    with pytest.raises(ckpt.CheckpointError):
        M._model_from_entry({"class": "PottsModel", "dims": 2, "L": 4}, mc_amd.SquareLattice(4))
    with pytest.raises(ckpt.CheckpointError):
        M._lattice_from_entry({"class": "os", "args": []})


def test_preambles_survive_the_container(mc_amd, ckpt):
    """a preamble as save() writes it, for each flavor: every value is JSON and comes back equal, doubles bit for bit"""
    betas = [0.1 + 0.2, 1.0 / 3.0, math.pi / 8.0]
    ising = {"format": 1, "flavor": "mc_ising", "model": {"class": "IsingModel", "dims": 2, "L": 6},
             "lattice": {"class": "SquareLattice", "args": [6]},
             "mc": {"beta": betas, "n_walkers": 3, "seed": 2 ** 40 + 5, "first_walker": 96, "thermalization": 3, "sweeps": 17,
                    "measure_rate": 3, "print_rate": 1000, "series_capacity": 64, "cluster_moves": True, "global_rate": 3,
                    "n_replicas": 3, "exchange_rate": 2, "update": "checkerboard", "colouring": [0, 1] * 18,
                    "fss": [[2.0 * math.pi / 6.0, 0.0], [0.0, 2.0 * math.pi / 6.0]], "binning": True,
                    "binning_capacity": 64},
             "seeds": [2 ** 40 + 101, 2 ** 40 + 102, 7], "last_sweep": 10}
    qstate = {"format": 1, "flavor": "mc_qstate",
              "model": {"class": "QStateModel", "q": 3, "J": 1.0 / 7.0, "pair_energy": [math.sqrt(2.0), 0.1, 0.1],
                        "twist": None, "dims": 2, "L": 3},
              "lattice": {"class": "TriangularLattice", "args": [3, 3, 3]},
              "mc": {"beta": betas, "n_walkers": 3, "seed": 9, "first_walker": 0, "thermalization": 3, "sweeps": 17,
                     "measure_rate": 1, "print_rate": 1000, "series_capacity": 0, "colouring": [0, 1, 2] * 3,
                     "cluster_rate": 2, "tempering": [3, 2], "binner": 64, "scaling": [[0.5, math.sqrt(3.0) / 7.0]],
                     "stiffness": [[1.0, 0.0], [0.0, 1.0]]},
              "seeds": [9, 10, 11], "last_sweep": 10}
    for pre in (ising, qstate):
        back = _through_the_container(ckpt, pre)
        assert back == pre and json.dumps(back, sort_keys=True) == json.dumps(pre, sort_keys=True)
        assert np.array(back["mc"]["beta"]).tobytes() == np.array(betas).tobytes()
    assert mc_amd.QStateMC._keywords(dict(qstate["mc"]))["tempering"] == (3, 2)


def test_files_of_another_flavor_are_refused_with_the_flavor_named(mc_amd, ckpt, tmp_path):
    """the flavor is checked before anything is constructed: no device is touched"""
    blob = np.arange(64, dtype=np.uint8)
    files = {}
    for flavor in ("mc_ising", "mc_qstate", None):
        pre = {"format": 1, "last_sweep": 4}
        if flavor:
            pre["flavor"] = flavor
        files[flavor or "dqmc"] = tmp_path / ("%s.ckpt" % (flavor or "dqmc"))
        ckpt.write(files[flavor or "dqmc"], pre, blob)
    loaders = {"mc_ising": mc_amd.MC, "mc_qstate": mc_amd.QStateMC, "dqmc": mc_amd.DQMC}
    for have, path in files.items():
        for want, cls in loaders.items():
            if have == want:
                continue
            with pytest.raises(ckpt.CheckpointError, match="flavor '%s'" % have):
                cls.load(path)
