"""Scalar thermodynamics without a GPU: the numpy restatement of the ten observables (tests/thermo_ref.py) against
exact diagonalisation where Wick's theorem is exact (U = 0), the doped repulsive model's matrices, the ABI surface, and
format versions 3 / 4 of the checkpoint blob under the host sanitizers (tests/checkpoint_blob_v3_check.cpp, its own
main, run as a child process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import thermo_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")
FUNCTIONS = ("dqmc_set_thermodynamics", "dqmc_accumulate_thermodynamics", "dqmc_thermodynamics_size",
             "dqmc_get_thermodynamics", "dqmc_export_thermodynamics")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqmc_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("mu", [0.0, 0.7])
def test_wick_formulas_equal_exact_diagonalisation_at_u_zero(O, R, mu):
    """2x2 lattice, U = 0, beta = 1: the state is Gaussian, so the ten values formed from ED's own G by the table's
    formulas equal <n_up>, <n_up n_dn>, <H>/N, <N^2>/N, <Mz^2>/N ... taken directly from rho, to 1e-12"""
    N, t, beta = 4, 1.0, 1.0
    neighs = O.square_neighs(2)
    rho, c, cd = R.ed_hubbard_greens(neighs, N, 0.0, t, mu, beta, return_state=True)
    G = TR.ed_greens_blocks(rho, c, cd, N)
    T = TR.hopping_from_neighs(neighs, N, t, mu)
    for U_s in (0.0, 3.0):  # (E_int's formula at a U_s the state was not made with is still the same expectation value)
        got = TR.thermo_ref(G, [T, T], U_s)
        want = TR.ed_thermo(rho, c, cd, neighs, N, U_s, t, mu)
        for k, a, b in zip(TR.FIELDS, got, want):
            assert abs(a - b) <= 1e-12, (mu, U_s, k, a, b)
    # one block counted twice is the two equal blocks
    assert np.array_equal(TR.thermo_ref([G[0]], [T], 0.0), TR.thermo_ref([G[0], G[0]], [T, T], 0.0))
    if mu == 0.0:  # half filling
        assert abs(got[2] - 1.0) < 1e-12


def test_repulsive_model_takes_mu(mc_amd):
    m0 = mc_amd.HubbardModelRepulsive(4, 2, U=4.0)
    T0 = np.zeros((16, 16))
    for src, trg in m0.l.neighbors(True):
        T0[trg - 1, src - 1] += -1.0
    blocks = m0.hopping_matrix()
    assert len(blocks) == 2 and all(b.tobytes() == T0.tobytes() for b in blocks), "mu = 0 must give exactly the matrices of before"
    assert m0.mu == 0.0
    m = mc_amd.HubbardModelRepulsive(4, 2, U=4.0, mu=0.4)
    for b in m.hopping_matrix():
        assert np.array_equal(np.diag(b), np.full(16, -0.4))
        assert np.array_equal(b - np.diag(np.diag(b)), T0)
    assert m.hopping_matrix()[0] is not m.hopping_matrix()[1]
    # the same diagonal as the attractive model's
    a = mc_amd.HubbardModelAttractive(4, 2, U=4.0, mu=0.4)
    assert np.array_equal(a.hopping_matrix()[0], m.hopping_matrix()[0])
    # HubbardModel(U > 0, mu=...) passes it on
    h = mc_amd.HubbardModel(4, 2, U=2.0, mu=0.25)
    assert isinstance(h, mc_amd.HubbardModelRepulsive) and h.mu == 0.25 and h.U == 2.0
    h = mc_amd.HubbardModel(4, 2, U=-2.0, mu=0.25)
    assert isinstance(h, mc_amd.HubbardModelAttractive) and h.mu == 0.25


def test_header_and_binding(mc_amd):
    from montecarlo_jl_amd import _lib
    src = header()
    assert re.search(r"\bint\s+dqmc_set_thermodynamics\s*\(\s*dqmc_handle\s*\*h,\s*const double \*T\)", src)
    ids = {k: int(v) for k, v in re.findall(r"(DQMC_(?:BIN|RED|THERMO)_\w+)\s*=\s*(-?\d+)", src)}
    assert ids["DQMC_RED_THERMODYNAMICS"] == 6 == _lib.RED_THERMODYNAMICS and ids["DQMC_RED_SIGN"] == 5
    assert ids["DQMC_BIN_THERMODYNAMICS"] == ids["DQMC_BIN_MOMENTUM_END"] == _lib.BIN_THERMODYNAMICS
    assert ids["DQMC_BIN_SIGN"] == 6 and ids["DQMC_THERMO_ELEMENTS"] == len(_lib.THERMO_FIELDS) == 10
    assert _lib.THERMO_FIELDS == TR.FIELDS
    L = C.CDLL(_lib.LIB_PATH)
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES and hasattr(L, f), f
        assert re.search(r"\bint\s+%s\s*\(" % f, src), f
    lib = _lib.lib()
    n, x = C.c_size_t(7), np.ones(12)
    assert lib.dqmc_set_thermodynamics(None, _lib.dptr(x)) == _lib.ERR_INVALID
    assert lib.dqmc_accumulate_thermodynamics(None) == _lib.ERR_INVALID
    assert lib.dqmc_thermodynamics_size(None, C.byref(n)) == _lib.ERR_INVALID and n.value == 7
    assert lib.dqmc_get_thermodynamics(None, _lib.dptr(x)) == _lib.ERR_INVALID
    for name in ("set_thermodynamics", "accumulate_thermodynamics", "thermodynamics"):
        assert callable(getattr(mc_amd.DQMC, name))


def test_blob_v3_code_under_address_and_undefined_sanitizers(tmp_path):
    """state_blob.cpp with tests/checkpoint_blob_v3_check.cpp (its own main), g++ -fsanitize=address,undefined, run as a
    child process on the CPU: with the section off the version-1 / 2 bytes are unchanged; version-3 and version-4 blobs
    round-trip; truncations, a trailing byte, a wrong checksum and every configuration field that differs are refused
    with the reason named, and neither sanitizer reports anything"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the build environment"
    exe = str(tmp_path / "blob_v3_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "checkpoint_blob_v3_check.cpp"), os.path.join(CSRC, "state_blob.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
