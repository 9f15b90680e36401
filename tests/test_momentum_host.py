"""Momentum-space observables without a GPU: the ABI surface (header, binding, NULL handles), the wave vectors of
lattices.momentum_grid for every lattice class, the host transform, and the version-2 checkpoint blob under the host
sanitizers (tests/checkpoint_blob_v2_check.cpp, its own main, run as a child process)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")
FUNCTIONS = ("dqmc_set_momenta", "dqmc_momenta_plan")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqmc_hip.h")).read(), flags=re.S)


def test_header_declares_functions_and_section_ids():
    src = header()
    assert re.search(r"\bint\s+dqmc_set_momenta\s*\(\s*dqmc_handle\s*\*h,\s*int32_t n_q,\s*const double \*cos_tab,\s*"
                     r"const double \*sin_tab\)", src)
    assert re.search(r"\bint\s+dqmc_momenta_plan\s*\(\s*dqmc_handle\s*\*h,\s*int32_t out\[4\]\)", src)
    ids = {k: int(v) for k, v in re.findall(r"(DQMC_(?:BIN|RED)_\w+)\s*=\s*(-?\d+)", src)}
    mom = [ids["DQMC_BIN_MOMENTUM_CORRELATIONS"], ids["DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES"],
           ids["DQMC_BIN_MOMENTUM_TIME_DISPLACED"]]
    # above every existing DQMC_BIN_* value, DQMC_BIN_SIGN + k for the five measurement sections included
    assert min(mom) > ids["DQMC_BIN_SIGN"] + ids["DQMC_RED_SIGN"] - 1 and len(set(mom)) == 3
    assert ids["DQMC_BIN_SIGN"] == 6 and ids["DQMC_RED_SIGN"] == 5  # no new reduction section


def test_binding_has_the_functions_and_null_handles_are_refused(mc_amd):
    from montecarlo_jl_amd import _lib
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES, f
        assert hasattr(C.CDLL(_lib.LIB_PATH), f)
    ids = {k: int(v) for k, v in re.findall(r"(DQMC_BIN_MOMENTUM_\w+)\s*=\s*(\d+)", header())}
    assert _lib.BIN_MOMENTUM == {"momentum_correlations": ids["DQMC_BIN_MOMENTUM_CORRELATIONS"],
                                 "momentum_susceptibilities": ids["DQMC_BIN_MOMENTUM_SUSCEPTIBILITIES"],
                                 "momentum_time_displaced": ids["DQMC_BIN_MOMENTUM_TIME_DISPLACED"]}
    lib = _lib.lib()
    tab, plan = np.ones(4), (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.dqmc_set_momenta(None, 1, _lib.dptr(tab), _lib.dptr(tab)) == _lib.ERR_INVALID
    assert lib.dqmc_set_momenta(None, 0, None, None) == _lib.ERR_INVALID
    assert lib.dqmc_momenta_plan(None, plan) == _lib.ERR_INVALID and list(plan) == [7, 7, 7, 7]
    for name in ("set_momenta", "momenta", "structure_factors", "static_susceptibilities", "momentum_time_displaced"):
        assert callable(getattr(mc_amd.DQMC, name))


def lattices(m):
    return [m.Chain(8), m.Chain(5), m.SquareLattice(4), m.SquareLattice(3), m.CubicLattice(3, 2), m.CubicLattice(3, 3),
            m.TriangularLattice(3), m.TriangularLattice(4, 4, 2)]


def test_momentum_grid_has_n_distinct_vectors_that_resolve_the_lattice(mc_amd):
    """N distinct wave vectors, and sum_q cos(q . r_d) = N delta_{d,0} to 1e-12 over the directions of
    EachSitePairByDistance: a wrong reciprocal basis, or a direction that is no lattice vector, breaks it"""
    for l in lattices(mc_amd):
        q, labels = mc_amd.momentum_grid(l)
        N = len(l)
        assert q.shape == (N, labels.shape[1]) and labels.dtype.kind == "i", type(l).__name__
        assert len({tuple(x) for x in labels}) == N
        d2 = ((q[:, None, :] - q[None, :, :]) ** 2).sum(axis=2) + np.eye(N)
        assert d2.min() > 1e-6, type(l).__name__  # distinct as vectors, too
        it = mc_amd.EachSitePairByDistance(l)
        dirs = np.array(it.directions)
        assert dirs.shape[0] == N
        assert np.linalg.norm(dirs[0]) == 0.0
        tot = np.cos(dirs @ q.T).sum(axis=1)
        want = np.zeros(N)
        want[0] = N
        assert np.abs(tot - want).max() <= 1e-12 * N, (type(l).__name__, np.abs(tot - want).max())
        assert np.abs(np.sin(dirs @ q.T).sum(axis=1)).max() <= 1e-12 * N


def test_host_transform_of_a_symmetric_row_has_no_sine_part(mc_amd):
    """X[d] = X[-d] (what the Wick expressions of the density-type rows give in every sample): sum_d sin(q . r_d) X[d]
    vanishes to rounding, which is why those rows are binned with the cosine alone"""
    rng = np.random.Generator(np.random.Philox(key=11))
    for l in (mc_amd.SquareLattice(4), mc_amd.TriangularLattice(3), mc_amd.Chain(8)):
        q, _ = mc_amd.momentum_grid(l)
        dirs = np.array(mc_amd.EachSitePairByDistance(l).directions)
        A = np.array(mc_amd.lattices._lattice_vectors(l))
        N = len(l)
        # the direction of -r_d under the periodic images
        minus = []
        for d in range(N):
            frac = np.linalg.solve(A.T, (dirs + dirs[d]).T).T
            hit = np.where(np.abs(frac - np.round(frac)).max(axis=1) < 1e-9)[0]
            assert hit.size == 1
            minus.append(int(hit[0]))
        x = rng.standard_normal(N)
        x = x + x[minus]
        S, Cs = np.sin(dirs @ q.T), np.cos(dirs @ q.T)
        assert np.abs(x @ S).max() <= 4 * N * np.finfo(float).eps * np.abs(x).sum()
        assert np.abs(x @ Cs).max() > 1e-3  # (the cosine part is not trivially zero)


def test_blob_v2_code_under_address_and_undefined_sanitizers(tmp_path):
    """state_blob.cpp with tests/checkpoint_blob_v2_check.cpp (its own main), g++ -fsanitize=address,undefined, run as a
    child process on the CPU: a shape without momentum binners writes the version-1 bytes; a version-2 blob round-trips;
    every truncation, flipped extension bytes, another n_q, a table byte that differs and a binner shape that differs are
    refused with the reason named, and neither sanitizer reports anything"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the blob code"
    exe = str(tmp_path / "blob_v2_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "checkpoint_blob_v2_check.cpp"), os.path.join(CSRC, "state_blob.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
