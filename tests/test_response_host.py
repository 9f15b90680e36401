"""Pair structure factors and superfluid stiffness, the parts that need no GPU: the ABI surface, the default symmetry
channels, the free-fermion reference checked against itself (tests/response_ref.py: real-space site quadruples against
closed forms in the band basis, which is also where the sign convention of superfluid_stiffness is fixed), and the blob
code of format versions 5 - 8 under the host sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import response_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")


# ---- the ABI surface
def test_header_ids_and_signatures(mc_amd):
    from montecarlo_jl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(DQMC_BIN_\w+)\s*=\s*(\d+)", src)}
    assert enums["DQMC_BIN_RESPONSE_PAIRING"] == 15 and enums["DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY"] == 16
    assert enums["DQMC_BIN_RESPONSE_CURRENT"] == 17 and enums["DQMC_BIN_RESPONSE_END"] == 18
    assert enums["DQMC_BIN_MOMENTUM_END"] == enums["DQMC_BIN_THERMODYNAMICS"] == 14
    assert _lib.BIN_MOMENTUM == {"momentum_correlations": 11, "momentum_susceptibilities": 12, "momentum_time_displaced": 13}
    assert _lib.BIN_RESPONSE == {"response_pairing": enums["DQMC_BIN_RESPONSE_PAIRING"],
                                 "response_pairing_susceptibility": enums["DQMC_BIN_RESPONSE_PAIRING_SUSCEPTIBILITY"],
                                 "response_current": enums["DQMC_BIN_RESPONSE_CURRENT"]}
    reds = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(DQMC_RED_\w+)\s*=\s*(\d+)", src)}
    assert reds["DQMC_RED_SIGN"] == 5 and reds["DQMC_RED_THERMODYNAMICS"] == 6 and max(reds.values()) == 6  # no new section
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (dqmc_(?:set_pair_channels|response_plan))\s*\(([^)]*)\)\s*;", src)}
    assert decl == {"dqmc_set_pair_channels": "dqmc_handle *h, int32_t n_ch, const double *F",
                    "dqmc_response_plan": "dqmc_handle *h, int32_t out[4]"}
    assert _lib.SIGNATURES["dqmc_set_pair_channels"][1][1:] == [C.c_int32, C.POINTER(C.c_double)]
    lib = _lib.lib()
    F, out = np.ones(1), (C.c_int32 * 4)()
    assert lib.dqmc_set_pair_channels(None, 1, _lib.dptr(F)) == _lib.ERR_INVALID  # NULL handles are refused
    assert lib.dqmc_response_plan(None, out) == _lib.ERR_INVALID


# ---- the default channels
def test_default_channels_on_the_square_lattice(mc_amd):
    from montecarlo_jl_amd import lattices as L
    l = mc_amd.SquareLattice(4)
    it = mc_amd.EachLocalQuadByDistance(l)
    r = np.array(it.pairs_by_dir.directions)
    ch = L.default_pair_channels(l, r, it.K)
    assert list(ch) == ["s", "s*", "d"] and it.K == 5
    assert np.array_equal(ch["s"], [1, 0, 0, 0, 0]) and np.array_equal(ch["s*"], [0, .5, .5, .5, .5])
    assert ch["d"].sum() == 0 and ch["s*"] @ ch["d"] == 0 and ch["s"] @ ch["d"] == 0 and ch["d"] @ ch["d"] == 1
    for k in range(1, 5):  # the sign from the directions themselves: + along x, - along y
        assert ch["d"][k] == (0.5 if abs(r[k][0]) == 1 else -0.5)
    tri = mc_amd.TriangularLattice(4)
    itt = mc_amd.EachLocalQuadByDistance(tri)
    cht = L.default_pair_channels(tri, np.array(itt.pairs_by_dir.directions), itt.K)
    assert list(cht) == ["s", "s*"] and itt.K == 7 and np.array_equal(cht["s*"], [0] + [.5] * 6)
    with pytest.raises(ValueError):
        L.default_pair_channels(l, r[1:], 4)  # direction 0 is not the on-site one
    with pytest.raises(ValueError):
        L.default_pair_channels(l, r, 3)      # the d channel without the four neighbours


# ---- the free-fermion reference against itself
def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("L,mu", [(4, 0.0), (4, 0.3), (6, 0.3)])
def test_free_fermion_routes_agree(mc_amd, L, mu):
    """real-space quadruples against the band basis, every quantity to 1e-12 of its largest magnitude, and the sign
    convention of the stiffness: -k_x > 0, and with Lambda = -CCS(q) the longitudinal limit all but cancels it"""
    from montecarlo_jl_amd import lattices as Lt
    l = mc_amd.SquareLattice(L)
    ff, loc, cur = R.free_fermions(mc_amd, l, 2.0, 0.1, mu=mu)
    ch = Lt.default_pair_channels(l, ff.r, loc.K)
    rs = ff.real_space()
    m1 = ff.momentum_space_from_real(rs, ch)
    bb, m2 = ff.band_basis(ch)
    for k in ("PS_l", "CCS_l", "PS", "CCS", "kbond", "PC"):
        assert _rel(rs[k], bb[k]) < 1e-12, (k, _rel(rs[k], bb[k]))
    for k in ("P", "chi"):
        for c in ch:
            assert _rel(m1[k][c], m2[k][c]) < 1e-12, (k, c)
    assert _rel(m1["Lambda"], m2["Lambda"]) < 1e-12
    q, d = ff.q, ff.r[:cur.K]
    iL = next(i for i in range(len(q)) if np.allclose(q[i], [2 * np.pi / L, 0]))
    iT = next(i for i in range(len(q)) if np.allclose(q[i], [0, 2 * np.pi / L]))
    kp = next(k for k in range(cur.K) if np.allclose(d[k], [1, 0]))
    km = next(k for k in range(cur.K) if np.allclose(d[k], [-1, 0]))
    st = R.stiffness(bb["kbond"], m2["Lambda"], kp, km, iL, iT)
    assert -st["k_axis"] > 0 and abs(st["drude"]) < abs(st["k_axis"])
    assert abs(st["drude"]) < 0.01 * abs(st["k_axis"])  # (what is left is the Riemann sum's and the finite q's)
    assert np.all(np.real(m2["Lambda"][kp]) <= 1e-14)   # the engine-convention sums are -<j j>


def test_tau_sum_is_the_riemann_sum(mc_amd):
    ff, _, _ = R.free_fermions(mc_amd, mc_amd.SquareLattice(4), 2.0, 0.1)
    a = np.array([-3.0, -1e-9, 0.0, 1e-12, 0.7, 4.0])
    want = np.array([sum(0.1 * np.exp(-l * 0.1 * x) for l in range(1, 21)) for x in a])
    assert np.allclose(ff._tau_sum(a), want, rtol=1e-13, atol=0)


# ---- the blob code of format versions 5 - 8
@pytest.mark.parametrize("prog", ["checkpoint_blob_v5_check.cpp", "checkpoint_blob_v3_check.cpp", "checkpoint_blob_v2_check.cpp"])
def test_blob_code_under_address_and_undefined_sanitizers(tmp_path, prog):
    """state_blob.cpp with a check program of its own main, g++ -fsanitize=address,undefined, run as a child process on
    the CPU: the new program for versions 5 - 8, and the two committed ones, which call validate_any / validate_all with
    their present signatures and must pass unchanged against the extended code"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the blob code"
    exe = str(tmp_path / "blob_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", prog),
                    os.path.join(CSRC, "state_blob.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
