"""Time-displaced recording without a GPU: the ABI surface (header, binding, NULL handles) and the numpy reference the
GPU tests compare against (tests/time_displaced_ref.py), checked against measurement_ref on a 4 x 4 random tuple.

Bound, as in test_gpu_measurement_sizes.py: |a - b| <= 2 (P + 16) eps abs_sum per element, P = the pairs summed into it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_tables as LT  # noqa: E402
import measurement_ref as MR  # noqa: E402
import time_displaced_ref as TR  # noqa: E402

EPS = np.finfo(np.float64).eps
FUNCTIONS = ("dqmc_set_time_displaced", "dqmc_time_displaced_size", "dqmc_get_time_displaced",
             "dqmc_export_time_displaced", "dqmc_time_displaced_plan")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqmc_hip.h")).read(), flags=re.S)


def enums(src):
    """every anonymous enum of the header as {name: value}"""
    out = []
    for body in re.findall(r"enum\s*\{([^}]*)\}", src):
        out.append({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)})
    return out


def test_header_declares_functions_and_enums():
    src = header()
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(\s*dqmc_handle\s*\*" % f, src), f
    es = enums(src)
    assert {"DQMC_TD_GREENS": 1, "DQMC_TD_DENSITY": 2} in es
    assert {"DQMC_BIN_TIME_DISPLACED": 5} in es  # enums of their own ...
    assert {"DQMC_RED_TIME_DISPLACED": 4} in es
    # ... and the pinned lists are what they were
    assert {"DQMC_BIN_GREENS": 0, "DQMC_BIN_CORRELATIONS": 1, "DQMC_BIN_PAIRING": 2, "DQMC_BIN_SUSCEPTIBILITIES": 3,
            "DQMC_BIN_USER": 4} in es
    assert {"DQMC_RED_GREENS": 0, "DQMC_RED_CORRELATIONS": 1, "DQMC_RED_PAIRING": 2, "DQMC_RED_SUSCEPTIBILITIES": 3} in es


def test_binding_has_the_functions_and_null_handles_are_refused(mc_amd):
    from montecarlo_jl_amd import _lib
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES, f
    assert _lib.BIN_SECTIONS == ("greens", "correlations", "pairing", "susceptibilities", "user")
    assert (_lib.BIN_TIME_DISPLACED, _lib.RED_TIME_DISPLACED, _lib.TD_GREENS, _lib.TD_DENSITY) == (5, 4, 1, 2)
    lib = _lib.lib()
    n, buf, plan = C.c_size_t(), np.zeros(4), (C.c_int32 * 4)()
    assert lib.dqmc_set_time_displaced(None, 1, 3) == _lib.ERR_INVALID
    assert lib.dqmc_set_time_displaced(None, 0, 0) == _lib.ERR_INVALID
    assert lib.dqmc_time_displaced_size(None, C.byref(n)) == _lib.ERR_INVALID
    assert lib.dqmc_get_time_displaced(None, _lib.dptr(buf)) == _lib.ERR_INVALID
    assert lib.dqmc_export_time_displaced(None, C.c_void_p(0)) == _lib.ERR_INVALID
    assert lib.dqmc_time_displaced_plan(None, plan) == _lib.ERR_INVALID


@pytest.fixture(scope="module")
def square4(mc_amd):
    l = mc_amd.SquareLattice(4)
    return l, LT.fast_pairs(l)


def random_tuple(nb, n, seed):
    rng = np.random.default_rng(seed)
    return [[rng.standard_normal((n, n)) for _ in range(nb)] for _ in range(4)]


@pytest.mark.parametrize("nb", [1, 2])
def test_row0_is_the_equal_time_measurement(square4, nb):
    """(G, G - I, G, G) in the packed kernels gives cdc / sdc_{x,y,z} of the equal-time kernels, both model kinds"""
    l, fp = square4
    n, nd, dir_of = l.sites, fp.ndirections(), fp.dir_of
    G = random_tuple(nb, n, 5)[0]
    pairs = np.bincount(dir_of.ravel(), minlength=nd).astype(float)
    got = TR.rows(G, [], dir_of, nd, every=1, what=TR.DENSITY)
    ref = MR.equal_time(G, dir_of, nd)
    for k in TR.DENSITY_NAMES:
        val, ab = got[k]
        assert val.shape == (1, nd)
        bound = 2.0 * (pairs + 16.0) * EPS * ref[k][1]
        assert bound.max() <= 1e-9 * np.abs(ref[k][0]).max()
        assert np.all(np.abs(val[0] - ref[k][0]) <= bound), k
        assert np.all(np.abs(ab[0] - ref[k][1]) <= bound), k  # the same terms, so the same abs_sum


@pytest.mark.parametrize("nb", [1, 2])
def test_rows_layout_and_greens_rows(square4, nb):
    """rows(): shapes, the `every` stride, G0l row 0 = G - I, and the Green's rows against a literal pair loop"""
    l, fp = square4
    n, nd, dir_of = l.sites, fp.ndirections(), fp.dir_of
    g00 = random_tuple(nb, n, 1)[0]
    steps = [tuple(random_tuple(nb, n, 10 + s)[:3]) for s in range(4)]
    full = TR.rows(g00, steps, dir_of, nd)
    half = TR.rows(g00, steps, dir_of, nd, every=2)
    assert sorted(full) == sorted(TR.names(3)) and full["Gl0"][0].shape == (nb, 5, nd) and full["CDC"][0].shape == (5, nd)
    for k in full:
        ax = 1 if k in ("Gl0", "G0l") else 0
        assert np.array_equal(np.take(full[k][0], [0, 2, 4], axis=ax), half[k][0]), k
    lit = np.zeros((nb, nd))
    for b in range(nb):
        for i in range(n):
            for j in range(n):
                lit[b, dir_of[i, j]] += (g00[b][i, j] - (i == j)) / n
    assert np.allclose(full["G0l"][0][:, 0], lit, rtol=0, atol=64 * EPS * full["G0l"][1][:, 0].max())
    assert np.array_equal(full["Gl0"][0][:, 0], TR.greens_row(g00, dir_of, nd)[0])
    assert np.array_equal(full["G0l"][0][:, 3], TR.greens_row(steps[2][0], dir_of, nd)[0])
    assert np.array_equal(full["Gl0"][0][:, 3], TR.greens_row(steps[2][1], dir_of, nd)[0])
    flat = np.concatenate([full[k][0].ravel() for k in TR.names(3)])
    assert flat.size == TR.size(nb, 5, nd, 3)
    back = TR.split(flat, nb, 5, nd, 3)
    assert all(np.array_equal(back[k], full[k][0]) for k in full)
    assert TR.size(nb, 5, nd, TR.GREENS) + TR.size(nb, 5, nd, TR.DENSITY) == flat.size


def test_src_of_reproduces_dir_of(square4):
    l, fp = square4
    n, nd, dir_of = l.sites, fp.ndirections(), fp.dir_of
    src_of = TR.src_of_table(dir_of, nd)
    assert src_of is not None and src_of.shape == (nd, n) and src_of.min() >= 0
    for d in range(nd):
        for j in range(n):
            assert dir_of[src_of[d, j], j] == d
    # tables the fast form must refuse: fewer directions than sites; a direction twice for one source
    ring = np.abs(np.subtract.outer(np.arange(9), np.arange(9)))
    assert TR.src_of_table(np.minimum(ring, 9 - ring), 5) is None
    rows_only = np.tile(np.arange(n), (n, 1))        # dir_of[i, j] = j: every source fine, every target one direction
    assert TR.src_of_table(rows_only, n) is None
    assert TR.src_of_table(rows_only.T, n) is None   # and the other way round
