"""The finite-size-scaling observables of the Ising flavor without a GPU: the wave vectors and fixed-point tables the
host builds (mc.reciprocal_vectors, mc.q30_tables), the restatement of tests/ising_fss_ref.py on configurations whose
structure factor is known, the delta-method errors of U4 and xi against a finite-difference propagation, and the C ABI."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ising_fss_ref as ref  # noqa: E402


def _lattices(m):
    return {"chain8": m.Chain(8), "square4": m.SquareLattice(4), "cubic3": m.CubicLattice(3, 3),
            "triangular4": m.TriangularLattice(4)}


def test_reciprocal_vectors_of_the_four_lattices(mc_amd):
    from montecarlo_jl_amd import lattices, mc
    want = {"chain8": [[2 * math.pi / 8]],
            "square4": [[2 * math.pi / 4, 0.0], [0.0, 2 * math.pi / 4]],
            "cubic3": (2 * math.pi / 3 * np.eye(3)).tolist(),
            # a1 = 4 (1/2, sqrt(3)/2), a2 = (4, 0): b1 = (0, 2 pi / (2 sqrt 3)), b2 = (2 pi / 4)(1, -1/sqrt 3)
            "triangular4": [[0.0, 2 * math.pi / (2 * math.sqrt(3))],
                            [2 * math.pi / 4, -2 * math.pi / (4 * math.sqrt(3))]]}
    for name, l in _lattices(mc_amd).items():
        k = mc.reciprocal_vectors(l)
        A = np.array(lattices._lattice_vectors(l))
        assert k.shape == (len(want[name]), A.shape[1]), name
        np.testing.assert_allclose(k, want[name], rtol=0, atol=1e-14, err_msg=name)
        np.testing.assert_allclose(A @ k.T, 2 * np.pi * np.eye(len(A)), rtol=0, atol=1e-13, err_msg=name)
        np.testing.assert_allclose(k, ref.reciprocal(A), rtol=0, atol=1e-14, err_msg=name)


def test_table_entries_are_llround_of_the_phases(mc_amd):
    from montecarlo_jl_amd import lattices, mc
    for name, l in _lattices(mc_amd).items():
        ks = mc.reciprocal_vectors(l)
        cq, sq, k = mc.q30_tables(l, ks)
        r = np.array(lattices._positions(l))
        assert cq.dtype == sq.dtype == np.int32 and cq.shape == sq.shape == (len(ks), len(l)), name
        for a in range(len(ks)):
            for i in range(len(l)):
                ph = float(np.dot(ks[a], r[i]))
                for got, x in ((cq[a, i], np.cos(ph) * 2.0 ** 30), (sq[a, i], np.sin(ph) * 2.0 ** 30)):
                    want = math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1)  # llround: half away from zero
                    assert int(got) == want, (name, a, i, got, want)
        rc, rs = ref.q30(r, ks)
        assert np.array_equal(cq, rc) and np.array_equal(sq, rs), name
        assert np.abs(cq).max() <= 2 ** 30 and np.abs(sq).max() <= 2 ** 30
    with pytest.raises(ValueError):
        mc.q30_tables(mc_amd.Chain(32), [[0.1 * j] for j in range(9)])
    assert mc.q30_tables(mc_amd.Chain(8), [])[0].shape == (0, 8)


def test_all_up_configuration_has_no_structure_factor_off_zero(mc_amd):
    """sum_i e^{i k . r_i} = 0 for a reciprocal k != 0; every entry is off by at most 1/2, so |F| <= N/2 and
    S_k <= N / 2^62, far below any signal (rounding is odd in its argument and the phases of these lattices come in
    opposite pairs, so the sums of these tables are in fact 0)"""
    from montecarlo_jl_amd import mc
    for name, l in _lattices(mc_amd).items():
        N = len(l)
        cq, sq, _ = mc.q30_tables(l, mc.reciprocal_vectors(l))
        up = np.ones(N, dtype=np.int8)
        fc, fs = ref.F(up, cq), ref.F(up, sq)
        assert np.abs(fc).max() <= N // 2 and np.abs(fs).max() <= N // 2, (name, fc, fs)
        assert ref.S(up, cq, sq).max() <= N / 2.0 ** 62, name
        assert ref.M2_M4(up) == (float(N * N), float(N) ** 4)
        v = ref.values(-up, cq, sq)
        assert v[0] == N * N and v[1] == float(N) ** 4 and v[2:].max() <= N / 2.0 ** 62


def test_staggered_configuration_at_pi_pi(mc_amd):
    from montecarlo_jl_amd import lattices, mc
    l = mc_amd.SquareLattice(4)
    r = np.array(lattices._positions(l))
    conf = np.where((r.sum(axis=1).astype(int)) % 2 == 0, 1, -1).astype(np.int8)
    cq, sq, _ = mc.q30_tables(l, [[math.pi, math.pi], [math.pi / 2, 0.0]])
    s = ref.S(conf, cq, sq)
    assert abs(s[0] - 16.0) <= 1e-8 * 16.0, s
    assert s[1] <= 16 / 2.0 ** 62, s
    assert ref.M2_M4(conf) == (0.0, 0.0)


def test_delta_method_errors_against_finite_differences(mc_amd):
    from montecarlo_jl_amd import mc
    rng = np.random.default_rng(5)
    N = 64
    for _ in range(20):
        M2 = rng.uniform(500.0, 3000.0)
        M4 = M2 * M2 * rng.uniform(1.05, 2.5)
        Sk = M2 / N / rng.uniform(1.5, 20.0)
        knorm = rng.uniform(0.05, 3.0)
        v2, v4, vs = (1e-3 * M2) ** 2, (2e-3 * M4) ** 2, (1.5e-3 * Sk) ** 2
        c4, cs = rng.uniform(-0.9, 0.9) * math.sqrt(v2 * v4), rng.uniform(-0.9, 0.9) * math.sqrt(v2 * vs)
        U, gU = mc._binder(M2, M4)
        assert U == pytest.approx(ref.binder(M2, M4), rel=1e-14)
        assert mc._delta_var(gU, v2, v4, c4) == pytest.approx(ref.fd_variance(ref.binder, M2, M4, v2, v4, c4), rel=1e-6)
        x, gx = mc._xi(M2, Sk, N, knorm)
        f = lambda a, b: ref.xi(a, b, N, knorm)  # noqa: E731
        assert x == pytest.approx(f(M2, Sk), rel=1e-14)
        assert mc._delta_var(gx, v2, vs, cs) == pytest.approx(ref.fd_variance(f, M2, Sk, v2, vs, cs), rel=1e-6)
    assert math.isnan(mc._xi(100.0, 10.0, 64, 1.0)[0])  # S(0) < S(k): no correlation length
    assert math.isnan(mc._delta_var((1.0, 1.0), float("nan"), 1.0, 0.0))
    assert mc._delta_var((1.0, -1.0), 1.0, 1.0, 1.0 + 1e-9) == 0.0  # clamped


def test_binner_restatement_cross_sums():
    """the FSS binner of the restatement against a direct evaluation: level l holds the means of 2^l consecutive values"""
    rng = np.random.default_rng(11)
    T, nk = 37, 2
    x = rng.uniform(0.0, 10.0, (T, 2 + nk))
    b = ref.FssBinnerRef(nk, capacity=100)
    for row in x:
        b.push(row)
    for l in range(b.L):
        n = T >> l
        blocks = x[:n << l].reshape(n, 1 << l, 2 + nk).mean(axis=1) if n else np.zeros((0, 2 + nk))
        assert b.count[l] == n
        np.testing.assert_allclose(b.x_sum[l], blocks.sum(axis=0), rtol=1e-13, atol=0)
        np.testing.assert_allclose(b.x2_sum[l], (blocks ** 2).sum(axis=0), rtol=1e-13, atol=0)
        np.testing.assert_allclose(b.xy_sum[l], (blocks[:, :1] * blocks[:, 1:]).sum(axis=0), rtol=1e-13, atol=0)


def test_new_symbols_and_invalid_arguments(mc_amd):
    from montecarlo_jl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    src = open(_lib.HEADER_PATH).read()
    for name in ("dqmc_mc_set_fss", "dqmc_mc_get_fss", "dqmc_mc_fss_binner_get_level", "dqmc_mc_fss_binner_finish"):
        assert hasattr(L, name) and name in _lib.SIGNATURES and name in src, name
    for t in ("dqmc_mc_fss;", "dqmc_mc_fss_binned;", "finite-size-scaling observables"):
        assert t in src, t
    assert C.sizeof(_lib.McFss) == 8 + 8 + 8 + 64 and C.sizeof(_lib.McFssBinned) == 8 * 49 + 8 + 8
    lib = _lib.lib()
    tab = (C.c_int32 * 16)()
    # n_k > 8 and a NULL table with n_k > 0 are refused before the handle is looked at
    for args, word in (((None, 9, tab, tab), "n_k"), ((None, -2, tab, tab), "n_k"), ((None, 2, None, tab), "table"),
                       ((None, 2, tab, None), "table"), ((None, 0, None, None), "handle"), ((None, -1, None, None), "handle")):
        assert lib.dqmc_mc_set_fss(*args) == _lib.ERR_INVALID, args
        assert word in lib.dqmc_mc_last_error(None).decode(), (args, lib.dqmc_mc_last_error(None))
    assert lib.dqmc_mc_get_fss(None, 0, C.byref(_lib.McFss())) == _lib.ERR_INVALID
    assert lib.dqmc_mc_fss_binner_get_level(None, 0, 0, None, None, None, None) == _lib.ERR_INVALID
    assert lib.dqmc_mc_fss_binner_finish(None, 0, -1, C.byref(_lib.McFssBinned())) == _lib.ERR_INVALID
