"""The q-state engine's scaling measurement on the host, no GPU: the restatement of tests/qstate_scaling_ref.py against
plain complex128 sums, its k = 0 and q = 2 limits, the launch cut with the measurement on (csrc/mc_tables.h,
qs_scaling_cut) under the host sanitizers, the keywords that are refused before a device is touched, and the restatement
alone at beta = 0.

On the plain sum.  The definition (include/dqmc_hip.h, "Scaling") is S_k = (F1^2 + F2^2 + F3^2 + F4^2) / (N 2^120): the
structure factor of the vector order parameter, (|sum_i cos theta_i e^{i k . r_i}|^2 + |sum_i sin theta_i e^{i k . r_i}|^2) / N.
The single complex sum Z = sum_i (cos theta_i + i sin theta_i) e^{i k . r_i} is (F1 - F4) + i (F2 + F3) in units of 2^60:
|Z|^2 / N differs from S_k by 2 (F2 F3 - F1 F4) / (N 2^120), which is zero at k = 0 and for q = 2 but of order 1 for a
random configuration otherwise (N = 36, q = 3: 2.88 against 1.64).  So each is compared with its own plain sum, at the
same tolerance: S_k with the two-component sum, and Z itself, real and imaginary part, with the restatement's
(F1 - F4, F2 + F3); |Z|^2 / N is compared with S_k where the two are the same quantity."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qstate_ref  # noqa: E402
import qstate_scaling_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")
LATTICES = {"cubic3": lambda g: g.CubicLattice(3, 3),    # N = 27: not a multiple of 4
            "square6": lambda g: g.SquareLattice(6),     # N = 36
            "square20": lambda g: g.SquareLattice(20)}   # N = 400


def _setup(mc_amd, shape, q):
    from montecarlo_jl_amd import lattices
    l = LATTICES[shape](mc_amd)
    r = np.array(lattices._positions(l), dtype=float)
    b = mc_amd.reciprocal_vectors(l)
    ks = np.array([b[0], b[-1] + b[0], 2.0 * b[-1], np.zeros(r.shape[1])])
    return l, r, ks, ref.q30(r, ks), ref.state_tables(q)


@pytest.mark.parametrize("q", [2, 3, 8, 64])
@pytest.mark.parametrize("shape", list(LATTICES))
def test_restatement_against_plain_sums(mc_amd, shape, q):
    """atol = 1e-8 N: a table entry is off by at most 2^-31 of the unit phase, which bounds the difference near
    2 2^-30 N = 1.9e-9 N; the fp64 roundings are far below"""
    l, r, ks, (cq, sq), (c, s) = _setup(mc_amd, shape, q)
    N = len(l)
    # the product's tables are the restatement's
    pc, ps, _ = mc_amd.mc.q30_tables(l, ks)
    assert np.array_equal(pc, cq) and np.array_equal(ps, sq) and pc.dtype == np.int32
    rng = np.random.default_rng(1000 * q + N)
    confs = [rng.integers(0, q, N) for _ in range(4)] + [np.zeros(N, dtype=np.int64), np.full(N, q - 1)]
    for conf in confs:
        theta = 2.0 * np.pi * conf / q
        phase = np.exp(1j * (r @ ks.T))                                    # [N][n_k] complex128
        zc, zs = np.cos(theta) @ phase, np.sin(theta) @ phase
        plain = (np.abs(zc) ** 2 + np.abs(zs) ** 2) / N
        got = ref.S(conf, c, s, cq, sq)
        print(shape, q, got, plain)
        np.testing.assert_allclose(got, plain, rtol=0, atol=1e-8 * N)
        # the single complex sum against the restatement's amplitude, and its square where it is S_k
        Z = (np.cos(theta) + 1j * np.sin(theta)) @ phase
        F = ref.amplitudes(conf, c, s, cq, sq) / 2.0 ** 60
        np.testing.assert_allclose(F[:, 0] - F[:, 3], Z.real, rtol=0, atol=1e-8 * N)
        np.testing.assert_allclose(F[:, 1] + F[:, 2], Z.imag, rtol=0, atol=1e-8 * N)
        same = np.ones(len(ks), dtype=bool) if q == 2 else np.array([not k.any() for k in ks])
        np.testing.assert_allclose(got[same], (np.abs(Z) ** 2 / N)[same], rtol=0, atol=1e-8 * N)


@pytest.mark.parametrize("q", [2, 3, 8, 64])
@pytest.mark.parametrize("shape", list(LATTICES))
def test_k0_is_m2_and_q2_has_no_sine_terms(mc_amd, shape, q):
    """constant tables (2^30, 0): S N against m2 from the integer (Mx, My) at atol 1e-12 N^2 (both are below N^2; the two
    differ by a handful of roundings)"""
    l, r, ks, _, (c, s) = _setup(mc_amd, shape, q)
    N = len(l)
    cq, sq = np.full((1, N), 2 ** 30, dtype=np.int64), np.zeros((1, N), dtype=np.int64)
    rng = np.random.default_rng(7 * q + N)
    for conf in [rng.integers(0, q, N) for _ in range(4)] + [np.zeros(N, dtype=np.int64)]:
        got = ref.S(conf, c, s, cq, sq)[0] * N
        want = ref.m2(conf, c, s)
        assert abs(got - want) <= 1e-12 * N * N, (got, want)
        Mx, My = ref.order_parameter(conf, c, s)
        assert want == pytest.approx((Mx * Mx + My * My) / 2.0 ** 60, rel=1e-15)
    if q == 2:
        assert list(s) == [0, 0]
        _, _, _, (cq, sq), _ = _setup(mc_amd, shape, q)
        F = ref.amplitudes(rng.integers(0, q, N), c, s, cq, sq)
        assert np.all(F[:, 2:] == 0.0) and not np.signbit(F[:, 2:]).any() and F[:, :2].any()


# ---- the launch cut
@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    """g++ -fsanitize=address,undefined, run once as a child process on the CPU"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host code"
    exe = str(tmp_path_factory.mktemp("qs_scaling_cut") / "qs_scaling_cut_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "qs_scaling_cut_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    blocks = re.findall(r"^case ((?:-?\d+ ?)+)\nplain(.*)\nscaling(.*)$", out.stdout, re.M)
    parse = lambda t: [tuple(int(x) for x in e.split(",")) for e in t.split()]  # noqa: E731
    return [(tuple(int(x) for x in c.split()), parse(p), parse(s)) for c, p, s in blocks]


def _measured(i, therm, rate):
    return i > therm and i % rate == 0


def test_cut_rule(cuts):
    """with the measurement on, every measured sweep ends a launch; the rounds and defer_last are those of the cut
    without it; T_at_start counts the measurements before the launch; the launches are the n sweeps in order"""
    seen = set()
    for (n, first, therm, rate, k, chunk, T0), plain, scaling in cuts:
        seen.add((rate, therm, k, chunk))
        for launches in (plain, scaling):
            at, T = first, T0
            for m, f, defer, Ts in launches:
                assert m >= 1 and f == at and Ts == T and m <= chunk, (launches, at, T)
                last = f + m - 1
                # a round only behind a launch's last sweep, and every round sweep is one
                assert not any(k > 0 and i % k == 0 for i in range(f, last)), launches
                assert defer == int(k > 0 and last % k == 0 and _measured(last, therm, rate))
                T += sum(_measured(i, therm, rate) for i in range(f, last + 1))
                at = last + 1
            assert at == first + n
        for m, f, defer, Ts in scaling:  # at most one measured sweep per launch, its last
            assert not any(_measured(i, therm, rate) for i in range(f, f + m - 1)), scaling
        ends = lambda ls: {f + m - 1 for m, f, _, _ in ls}  # noqa: E731
        meas = {i for i in range(first, first + n) if _measured(i, therm, rate)}
        rounds = {i for i in range(first, first + n) if k > 0 and i % k == 0}
        assert meas <= ends(scaling) and rounds <= ends(scaling) and rounds <= ends(plain)
        # nothing else cuts: a launch ends at a measured sweep, at a round, at the work bound or with the call
        for m, f, _, _ in scaling:
            assert f + m - 1 in meas | rounds | {first + n - 1} or m == chunk, scaling
        for m, f, _, _ in plain:
            assert f + m - 1 in rounds | {first + n - 1} or m == chunk, plain
        assert {(f + m - 1, d) for m, f, d, _ in plain if d} == {(f + m - 1, d) for m, f, d, _ in scaling if d}
        if rate == 1 and therm == 0:
            assert all(m == 1 for m, _, _, _ in scaling)
    assert seen == {(r, t, k, c) for r in (1, 3) for t in (0, 4) for k in (0, 1, 2, 5) for c in (1, 7)}
    assert len(cuts) == 4 * 32


# ---- keywords, before any device is touched
def test_keywords(mc_amd):
    model = mc_amd.PottsModel(3, dims=2, L=4)
    b = mc_amd.reciprocal_vectors(model.l)
    nine = [i * b[0] + b[1] for i in range(9)]
    with pytest.raises(ValueError, match="wave vectors"):
        mc_amd.MC(model, beta=0.5, scaling=nine)
    with pytest.raises(ValueError, match="wave vectors"):
        mc_amd.MC(model, beta=0.5, scaling=[])
    with pytest.raises(NotImplementedError, match="IsingModel only"):
        mc_amd.MC(model, beta=0.5, fss=True)
    with pytest.raises(NotImplementedError, match="D = 3 only"):  # a lattice without positions: what _positions raises
        mc_amd.MC(mc_amd.PottsModel(3, l=mc_amd.CubicLattice(4, 2)), beta=0.5, scaling=True)


def test_abi_is_declared(mc_amd):
    from montecarlo_jl_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqmc_hip.h")).read()
    for name in ("dqmc_qs_set_scaling", "dqmc_qs_get_scaling", "dqmc_qs_scaling_binner_get_level",
                 "dqmc_qs_scaling_binner_finish"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(_lib.lib(), name), name


# ---- physics: the restatement alone at beta = 0
def hot_binners(l, confs_of):
    """one ScalingBinnerRef per walker, fed [M2, S_0, S_1] of the HOT_MEAS configurations confs_of(m) -> [W][N]"""
    from montecarlo_jl_amd import lattices, mc
    cq, sq = ref.q30(lattices._positions(l), mc.reciprocal_vectors(l))
    c, s = ref.state_tables(ref.HOT_Q)
    bins = [ref.ScalingBinnerRef(2, capacity=ref.HOT_MEAS) for _ in range(ref.HOT_W)]
    for m in range(ref.HOT_MEAS):
        for w, conf in enumerate(confs_of(m)):
            bins[w].push(ref.values(conf, c, s, cq, sq))
    return bins


def test_restatement_at_beta_zero(mc_amd):
    """PottsModel(3, dims=2, L=8), 64 walkers (keys HOT_SEED + w), 200 measured sweeps at beta = 0: the four amplitudes are
    sums of N independent terms, so <S_k> = 1 for k != 0.  The restatement's chain and measurement alone: the pooled
    means are 1.004594 +- 0.007274 and 1.007452 +- 0.007533 (level 2, 50 bins per walker), 0.63 and 0.99 pooled standard
    errors from 1: inside the bound of 5."""
    l = mc_amd.SquareLattice(ref.HOT_L)
    wk = qstate_ref.Walkers(l, ref.HOT_Q, qstate_ref.potts_table(ref.HOT_Q), [0.0] * ref.HOT_W,
                            [ref.HOT_SEED + w for w in range(ref.HOT_W)])

    def confs_of(m):
        wk.sweep()
        return wk.c

    bins = hot_binners(l, confs_of)
    assert bins[0].reliable_level() == 2
    for e in (1, 2):
        mean, err = ref.pooled(bins, e)
        print("S_%d" % (e - 1), mean, err, (mean - 1.0) / err)
        assert err > 0 and abs(mean - 1.0) <= 5.0 * err, (e, mean, err)
