"""GPU parity of the batched linalg primitives against the CPU oracle and against the
algebraic contracts of the reference's test/slice_matrices.jl:141-235."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-10  # north_star: Green's-function elements within 1e-10 relative


@pytest.mark.parametrize("n,batch", [(16, 3), (64, 2), (100, 1), (256, 9)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_vmul_variants(gpu, n, batch, ta, tb):
    rng = np.random.default_rng(n + 2 * ta + tb)
    A = rng.standard_normal((batch, n, n))
    B = rng.standard_normal((batch, n, n))
    C = gpu.vmul(A, B, bool(ta), bool(tb))
    for i in range(batch):
        ref = (A[i].T if ta else A[i]) @ (B[i].T if tb else B[i])
        assert relerr(C[i], ref) < 1e-13


@pytest.mark.parametrize("n,batch", [(257, 2), (300, 1), (600, 2), (1024, 1)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_vmul_variants_n_above_256(gpu, n, batch, ta, tb):
    """n > 256, off and on the tile grid up to the ceiling: every entry within the dot product's error bound
    |C - ref| <= 2 n eps (|op(A)| |op(B)|), which a dropped or doubled k-term in any entry breaks (a max-norm relative
    error lets a wrong small entry through)"""
    rng = np.random.default_rng(n + 2 * ta + tb)
    A = rng.standard_normal((batch, n, n))
    B = rng.standard_normal((batch, n, n))
    C = gpu.vmul(A, B, bool(ta), bool(tb))
    eps = np.finfo(np.float64).eps
    for i in range(batch):
        opA, opB = (A[i].T if ta else A[i]), (B[i].T if tb else B[i])
        bound = 2 * n * eps * (np.abs(opA) @ np.abs(opB))
        assert np.all(np.abs(C[i] - opA @ opB) <= bound), (i, (np.abs(C[i] - opA @ opB) / bound).max())


def test_vmul_layout_asymmetric(gpu):
    """A = I against an asymmetric B catches a transposed accumulator map"""
    n = 32
    B = np.arange(n * n, dtype=np.float64).reshape(n, n)
    C = gpu.vmul(np.eye(n), B)
    assert np.array_equal(C[0], B)
    C = gpu.vmul(B, np.eye(n))
    assert np.array_equal(C[0], B)


@pytest.mark.parametrize("n", [16, 64, 256])
@pytest.mark.parametrize("apply_pivot", [True, False])
def test_udt_contracts(gpu, O, n, apply_pivot):
    """test/slice_matrices.jl:202-234: U*Diagonal(D)*T ≈ X, U unitary, D sorted positive;
    Val(false): U*D*UpperTriangular(T)*P ≈ X with P[i, pivot[i]] = 1"""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((4, n, n))
    X[1] *= np.exp(rng.uniform(-20, 20, size=n))[None, :]   # graded columns as in a DQMC chain
    U, D, T, piv = gpu.udt_AVX_pivot(X, apply_pivot)
    # n = 256 takes the one-launch form whose pivot order is fixed up front (csrc/qrb.hip; tests/test_gpu_udt_blocked.py):
    # D is then not sorted (the reference's contracts, test/slice_matrices.jl:202-234, do not ask for it) and the oracle to
    # compare the factors with is the oracle run with the same pre-sorted order
    presorted = n == 256
    for i in range(X.shape[0]):
        assert relerr(U[i].T @ U[i], np.eye(n)) < 1e-12
        assert np.all(D[i] > 0)
        if not presorted:
            assert np.all(np.diff(D[i]) <= 1e-12 * D[i][:-1])
        assert sorted(piv[i]) == list(range(1, n + 1))
        if apply_pivot:
            rec = (U[i] * D[i]) @ T[i]
        else:
            P = np.zeros((n, n)); P[np.arange(n), piv[i] - 1] = 1
            rec = (U[i] * D[i]) @ np.triu(T[i]) @ P
        scale = np.abs(X[i]).max(axis=0)
        assert (np.abs(rec - X[i]) / scale[None, :]).max() < 1e-12
        # same decomposition as the oracle when no pivot tie flips
        O.lib().orc_set_udt_presort(1 if presorted else 0)
        try:
            Uo, Do, To, po = O.udt_pivot(X[i], apply_pivot)
        finally:
            O.lib().orc_set_udt_presort(0)
        if np.array_equal(po, piv[i]):
            assert relerr(D[i], Do) < 1e-10
            assert relerr(U[i], Uo) < 1e-9


@pytest.mark.parametrize("n,batch", [(257, 2), (320, 3), (576, 2), (600, 1), (1024, 1)])
def test_udt_panel_kernel_n_above_256(gpu, O, n, batch):
    """n > 256: the panel (dlaqps-style) QR - one read of the trailing matrix per step, norms down-dated with the row of R
    and recomputed on cancellation - against the contracts of test/slice_matrices.jl:202-234, against the oracle's
    decomposition (same pivots unless a near-tie flips, same D) and against the streaming kernel it replaces
    (DQMC_QR_NOPANEL: the reference's from-scratch norms)"""
    import os
    rng = np.random.default_rng(n)
    X = rng.standard_normal((batch, n, n))
    X[0] *= np.exp(rng.uniform(-20, 20, size=n))[None, :]      # graded columns as in a DQMC chain
    if batch > 1:
        X[1] = X[1] @ np.diag(np.exp(np.linspace(15, -15, n))) @ rng.standard_normal((n, n)) / n  # graded, mixed
    for apply_pivot in (True, False):
        U, D, T, piv = gpu.udt_AVX_pivot(X, apply_pivot)
        os.environ["DQMC_QR_NOPANEL"] = "1"
        try:
            U0, D0, T0, piv0 = gpu.udt_AVX_pivot(X, apply_pivot)
        finally:
            del os.environ["DQMC_QR_NOPANEL"]
        for i in range(batch):
            assert relerr(U[i].T @ U[i], np.eye(n)) < 1e-12
            assert np.all(D[i] > 0) and np.all(np.diff(D[i]) <= 1e-9 * D[i][:-1])
            assert sorted(piv[i]) == list(range(1, n + 1))
            if apply_pivot:
                rec = (U[i] * D[i]) @ T[i]
            else:
                P = np.zeros((n, n)); P[np.arange(n), piv[i] - 1] = 1
                rec = (U[i] * D[i]) @ np.triu(T[i]) @ P
            scale = np.abs(X[i]).max(axis=0)
            assert (np.abs(rec - X[i]) / scale[None, :]).max() < 1e-11
            if np.array_equal(piv[i], piv0[i]):
                assert relerr(D[i], D0[i]) < 1e-10
            else:  # a near-tie went the other way: D is still the same to the size of the tie
                assert np.abs(np.log(D[i] / D0[i])).max() < 1e-6
        if n <= 320 and apply_pivot:
            Uo, Do, To, po = O.udt_pivot(X[0], True)
            if np.array_equal(po, piv[0]):
                assert relerr(D[0], Do) < 1e-10


def test_two_phase_qr_against_cooperative_alone(gpu):
    """n = 256, the pivoted factorisation behind DQMC_QR_NOBLOCKED (more than 32 units per GPU, fallback): 128 cooperative
    steps + qr_tail_kernel (one CU per matrix, last 64 steps one column per lane) against the cooperative kernel factoring
    everything (DQMC_QR_TAIL=0): same pivots, same factors up to rounding"""
    import os
    rng = np.random.default_rng(5)
    X = rng.standard_normal((8, 256, 256))
    X[1] *= np.exp(rng.uniform(-20, 20, size=256))[None, :]
    X[2][:, 7] = 0.0                      # a zero column (tau = 0 branch)
    X[3][:, 9] = X[3][:, 200]             # equal norms: the tie goes to the smaller position
    os.environ["DQMC_QR_NOBLOCKED"] = "1"   # (the reference's pivot rule; the default at n = 256 is the pre-pivoted one-launch UDT)
    try:
        U1, D1, T1, p1 = gpu.udt_AVX_pivot(X, False)
        os.environ["DQMC_QR_TAIL"] = "0"
        try:
            U0, D0, T0, p0 = gpu.udt_AVX_pivot(X, False)
        finally:
            del os.environ["DQMC_QR_TAIL"]
    finally:
        del os.environ["DQMC_QR_NOBLOCKED"]
    for i in range(X.shape[0]):
        assert sorted(p1[i]) == list(range(1, 257))
        if i == 2:  # singular input: D[255] = 0 and T = D^-1 R is not finite (as in the reference); the zero column
            assert p1[i][255] == 8 and D1[i][255] == 0.0  # must come out last, with tau = 0 and nothing hanging
            continue
        P = np.zeros((256, 256)); P[np.arange(256), p1[i] - 1] = 1
        rec = (U1[i] * D1[i]) @ np.triu(T1[i]) @ P
        scale = np.abs(X[i]).max(axis=0)
        assert (np.abs(rec - X[i]) / scale[None, :]).max() < 1e-12
        assert np.array_equal(p0[i], p1[i])
        assert relerr(D1[i], D0[i]) < 1e-12


def test_two_phase_qr_many_units(gpu):
    """more matrices than the cooperative kernel can hold (> 64 at n = 256): the single-workgroup tile kernel does the
    first 128 steps and hands over to qr_tail_kernel; against the tile kernel alone (DQMC_QR_TAIL=0)"""
    import os
    rng = np.random.default_rng(6)
    X = rng.standard_normal((72, 256, 256))
    X[5] *= np.exp(rng.uniform(-20, 20, size=256))[None, :]
    U1, D1, T1, p1 = gpu.udt_AVX_pivot(X, True)
    os.environ["DQMC_QR_TAIL"] = "0"
    try:
        U0, D0, T0, p0 = gpu.udt_AVX_pivot(X, True)
    finally:
        del os.environ["DQMC_QR_TAIL"]
    for i in (0, 5, 37, 71):
        rec = (U1[i] * D1[i]) @ T1[i]
        scale = np.abs(X[i]).max(axis=0)
        assert (np.abs(rec - X[i]) / scale[None, :]).max() < 1e-12
        assert relerr(U1[i].T @ U1[i], np.eye(256)) < 1e-12
    assert np.array_equal(p0, p1)
    assert relerr(D1, D0) < 1e-12


@pytest.mark.parametrize("n", [16, 64, 256])
def test_rdivp(gpu, O, n):
    """test/slice_matrices.jl:226-234: rdivp!(u, t, tmp, pivot) ≈ U*P'/UpperTriangular(T)"""
    rng = np.random.default_rng(n + 1)
    X = rng.standard_normal((n, n))
    _, _, T, piv = O.udt_pivot(X, False)
    A = rng.standard_normal((3, n, n))
    out = gpu.rdivp(A, np.stack([T] * 3), np.stack([piv] * 3))
    for i in range(3):
        ref = O.rdivp(A[i], T, piv)
        assert relerr(out[i], ref) < 1e-10


@pytest.mark.parametrize("n", [257, 291, 292, 574, 575, 1024])
def test_rdivp_n_above_256(gpu, O, n):
    """n > 256: the substitution on an LDS row slab (trsm_kernel<RS>) on both sides of each switch of its height
    (64 rows up to 291, 32 up to 574, 16 up to 1024), with the non-identity pivots of a pivoted UDT: against the oracle,
    and the residual Out triu(T) = A[:, pivot] in every entry, scaled by the column norms"""
    rng = np.random.default_rng(n + 1)
    X = rng.standard_normal((n, n))
    _, _, T, piv = O.udt_pivot(X, False)
    assert not np.array_equal(piv, np.arange(1, n + 1))
    A = rng.standard_normal((2, n, n))
    A[1] *= np.exp(rng.uniform(-10, 10, size=n))[:, None]   # graded rows
    out = gpu.rdivp(A, np.stack([T] * 2), np.stack([piv] * 2))
    Tu = np.triu(T)
    for i in range(2):
        ref = O.rdivp(A[i], T, piv)
        assert relerr(out[i], ref) < 1e-10
        Ap = A[i][:, piv - 1]
        res = np.abs(out[i] @ Tu - Ap) / np.linalg.norm(Ap, axis=0)[None, :]
        assert res.max() < 1e-12, res.max()


@pytest.mark.parametrize("n", [16, 64, 256, 257, 324, 600, 1024])
def test_calculate_greens_AVX(gpu, O, n):
    """G = [I + Ul Dl Tl (Ur Dr Tr)']^-1 (stack.jl:337-393) against the oracle and a direct inverse"""
    rng = np.random.default_rng(n + 2)
    batch = 2
    args = []
    for _ in range(batch):
        Ul, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Ur, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Dl = np.sort(np.exp(rng.uniform(-3, 3, n)))[::-1]
        Dr = np.sort(np.exp(rng.uniform(-3, 3, n)))[::-1]
        Tl = np.eye(n) + 0.1 * rng.standard_normal((n, n))
        Tr = np.eye(n) + 0.1 * rng.standard_normal((n, n))
        args.append((Ul, Dl, Tl, Ur, Dr, Tr))
    stack = lambda k: np.stack([a[k] for a in args])
    G = gpu.calculate_greens_AVX(stack(0), stack(1), stack(2), stack(3), stack(4), stack(5))
    worst = 0.0
    for i, a in enumerate(args):
        Go = O.calculate_greens(*a)
        worst = max(worst, relerr(G[i], Go))
        assert relerr(G[i], Go) < TOL
        Ul, Dl, Tl, Ur, Dr, Tr = a
        direct = np.linalg.inv(np.eye(n) + (Ul * Dl) @ Tl @ ((Ur * Dr) @ Tr).T)
        assert relerr(G[i], direct) < 1e-8
    print("n = %d: worst rel |G - G_oracle| = %.3g" % (n, worst))


@pytest.mark.parametrize("n", [16, 64, 256, 257, 324, 600, 1024])
def test_calculate_greens_AVX_chain_graded(gpu, O, n):
    """the sizes of test_calculate_greens_AVX with Dl, Dr = exp(linspace(+20, -20, n)) (greens_ref.graded_udt_inputs at
    g = 20, the grading that test_gpu_greens_graded.py asks of every size; more than 17 decades on each side of 1)
    against the reference-rule oracle at TOL.  At n = 256 the device takes the pre-pivoted one-launch UDT.  A direct
    float64 inverse is no reference at this grading; the extended-precision one is in test_gpu_greens_graded.py."""
    import greens_ref
    batch = 2
    args = greens_ref.graded_udt_inputs(n, 20, 5000 + n, batch)
    G = gpu.calculate_greens_AVX(*args)
    worst = 0.0
    for i in range(batch):
        assert greens_ref.straddles_one(args[1][i]) and greens_ref.straddles_one(args[4][i])
        worst = max(worst, relerr(G[i], O.calculate_greens(*greens_ref.unit(args, i))))
    print("n = %d, g = 20: worst rel |G - G_oracle| = %.3g" % (n, worst))
    assert worst < TOL


@pytest.mark.parametrize("batch", [9, 33])
def test_rdivp_partial_later_group(gpu, O, batch):
    """n = 256 with units that end inside a later group of eight (trsm_rl_kernel's block map pads them to whole groups):
    every unit against the oracle, and the residual Out triu(T) = A[:, pivot] in every entry, scaled by the column norms,
    within the bound of test_rdivp_n_above_256.  Every unit has its own T and pivot, so a unit served another unit's
    operands fails."""
    n = 256
    rng = np.random.default_rng(1000 + batch)
    Ts, pivs = [], []
    for i in range(batch):
        _, _, T, piv = O.udt_pivot(rng.standard_normal((n, n)), False)
        assert not np.array_equal(piv, np.arange(1, n + 1))
        Ts.append(T)
        pivs.append(piv)
    A = rng.standard_normal((batch, n, n))
    A[batch - 1] *= np.exp(rng.uniform(-10, 10, size=n))[:, None]   # graded rows in the last unit
    out = gpu.rdivp(A, np.stack(Ts), np.stack(pivs))
    worst = 0.0
    for i in range(batch):
        assert relerr(out[i], O.rdivp(A[i], Ts[i], pivs[i])) < 1e-10, i
        Ap = A[i][:, pivs[i] - 1]
        res = np.abs(out[i] @ np.triu(Ts[i]) - Ap) / np.linalg.norm(Ap, axis=0)[None, :]
        worst = max(worst, res.max())
        assert res.max() < 1e-12, (i, res.max())
    print("rdivp, n = 256, batch %d: worst scaled residual %.3g" % (batch, worst))


@pytest.mark.parametrize("batch", [9, 33])
def test_calculate_greens_AVX_partial_later_group(gpu, O, batch):
    """n = 256 with a partial later group of eight units: every unit against the oracle (1e-10) and a direct inverse (1e-8),
    as test_calculate_greens_AVX"""
    n = 256
    rng = np.random.default_rng(2000 + batch)
    args = []
    for _ in range(batch):
        Ul, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Ur, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Dl = np.sort(np.exp(rng.uniform(-3, 3, n)))[::-1]
        Dr = np.sort(np.exp(rng.uniform(-3, 3, n)))[::-1]
        Tl = np.eye(n) + 0.1 * rng.standard_normal((n, n))
        Tr = np.eye(n) + 0.1 * rng.standard_normal((n, n))
        args.append((Ul, Dl, Tl, Ur, Dr, Tr))
    stack = lambda k: np.stack([a[k] for a in args])
    G = gpu.calculate_greens_AVX(stack(0), stack(1), stack(2), stack(3), stack(4), stack(5))
    worst = 0.0
    for i, a in enumerate(args):
        e = relerr(G[i], O.calculate_greens(*a))
        worst = max(worst, e)
        assert e < TOL, (i, e)
        Ul, Dl, Tl, Ur, Dr, Tr = a
        direct = np.linalg.inv(np.eye(n) + (Ul * Dl) @ Tl @ ((Ur * Dr) @ Tr).T)
        assert relerr(G[i], direct) < 1e-8, i
    print("n = 256, batch %d: worst rel |G - G_oracle| = %.3g" % (batch, worst))


@pytest.mark.parametrize("batch", [33, 64, 65])
@pytest.mark.parametrize("apply_pivot", [True, False])
def test_udt_natural_dispatch_at_the_qr_edges(gpu, O, batch, apply_pivot):
    """n = 256 with no switch set, either side of the two limits of the pivoted factorisation (on 256 CUs: 33 units are the
    first past the one-launch UDT, 64 the last the cooperative QR admits, 65 take the tile kernel and qr_tail_kernel): the
    contracts of test_udt_contracts for every unit, and units 0, the first of the last group of eight and the last against
    the oracle run under the pivot rule of the form that the admission rules select.  The last unit has graded columns."""
    import launch_rules as R
    n = 256
    caps = R.capacities(gpu)
    presorted = R.udt_one_launch(n, batch, caps)
    print("batch %d: %s" % (batch, "one-launch UDT" if presorted else
                            ("cooperative QR" if R.qr_coop(n, batch, caps) else "tile QR + tail")))
    rng = np.random.default_rng(3000 + batch)
    X = rng.standard_normal((batch, n, n))
    X[batch - 1] *= np.exp(rng.uniform(-20, 20, size=n))[None, :]
    U, D, T, piv = gpu.udt_AVX_pivot(X, apply_pivot)
    for i in range(batch):
        assert relerr(U[i].T @ U[i], np.eye(n)) < 1e-12, i
        assert np.all(D[i] > 0)
        if not presorted:
            assert np.all(np.diff(D[i]) <= 1e-12 * D[i][:-1])
        assert sorted(piv[i]) == list(range(1, n + 1))
        if apply_pivot:
            rec = (U[i] * D[i]) @ T[i]
        else:
            P = np.zeros((n, n)); P[np.arange(n), piv[i] - 1] = 1
            rec = (U[i] * D[i]) @ np.triu(T[i]) @ P
        scale = np.abs(X[i]).max(axis=0)
        assert (np.abs(rec - X[i]) / scale[None, :]).max() < 1e-12, i
    O.lib().orc_set_udt_presort(1 if presorted else 0)
    try:
        for i in sorted({0, 8 * ((batch - 1) // 8), batch - 1}):
            Uo, Do, To, po = O.udt_pivot(X[i], apply_pivot)
            assert np.array_equal(po, piv[i]), "unit %d: pivots differ from the oracle's" % i
            assert relerr(D[i], Do) < 1e-10
            assert relerr(U[i], Uo) < 1e-9
    finally:
        O.lib().orc_set_udt_presort(0)


def test_mfma_peak_probe(gpu):
    tf = gpu.mfma_f64_peak(20000)
    print("fp64 MFMA probe: %.1f TFLOP/s" % tf)
    assert tf > 10.0
