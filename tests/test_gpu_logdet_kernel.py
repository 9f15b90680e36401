"""logdet_kernel (csrc/logdet.hip) on its own, through dqmc_logdet_matrices: sum log D and the sign of det A from the
partial-pivoting LU, on matrices whose sign is known, at every size at which the kernel changes its way of working.

Sizes.  1, 2, 3: the loops' first and last turns coincide.  36, 63: the LDS path with n and n * n off the 64-lane and
256-thread strides.  64: the last LDS size.  65: the first size eliminated in place in memory, leading dimension n.  100,
255, 256, 257, 320: the pivot search's `i += 256` stride with idle threads (their bi = n sentinel), one full turn, and a
second turn; the lane / wave loops of the trailing update off their strides.

Every case is a batch of three different matrices.  References: numpy.linalg.slogdet in float64 on matrices with
cond_2 < 1e6 (a sign error of the LU needs a backward error of 1 / cond), or a parity known exactly.  lu_sign_host is
the documented rule (largest magnitude on or below the diagonal, lowest row among equals) in float64 on the host; it is
used to count the ties a matrix really presents and to check that the graded inputs are within reach of a float64 LU, not
as the expected value.

logabsdet: |device - math.fsum(log d)| <= 2 n 2^-53 sum_i |log d_i|: one ulp per log and n - 1 roundings of partial sums
that are at most the absolute sum."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 36, 63, 64, 65, 100, 255, 256, 257, 320)
SENTINEL = -777.25
COND_MAX = 1e6


# ---- host side -------------------------------------------------------------------------------------------------------
def run(gpu, mats, ds=None, padded=False):
    """-> (logabsdet [batch], sign [batch]) of the kernel; padded: strideA = n n + 7, strideD = n + 3, the gaps filled
    with SENTINEL, which must come back as it went in (and D whole: the kernel only reads it)"""
    n, batch = mats[0].shape[0], len(mats)
    sa, sd = (n * n + 7, n + 3) if padded else (n * n, n)
    a = np.full(batch * sa, SENTINEL)
    d = np.full(batch * sd, SENTINEL)
    for u, m in enumerate(mats):
        a[u * sa:u * sa + n * n] = np.asarray(m, dtype=np.float64).reshape(-1, order="F")
        d[u * sd:u * sd + n] = 1.0 if ds is None else ds[u]
    lad, sg, a_out, d_out = gpu.logdet_matrices(a, d, n, strideA=sa, strideD=sd)
    for u in range(batch):
        assert np.array_equal(a_out[u * sa + n * n:(u + 1) * sa], a[u * sa + n * n:(u + 1) * sa]), "padding of A, unit %d" % u
    assert np.array_equal(d_out, d, equal_nan=True), "D or its padding was written"
    return lad, sg


def lu_sign_host(A):
    """the documented rule in float64 -> (sign, ties): ties counts the columns whose pivot magnitude occurred in several
    candidate rows ("any"), and of these, per kind: "lane" (a row 64 k further down: the same lane of another wave or turn), "wave" (a row
    of another wave), "stride" (a row of another turn of the 256-thread search); ties["unit_pivots"]: every pivot was +-1,
    so on an integer matrix every multiplier and every value stayed an integer and the sign is exact"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    sgn, ties = 1, dict(any=0, lane=0, wave=0, stride=0, unit_pivots=True)
    for k in range(n):
        col = np.abs(A[k:, k])
        with np.errstate(invalid="ignore"):
            if not np.isfinite(col).all():
                return 0, ties
        bi = k + int(np.argmax(col))  # (the first of equals)
        bv = col[bi - k]
        if not bv > 0:
            return 0, ties
        other = k + np.nonzero(col == bv)[0][1:] - bi  # distances of the other rows with the same magnitude
        if other.size:
            ties["any"] += 1
            ties["lane"] += bool((other % 64 == 0).any())
            ties["wave"] += bool((((other + (bi - k)) // 64) % 4 != ((bi - k) // 64) % 4).any())
            ties["stride"] += bool((((other + (bi - k)) // 256) != (bi - k) // 256).any())
        ties["unit_pivots"] &= bool(bv == 1.0)
        if A[bi, k] < 0:
            sgn = -sgn
        if bi != k:
            sgn = -sgn
            A[[k, bi]] = A[[bi, k]]
        if k < n - 1:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k, k + 1:])
    return sgn, ties


@functools.lru_cache(maxsize=None)
def gaussian_set(n):
    """three seeded Gaussian n x n matrices with cond_2 < COND_MAX, both signs among them -> (matrices, signs)"""
    rng = np.random.Generator(np.random.Philox(key=1000 + n))
    mats, signs = [], []
    for _ in range(200):
        m = rng.standard_normal((n, n))
        if not np.linalg.cond(m) < COND_MAX:
            continue
        s = int(np.linalg.slogdet(m)[0])
        if len(mats) == 2 and signs[0] == signs[1] == s:
            continue  # the third must bring the other sign
        mats.append(m)
        signs.append(s)
        if len(mats) == 3:
            break
    assert len(mats) == 3 and set(signs) == {-1, 1}, (n, signs)
    for m in mats:
        m.setflags(write=False)
    return tuple(mats), tuple(signs)


def parity(perm):
    """+1 / -1 of a permutation, from its cycles"""
    seen, sign = np.zeros(len(perm), dtype=bool), 1
    for i in range(len(perm)):
        length = 0
        while not seen[i]:
            seen[i] = True
            i = perm[i]
            length += 1
        if length and length % 2 == 0:
            sign = -sign
    return sign


def permutation(rng, n, want):
    """a random permutation of the wanted parity (n = 1 has the even one only)"""
    p = rng.permutation(n)
    if n > 1 and parity(p) != want:
        p[[0, 1]] = p[[1, 0]]
    return p


def perm_matrix(p):
    m = np.zeros((len(p), len(p)))
    m[np.arange(len(p)), p] = 1.0
    return m


# ---- 1. well-conditioned signs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("n", SIZES)
def test_gaussian_signs(gpu, n, padded):
    mats, signs = gaussian_set(n)
    lad, sg = run(gpu, mats, padded=padded)
    print("n = %d %s: negative blocks %d of 3, device signs %s" % (n, "padded" if padded else "packed",
                                                                  signs.count(-1), list(sg)))
    assert tuple(sg) == signs
    assert np.array_equal(lad, np.zeros(3))  # D = 1: every log is exactly 0


# ---- 2. exact signs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["permutation", "signed_permutation", "triangular"])
@pytest.mark.parametrize("n", SIZES)
def test_exact_signs(gpu, n, kind):
    """permutation matrices (odd, even, odd): the sign is the parity of the row exchanges alone.  The same with about
    half of the entries negated: times (-1)^(negated pivots).  diag(+-1) times a unit lower triangular matrix with entries
    -1, 0, 1 below the diagonal: every column ties the diagonal with rows below it, the lowest row - the diagonal - is
    the pivot, the pivot row is zero to the right, so the elimination changes nothing and the sign is prod(+-1)."""
    rng = np.random.Generator(np.random.Philox(key=2000 + n))
    mats, want = [], []
    for odd in (True, False, True):
        if kind == "triangular":
            s = rng.choice([-1.0, 1.0], size=n)
            if n > 1:
                s[0] = s[0] if (np.prod(s) < 0) == odd else -s[0]
            mats.append(s[:, None] * (np.tril(rng.integers(-1, 2, size=(n, n)).astype(np.float64), -1) + np.eye(n)))
            want.append(int(np.prod(s)))
            continue
        p = permutation(rng, n, -1 if odd else 1)
        m, w = perm_matrix(p), parity(p)
        if kind == "signed_permutation":
            neg = rng.integers(0, 2, size=n).astype(bool)
            if n > 1 and neg.sum() % 2:
                neg[n - 1] = not neg[n - 1]  # an even number: the parity of the permutation still decides the sign
            m[neg] = -m[neg]
            w *= -1 if neg.sum() % 2 else 1
        mats.append(m)
        want.append(w)
    lad, sg = run(gpu, mats)
    print("n = %d %s: negative blocks %d of 3" % (n, kind, want.count(-1)))
    assert list(sg) == want
    if n > 1:
        assert set(want) == {-1, 1}


# ---- 3. ties ----------------------------------------------------------------------------------------------------------
TIE_OFFSETS = (1, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("n", SIZES)
def test_ties_take_the_lowest_row(gpu, n):
    """diag(+-1) times a unit lower triangular matrix whose column k holds +-1 exactly in the rows k + 1, 63, 64, 65, 255,
    256, 257 that exist: every column's largest magnitude, 1, occurs on the diagonal and in rows of the same lane in
    another wave (64), of neighbouring lanes across a wave's edge (63, 65) and of the next turn of the 256-thread search
    (255, 256, 257).  With the lowest row among equals - the diagonal - as the pivot there is no exchange, the pivot
    row is zero to the right, and the sign is prod(+-1) exactly; a search that took a tied row's index from one thread
    and another's value, or lost a candidate between the lanes, the waves or the turns, would exchange rows and, with
    the fill-in that follows, land on another sign in two of the three units (the signs of the tied entries are random).
    The host elimination counts the tied columns of each kind and confirms that every pivot is +-1."""
    rng = np.random.Generator(np.random.Philox(key=3000 + n))
    mats, want, ties = [], [], dict(any=0, lane=0, wave=0, stride=0)
    for odd in (True, False, True):
        m = np.eye(n)
        for k in range(n):
            for off in TIE_OFFSETS:
                if k + off < n:
                    m[k + off, k] = rng.choice([-1.0, 1.0])
        s = rng.choice([-1.0, 1.0], size=n)
        if n > 1:
            s[0] = s[0] if (np.prod(s) < 0) == odd else -s[0]
        m = s[:, None] * m
        hs, t = lu_sign_host(m)
        assert t["unit_pivots"] and hs == int(np.prod(s))
        mats.append(m)
        want.append(int(np.prod(s)))
        for k in ties:
            ties[k] += int(t[k])
    print("n = %d: tied columns %s, negative blocks %d of 3" % (n, ties, want.count(-1)))
    assert ties["any"] == 3 * (n - 1)
    if n > 64:
        assert ties["lane"] >= 3 * (n - 64) and ties["wave"] >= 3 * (n - 64)
    if n > 256:
        assert ties["stride"] >= 3 * (n - 256)
    lad, sg = run(gpu, mats)
    assert list(sg) == want


# ---- 4. grading ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_graded_matrices(gpu, n):
    """diag(r) G diag(c), r and c = +-10^e with e uniform in [-100, 100], G of the Gaussian set: the scaling of A2 =
    U1' Ur + D1 at low temperature.  sign = sign det G prod sign(r) prod sign(c)."""
    rng = np.random.Generator(np.random.Philox(key=4000 + n))
    mats, signs = gaussian_set(n)
    graded, want = [], []
    for m, s in zip(mats, signs):
        r = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-100, 100, size=n)
        c = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-100, 100, size=n)
        graded.append(r[:, None] * m * c[None, :])
        want.append(int(s * np.prod(np.sign(r)) * np.prod(np.sign(c))))
        assert lu_sign_host(graded[-1])[0] == want[-1], "the input is out of a float64 LU's reach"
    lad, sg = run(gpu, graded, padded=True)
    print("n = %d graded: negative blocks %d of 3" % (n, want.count(-1)))
    assert list(sg) == want


# ---- 5. degenerate inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["zero_column", "nan", "inf"])
@pytest.mark.parametrize("n", SIZES)
def test_degenerate_unit_gives_zero_and_leaves_the_others(gpu, n, what):
    rng = np.random.Generator(np.random.Philox(key=5000 + n))
    mats, signs = gaussian_set(n)
    bad = mats[1].copy()
    i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
    if what == "zero_column":
        bad[:, j] = 0.0
    else:
        bad[i, j] = np.nan if what == "nan" else np.inf
    ds = [10.0 ** rng.uniform(-3, 3, size=n) for _ in range(3)]
    lad, sg = run(gpu, [mats[0], bad, mats[2]], ds=ds)
    lad0, sg0 = run(gpu, list(mats), ds=ds)
    assert list(sg) == [signs[0], 0, signs[2]]
    assert np.array_equal(lad, lad0) and sg0[1] == signs[1]


# ---- 6. logabsdet -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_logabsdet_against_fsum(gpu, n):
    rng = np.random.Generator(np.random.Philox(key=6000 + n))
    ds = [10.0 ** rng.uniform(-150, 150, size=n) for _ in range(3)]
    ds[2] = np.sort(ds[2])[::-1]  # the order a UDT with the reference's pivot rule leaves
    lad, sg = run(gpu, [np.eye(n)] * 3, ds=ds, padded=True)
    assert list(sg) == [1, 1, 1]
    for u, d in enumerate(ds):
        logs = [math.log(x) for x in d]
        bound = 2 * n * 2.0 ** -53 * math.fsum(abs(x) for x in logs)
        err = abs(lad[u] - math.fsum(logs))
        print("n = %d unit %d: |device - fsum| = %.3e, bound %.3e" % (n, u, err, bound))
        assert err <= bound


# ---- 7. batch independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_a_unit_does_not_depend_on_its_batch(gpu, n):
    rng = np.random.Generator(np.random.Philox(key=7000 + n))
    mats, signs = gaussian_set(n)
    ds = [10.0 ** rng.uniform(-150, 150, size=n) for _ in range(3)]
    lad, sg = run(gpu, list(mats), ds=ds)
    lad1, sg1 = run(gpu, [mats[1]], ds=[ds[1]])
    assert sg1[0] == sg[1] == signs[1]
    assert lad1[0].tobytes() == lad[1].tobytes()
