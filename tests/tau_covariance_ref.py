"""A numpy restatement of the tau-tau' covariance accumulator (include/dqmc_hip.h "tau-tau' covariance"; csrc/taucov.hip)
in the order of the device - samples in ascending order, one accumulator per element, the shift taken from the first
closed bin - and of the pooling of dqmc.tau_covariance_from_moments, plus what the tests compare them with: the
covariance of the bin means in np.longdouble and the un-shifted textbook formula."""
import numpy as np

EPS = 2.0 ** -52


class Accumulator:
    """push(x [W, S, R]) as the kernel does it.  Beside the state it keeps the sums of the absolute values of the terms
    of S1 and S2 (abs1, abs2: what a forward error bound of the fixed-order sums scales with) and, where push is given
    an absolute uncertainty dx of its input, first-order bounds on what that does to shift, S1 and S2 (e_shift, e1,
    e2)."""

    def __init__(self, W, S, R, bin_size, dtype=np.float64):
        self.W, self.S, self.R, self.bin_size = W, S, R, int(bin_size)
        z = lambda *sh: np.zeros(sh, dtype=dtype)
        self.a, self.c, self.S1, self.S2 = z(W, S, R), z(W, S, R), z(W, S, R), z(W, S, R, R)
        self.abs1, self.abs2 = z(W, S, R), z(W, S, R, R)
        self.ea, self.e_shift, self.e1, self.e2 = z(W, S, R), z(W, S, R), z(W, S, R), z(W, S, R, R)
        self.open, self.nb = 0, 0
        self.dtype = dtype

    def push(self, x, dx=None):
        x = np.asarray(x, dtype=self.dtype).reshape(self.W, self.S, self.R)
        self.a = self.a + x
        if dx is not None:
            self.ea = self.ea + np.asarray(dx, dtype=self.dtype).reshape(x.shape)
        self.open += 1
        if self.open < self.bin_size:
            return
        b = self.a / self.dtype(self.bin_size)
        eb = self.ea / self.bin_size
        if self.nb == 0:
            self.c = b.copy()
            self.e_shift = eb.copy()
        d = b - self.c
        ed = eb + self.e_shift if self.nb else np.zeros_like(eb)  # (the first bin's d is b - b = 0 whatever b is)
        self.S1 = self.S1 + d
        self.S2 = self.S2 + d[..., :, None] * d[..., None, :]
        ad = np.abs(d)
        self.abs1 = self.abs1 + ad
        self.abs2 = self.abs2 + ad[..., :, None] * ad[..., None, :]
        self.e1 = self.e1 + ed
        self.e2 = self.e2 + (ed[..., :, None] * ad[..., None, :] + ad[..., :, None] * ed[..., None, :]
                             + ed[..., :, None] * ed[..., None, :])
        self.a = np.zeros_like(self.a)
        self.ea = np.zeros_like(self.ea)
        self.open = 0
        self.nb += 1

    def moments(self):
        return {"nb": np.full(self.W, self.nb, dtype=np.int64), "shift": self.c.copy(), "S1": self.S1.copy(),
                "S2": self.S2.copy(), "bin_size": self.bin_size}

    def bounds(self):
        """(bound on S1, bound on S2): 4 (n_closed + 2) eps sum |terms|, the forward error of a sum of n_closed terms
        taken in a fixed order (n eps sum |terms| to first order) with room for the bin mean's division and the
        subtraction of the shift in every term and for a fused or an unfused product"""
        f = 4.0 * (self.nb + 2) * EPS
        return f * self.abs1, f * self.abs2


def bin_means(samples, bin_size, dtype=np.float64):
    """samples [T, W, S, R] -> the means of the closed bins [n, W, S, R], the partial bin at the end left out"""
    x = np.asarray(samples, dtype=dtype)
    n = x.shape[0] // bin_size
    return x[:n * bin_size].reshape((n, bin_size) + x.shape[1:]).sum(axis=1) / dtype(bin_size)


def covariance_of_mean(bins, dtype=np.longdouble):
    """bins [n, S, R] (every walker's bins stacked along the first axis) -> (mean [S, R], covariance of the mean
    [S, R, R] = sum (b - mean)(b - mean)^T / (n (n - 1))), two passes in `dtype`"""
    b = np.asarray(bins, dtype=dtype)
    n = b.shape[0]
    mean = b.sum(axis=0) / dtype(n)
    d = b - mean
    return mean, np.einsum("nsi,nsj->sij", d, d) / dtype(n * (n - 1))


def textbook_covariance_of_mean(bins):
    """the un-shifted one-pass formula in float64: (sum b b^T / n - m m^T) / (n - 1)"""
    b = np.asarray(bins, dtype=np.float64)
    n = b.shape[0]
    m = b.sum(axis=0) / n
    S2 = np.zeros(b.shape[1:] + b.shape[-1:])
    for k in range(n):
        S2 = S2 + b[k][:, :, None] * b[k][:, None, :]
    return (S2 / n - m[:, :, None] * m[:, None, :]) / (n - 1)


def near_one_samples(T, W, S, R, seed=5):
    """series with mean 1 and fluctuations of 1e-8, correlated along tau"""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((T, W, S, R))
    z = z + 0.5 * np.roll(z, 1, axis=3)
    return 1.0 + 1e-8 * z


def near_one_tolerance(samples, bin_size):
    """What float64 can give for the covariance of the mean of near_one_samples, element by element [S, R, R].  A bin
    mean b = (x_1 + .. + x_k) / k carries an absolute rounding error of at most eta = (k + 1) eps max|x|, and so does
    the shift; with d the bins' deviations from the first bin (all walkers' bins as one sample of n), a perturbation of
    every d by 2 eta moves sum d_i d_j by at most 2 eta (sum |d_i| + sum |d_j|), and the sums themselves round by
    4 (n + 2) eps sum |d_i d_j| (Accumulator.bounds).  The pooling across walkers adds the difference of two walkers'
    means, known to eta as well: the same term once more.  Divided by n (n - 1)."""
    b = bin_means(samples, bin_size, np.longdouble)           # [n, W, S, R]
    d = np.abs(b - b[:1]).reshape((-1,) + b.shape[2:]).astype(np.float64)
    n = d.shape[0]
    eta = (bin_size + 1) * EPS * float(np.abs(samples).max())
    s1 = d.sum(axis=0)
    s2 = np.einsum("nsi,nsj->sij", d, d)
    return (4.0 * eta * (s1[:, :, None] + s1[:, None, :]) + 4.0 * (n + 2) * EPS * s2) / (n * (n - 1.0))
