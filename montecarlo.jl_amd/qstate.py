"""q-state models for the classical MC flavor: Potts and clock (include/dqmc_hip.h, "the classical MC flavor with q-state
models"; csrc/qstate.hip).  The reference's MC flavor is a plugin surface (energy, propose_local, accept_local!) whose one
model is the IsingModel; these models, their checkerboard update and their two-component order parameter are a defined
extension.  The host holds the model, the fixed-point tables, the colouring and the loop control; every site update and
every measurement runs on the device, one workgroup per walker.

Walker w draws from the Philox4x32-10 streams keyed by `seed + first_walker + w`, as the Ising walkers do, on domains of
its own."""
import ctypes as C
import math

import numpy as np

from . import checkpoint as _ckpt
from ._lib import (DQMCError, ERR_INVALID, ERR_STATE, QsBinned, QsClusterStats, QsExchangeStats, QsParams, QsScaling,
                   QsScalingBinned, QsStats, QsStiffness, QsStiffnessBinned, lib)
from .lattices import bond_classes
from .mc import _MCBase, _choose_lattice, _delta_var, _llround, _xi, pool_walkers, q30_tables, reciprocal_vectors

Q_MAX = 64
Q30 = 2.0 ** 30


def qstate_tables(q, pair_energy, J=1.0):
    """(e_q30 int64 [q], c_q30 int32 [q], s_q30 int32 [q]): llround(J e[d] 2^30), symmetric by construction (d <= q / 2
    computed, the rest mirrored), and llround(cos(2 pi s / q) 2^30) with the sine likewise"""
    e = np.asarray(pair_energy, dtype=np.float64)
    e_q30 = np.zeros(q, dtype=np.int64)
    for d in range(q // 2 + 1):
        e_q30[d] = e_q30[(q - d) % q] = _llround(J * e[d] * Q30)
    ang = 2.0 * np.pi * np.arange(q) / q
    return (e_q30, np.ascontiguousarray(_llround(np.cos(ang) * Q30).astype(np.int32)),
            np.ascontiguousarray(_llround(np.sin(ang) * Q30).astype(np.int32)))


def twist_tables(q, d1, d2, J=1.0):
    """(d1_q30, d2_q30) int64 [q]: llround(J d[k] 2^30) for k <= q / 2, the rest mirrored: d1 exactly antisymmetric
    (d1_q30[0] = 0, and d1_q30[q / 2] = 0 for even q), d2 exactly symmetric"""
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    a, b = np.zeros(q, dtype=np.int64), np.zeros(q, dtype=np.int64)
    for k in range(q // 2 + 1):
        v = int(_llround(J * d1[k] * Q30))
        a[k] = v
        a[(q - k) % q] = -v if (q - k) % q != k else 0
        b[k] = b[(q - k) % q] = _llround(J * d2[k] * Q30)
    return a, b


class QStateModel:
    """QStateModel(q, pair_energy; dims, L | l, J, twist): s_i in {0 .. q - 1}, 2 <= q <= 64, and
    E = -J sum_bonds e[(s_i - s_j) mod q] over the lattice's undirected bonds table, with the length-q table
    e = pair_energy, e[d] == e[(q - d) % q].  Any project lattice may be given as `l`.  `twist=(d1, d2)`: the first and
    second derivative of the pair energy with respect to the angle 2 pi d / q as length-q tables, d1[d] == -d1[(q - d) % q]
    and d2[d] == d2[(q - d) % q], |J d| <= 4: what the helicity modulus needs (MC(..., stiffness=True)); None for a
    model whose pair energy is no function of an angle."""
    is_qstate = True

    def __init__(self, q, pair_energy, dims=None, L=None, l=None, J=1.0, twist=None):
        if int(q) != q or not 2 <= q <= Q_MAX:
            raise ValueError("QStateModel: q must be an integer in 2..%d, got %r" % (Q_MAX, q))
        q = int(q)
        e = np.array(pair_energy, dtype=np.float64).reshape(-1)
        if e.size != q or not np.all(np.isfinite(e)):
            raise ValueError("QStateModel: pair_energy must hold q = %d finite values" % q)
        for d in range(q):
            if e[d] != e[(q - d) % q]:
                raise ValueError("QStateModel: pair_energy[%d] != pair_energy[%d]: the table must be symmetric, "
                                 "e[d] == e[(q - d) %% q]" % (d, (q - d) % q))
        if not math.isfinite(J) or np.max(np.abs(J * e)) > 4.0:
            raise ValueError("QStateModel: |J e[d]| must be finite and at most 4")
        if l is None:
            if dims is None or L is None:
                raise ValueError("QStateModel needs dims and L, or a lattice l")
            l = _choose_lattice(dims, L)
        self.q, self.pair_energy, self.J = q, e, float(J)
        self.l = l
        self.L = L if L is not None else getattr(l, "L", len(l))
        self.dims = dims if dims is not None else getattr(l, "dim", 2 if hasattr(l, "lattice") else 1)
        self.e_q30, self.c_q30, self.s_q30 = qstate_tables(q, e, self.J)
        self.twist, self.twist_q30 = None, None
        if twist is not None:
            try:
                d1, d2 = (np.array(t, dtype=np.float64).reshape(-1) for t in twist)
            except (TypeError, ValueError):
                raise ValueError("QStateModel: twist must be a pair (d1, d2) of length-q tables")
            if d1.size != q or d2.size != q or not (np.all(np.isfinite(d1)) and np.all(np.isfinite(d2))):
                raise ValueError("QStateModel: twist=(d1, d2) must hold q = %d finite values each" % q)
            for d in range(q):
                if d1[d] != -d1[(q - d) % q]:
                    raise ValueError("QStateModel: twist d1[%d] != -d1[%d]: the first derivative must be antisymmetric, "
                                     "d1[d] == -d1[(q - d) %% q]" % (d, (q - d) % q))
                if d2[d] != d2[(q - d) % q]:
                    raise ValueError("QStateModel: twist d2[%d] != d2[%d]: the second derivative must be symmetric, "
                                     "d2[d] == d2[(q - d) %% q]" % (d, (q - d) % q))
            if max(np.max(np.abs(J * d1)), np.max(np.abs(J * d2))) > 4.0:
                raise ValueError("QStateModel: |J d1[d]| and |J d2[d]| of twist must be at most 4")
            self.twist = (d1 + 0.0, d2)  # (+ 0.0: no -0.0 entries)
            self.twist_q30 = twist_tables(q, d1, d2, self.J)

    def __len__(self):
        return len(self.l)

    def _conf(self, conf):
        c = np.asarray(conf).reshape(-1, order="F").astype(np.int64)
        if c.size != len(self.l) or np.any(c < 0) or np.any(c >= self.q):
            raise ValueError("conf must hold %d states in 0..%d" % (len(self.l), self.q - 1))
        return c

    def energy_q30(self, conf):
        """E_int = -sum_bonds e_q30[(s_i - s_j) mod q]: the device's exact integer energy"""
        c = self._conf(conf)
        b = np.asarray(self.l.bonds, dtype=np.int64)[:, :2] - 1
        return -int(np.sum(self.e_q30[(c[b[:, 0]] - c[b[:, 1]]) % self.q]))

    def energy(self, conf):
        """energy(mc, m, conf): -J sum over the undirected bonds table of e[(s_i - s_j) mod q]"""
        c = self._conf(conf)
        b = np.asarray(self.l.bonds, dtype=np.int64)[:, :2] - 1
        return float(-self.J * np.sum(self.pair_energy[(c[b[:, 0]] - c[b[:, 1]]) % self.q]))

    def propose_local(self, i, t, conf):
        """propose_local(mc, m, i, conf) for the proposal s_i -> t: delta_E = J sum_{j in neighs[:, i]} (e[(s_i - s_j) mod q]
        - e[(t - s_j) mod q]), a repeated neighbour counted twice; i 1-based"""
        c = self._conf(conf)
        sj = c[np.asarray(self.l.neighs, dtype=np.int64)[:, i - 1] - 1]
        e = self.pair_energy
        return float(self.J * np.sum(e[(c[i - 1] - sj) % self.q] - e[(int(t) - sj) % self.q]))

    def order_parameter_q30(self, conf):
        """(Mx, My) = sum_i (c_q30[s_i], s_q30[s_i]) as exact integers"""
        c = self._conf(conf)
        return int(self.c_q30[c].astype(np.int64).sum()), int(self.s_q30[c].astype(np.int64).sum())


class PottsModel(QStateModel):
    """PottsModel(q; dims, L | l, J): e[d] = delta_{d,0}, E = -J sum_bonds delta(s_i, s_j)"""

    def __init__(self, q, dims=None, L=None, l=None, J=1.0):
        e = np.zeros(max(int(q), 1) if int(q) == q else 1)
        e[0] = 1.0
        super().__init__(q, e, dims=dims, L=L, l=l, J=J)


class ClockModel(QStateModel):
    """ClockModel(q; dims, L | l, J): e[d] = cos(2 pi d / q), E = -J sum_bonds cos(theta_i - theta_j) with
    theta = 2 pi s / q (d <= q / 2 computed, the rest mirrored: exactly symmetric).  Its twist tables are
    d1[d] = sin(2 pi d / q), mirrored with the opposite sign (0 at d = 0 and d = q / 2), and d2 = e."""

    def __init__(self, q, dims=None, L=None, l=None, J=1.0):
        n = max(int(q), 1) if int(q) == q else 1
        e, d1 = np.zeros(n), np.zeros(n)
        for d in range(n // 2 + 1):
            e[d] = e[(n - d) % n] = math.cos(2.0 * math.pi * d / n)
            if (n - d) % n != d:
                d1[d] = math.sin(2.0 * math.pi * d / n)
                d1[(n - d) % n] = -d1[d]
        super().__init__(q, e, dims=dims, L=L, l=l, J=J, twist=(d1, e))


_ISING_ONLY = "MC with a q-state model: %s is implemented for the IsingModel only (the q-state engine has local " \
              "checkerboard sweeps and keywords of its own: cluster_rate=k for its reflection cluster moves, " \
              "tempering=(R, k) for replica exchange, binner=True | capacity for the device binner, " \
              "scaling=True | [k vectors] for S(k) and xi and stiffness=True | [unit vectors] for the helicity " \
              "modulus; the sequential sweep is out of scope)"


class QStateMC(_MCBase):
    """What MC(model; beta | T, ...) returns for a q-state model: `n_walkers` chains, one workgroup each, swept colour
    class by colour class (`colouring=None`: greedy_colouring(lattice)) under the rule of include/dqmc_hip.h.  `beta`
    may be a sequence of n_walkers values.  `cluster_rate=k > 0` runs one reflection cluster move per walker behind every
    sweep whose index is a multiple of k, before its measurement (the header's "Cluster move": the Wolff move for Potts
    models, Wolff's reflection along the q lattice axes for clock models); 0, the default, runs none.

    The domain of beta: a site's acceptance is a product of z table entries exp(-beta (e[a] - e[b])), each partial
    product the exponential of at most z exponents within beta * range of zero, range = max(J e) - min(J e) of the
    fixed-point table.  With beta * z * range <= 700 every partial product stays in [e^-700, e^700], finite and
    non-zero; beyond it one could become inf or 0 and decide an uphill move wrongly, so MC(...) and set_beta raise
    DQMCError (ERR_INVALID) there and leave the walker as it was.

    `tempering=(R, k)` makes every R consecutive walkers a ladder for replica exchange (the header's "Replica exchange";
    n_walkers a multiple of R) and runs one round behind every k-th sweep: after its cluster move, before its
    measurement.  A `beta` or `T` sequence of R values is tiled over the ladders.  Walker w stays at beta_w with its
    streams, sums, series and binner; an accepted exchange swaps the configurations (states, E_int, Mx, My and the
    replica label) of two neighbouring walkers, so measurements(w), series(w), binned(w) and exchange_stats(w) remain
    "at beta_w".  `binner=True | capacity` gives every walker a logarithmic binner over [E, E2, |M|, M2, M2, M4], pushed
    on the device where the measurement is taken (enable_binning); binned() answers mean, std_error and tau.

    `scaling=True` (or a list of at most 8 wave vectors; True: reciprocal_vectors(lattice)) also measures the structure
    factor S(k) of the two-component order parameter wherever E and M are measured (the header's "Scaling", set_scaling):
    `scaling()` gives S and the second-moment correlation length xi_k = sqrt(S(0)/S(k) - 1) / (2 sin(|k|/2)) with
    S(0) = <M2>/N, whose xi/L crossings locate the transitions, and with a binner `binned_scaling()` gives their error
    bars.  The chains, the sums and binned() are those of a handle without it.

    `stiffness=True` (or a list of at most 4 unit vectors; True: the lattice's cartesian axes) also measures the helicity
    modulus Upsilon_mu = (<T_mu> - beta <J_mu^2>) / N along each direction wherever E and M are measured (the header's
    "Stiffness", set_stiffness), for a model with twist tables (ClockModel, or QStateModel(..., twist=(d1, d2))):
    `stiffness()` gives the plain means, and with a binner `binned_stiffness()` gives the error bars.  The chains, the
    sums and the other binner sections are those of a handle without it.

    The Ising-only options (cluster_moves, global_moves, n_replicas, exchange_rate, fss, binning, update="sequential")
    raise NotImplementedError."""
    _abi = "dqmc_qs_"
    _flavor = "mc_qstate"
    _ExchangeStats = QsExchangeStats

    def __init__(self, model, beta=None, T=None, n_walkers=1, seed=123, first_walker=0, thermalization=0, sweeps=1000,
                 measure_rate=1, print_rate=1000, global_moves=False, global_rate=5, device_id=0, series_capacity=0,
                 cluster_moves=False, binning=False, binning_capacity=None, n_replicas=0, exchange_rate=0,
                 fss=False, update=None, colouring=None, cluster_rate=0, tempering=None, binner=False, scaling=False,
                 stiffness=False):
        for name, on in (("global_moves", global_moves), ("cluster_moves", cluster_moves), ("binning", binning),
                         ("n_replicas", n_replicas), ("exchange_rate", exchange_rate),
                         ("fss", fss is not False and fss is not None),
                         ('update="%s"' % update, update not in (None, "checkerboard"))):
            if on:
                raise NotImplementedError(_ISING_ONLY % name)
        beta = self._resolve_beta(beta, T)
        R, k = self._tempering(tempering, n_walkers)
        capacity = self._binner_capacity(binner)
        tables = self._scaling_tables(model.l, scaling)  # (refused before the device is touched)
        twist = self._stiffness_tables(model, stiffness)  # (likewise)
        if R >= 2 and beta.ndim == 1 and len(beta) == R:
            beta = np.tile(beta, n_walkers // R)  # one ladder's temperatures, the same in every ladder
        self._init_common(model, beta, n_walkers, seed, first_walker, thermalization, sweeps, measure_rate, print_rate,
                          series_capacity)
        cluster_rate = self._cluster_rate(cluster_rate)
        self.q = model.q
        self.update = "checkerboard"
        col, n_col = self._colouring(colouring)
        self._tables = [np.ascontiguousarray(model.e_q30, dtype=np.int64), np.ascontiguousarray(model.c_q30, dtype=np.int32),
                        np.ascontiguousarray(model.s_q30, dtype=np.int32)]
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._create(QsParams(n_sites=self.N, z=self._neighs.shape[0], q=self.q, n_walkers=n_walkers, device_id=device_id,
                              n_bonds=self._bonds.shape[0], series_capacity=series_capacity, n_colours=n_col,
                              neighs=self._neighs.ctypes.data_as(i64), bonds=self._bonds.ctypes.data_as(i64),
                              e_q30=self._tables[0].ctypes.data_as(i64), c_q30=self._tables[1].ctypes.data_as(i32),
                              s_q30=self._tables[2].ctypes.data_as(i32), colour=col.ctypes.data_as(i32)))
        self.colouring = col
        self.cluster_rate = 0
        if cluster_rate:
            self.set_cluster_rate(cluster_rate)
        self.n_replicas, self.exchange_rate = 0, 0
        if R or k:
            self.set_exchange(R, k)
        self.k_vectors = None
        if tables is not None:
            self._put_scaling(tables)
        self.stiffness_directions, self.bond_vectors = None, None
        if twist is not None:
            self._put_stiffness(twist)
        if capacity is not False:
            self.enable_binning(capacity)

    @staticmethod
    def _tempering(tempering, n_walkers):
        """(R, k) of tempering=(R, k); None: (0, 0)"""
        if tempering is None:
            return 0, 0
        try:
            R, k = tempering
        except (TypeError, ValueError):
            raise ValueError("tempering must be a pair (n_replicas, rate), got %r" % (tempering,))
        for v in (R, k):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("tempering=(n_replicas, rate): integers >= 0, got %r" % (tempering,))
        if R >= 2 and n_walkers % R != 0:
            raise ValueError("tempering: n_walkers = %d is not a multiple of n_replicas = %d" % (n_walkers, R))
        return int(R), int(k)

    @staticmethod
    def _binner_capacity(binner):
        """False: no binner; None: the default capacity; else the capacity"""
        if binner is False or binner is None:
            return False
        if binner is True:
            return None
        if not isinstance(binner, (int, np.integer)) or binner < 1:
            raise ValueError("binner must be True, False or a capacity >= 1, got %r" % (binner,))
        return int(binner)

    @staticmethod
    def _cluster_rate(k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError("cluster_rate must be an integer >= 0, got %r" % (k,))
        return int(k)

    def _colouring(self, colouring):
        return self._colours(colouring, "colouring")

    # ---- state
    def conf(self, walker=0):
        out = np.zeros(self.N, dtype=np.uint8)
        self._c(lib().dqmc_qs_get_conf(self._h, walker, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def set_conf(self, walker, conf):
        c = np.asarray(conf).reshape(-1, order="F")
        if c.size != self.N:
            raise DQMCError(ERR_INVALID, "set_conf: expected %d states" % self.N)
        if np.any(c < 0) or np.any(c >= self.q):
            raise DQMCError(ERR_INVALID, "set_conf: the states must lie in 0..%d" % (self.q - 1))
        c = np.ascontiguousarray(c, dtype=np.uint8)
        self._c(lib().dqmc_qs_set_conf(self._h, walker, c.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_colouring(self, colouring=None):
        """dqmc_qs_set_colouring: another colouring from now on (None: greedy_colouring(lattice)); a colouring that is
        refused leaves the handle as it was"""
        col, n_col = self._colouring(colouring)
        self._c(lib().dqmc_qs_set_colouring(self._h, col.ctypes.data_as(C.POINTER(C.c_int32)), n_col))
        self.colouring = col

    def set_cluster_rate(self, k):
        """dqmc_qs_set_cluster_rate: from now on one cluster move per walker behind every sweep whose index is a multiple
        of k, before its measurement; 0 = none"""
        k = self._cluster_rate(k)
        self._c(lib().dqmc_qs_set_cluster_rate(self._h, k))
        self.cluster_rate = k

    def cluster_move(self, walker=-1):
        """one cluster move of the walker by hand, or of every walker (-1); no measurement is taken"""
        self._c(lib().dqmc_qs_cluster_move(self._h, walker))

    def cluster_stats(self, walker=0):
        """prop_global, acc_global (moves with |C| > 1), sum_cluster_size and moves_drawn (the move cursor)"""
        st = QsClusterStats()
        self._c(lib().dqmc_qs_get_cluster_stats(self._h, walker, C.byref(st)))
        return st

    # ---- replica exchange: set_exchange, exchange, exchange_stats, replicas (_MCBase)
    # ---- error bars (enable_binning, binner_size, binner_reliable_level: _MCBase)
    def binner_level(self, walker, level):
        """(x_sum[6], x2_sum[6], xy_sum[3], count) of one level of one walker: elements [E, E2, |M|, M2, M2, M4], pairs
        (E, E2), (|M|, M2) and (M2, M4)"""
        return self._section_level("", 6, 3, walker, level)

    def binner_finish(self, walker=0, level=None):
        """dqmc_qs_binned of one walker at `level` (None: the reliable level)"""
        return self._section_finish("", QsBinned, walker, level)

    def _binned_walker(self, walker, level):
        """per observable (mean, variance of the mean at `level`, the same at level 0 or None) of one walker"""
        b = self.binner_finish(walker, level)
        beta, invN = float(self.betas[walker]), 1.0 / self.N
        E, E2, M, M2, M2b, M4 = b.mean
        v, v0 = b.varN, b.varN0

        def fluct(scale, x, x2, vx, vx2, cov):  # scale (<x2> - <x>^2): gradient (-2 x, 1) with respect to (x, x2)
            return scale * (x2 - x * x), scale * scale * _delta_var((-2.0 * x, 1.0), vx, vx2, cov), None

        with np.errstate(invalid="ignore", divide="ignore"):
            m2, m4 = np.float64(M2b), np.float64(M4)
            U4 = float(1.0 - m4 / (2.0 * m2 * m2))
            gU = (float(m4 / (m2 * m2 * m2)), float(-1.0 / (2.0 * m2 * m2)))
        obs = {"E": (E, v[0], v0[0]), "E2": (E2, v[1], v0[1]), "e": (E * invN, v[0] * invN * invN, v0[0] * invN * invN),
               "C": fluct(beta * beta * invN, E, E2, v[0], v[1], b.covN[0]),
               "M": (M, v[2], v0[2]), "M2": (M2, v[3], v0[3]), "M4": (M4, v[5], v0[5]),
               "m": (M * invN, v[2] * invN * invN, v0[2] * invN * invN),
               "chi": fluct(beta * invN, M, M2, v[2], v[3], b.covN[1]),
               "U4": (U4, _delta_var(gU, v[4], v[5], b.covN[2]), None)}
        return obs, int(b.count), int(b.level)

    def binned(self, walker=0, level=None, walkers=None):
        """mean, std_error and tau from the device binner at `level` (None: the reliable one): {"Energy": {E, E2, e, C},
        "Magn": {M, M2, M4, m, chi, U4}, "count", "level"}, each observable {mean, std_error, tau}.  C, chi and
        U4 = 1 - <M4> / (2 <M2>^2) get their error by the delta method on the binned covariances of (E, E2), (|M|, M2)
        and (M2, M4); their tau is NaN (they are no time series).  `walkers=[...]` pools chains of equal beta as
        MC.binned does: mean = sum_w mean_w / W, std_error = sqrt(sum_w var_w) / W (C, chi and U4 formed per walker
        first), tau from the summed variances, plus std_error_walkers = sqrt(sum_w (mean_w - mean)^2 / (W (W - 1))).
        Under replica exchange the values are those of the slot: "at beta_w"."""
        p = pool_walkers("binned", self.betas, walker, walkers, lambda w: self._binned_walker(w, level),
                         derived_tau=float("nan"))
        out = {"Energy": {k: p.pop(k) for k in ("E", "E2", "e", "C")},
               "Magn": {k: p.pop(k) for k in ("M", "M2", "M4", "m", "chi", "U4")}}
        out.update(p)
        return out

    # ---- finite-size scaling
    def set_scaling(self, k_vectors=True):
        """dqmc_qs_set_scaling: from now on every measurement also takes S(k) at the given wave vectors (True:
        reciprocal_vectors(lattice), the smallest ones, one per lattice dimension; else 1 to 8 vectors of the lattice's
        dimension; None or False: off).  Resets the scaling sums and, if a binner is on, restarts it with every section
        empty and its capacity kept."""
        self._put_scaling(self._scaling_tables(self.model.l, k_vectors))

    @staticmethod
    def _scaling_tables(l, k_vectors):
        """(cos_q30, sin_q30, k) of a scaling argument, None for None or False; ValueError unless 1 to 8 vectors"""
        if k_vectors is None or k_vectors is False:
            return None
        ks = reciprocal_vectors(l) if k_vectors is True else k_vectors
        if not 1 <= len(ks) <= 8:
            raise ValueError("scaling: 1 to 8 wave vectors, got %d" % len(ks))
        return q30_tables(l, ks)

    def _put_scaling(self, tables):
        if tables is None:
            self._c(lib().dqmc_qs_set_scaling(self._h, 0, None, None))
            self.k_vectors = None
            return
        cq, sq, k = tables
        i32 = C.POINTER(C.c_int32)
        self._c(lib().dqmc_qs_set_scaling(self._h, len(k), cq.ctypes.data_as(i32), sq.ctypes.data_as(i32)))
        self.k_vectors = k

    def scaling_sums(self, walker=0):
        """dqmc_qs_scaling of one walker: n_meas, n_k (0: off), sum_S[8]"""
        out = QsScaling()
        self._c(lib().dqmc_qs_get_scaling(self._h, walker, C.byref(out)))
        return out

    def _knorm(self, k):
        return float(np.linalg.norm(self.k_vectors[k]))

    def scaling(self, walker=0):
        """the plain means of one walker: S (one per wave vector), M2, k and the second-moment correlation length
        xi_k = sqrt(S(0)/S_k - 1) / (2 sin(|k|/2)) with S(0) = <M2>/N (NaN where S(0) < S_k), xi_over_L where the lattice
        has an L.  <M2> is the one of measurements(): the two counts must agree (after switching the measurement on
        mid-run, reset_accumulators() first)."""
        f, st = self.scaling_sums(walker), self.stats(walker)
        if f.n_k < 1:
            raise DQMCError(ERR_STATE, "scaling: the measurement is off (MC(scaling=True) or set_scaling)")
        if f.n_meas == 0:
            raise DQMCError(ERR_INVALID, "scaling: no measurement has been taken")
        if f.n_meas != st.n_meas:
            raise DQMCError(ERR_STATE, "scaling: %d scaling measurements but %d of M2 (the measurement was switched on "
                                       "mid-run: reset_accumulators() first)" % (f.n_meas, st.n_meas))
        n = float(f.n_meas)
        M2 = st.sum_M2 / n
        S = np.array([f.sum_S[k] / n for k in range(f.n_k)])
        xi = np.array([_xi(M2, S[k], self.N, self._knorm(k))[0] for k in range(f.n_k)])
        out = {"S": S, "xi": xi, "M2": M2, "k": self.k_vectors.copy(), "n_meas": int(f.n_meas)}
        L = getattr(self.model.l, "L", None)
        if L is not None:
            out["xi_over_L"] = xi / float(L)
        return out

    def scaling_binner_level(self, walker, level):
        """(x_sum[1 + n_k], x2_sum[1 + n_k], xy_sum[n_k], count) of one level of one walker of the binner's scaling
        section: elements [M2, S_0 ..], pairs (M2, S_0) .."""
        nk = 0 if self.k_vectors is None else len(self.k_vectors)
        return self._section_level("scaling_", 1 + nk, nk, walker, level)

    def scaling_binner_finish(self, walker=0, level=None):
        """dqmc_qs_scaling_binned of one walker at `level` (None: the reliable level)"""
        return self._section_finish("scaling_", QsScalingBinned, walker, level)

    def _binned_scaling_walker(self, walker, level):
        """{name: (mean, variance of the mean at `level`, the same at level 0 or None)} of one walker; S, xi as lists"""
        b = self.scaling_binner_finish(walker, level)
        M2 = b.mean[0]
        obs = {"M2": (M2, b.varN[0], b.varN0[0]), "S": [], "xi": []}
        for k in range(b.n_k):
            S = b.mean[1 + k]
            xi, g = _xi(M2, S, self.N, self._knorm(k))
            obs["S"].append((S, b.varN[1 + k], b.varN0[1 + k]))
            obs["xi"].append((xi, _delta_var(g, b.varN[0], b.varN[1 + k], b.covN[k]), None))
        return obs, int(b.count), int(b.level)

    def binned_scaling(self, walker=0, level=None, walkers=None):
        """mean, std_error and tau of M2 and each S_k from the binner's scaling section at `level` (None: the reliable
        one), and mean and std_error of each xi_k (xi_over_L where the lattice has an L) by the delta method on the binned
        covariance of (M2, S_k): {"M2": {...}, "S", "xi": [{...} per k], "count", "level"}.  `walkers=[...]` pools chains
        of equal beta under the rules of binned(): xi is formed per walker first, std_error = sqrt(sum_w var_w) / W,
        plus std_error_walkers."""
        out = pool_walkers("binned_scaling", self.betas, walker, walkers, lambda w: self._binned_scaling_walker(w, level))
        L = getattr(self.model.l, "L", None)
        if L is not None:
            out["xi_over_L"] = [{key: v / float(L) for key, v in o.items()} for o in out["xi"]]
        return out

    # ---- helicity modulus
    def set_stiffness(self, directions=True):
        """dqmc_qs_set_stiffness: from now on every measurement also takes T_mu and J_mu of the helicity modulus along the
        given unit vectors (True: the lattice's cartesian axes, lattices.bond_classes; else 1 to 4 vectors of the
        lattice's dimension; None or False: off).  Resets the stiffness sums and, if a binner is on, restarts it with
        every section empty and its capacity kept.  ValueError for a model without twist tables."""
        self._put_stiffness(self._stiffness_tables(self.model, directions))

    @staticmethod
    def _stiffness_tables(model, directions):
        """(slot_class, class vectors, x, directions, d1_q30, d2_q30) of a stiffness argument, None for None or False"""
        if directions is None or directions is False:
            return None
        if getattr(model, "twist_q30", None) is None:
            raise ValueError("stiffness: the model has no twist tables: its pair energy is no function of an angle "
                             "(PottsModel); give QStateModel(..., twist=(d1, d2)) the derivatives of the pair energy")
        slot_class, vectors, x = bond_classes(model.l, directions)
        dirs = np.eye(vectors.shape[1])[:x.shape[0]] if directions is True else np.array(directions, dtype=np.float64)
        d1, d2 = model.twist_q30
        return (np.asfortranarray(slot_class, dtype=np.int8), vectors, np.ascontiguousarray(x, dtype=np.float64), dirs,
                np.ascontiguousarray(d1, dtype=np.int64), np.ascontiguousarray(d2, dtype=np.int64))

    def _put_stiffness(self, tables):
        if tables is None:
            self._c(lib().dqmc_qs_set_stiffness(self._h, 0, 0, None, None, None, None))
            self.stiffness_directions, self.bond_vectors = None, None
            return
        slot_class, vectors, x, dirs, d1, d2 = tables
        i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        self._c(lib().dqmc_qs_set_stiffness(self._h, x.shape[0], x.shape[1], slot_class.ctypes.data_as(C.POINTER(C.c_int8)),
                                            d1.ctypes.data_as(i64), d2.ctypes.data_as(i64), x.ctypes.data_as(dp)))
        self.stiffness_directions, self.bond_vectors = dirs, vectors

    def _n_dir(self):
        return 0 if self.stiffness_directions is None else len(self.stiffness_directions)

    def stiffness_sums(self, walker=0):
        """dqmc_qs_stiffness of one walker: n_meas, n_dir (0: off), sum_T[4], sum_J[4], sum_J2[4]"""
        out = QsStiffness()
        self._c(lib().dqmc_qs_get_stiffness(self._h, walker, C.byref(out)))
        return out

    def stiffness_sample(self, walker=0):
        """(I[n_c], K[n_c]) of the walker's last measurement: the exact int64 class sums of d1_q30 and d2_q30"""
        I, K = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        p = C.POINTER(C.c_int64)
        self._c(lib().dqmc_qs_get_stiffness_sample(self._h, walker, I.ctypes.data_as(p), K.ctypes.data_as(p)))
        n_c = 0 if self.bond_vectors is None else len(self.bond_vectors)
        return I[:n_c].copy(), K[:n_c].copy()

    def stiffness(self, walker=0):
        """the plain means of one walker: Upsilon_mu = (<T_mu> - beta <J_mu^2>) / N per direction, with T, J, J2 (the
        means of T_mu, J_mu and J_mu^2), the directions and n_meas"""
        f = self.stiffness_sums(walker)
        if f.n_dir < 1:
            raise DQMCError(ERR_STATE, "stiffness: the measurement is off (MC(stiffness=True) or set_stiffness)")
        if f.n_meas == 0:
            raise DQMCError(ERR_INVALID, "stiffness: no measurement has been taken")
        n, beta = float(f.n_meas), float(self.betas[walker])
        T, J, J2 = (np.array(s[:f.n_dir]) / n for s in (f.sum_T, f.sum_J, f.sum_J2))
        return {"Upsilon": (T - beta * J2) / self.N, "T": T, "J": J, "J2": J2,
                "directions": self.stiffness_directions.copy(), "n_meas": int(f.n_meas)}

    def stiffness_binner_level(self, walker, level):
        """(x_sum[2 n_dir], x2_sum[2 n_dir], xy_sum[n_dir], count) of one level of one walker of the binner's stiffness
        section: elements [T_0, J2_0, T_1, J2_1 ..], pairs (T_mu, J2_mu)"""
        nd = self._n_dir()
        return self._section_level("stiffness_", 2 * nd, nd, walker, level)

    def stiffness_binner_finish(self, walker=0, level=None):
        """dqmc_qs_stiffness_binned of one walker at `level` (None: the reliable level)"""
        return self._section_finish("stiffness_", QsStiffnessBinned, walker, level)

    def _binned_stiffness_walker(self, walker, level):
        """{name: [(mean, variance of the mean at `level`, the same at level 0 or None) per direction]} of one walker"""
        b = self.stiffness_binner_finish(walker, level)
        beta, invN = float(self.betas[walker]), 1.0 / self.N
        obs = {"T": [], "J2": [], "Upsilon": []}
        for m in range(b.n_dir):
            T, J2 = b.mean[2 * m], b.mean[2 * m + 1]
            obs["T"].append((T, b.varN[2 * m], b.varN0[2 * m]))
            obs["J2"].append((J2, b.varN[2 * m + 1], b.varN0[2 * m + 1]))
            obs["Upsilon"].append(((T - beta * J2) * invN,
                                   _delta_var((invN, -beta * invN), b.varN[2 * m], b.varN[2 * m + 1], b.covN[m]), None))
        return obs, int(b.count), int(b.level)

    def binned_stiffness(self, walker=0, level=None, walkers=None):
        """mean, std_error and tau of T_mu and J2_mu from the binner's stiffness section at `level` (None: the reliable
        one), and mean and std_error of Upsilon_mu = (<T_mu> - beta <J2_mu>) / N by the delta method with the gradient
        (1 / N, -beta / N) on the binned covariance of (T_mu, J2_mu): {"T", "J2", "Upsilon": [{...} per direction],
        "count", "level"}.  `walkers=[...]` pools chains of equal beta under the rules of binned_scaling(): Upsilon is
        formed per walker first, std_error = sqrt(sum_w var_w) / W, plus std_error_walkers."""
        return pool_walkers("binned_stiffness", self.betas, walker, walkers,
                            lambda w: self._binned_stiffness_walker(w, level))

    def stats(self, walker=0):
        st = QsStats()
        self._c(lib().dqmc_qs_get_stats(self._h, walker, C.byref(st)))
        return st

    def energy(self, walker=0):
        """the walker's energy, tracked on the device as an exact integer in units of 2^-30"""
        return self.stats(walker).energy_q30 / Q30

    def order_parameter(self, walker=0):
        """(Mx, My) = sum_i (cos, sin)(2 pi s_i / q) from the device's exact integers"""
        st = self.stats(walker)
        return st.mx_q30 / Q30, st.my_q30 / Q30

    # ---- the loop
    def run(self, verbose=False, sweeps=None, thermalization=None, checkpoint=None, checkpoint_every=None):
        """run!(mc) for every walker, resuming after last_sweep.  `checkpoint=path` saves the run (save()) after every
        sweep whose index is a multiple of `checkpoint_every` and after the last one; the sweep calls are cut there, which
        changes no bit of the results."""
        return self._run(verbose, None, sweeps, thermalization, checkpoint, checkpoint_every)

    # ---- checkpoint and resume (state, set_state, save, load: _MCBase)
    @staticmethod
    def _model_entry(m):
        """the "model" entry of a checkpoint preamble.  JSON floats give back the same doubles, so pair_energy, J and
        twist construct the same fixed-point tables again."""
        if not isinstance(m, QStateModel):
            raise ValueError("save(): %s is not a model a checkpoint can name" % type(m).__name__)
        name = type(m).__name__ if type(m) in (PottsModel, ClockModel) else "QStateModel"
        return {"class": name, "q": int(m.q), "J": float(m.J), "pair_energy": [float(x) for x in m.pair_energy],
                "twist": None if m.twist is None else [[float(x) for x in t] for t in m.twist],
                "dims": int(m.dims), "L": int(m.L)}

    @staticmethod
    def _model_from_entry(entry, l):
        kw = dict(dims=entry["dims"], L=entry["L"], l=l, J=entry["J"])
        if entry.get("class") == "PottsModel":
            return PottsModel(entry["q"], **kw)
        if entry.get("class") == "ClockModel":
            return ClockModel(entry["q"], **kw)
        if entry.get("class") != "QStateModel":
            raise _ckpt.CheckpointError("the checkpoint names an unknown model")
        return QStateModel(entry["q"], entry["pair_energy"], twist=entry["twist"], **kw)

    def _settings(self):
        R, k = int(self.n_replicas), int(self.exchange_rate)
        return {"colouring": [int(c) for c in self.colouring], "cluster_rate": int(self.cluster_rate),
                "tempering": [R, k] if R or k else None,
                "binner": False if self._binning is None else (self._binning or True),
                "scaling": False if self.k_vectors is None else np.asarray(self.k_vectors, dtype=np.float64).tolist(),
                "stiffness": False if self.stiffness_directions is None
                else np.asarray(self.stiffness_directions, dtype=np.float64).tolist()}

    @staticmethod
    def _keywords(kw):
        if kw.get("tempering") is not None:
            kw["tempering"] = tuple(kw["tempering"])
        return kw

    # ---- results
    def analysis(self, walker=0):
        """MCAnalysis (MC.jl:1-11) of one walker"""
        st, cl = self.stats(walker), self.cluster_stats(walker)
        return {"acc_rate": st.acc_local / st.prop_local if st.prop_local else 0.0, "prop_local": int(st.prop_local),
                "acc_local": int(st.acc_local), "prop_global": int(cl.prop_global), "acc_global": int(cl.acc_global)}

    def measurements(self, walker=0):
        """{"Energy": {E, E2, e, C}, "Magn": {M, M2, M4, m, chi, U4}, "n_meas"}: means over the walker's measurements,
        in units of J-scaled energy and of unit vectors (the 2^30 of the device's integers removed).  M = <|M|> with
        |M| = sqrt(Mx^2 + My^2), m = M / N, C = beta^2 / N (<E2> - <E>^2), chi = beta N (<m^2> - <m>^2) =
        beta / N (<M2> - <M>^2), and U4 = 1 - <M4> / (2 <M2>^2), the Binder cumulant of a two-component order parameter
        (0 in the disordered phase, 1/2 in the ordered one).  For q = 2, My = 0."""
        st = self.stats(walker)
        n = st.n_meas
        if n == 0:
            raise DQMCError(ERR_INVALID, "measurements: no measurement has been taken")
        beta, invN = float(self.betas[walker]), 1.0 / self.N
        E, E2, M, M2, M4 = st.sum_E / n, st.sum_E2 / n, st.sum_absM / n, st.sum_M2 / n, st.sum_M4 / n
        with np.errstate(invalid="ignore", divide="ignore"):
            U4 = float(1.0 - np.float64(M4) / (2.0 * np.float64(M2) * np.float64(M2)))
        return {"Magn": {"M": M, "M2": M2, "M4": M4, "m": M * invN, "chi": beta * invN * (M2 - M * M), "U4": U4},
                "Energy": {"E": E, "E2": E2, "e": E * invN, "C": beta * beta * invN * (E2 - E * E)},
                "n_meas": int(n)}

    def series(self, walker=0):
        """per-measurement (E_int, Mx, My) of the walker as recorded, exact int64 in units of 2^-30 (at most
        series_capacity entries)"""
        cap = max(self.series_capacity, 1)
        e, mx, my = (np.zeros(cap, dtype=np.int64) for _ in range(3))
        n = C.c_int64()
        p = C.POINTER(C.c_int64)
        self._c(lib().dqmc_qs_get_series(self._h, walker, e.ctypes.data_as(p), mx.ctypes.data_as(p), my.ctypes.data_as(p),
                                         C.byref(n)))
        return e[:n.value].copy(), mx[:n.value].copy(), my[:n.value].copy()
