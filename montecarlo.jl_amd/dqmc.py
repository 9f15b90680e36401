"""DQMC flavor for a batch of walkers on one MI355X (mirror of src/flavors/DQMC/DQMC.jl).

The object keeps the reference's names (`p`, `a`, `conf`, `propagate`, `sweep_spatial`,
`update`, `run`, `greens`, `current_slice`, ...) so that parity tests read like the
reference's tests; every numerical method is a call into libdqmc_hip.so.  One DQMC
object = `n_walkers` independent Markov chains advancing in lockstep."""
import base64
import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib, checkpoint as _ckpt
from ._lib import check, dptr, i64ptr, lib
from .lattices import _lattice_vectors as _lat_vectors
from .configurations import CompressedConf, ConfigRecorder
from .models import rand_conf


@dataclass
class DQMCParameters:
    """DQMC.jl:52-125"""
    thermalization: int = 100
    sweeps: int = 100
    check_sign_problem: bool = True
    check_propagation_error: bool = True
    safe_mult: int = 10
    delta_tau: float = 0.1
    beta: float = 1.0
    slices: int = 10
    measure_rate: int = 10
    global_moves: bool = False
    global_rate: int = 5

    @staticmethod
    def resolve(**kw):
        """the (beta, delta_tau, slices) resolution rules of DQMC.jl:84-110"""
        keys = set(k for k in ("beta", "delta_tau", "slices") if k in kw)
        if keys == {"beta"}:
            kw["delta_tau"] = 0.1
            keys.add("delta_tau")
        if keys == {"delta_tau", "beta", "slices"}:
            slices = int(round(kw["beta"] / kw["delta_tau"]))
            if slices != kw["slices"]:
                raise ValueError("Given slices (%d) does not match calculated slices beta/delta_tau ≈ %d"
                                 % (kw["slices"], slices))
        elif keys == {"beta", "slices"}:
            kw["delta_tau"] = kw["beta"] / kw["slices"]
        elif keys == {"delta_tau", "slices"}:
            kw["beta"] = kw["delta_tau"] * kw["slices"]
        elif keys == {"delta_tau", "beta"}:
            kw["slices"] = int(round(kw["beta"] / kw["delta_tau"]))
        else:
            raise ValueError("Invalid keyword arguments to DQMCParameters: %s" % sorted(keys))
        return DQMCParameters(**kw)


def hopping_exponentials(T, delta_tau):
    """init_hopping_matrix_exp (stack.jl:167-181).  Julia's exp(::Matrix) uses the
    Hermitian eigen-decomposition for a symmetric argument."""
    w, V = np.linalg.eigh(-0.5 * delta_tau * T)
    eT = (V * np.exp(w)) @ V.T
    w, V = np.linalg.eigh(0.5 * delta_tau * T)
    eTinv = (V * np.exp(w)) @ V.T
    return eT, eTinv, eT @ eT, eTinv @ eTinv


_ERR_INVALID = -1  # DQMC_ERR_INVALID (include/dqmc_hip.h)


def _ring_exponentials(h, delta_tau):
    """exp(-dtau h) and exp(+dtau h) of a 16 x 16 one-dimensional hopping h with the recipe of hopping_exponentials:
    the half-step exponential from eigh, squared"""
    w, V = np.linalg.eigh(-0.5 * delta_tau * h)
    e = (V * np.exp(w)) @ V.T
    w, V = np.linalg.eigh(0.5 * delta_tau * h)
    ei = (V * np.exp(w)) @ V.T
    return e @ e, ei @ ei


def triangular_factors(model, delta_tau):
    """The factors dqmc_set_triangular_factors takes for a model on TriangularLattice(16): per block
    [eT2: Fx Fy Fd][eTinv2: Fx Fy Fd], each 16 x 16 column-major, such that eT2 = (Fy (x) Fx) Ed(Fd) (and eTinv2 alike)
    in the site order x + 16 y, where Ed applies Fd along the diagonals x - y = const.  T = -mu - t (X + X' + Y + Y' + D + D')
    with X, Y and D = XY commuting shifts, so exp(-dtau T) = e^{dtau mu} f(X) f(Y) f(D), f = exp(dtau t (S + S')) on a
    16-ring; mu is folded into Fx.  The engine checks them against the dense exponentials."""
    L = 16
    S = np.roll(np.eye(L), 1, axis=0)
    ring = -model.t * (S + S.T)
    ex, exi = _ring_exponentials(ring - model.mu * np.eye(L), delta_tau)
    e1, e1i = _ring_exponentials(ring, delta_tau)
    per_block = np.concatenate([m.reshape(-1, order="F") for m in (ex, e1, e1, exi, e1i, e1i)])
    return np.ascontiguousarray(np.tile(per_block, model.flv))


def square_tp_factors(model, delta_tau):
    """The factors dqmc_set_square_tp_factors takes for a model with next-nearest-neighbour hopping tp on SquareLattice(16):
    per block [eT2: Fx Fy Fd Fa][eTinv2: Fx Fy Fd Fa], each 16 x 16 column-major, such that eT2 = (Fy (x) Fx) Ed(Fd) Ea(Fa)
    (and eTinv2 alike) in the site order x + 16 y, where Ed applies Fd along the diagonals x - y = const and Ea applies Fa
    along the anti-diagonals x + y = const.  T = -mu - t (X + X' + Y + Y') - tp (D + D' + A + A') with X, Y, D = XY and
    A = X Y^-1 commuting shifts, so exp(-dtau T) = e^{dtau mu} f_t(X) f_t(Y) f_tp(D) f_tp(A), f_s = exp(dtau s (S + S')) on a
    16-ring; mu is folded into Fx.  The engine checks them against the dense exponentials."""
    L = 16
    S = np.roll(np.eye(L), 1, axis=0)
    ring = -model.t * (S + S.T)
    ex, exi = _ring_exponentials(ring - model.mu * np.eye(L), delta_tau)
    e1, e1i = _ring_exponentials(ring, delta_tau)
    ep, epi = _ring_exponentials(-model.tp * (S + S.T), delta_tau)
    per_block = np.concatenate([m.reshape(-1, order="F") for m in (ex, e1, ep, ep, exi, e1i, epi, epi)])
    return np.ascontiguousarray(np.tile(per_block, model.flv))


def checkerboard_exponentials(T, lattice, delta_tau, return_factors=False):
    """CheckerboardTrue (init_checkerboard_matrices, stack.jl:185-235; slice_matrices.jl:79-222;
    _greens! DQMC.jl:731-750) as the four constant matrices of the dense code path.  The reference
    keeps one sparse matrix per bond group, chkr_hop_half[g] = exp(-dtau/2 Tg) with
    Tg[trg, src] = T[trg, src] over the group's (disjoint) bonds, and applies
        B_l      = H_n ... H_2 C_1 H_2 ... H_n Mu eV_l,       C_1 = chkr_hop[1],  Mu = exp(-dtau diag(T))
        B_l^-1   = eV_l^-1 Mu^-1 (H_n ... H_2 C_1 H_2 ... H_n)^-1
        greens() = H_1^-1 ... H_n^-1  G  H_n ... H_1
    group by group.  On MI355X a pass of O(n^2 groups) sparse row updates is HBM-bound and slower than one
    MFMA GEMM at these sizes, so the group products are multiplied out once here (same order of factors)
    and handed to the same kernels: eT2 -> P Mu, eTinv2 -> Mu^-1 P^-1, eT -> H_n...H_1, eTinv -> its inverse."""
    from .lattices import build_checkerboard
    from scipy.linalg import expm
    N = T.shape[0]
    cb, groups, n_groups = build_checkerboard(lattice)

    def rem_eff_zeros(X):  # stack.jl:184
        X = X.copy()
        X[np.abs(X) < 1e-15] = 0.0
        return X

    H, Hinv, Cm, Cinv = [], [], [], []
    for (gs, ge) in groups:
        Tg = np.zeros((N, N))
        for i in range(gs, ge + 1):
            src, trg = cb[0, i - 1], cb[1, i - 1]
            Tg[trg - 1, src - 1] = T[trg - 1, src - 1]
        H.append(rem_eff_zeros(expm(-0.5 * delta_tau * Tg)))
        Hinv.append(rem_eff_zeros(expm(0.5 * delta_tau * Tg)))
        Cm.append(rem_eff_zeros(expm(-delta_tau * Tg)))
        Cinv.append(rem_eff_zeros(expm(delta_tau * Tg)))
    mus = np.diag(T)
    Mu, Muinv = np.diag(np.exp(-delta_tau * mus)), np.diag(np.exp(delta_tau * mus))

    if return_factors:
        return H, Hinv, Cm, Cinv, np.exp(-delta_tau * mus), np.exp(delta_tau * mus), n_groups

    def sandwich(half, full):  # the factor applied by multiply_slice_matrix_left! (slice_matrices.jl:109-121)
        M = np.eye(N)
        for i in reversed(range(1, n_groups)):
            M = half[i] @ M
        M = full[0] @ M
        for i in range(1, n_groups):
            M = half[i] @ M
        return M

    P, Pinv = sandwich(H, Cm), sandwich(Hinv, Cinv)
    eT = np.eye(N)
    for i in reversed(range(n_groups)):     # target * chkr_hop_half[i], i = n..1
        eT = eT @ H[i]
    eTinv = np.eye(N)
    for i in reversed(range(n_groups)):     # chkr_hop_half_inv[i] * target, i = n..1
        eTinv = Hinv[i] @ eTinv
    return eT, eTinv, P @ Mu, Muinv @ Pinv


def checkerboard_tables(T, lattice, delta_tau):
    """The sparse factors of init_checkerboard_matrices (stack.jl:185-235) in the ELL form dqmc_set_checkerboard takes:
    factor list = [H_1..H_n, C_1, Hinv_1..Hinv_n, Cinv_1] followed by their transposes (offset n_f), each as
    (vals, cols)[n_sites][kmax]; plus the seven sequences of include/dqmc_hip.h (0-based factor indices)."""
    H, Hinv, Cm, Cinv, mu, mu_inv, ng = checkerboard_exponentials(T, lattice, delta_tau, return_factors=True)
    mats = list(H) + [Cm[0]] + list(Hinv) + [Cinv[0]]
    nf = len(mats)
    mats = mats + [m.T for m in mats]
    N = T.shape[0]
    kmax = max(int((np.abs(m) > 0).sum(axis=1).max()) for m in mats)
    vals = np.zeros((len(mats), N, kmax))
    cols = np.zeros((len(mats), N, kmax), dtype=np.int32)
    for i, m in enumerate(mats):
        for r in range(N):
            nz = np.nonzero(m[r])[0]
            vals[i, r, :len(nz)] = m[r, nz]
            cols[i, r, :len(nz)] = nz
            cols[i, r, len(nz):] = r
    iH = lambda g: g              # H_g (g = 0..ng-1)
    iC = ng                       # C_1
    iHi = lambda g: ng + 1 + g    # Hinv_g
    iCi = 2 * ng + 1              # Cinv_1
    sand = lambda h, c: [h(g) for g in range(ng - 1, 0, -1)] + [c] + [h(g) for g in range(1, ng)]
    tr = lambda seq: [nf + i for i in seq]
    seqs = [sand(iH, iC),                                 # B X
            sand(iHi, iCi),                               # B^-1 X
            tr(sand(iH, iC)),                             # B' X
            tr(sand(iH, iC)),                             # X B  (columns mixed by rows of the transposes)
            tr(sand(iHi, iCi)),                           # X B^-1
            tr([iH(g) for g in range(ng - 1, -1, -1)]),   # X eT = X H_n ... H_1
            [iHi(g) for g in range(ng - 1, -1, -1)]]      # eTinv X = Hinv_1 ... Hinv_n X (Hinv_n applied first)
    return dict(kmax=kmax, vals=vals, cols=cols, mu=mu, mu_inv=mu_inv, seqs=seqs)


def checkerboard_seqs(tables):
    """The seven factor sequences of checkerboard_tables as the [7][32] array and the lengths dqmc_set_checkerboard takes;
    a lattice with more than 16 bond groups has longer sequences and cannot use the sparse form"""
    seqs = np.zeros((7, 32), dtype=np.int32)
    lens = np.zeros(7, dtype=np.int32)
    for q, sq in enumerate(tables["seqs"]):
        if len(sq) > 32:
            raise ValueError("sparse checkerboard: a factor sequence of %d entries exceeds the 32 the engine takes (%d bond "
                             "groups); use checkerboard=\"dense\"" % (len(sq), (len(sq) + 1) // 2))
        lens[q] = len(sq)
        seqs[q, :len(sq)] = sq
    return seqs, lens


def checkerboard_slab(n):
    """(slab width, dynamic LDS bytes) of the sparse-factor kernel at n sites, as dqmc_checkerboard_plan reports them: two
    images of n x (width + 1) doubles and two scaling vectors in the 160 KiB of LDS; 32 columns up to n = 256, 16 up to
    568, 8 up to 1024.  Beyond that no width fits and dqmc_set_checkerboard refuses the tables."""
    qw = 32 if n <= 256 else 16 if n <= 568 else 8
    lds = (2 * n * (qw + 1) + 2 * n) * 8
    if n < 1 or lds > 160 * 1024:
        raise ValueError("sparse checkerboard: %d sites are beyond the slab kernel (8 columns need 160 n bytes of 163840 B of "
                         "LDS: n <= 1024); use checkerboard=\"dense\"" % n)
    return qw, lds


class DQMCAnalysis:
    """DQMC.jl:36-47 for one walker"""

    def __init__(self, st, gst=None):
        self.prop_global = gst.prop_global if gst is not None else 0
        self.acc_global = gst.acc_global if gst is not None else 0
        self.acc_rate_global = self.acc_global / self.prop_global if self.prop_global else 0.0
        self.prop_local = st.prop_local
        self.acc_local = st.acc_local
        self.acc_rate = st.acc_local / st.prop_local if st.prop_local else 0.0
        self.imaginary_probability = st.imaginary_probability
        self.negative_probability = st.negative_probability
        self.propagation_error = st.propagation_error


class DQMC:
    """DQMC(model; beta, delta_tau=0.1, safe_mult=10, ...) (DQMC.jl:250-289) for
    `n_walkers` chains on device `device_id`.  `seed` keys the initial HS fields and the
    Metropolis streams of walker w as `seed + first_walker + w`, so results do not depend
    on how walkers are distributed over devices.  `global_moves=True` runs one global move of `global_kind` ("site": one
    site's whole time line is flipped, "all": the whole field) per walker in every `global_rate`-th sweep, where the
    reference keeps its hook (DQMC.jl:526-532); see global_move().  `sign_weighting=True` makes every measurement sum
    and binner take s O in the place of O, s = the sign of the walker's field, next to the sum of s (see
    set_sign_weighting(), signed()): the averages of a model whose weight is not positive."""

    def __init__(self, model, n_walkers=1, device_id=0, seed=123, first_walker=0, thermalization=100, sweeps=100,
                 safe_mult=10, measure_rate=10, check_sign_problem=True, check_propagation_error=True,
                 checkerboard=False, global_moves=False, global_rate=5, global_kind="site", sign_weighting=False,
                 **kw):
        self.model = model
        self.checkerboard = bool(checkerboard)
        if getattr(model, "tp", 0.0) != 0.0 and self.checkerboard:
            raise ValueError("checkerboard: the bond table has no diagonal bonds, so it cannot decompose a model with tp != 0")
        # what save() writes down so that load() can construct and configure the object again
        self._ctor = dict(n_walkers=int(n_walkers), seed=int(seed), first_walker=int(first_walker),
                          checkerboard=checkerboard if isinstance(checkerboard, str) else bool(checkerboard),
                          global_kind=global_kind)
        self._tables, self._td_args, self._bin_caps, self._user_bin = {}, None, {}, None
        self._dirs, self._mom = None, None  # the directions of set_pair_directions' iterator; (q, cos table, sin table) of set_momenta
        self._gm_set = None       # (rate, kind) of the last set_global_rate
        self._sus_layout = False  # the susceptibility section is laid out (by its first use)
        self._thermo = False      # set_thermodynamics is on
        self._channels = None     # {name: weights} of set_pair_channels
        self._ent = None          # (names or None, site lists) of set_entanglement
        self._ctd = 0             # `every` of set_current_time_displaced (0: off)
        self._tcov = None         # (bin_size, what) of set_tau_covariance
        self._ucov = None         # (n_series, R, bin_size) of user_covariance
        self._mid_sweep = False  # set by load(): run() finishes the sweep the checkpoint was taken in
        if int(global_rate) < 1:
            raise ValueError("global_rate must be at least 1")
        self.global_kind = self._global_kind(global_kind)
        self.p = DQMCParameters.resolve(thermalization=thermalization, sweeps=sweeps, safe_mult=safe_mult,
                                        measure_rate=measure_rate, check_sign_problem=check_sign_problem,
                                        check_propagation_error=check_propagation_error,
                                        global_moves=bool(global_moves), global_rate=int(global_rate), **kw)
        self.n_walkers = n_walkers
        self._device_id = device_id
        self.N = len(model.l)
        self.nb = model.flv
        self.last_sweep = 0
        Ts = model.hopping_matrix()
        if self.checkerboard:  # DQMC(m; checkerboard=true) (DQMC.jl:250-263)
            exps = [checkerboard_exponentials(T, model.l, self.p.delta_tau) for T in Ts]
        else:
            exps = [hopping_exponentials(T, self.p.delta_tau) for T in Ts]
        cat = lambda k: np.ascontiguousarray(np.concatenate([e[k].reshape(-1, order="F") for e in exps]))
        self._eT, self._eTinv, self._eT2, self._eTinv2 = cat(0), cat(1), cat(2), cat(3)
        self.hopping_matrix_exp = [e[0] for e in exps]
        self.hopping_matrix_exp_inv = [e[1] for e in exps]
        self.hopping_matrix_exp_squared = [e[2] for e in exps]
        self.hopping_matrix_exp_inv_squared = [e[3] for e in exps]
        prm = _lib.Params(self.N, model.kind, self.p.slices, self.p.safe_mult, n_walkers, device_id,
                          int(self.p.check_propagation_error), int(self.p.check_sign_problem), self.p.delta_tau,
                          model.U, dptr(self._eT), dptr(self._eTinv), dptr(self._eT2), dptr(self._eTinv2))
        self._h = C.c_void_p()
        check(lib().dqmc_create(C.byref(prm), C.byref(self._h)))
        # checkerboard=True picks the faster execution of the same decomposition: measured on MI355X (config 3 shape,
        # tools/time_parts.py checkerboard) the sparse-factor kernel takes 32.5 us per product against 31.2 us for the dense
        # MFMA GEMM with the multiplied-out constants at n = 256, so dense up to n = 256 and sparse (O(n^2) work per
        # product) above; checkerboard="sparse" / "dense" force one.  The cross-over was measured at n = 256 only.
        sparse = checkerboard == "sparse" or (checkerboard is True and self.N > 256)
        if self.checkerboard and sparse:
            checkerboard_slab(self.N)  # ValueError where no slab width fits (the engine refuses such tables as well)
            tb = [checkerboard_tables(T, model.l, self.p.delta_tau) for T in Ts]
            t0 = tb[0]  # both spin blocks of the repulsive model share T (HubbardModelRepulsive.jl:87-100)
            seqs, lens = checkerboard_seqs(t0)
            mu = np.ascontiguousarray(np.concatenate([t["mu"] for t in tb]))
            mui = np.ascontiguousarray(np.concatenate([t["mu_inv"] for t in tb]))
            vals, cols = np.ascontiguousarray(t0["vals"]), np.ascontiguousarray(t0["cols"])
            check(lib().dqmc_set_checkerboard(self._h, t0["kmax"], vals.shape[0], dptr(vals),
                                              cols.ctypes.data_as(C.POINTER(C.c_int32)), dptr(mu), dptr(mui),
                                              seqs.ctypes.data_as(C.POINTER(C.c_int32)),
                                              lens.ctypes.data_as(C.POINTER(C.c_int32))), self._h)
        # the triangular 16 x 16 lattice: its exponentials in three-factor form (tri.hip).  The engine tests the factors
        # against its own eT2 / eTinv2 and refuses ones that do not reproduce them (a hopping other than the model's
        # t and mu): the handle then keeps the dense path.
        from .lattices import TriangularLattice
        l = model.l
        if isinstance(l, TriangularLattice) and l.Lx == l.Ly == 16 and not self.checkerboard:
            f = triangular_factors(model, self.p.delta_tau)
            rc = lib().dqmc_set_triangular_factors(self._h, dptr(f))
            if rc != _ERR_INVALID:
                self._c(rc)
        # the t-t' square 16 x 16 lattice: its exponentials in four-factor form (ttp.hip), under the same gate
        from .lattices import SquareLattice
        if isinstance(l, SquareLattice) and l.L == 16 and getattr(model, "tp", 0.0) != 0.0 and not self.checkerboard:
            f = square_tp_factors(model, self.p.delta_tau)
            rc = lib().dqmc_set_square_tp_factors(self._h, dptr(f))
            if rc != _ERR_INVALID:
                self._c(rc)
        # rand(DQMC, m, slices) per walker (DQMC.jl:273), then the Metropolis stream
        self.seeds = [seed + first_walker + w for w in range(n_walkers)]
        for w, s in enumerate(self.seeds):
            rng = np.random.Generator(np.random.Philox(key=s))
            self.set_conf(w, rand_conf(rng, self.N, self.p.slices))
            self.seed(w, s)
        if self.p.global_moves:
            self.set_global_rate(self.p.global_rate, self.global_kind)
        if sign_weighting:
            self.set_sign_weighting(True)

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().dqmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        check(rc, self._h)

    # ---- state
    def set_conf(self, walker, conf):
        c = np.asfortranarray(np.asarray(conf, dtype=np.int8))
        if c.shape != (self.N, self.p.slices):
            raise ValueError("conf must have shape (n_sites, slices)")
        self._c(lib().dqmc_set_conf(self._h, walker, c.ctypes.data))

    def conf(self, walker=0):
        c = np.zeros((self.N, self.p.slices), dtype=np.int8, order="F")
        self._c(lib().dqmc_get_conf(self._h, walker, c.ctypes.data))
        return c

    def conf_bits(self, walker=0):
        """compress(mc, model, conf(mc)) packed on the device (HubbardModel.jl:56-59)"""
        n = (self.N * self.p.slices + 63) // 64
        ch = np.zeros(n, dtype=np.uint64)
        self._c(lib().dqmc_get_conf_bits(self._h, walker, ch.ctypes.data_as(C.POINTER(C.c_uint64))))
        return CompressedConf(ch, (self.N, self.p.slices))

    def set_conf_bits(self, walker, cc):
        """mc.conf = decompress(mc, model, c), unpacked on the device"""
        if cc.shape != (self.N, self.p.slices):
            raise ValueError("compressed configuration has the wrong shape")
        ch = np.ascontiguousarray(cc.chunks, dtype=np.uint64)
        self._c(lib().dqmc_set_conf_bits(self._h, walker, ch.ctypes.data_as(C.POINTER(C.c_uint64))))

    def seed(self, walker, seed):
        self._c(lib().dqmc_seed(self._h, walker, seed))

    def set_uniforms(self, walker, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        self._c(lib().dqmc_set_uniforms(self._h, walker, dptr(u), u.size))

    def uniforms_used(self, walker=0):
        n = C.c_uint64()
        self._c(lib().dqmc_uniforms_used(self._h, walker, C.byref(n)))
        return n.value

    def _state(self):
        cs, d = C.c_int32(), C.c_int32()
        self._c(lib().dqmc_get_state(self._h, C.byref(cs), C.byref(d)))
        return cs.value, d.value

    @property
    def current_slice(self):
        return self._state()[0]

    @property
    def direction(self):
        return self._state()[1]

    # ---- the sweep loop
    def prepare(self):
        """init!, build_stack, propagate (DQMC.jl:412-414)"""
        self._c(lib().dqmc_prepare(self._h))

    def build_stack(self):
        self._c(lib().dqmc_build_stack(self._h))

    def propagate(self):
        self._c(lib().dqmc_propagate(self._h))

    def sweep_spatial(self):
        self._c(lib().dqmc_sweep_spatial(self._h))

    def update(self):
        self._c(lib().dqmc_update(self._h))

    def sweep(self, n=1):
        self._c(lib().dqmc_sweep(self._h, n))

    def update_until_measure(self):
        n = C.c_int32()
        self._c(lib().dqmc_update_until_measure(self._h, C.byref(n)))
        return n.value

    def synchronize(self):
        self._c(lib().dqmc_synchronize(self._h))

    def replay_greens(self, slice_=0):
        """calculate_greens(mc, slice) into mc.s.greens for every walker (DQMC.jl:651-652)"""
        self._c(lib().dqmc_replay_greens(self._h, slice_))

    def replay(self, configurations, measure_rate=1):
        """replay!(mc, configurations) (DQMC.jl:605-697): the recorded configurations are decompressed
        on the device, `n_walkers` at a time, the Green's function is rebuilt from scratch at slice 0
        (calculate_greens(mc, 0), DQMC.jl:652) and the measurement sums are accumulated.
        Returns the accumulator vector (layout of include/dqmc_hip.h)."""
        cfgs = list(configurations)[::measure_rate]
        self.reset_accumulators()
        W, n, B = self.n_walkers, self.N, self.nb
        tail = np.zeros(self.accumulator_size())
        for i0 in range(0, len(cfgs), W):
            batch = cfgs[i0:i0 + W]
            for w in range(W):  # a short last batch repeats its last configuration in the idle walkers
                self.set_conf_bits(w, batch[min(w, len(batch) - 1)])
            self.replay_greens(0)
            if len(batch) == W:
                self.accumulate_greens()
            else:  # partial batch: only the filled walkers count
                for w in range(len(batch)):
                    G = self.greens(w)
                    g = np.concatenate([x.reshape(-1, order="F") for x in G])
                    tail[:B * n * n] += g
                    tail[B * n * n:2 * B * n * n] += g * g
                    for b in range(B):
                        tail[2 * B * n * n + b * n:2 * B * n * n + (b + 1) * n] += 1.0 - np.diag(G[b])
                    tail[-1] += 1
        return self.accumulators() + tail

    def run(self, verbose=False, on_measure=None, recorder=None, measurements=("greens",), binning=False,
            checkpoint=None, checkpoint_every=None):
        """run!(mc) (DQMC.jl:369-515) without the host-side measurement framework: the selected
        measurements are accumulated on the device every `measure_rate`-th sweep after thermalization,
        at current_slice == 1 && direction == +1 (DQMC.jl:425-436).  `measurements` may contain
        "greens" (greens_measurement, occupation), "correlations" (charge/spin density correlations,
        magnetization; needs set_pair_directions), "pairing" (needs set_local_targets) and
        "susceptibilities" (the CombinedGreensIterator measurements) and "time_displaced" (the tau-resolved rows; needs
        set_time_displaced; shares the one iterator pass with "susceptibilities"), and "thermodynamics" (energy, filling,
        double occupancy ...; needs set_thermodynamics) and "entanglement" (the Renyi-2 pair samples; needs
        set_entanglement; it has no binner: its error bar is the jackknife over walkers of entanglement()).  `binning=True` enables the device-side
        LogBinner of every selected measurement before the first sweep (enable_binning; read with binned()).
        `checkpoint=path` saves the run (save()) in every `checkpoint_every`-th sweep and in the last one, thermalization
        included, at the sweep's measurement point behind its measurements: the one place of a sweep where the chain stands
        where the engine exports its state.  On an object that load() returned from such a file, run() first finishes that
        sweep (the up pass behind the measurement point) and goes on with the next one up to thermalization + sweeps, as
        resume! does (DQMC.jl:463-477)."""
        if checkpoint is not None and (checkpoint_every is None or int(checkpoint_every) < 1):
            raise ValueError("run(checkpoint=path) needs checkpoint_every >= 1")
        known = {"greens": lib().dqmc_accumulate_greens, "correlations": lib().dqmc_accumulate_correlations,
                 "pairing": lib().dqmc_accumulate_pairing, "thermodynamics": lib().dqmc_accumulate_thermodynamics,
                 "entanglement": lib().dqmc_accumulate_entanglement}
        for m in measurements:
            if m not in known and m not in ("susceptibilities", "time_displaced"):
                raise ValueError("unknown measurement %r" % (m,))
        if "time_displaced" in measurements and not self.time_displaced_plan()["every"]:
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_time_displaced before run(measurements=(..., 'time_displaced'))")
        resumed, self._mid_sweep = self._mid_sweep, False
        if not resumed:  # (a loaded object stands at its measurement point, the stack rebuilt by the import)
            self.prepare()
        if binning:  # a resumed run! keeps the binners it has (DQMC.jl:395-411)
            self.enable_binning([m for m in measurements if m != "entanglement" and not self._binning_enabled(m)])
            if self._mom is not None:  # and, with momenta set, the momentum binner of every section that has one
                self.enable_binning([k for k in ("momentum_" + m for m in measurements)
                                     if k in _lib.BIN_MOMENTUM and not self._binning_enabled(k)])
        if self.last_sweep == 0:  # a resumed run! keeps the measurement state (DQMC.jl:395-411)
            self.reset_accumulators()
        total = self.p.thermalization + self.p.sweeps
        t0 = time.time()
        while resumed and self._state() != (self.p.slices, -1):  # the rest of sweep last_sweep: no measurement point in it
            self._c(lib().dqmc_update(self._h))
        for i in range(self.last_sweep + 1, total + 1):
            for _ in range(2 * self.p.slices):
                self._c(lib().dqmc_update(self._h))
                cs, d = self._state()
                if cs == 1 and d == 1 and i > self.p.thermalization and recorder is not None:
                    recorder.push(self, i)  # push!(mc.configs, mc, mc.model, i) (DQMC.jl:430)
                if cs == 1 and d == 1 and i > self.p.thermalization and i % self.p.measure_rate == 0:
                    ut_pass = False  # one CombinedGreensIterator pass serves both of its measurements
                    for m in measurements:
                        if m in known:
                            self._c(known[m](self._h))
                        elif not ut_pass:
                            self.accumulate_susceptibilities()
                            ut_pass = True
                    if on_measure is not None:
                        on_measure(self, i)
                if cs == 1 and d == 1 and checkpoint is not None and (i % int(checkpoint_every) == 0 or i == total):
                    self.save(checkpoint, _sweep=i)
            self.last_sweep = i
            if verbose and i % 10 == 0:
                print("\t%d\n\t\tsweep dur: %.3fs" % (i, (time.time() - t0) / 10))
                t0 = time.time()
        self.synchronize()
        return True

    # ---- checkpoint and resume (include/dqmc_hip.h "checkpoint and resume"; the file: checkpoint.py)
    def state_size(self):
        n = C.c_size_t()
        self._c(lib().dqmc_state_size(self._h, C.byref(n)))
        return n.value

    def state(self):
        """dqmc_state_export: the engine's state as a numpy.uint8 array - the HS fields, RNG cursors, counters, every
        accumulator and binner level.  Only at the measurement point (current_slice == 1, direction == +1: where
        update_until_measure() returns, and sweep() when it started there); the chain is left exactly as it was."""
        buf = np.empty(self.state_size(), dtype=np.uint8)
        self._c(lib().dqmc_state_export(self._h, buf.ctypes.data, buf.size))
        return buf

    def set_state(self, buf):
        """dqmc_state_import into this object, which must be configured as the exporting one was (the same constructor
        arguments, tables, time-displaced setting, binners, sign weighting, global moves): ERR_INVALID naming the first
        field that differs otherwise, and the object stays as it was.  Afterwards the chains stand at the measurement
        point with the stack and G rebuilt from the fields."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        self._c(lib().dqmc_state_import(self._h, buf.ctypes.data, buf.size))

    _MODELS = ("HubbardModelAttractive", "HubbardModelRepulsive")
    _LATTICES = {"SquareLattice": ("L",), "Chain": ("sites",), "CubicLattice": ("dim", "L"),
                 "TriangularLattice": ("L", "Lx", "Ly"), "BilayerSquareLattice": ("L",), "HoneycombLattice": ("L",)}  # class -> the attributes its constructor takes, in order
    # the lattices added since: a table of their own, because tests/test_honeycomb_tables.py pins the one above entry by entry
    _LATTICES_MORE = {"RectangularLattice": ("Lx", "Ly")}

    @classmethod
    def _lattice_args(cls, name):
        """the constructor attributes of a lattice class a checkpoint can name, None for any other"""
        return cls._LATTICES.get(name, cls._LATTICES_MORE.get(name))

    @staticmethod
    def _model_entry(m):
        """the "model" entry of a checkpoint preamble: the class and the keywords that construct it again"""
        model = {"class": type(m).__name__, "U": m.U, "t": m.t}
        if m.kind == _lib.ATTRACTIVE or m.mu != 0.0:  # (an undoped repulsive model is written as it always was)
            model["mu"] = m.mu
        if getattr(m, "tp", 0.0) != 0.0:  # (absent at 0: the preamble of before)
            model["tp"] = m.tp
        if getattr(m, "t_perp", None) is not None:  # (a BilayerSquareLattice's model only)
            model["t_perp"] = m.t_perp
        return model

    @classmethod
    def _model_from_entry(cls, entry, l):
        from . import models as _mod
        mdl = dict(entry)
        if mdl["class"] not in cls._MODELS:
            raise _ckpt.CheckpointError("the checkpoint names an unknown model or lattice")
        return getattr(_mod, mdl.pop("class"))(l=l, **mdl)

    def _preamble(self, sweep, mid_sweep):
        m, l, p = self.model, self.model.l, self.p
        if type(m).__name__ not in self._MODELS or self._lattice_args(type(l).__name__) is None:
            raise ValueError("save(): %s on %s is not a model / lattice a checkpoint can name"
                             % (type(m).__name__, type(l).__name__))
        model = self._model_entry(m)
        tables = {}
        for name, entry in self._tables.items():
            tables[name] = {"table": _ckpt.pack_table(entry[0]), "count": entry[1]}
            if name == "current_targets":
                tables[name]["hopping"] = entry[2]
        extra = {"thermodynamics": self._thermo} if self._thermo else {}  # (absent while off: the preamble of before)
        if self._channels is not None:  # the names and weights of set_pair_channels (absent while off as well)
            extra["pair_channels"] = [[k, [float(x) for x in v]] for k, v in self._channels.items()]  # (a list: the order is the engine's)
        if self._ent is not None:  # the site lists of set_entanglement and its sums, which no blob section holds (absent while off)
            raw = self._entanglement_raw()
            extra["entanglement"] = {"names": self._ent[0], "sites": [list(a) for a in self._ent[1]],
                                     "count": int(raw[-2]), "failures": int(raw[-1]),
                                     "sums": base64.b64encode(raw[:-2].astype("<f8").tobytes()).decode("ascii")}
        if self._ctd:  # the setting of set_current_time_displaced and its per-walker sums, which no blob section holds either
            extra["current_time_displaced"] = {
                "every": int(self._ctd),
                "sums": base64.b64encode(self._current_tau_raw().astype("<f8").tobytes()).decode("ascii")}
        return {
            **extra,
            "format": 1,
            "model": model,
            "lattice": {"class": type(l).__name__, "args": [int(getattr(l, a)) for a in self._lattice_args(type(l).__name__)]},
            "dqmc": dict(self._ctor, beta=p.beta, delta_tau=p.delta_tau, slices=p.slices, safe_mult=p.safe_mult,
                         thermalization=p.thermalization, sweeps=p.sweeps, measure_rate=p.measure_rate,
                         check_sign_problem=bool(p.check_sign_problem),
                         check_propagation_error=bool(p.check_propagation_error), global_moves=bool(p.global_moves),
                         global_rate=p.global_rate, sign_weighting=self.sign_weighting()),
            "tables": tables,
            "time_displaced": list(self._td_args) if self._td_args else None,
            # the wave vectors and both phase tables of set_momenta (the tables as handed to the engine, d fastest); the
            # momentum binners that are on stand among the sections of "binning"
            "momenta": None if self._mom is None else {"q": self._mom[0].tolist(), "cos": self._mom[1].tolist(),
                                                       "sin": self._mom[2].tolist()},
            "binning": {"sections": dict(self._bin_caps), "user": list(self._user_bin) if self._user_bin else None},
            "global": list(self._gm_set) if self._gm_set else None,  # the last set_global_rate: (rate, DQMC_GLOBAL_* kind)
            "susceptibilities_layout": bool(self._sus_layout),
            "last_sweep": int(sweep),
            "mid_sweep": bool(mid_sweep),  # saved by run() inside sweep last_sweep: its up pass is still to come
        }

    def save(self, path, _sweep=None):
        """save(filename, mc) (FileIO.jl:38-79) for what lives on the device: one file (checkpoint.py) with a JSON
        preamble - model, lattice, the constructor's arguments, the integer tables handed to set_pair_directions /
        set_local_targets / set_current_targets, the time-displaced, binning, sign and global-move settings and the run
        loop's last sweep - and the blob of state().  Written to a temporary file in the same directory and moved into
        place, so `path` always holds a whole checkpoint.  Only at the measurement point (see state()): run(checkpoint=...)
        calls it there, and so may the caller on an object that load() returned or that went there with
        update_until_measure(); an object whose run() has returned stands at current_slice == slices, direction == -1 and
        is refused (ERR_STATE).  A ConfigRecorder's configurations are the caller's and are not part of the file.  The
        moments of set_tau_covariance / user_covariance are not checkpointed: with either on, save() raises ERR_STATE."""
        if self._tcov is not None or self._ucov is not None:
            raise _lib.DQMCError(_lib.ERR_STATE, "save: the tau-tau' covariance moments are not part of a checkpoint: read "
                                 "them (tau_covariance_moments, user_covariance_result), then turn the accumulators off "
                                 "with set_tau_covariance(0) / user_covariance(0, 0, 0)")
        blob = self.state()
        # (a loaded object saved again before its run() is still inside the sweep its file was taken in)
        mid = self._mid_sweep if _sweep is None else True
        _ckpt.write(path, self._preamble(self.last_sweep if _sweep is None else _sweep, mid), blob)

    @classmethod
    def load(cls, path, device_id=0):
        """load(filename) (FileIO.jl:95-156): an object constructed and configured as the saved one, with its state
        imported (set_state) on device `device_id`.  seed and first_walker are the saved ones, so the files of the ranks of
        a sharded run give back distinct walkers.  last_sweep is the saved one; run() continues behind it."""
        from . import lattices as _lat
        pre, blob = _ckpt.read(path)
        if pre.get("flavor", "dqmc") != "dqmc":  # a file of the classical flavor (MC.save, QStateMC.save)
            raise _ckpt.CheckpointError("the checkpoint holds a run of flavor %r, DQMC.load reads flavor 'dqmc'"
                                        % (pre["flavor"],))
        if pre.get("format") != 1:
            raise _ckpt.CheckpointError("checkpoint preamble format %r, this package reads format 1" % (pre.get("format"),))
        lat = pre["lattice"]
        if cls._lattice_args(lat["class"]) is None or pre["model"]["class"] not in cls._MODELS:
            raise _ckpt.CheckpointError("the checkpoint names an unknown model or lattice")
        l = getattr(_lat, lat["class"])(*lat["args"])
        model = cls._model_from_entry(pre["model"], l)
        kw = dict(pre["dqmc"])
        mc = cls(model, device_id=device_id, **kw)
        try:
            t = pre["tables"]
            if "pair_directions" in t:
                mc._set_pair_directions(_ckpt.unpack_table(t["pair_directions"]["table"]), t["pair_directions"]["count"])
                # the displacements r_d are not in the file: where the saved table is the lattice's own, they are those of
                # its EachSitePairByDistance (what set_pair_channels("default") and superfluid_stiffness read)
                it = _lat.EachSitePairByDistance(l)
                if it.ndirections() == mc._ndirs and np.array_equal(np.asarray(it.dir_of), mc._tables["pair_directions"][0]):
                    mc._dirs = np.array(it.directions, dtype=np.float64)
            if "local_targets" in t:
                mc._set_local_targets(_ckpt.unpack_table(t["local_targets"]["table"]), t["local_targets"]["count"])
            if "current_targets" in t:
                hop = t["current_targets"]["hopping"]
                if hop is not None:
                    hop = [np.asarray(hop[b * mc.N * mc.N:(b + 1) * mc.N * mc.N]).reshape((mc.N, mc.N), order="F")
                           for b in range(mc.nb)]
                mc._set_current_targets(_ckpt.unpack_table(t["current_targets"]["table"]), t["current_targets"]["count"], hop)
            if pre["time_displaced"]:
                mc.set_time_displaced(*pre["time_displaced"])
            if pre["global"]:
                mc.set_global_rate(*pre["global"])
            if pre.get("momenta"):
                mo = pre["momenta"]
                mc._set_momenta(np.array(mo["q"], dtype=np.float64), np.array(mo["cos"], dtype=np.float64),
                                np.array(mo["sin"], dtype=np.float64))
            if pre.get("thermodynamics"):
                hop = pre["thermodynamics"]
                if hop is not True:
                    hop = [np.asarray(hop[b * mc.N * mc.N:(b + 1) * mc.N * mc.N]).reshape((mc.N, mc.N), order="F")
                           for b in range(mc.nb)]
                mc.set_thermodynamics(True, hopping=None if hop is True else hop)
            if pre.get("pair_channels"):
                mc.set_pair_channels({k: v for k, v in pre["pair_channels"]})
            ent = pre.get("entanglement")
            if ent:
                mc.set_entanglement(ent["sites"] if ent["names"] is None else dict(zip(ent["names"], ent["sites"])))
            mc.prepare()  # (the susceptibility layout and two of the binners need a prepared handle)
            ctd = pre.get("current_time_displaced")
            if ctd:
                mc.set_current_time_displaced(ctd["every"])
            if pre["susceptibilities_layout"]:
                mc._section_size("susceptibilities")
            for m, cap in pre["binning"]["sections"].items():
                mc.enable_binning(m, capacity=cap or None)
            if pre["binning"]["user"]:
                mc.user_binner(pre["binning"]["user"][0], pre["binning"]["user"][1] or None)
            mc.set_state(blob)
            if ent:  # the sums go back bit for bit; the import above does not know them
                sums = np.frombuffer(base64.b64decode(ent["sums"]), dtype="<f8").astype(np.float64)
                raw = np.ascontiguousarray(np.concatenate([sums, [float(ent["count"]), float(ent["failures"])]]))
                mc._c(lib().dqmc_set_entanglement_sums(mc._h, dptr(raw), raw.size))
            if ctd:  # and so do these
                raw = np.ascontiguousarray(np.frombuffer(base64.b64decode(ctd["sums"]), dtype="<f8").astype(np.float64))
                if raw.size != mc._current_tau_raw().size:
                    raise _ckpt.CheckpointError("the checkpoint's current_time_displaced sums do not fit its own tables")
                mc._c(lib().dqmc_set_current_time_displaced_sums(mc._h, dptr(raw)))
        except BaseException:
            mc.close()
            raise
        mc.last_sweep = int(pre["last_sweep"])
        mc._mid_sweep = bool(pre["mid_sweep"])
        return mc

    # ---- Green's functions
    def _blocks(self, flat):
        n = self.N
        return [flat[b * n * n:(b + 1) * n * n].reshape((n, n), order="F") for b in range(self.nb)]

    def greens_eff(self, walker=0):
        """mc.s.greens"""
        out = np.zeros(self.nb * self.N * self.N)
        self._c(lib().dqmc_get_greens_eff(self._h, walker, dptr(out)))
        return self._blocks(out)

    def set_greens_eff(self, walker, blocks):
        flat = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, order="F") for b in blocks]))
        self._c(lib().dqmc_set_greens_eff(self._h, walker, dptr(flat)))

    def greens(self, walker=0):
        """greens(mc) (DQMC.jl:711-730)"""
        out = np.zeros(self.nb * self.N * self.N)
        self._c(lib().dqmc_get_greens(self._h, walker, dptr(out)))
        return self._blocks(out)

    def calculate_greens(self, slice_, walker=0):
        """calculate_greens(mc, slice) (stack.jl:422-480)"""
        out = np.zeros(self.nb * self.N * self.N)
        self._c(lib().dqmc_calculate_greens_at(self._h, walker, slice_, dptr(out)))
        return self._blocks(out)

    def wrap_greens(self, slice_, direction):
        self._c(lib().dqmc_wrap_greens(self._h, slice_, direction))

    # ---- sparse checkerboard products (diagnostics)
    def checkerboard_plan(self):
        """dqmc_checkerboard_plan: dict(sparse, kmax, slab_width, lds_bytes); zeros on the dense constants"""
        out = (C.c_int32 * 4)()
        self._c(lib().dqmc_checkerboard_plan(self._h, out))
        return dict(sparse=int(out[0]), kmax=int(out[1]), slab_width=int(out[2]), lds_bytes=int(out[3]))

    def checkerboard_apply(self, which, slice_, X, qscale=None, in_place=False):
        """dqmc_checkerboard_apply: sequence `which` (0 B X, 1 B^-1 X, 2 B' X, 3 X B, 4 X B^-1, 5 X eT, 6 eTinv X) at HS
        slice `slice_` on X [n_walkers * n_blocks, n, n] (unit = walker * n_blocks + block), with the launch the
        propagation issues; qscale [units, n] scales the index that is not mixed; in_place: source = destination"""
        units, n = self.n_walkers * self.nb, self.N
        X = np.asarray(X, dtype=np.float64)
        if X.shape != (units, n, n):
            raise ValueError("X must have shape (n_walkers * n_blocks, n_sites, n_sites)")
        x = _pack(X)
        q = None
        if qscale is not None:
            q = np.ascontiguousarray(qscale, dtype=np.float64)
            if q.shape != (units, n):
                raise ValueError("qscale must have shape (n_walkers * n_blocks, n_sites)")
        out = np.zeros_like(x)
        self._c(lib().dqmc_checkerboard_apply(self._h, int(which), int(slice_), dptr(x), dptr(q) if q is not None else None,
                                              int(bool(in_place)), dptr(out)))
        return _unpack(out, units, n)

    # ---- global moves (include/dqmc_hip.h "global moves")
    @staticmethod
    def _global_kind(kind):
        if kind in _lib.GLOBAL_KINDS:
            return _lib.GLOBAL_KINDS.index(kind)
        return int(kind)  # the engine refuses a number it does not know

    def logdet(self):
        """-> (logabsdet, sign), arrays [n_walkers, n_blocks]: log|det(I + B_M ... B_1)| and its sign per block for the
        current field of every walker, computed from scratch on the device"""
        lad = np.zeros(self.n_walkers * self.nb)
        sg = np.zeros(self.n_walkers * self.nb, dtype=np.int32)
        self._c(lib().dqmc_logdet(self._h, dptr(lad), sg.ctypes.data_as(C.POINTER(C.c_int32))))
        return lad.reshape(self.n_walkers, self.nb), sg.reshape(self.n_walkers, self.nb)

    def global_move(self, kind="site", walker=-1):
        """one global move ("all": conf -> -conf, "site": one site's time line) of `walker` (-1: every walker), accepted
        with the determinant ratio; afterwards the handle is in the state prepare() leaves for the resulting fields"""
        self._c(lib().dqmc_global_move(self._h, self._global_kind(kind), walker))

    def set_global_rate(self, rate, kind="site"):
        """one global move per walker in every sweep whose index is a multiple of `rate` (0: off)"""
        self._c(lib().dqmc_set_global_rate(self._h, rate, self._global_kind(kind)))
        self._gm_set = (int(rate), self._global_kind(kind))

    def global_stats(self, walker=0):
        """-> dict(prop_global, acc_global, moves_drawn) of one walker"""
        g = _lib.GlobalStats()
        self._c(lib().dqmc_get_global_stats(self._h, walker, C.byref(g)))
        return dict(prop_global=g.prop_global, acc_global=g.acc_global, moves_drawn=g.moves_drawn)

    def global_last(self, walker=0):
        """-> dict(p, accepted, site) of the latest global move the walker took part in"""
        p, acc, site = C.c_double(), C.c_int32(), C.c_int32()
        self._c(lib().dqmc_get_global_last(self._h, walker, C.byref(p), C.byref(acc), C.byref(site)))
        return dict(p=p.value, accepted=bool(acc.value), site=site.value)

    # ---- sign reweighting (include/dqmc_hip.h "sign reweighting")
    def set_sign_weighting(self, on=True):
        """from now on every accumulate_* adds s_w O_w, s_w = the sign of walker w's field, and the section's sum of s_w
        (off: the bare samples, the default).  Refused (ERR_STATE) while a section or a binner holds samples:
        reset_accumulators() first.  Read the results with signed(), mean_sign(), sign_sums()."""
        self._c(lib().dqmc_set_sign_weighting(self._h, int(bool(on))))
        if on:
            self._tcov = None  # (the engine turns the tau-tau' covariance off: it is that of the bare samples)

    def sign_weighting(self):
        on = C.c_int32()
        self._c(lib().dqmc_get_sign_weighting(self._h, C.byref(on)))
        return bool(on.value)

    def sign(self):
        """-> int array [n_walkers]: the sign of every walker's current field, the product of logdet()'s signs over the
        blocks (+1 for the attractive model without a launch; 0: a singular or non-finite block)"""
        sg = np.zeros(self.n_walkers, dtype=np.int32)
        self._c(lib().dqmc_get_sign(self._h, sg.ctypes.data_as(C.POINTER(C.c_int32))))
        return sg

    def impose_unit_signs(self, signs):
        """dqmc_impose_unit_signs (diagnostic): the per-unit signs, an int array [n_walkers, n_blocks] of -1, 0 or +1, in
        the place of the ones of the current field, for sign() and every signed accumulate_* until the field changes or
        logdet() recomputes them.  Repulsive model, after prepare().  Take no global move while it is in force."""
        sg = np.asarray(signs)
        if not np.issubdtype(sg.dtype, np.integer) or sg.shape != (self.n_walkers, self.nb):
            raise ValueError("signs must be an int array of shape (n_walkers, n_blocks) = (%d, %d)" % (self.n_walkers, self.nb))
        sg = np.ascontiguousarray(sg, dtype=np.int32)
        self._c(lib().dqmc_impose_unit_signs(self._h, sg.ctypes.data_as(C.POINTER(C.c_int32))))

    def sign_failures(self):
        """-> int array [n_walkers]: samples left out of the signed sums because the walker's sign came out 0"""
        out = np.zeros(self.n_walkers, dtype=np.int64)
        self._c(lib().dqmc_get_sign_failures(self._h, i64ptr(out)))
        return out

    _SIGN_ORDER = ("greens", "correlations", "pairing", "susceptibilities", "time_displaced")  # DQMC_RED_* order
    _NE = len(_lib.THERMO_FIELDS)  # DQMC_THERMO_ELEMENTS: the thermodynamics section is [_NE sums][sum of s][count]

    def sign_sums(self, reduced=False):
        """-> {section: sum of s over its samples} (the DQMC_RED_SIGN section; `reduced`: of the last reduction)"""
        return dict(zip(self._SIGN_ORDER, self._section("sign", reduced=reduced)))

    def mean_sign(self, which="greens"):
        """<s> of the samples of one section: its sum of signs over its sample count"""
        if which == "thermodynamics":  # (the section carries its own sum of signs)
            raw = self._section(which)
            return raw[-2] / raw[-1]
        if which not in self._SIGN_ORDER:
            raise ValueError("unknown section %r" % (which,))
        return self.sign_sums()[which] / self._section(which)[-1]

    def signed(self, which="greens"):
        """<O s> / <s> of a section measured with sign weighting on: the section's usual dict (greens -> G, G2,
        occupation; correlations; pairing -> PC; susceptibilities; time_displaced), every sum divided by the section's
        sum of signs instead of its sample count; plus count, sign_sum and mean_sign.  With the section's binner on every
        field X also comes with X_std_error: the jackknife over the walkers of the ratio (jackknife_ratio), from each
        walker's level-0 sums of s x and of s; that needs at least two walkers.  ValueError when the sum of signs is 0."""
        if which not in self._SIGN_ORDER + ("thermodynamics",):
            raise ValueError("unknown section %r" % (which,))
        if not self.sign_weighting():
            raise _lib.DQMCError(_lib.ERR_STATE, "signed(): sign weighting is off (set_sign_weighting)")
        raw = self._section(which)
        cnt, S = raw[-1], (raw[-2] if which == "thermodynamics" else self.sign_sums()[which])
        if S == 0:
            raise ValueError("signed(%r): the sum of signs is 0 over %d samples: <O s> / <s> is undefined" % (which, cnt))
        raw = raw.copy()
        raw[-1] = S
        if which == "thermodynamics":  # (thermodynamics() divides by the sum of signs itself and adds the jackknife errors)
            return self.thermodynamics()
        if which == "greens":
            res = self.unpack_accumulators(raw)
        elif which == "correlations":
            res = self.correlations(_raw=raw)
        elif which == "pairing":
            res = dict(PC=self.pairing(_raw=raw)[0])
        elif which == "susceptibilities":
            res = self.susceptibilities(_raw=raw)
        else:
            res = self.time_displaced(_raw=raw)
        res.update(count=cnt, sign_sum=S, mean_sign=S / cnt)
        if self._binning_enabled(which):
            sx, sg = self.signed_walker_sums(which)
            _, err = jackknife_ratio(sx, sg)
            for name, v in self._bin_shape(which, err).items():
                res[name + "_std_error"] = v
        return res

    def signed_walker_sums(self, which):
        """-> (sx [n_walkers, E], s [n_walkers]): level 0 of every walker's binners of a section, the sums of s x in the
        section's element order, and of its sign binner, the sums of s"""
        if which == "thermodynamics":  # one binner: the sample ends with s
            lv0 = np.stack([self.binner_level(which, w, 0)[0] for w in range(self.n_walkers)])
            return lv0[:, :self._NE], lv0[:, self._NE]
        bid = _lib.BIN_SIGN + self._SIGN_ORDER.index(which)
        sx = np.stack([self.binner_level(which, w, 0)[0] for w in range(self.n_walkers)])
        sg = np.zeros(self.n_walkers)
        for w in range(self.n_walkers):
            x = np.zeros(1)
            self._c(lib().dqmc_binner_get_level(self._h, bid, w, 0, dptr(x), None, None))
            sg[w] = x[0]
        return sx, sg

    # ---- analysis / measurement sums
    def analysis(self, walker=0):
        st = _lib.Stats()
        self._c(lib().dqmc_get_stats(self._h, walker, C.byref(st)))
        g = _lib.GlobalStats()
        self._c(lib().dqmc_get_global_stats(self._h, walker, C.byref(g)))
        return DQMCAnalysis(st, g)

    def analysis_sum(self):
        """(prop_local, acc_local) summed over the walkers of this handle"""
        tot = [0, 0]
        for w in range(self.n_walkers):
            a = self.analysis(w)
            tot[0] += a.prop_local
            tot[1] += a.acc_local
        return tuple(tot)

    def accumulate_greens(self):
        self._c(lib().dqmc_accumulate_greens(self._h))

    # ---- measurement reduction over ranks (inside the library: RCCL all-reduce on the engine's stream)
    def reduce(self, comm=None):
        """dqmc_reduce: every accumulator and the DQMCAnalysis counters summed (max / min for the magnitude
        statistics) over all ranks of `comm` (a sharding.Communicator, or None for this handle alone)"""
        self._c(lib().dqmc_reduce(self._h, comm.handle if comm is not None else None))

    def reduced(self, which="greens"):
        """dqmc_get_reduced: the global sums of the last reduction (the handle's own accumulators keep the local sums);
        `which` = greens | correlations | pairing | susceptibilities | time_displaced | sign (the sums of signs, packed
        only with sign weighting on) | thermodynamics, layouts as the local getters"""
        return self._section(which, reduced=True)

    def reduced_analysis(self):
        st = _lib.Stats()
        self._c(lib().dqmc_get_reduced_stats(self._h, C.byref(st)))
        return DQMCAnalysis(st)

    def reduce_size(self):
        n = C.c_size_t()
        self._c(lib().dqmc_reduce_size(self._h, C.byref(n)))
        return n.value

    def reduce_export(self):
        """packed [sums | 2 maxima | 2 minima] for a host-side collective"""
        out = np.zeros(self.reduce_size())
        self._c(lib().dqmc_reduce_export(self._h, dptr(out)))
        return out

    def reduce_import(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.float64)
        self._c(lib().dqmc_reduce_import(self._h, dptr(buf)))

    def reduce_host(self, dist):
        """the same reduction through a torch.distributed process group on host buffers (gloo): what a host with
        its own collective (MPI from Julia) does around dqmc_reduce_export / dqmc_reduce_import"""
        import torch
        buf = torch.from_numpy(self.reduce_export())
        n = buf.numel() - 4
        if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(buf[:n], op=dist.ReduceOp.SUM)
            dist.all_reduce(buf[n:n + 2], op=dist.ReduceOp.MAX)
            dist.all_reduce(buf[n + 2:], op=dist.ReduceOp.MIN)
        self.reduce_import(buf.numpy())

    def reset_accumulators(self):
        self._c(lib().dqmc_reset_accumulators(self._h))

    # the accumulator sections: name -> (DQMC_RED_* index, size function, local getter)
    _SECTIONS = {"greens": (0, "dqmc_accumulator_size", "dqmc_get_accumulators"),
                 "correlations": (1, "dqmc_correlations_size", "dqmc_get_correlations"),
                 "pairing": (2, "dqmc_pairing_size", "dqmc_get_pairing"),
                 "susceptibilities": (3, "dqmc_susceptibilities_size", "dqmc_get_susceptibilities"),
                 "time_displaced": (_lib.RED_TIME_DISPLACED, "dqmc_time_displaced_size", "dqmc_get_time_displaced"),
                 "sign": (_lib.RED_SIGN, "dqmc_sign_sums_size", "dqmc_get_sign_sums"),
                 "thermodynamics": (_lib.RED_THERMODYNAMICS, "dqmc_thermodynamics_size", "dqmc_get_thermodynamics")}

    def _section_size(self, which):
        n = C.c_size_t()
        self._c(getattr(lib(), self._SECTIONS[which][1])(self._h, C.byref(n)))
        if which == "susceptibilities":  # (dqmc_susceptibilities_size lays the section out)
            self._sus_layout = True
        return n.value

    def _section(self, which, reduced=False):
        """the raw sums of a section: ask its size, allocate, fetch the local sums or those of the last reduction"""
        idx, _, getter = self._SECTIONS[which]
        out = np.zeros(self._section_size(which))
        if reduced:
            self._c(lib().dqmc_get_reduced(self._h, idx, dptr(out)))
        else:
            self._c(getattr(lib(), getter)(self._h, dptr(out)))
        return out

    def accumulator_size(self):
        return self._section_size("greens")

    def accumulators(self):
        return self._section("greens")

    def export_accumulators(self, device_ptr):
        self._c(lib().dqmc_export_accumulators(self._h, C.c_void_p(device_ptr)))

    def unpack_accumulators(self, acc):
        """-> dict(G_mean, G2_mean, occupation_mean, count) per block"""
        n, B = self.N, self.nb
        cnt = acc[-1]
        G = [acc[b * n * n:(b + 1) * n * n].reshape((n, n), order="F") / cnt for b in range(B)]
        G2 = [acc[(B + b) * n * n:(B + b + 1) * n * n].reshape((n, n), order="F") / cnt for b in range(B)]
        occ = [acc[2 * B * n * n + b * n:2 * B * n * n + (b + 1) * n] / cnt for b in range(B)]
        return dict(G=G, G2=G2, occupation=occ, count=cnt)

    # ---- error bars: per-walker logarithmic binning on the device (include/dqmc_hip.h "error bars")
    @staticmethod
    def _bin(which):
        if which == "time_displaced":  # DQMC_BIN_TIME_DISPLACED, an enum of its own
            return _lib.BIN_TIME_DISPLACED
        if which in _lib.BIN_MOMENTUM:
            return _lib.BIN_MOMENTUM[which]
        if which == "thermodynamics":
            return _lib.BIN_THERMODYNAMICS
        if which in _lib.BIN_RESPONSE:
            return _lib.BIN_RESPONSE[which]
        if which not in _lib.BIN_SECTIONS:
            raise ValueError("unknown binner section %r" % (which,))
        return _lib.BIN_SECTIONS.index(which)

    @staticmethod
    def _capacity(capacity):
        if capacity is None:
            return 0  # the library's default, 100000
        if int(capacity) < 1:
            raise _lib.DQMCError(_lib.ERR_INVALID, "binner capacity must be at least 1")
        return int(capacity)

    def enable_binning(self, which=("greens",), capacity=None):
        """a LogBinner (capacity: default 100000) per walker and element of the given measurement sections; from then
        on every accumulate_* of such a section also pushes each walker's sample.  Costs
        (3 L - 1) * n_walkers * n_elements doubles of device memory per section, L = ceil(log2(capacity + 1))."""
        cap = self._capacity(capacity)
        for m in ((which,) if isinstance(which, str) else which):
            if m == "user":
                raise ValueError("the user binner is made by user_binner(n_elements)")
            self._c(lib().dqmc_binner_enable(self._h, self._bin(m), cap))
            self._binned = getattr(self, "_binned", set()) | {m}
            self._bin_caps[m] = cap
            if m in ("susceptibilities", "response_pairing_susceptibility", "response_current"):  # (its binner lays the section out)
                self._sus_layout = True

    def _binning_enabled(self, which):
        return which in getattr(self, "_binned", ())

    def user_binner(self, n_elements, capacity=None):
        """a binner over `n_elements` samples per walker that the caller computes on the device"""
        self._c(lib().dqmc_binner_user_create(self._h, int(n_elements), self._capacity(capacity)))
        self._user_bin = (int(n_elements), self._capacity(capacity))

    def user_push(self, samples):
        """push one sample [n_walkers, n_elements]: a contiguous float64 device tensor (torch) or a device address"""
        if hasattr(samples, "data_ptr"):
            E = self.binner_size("user")[0]
            if str(samples.dtype) != "torch.float64" or not samples.is_contiguous() or not samples.is_cuda \
                    or samples.numel() != self.n_walkers * E:
                raise ValueError("samples must be a contiguous float64 device tensor of n_walkers x %d" % E)
            import torch
            torch.cuda.current_stream(samples.device).synchronize()  # the engine reads it on its own stream
            samples = samples.data_ptr()
        self._c(lib().dqmc_binner_user_push(self._h, C.c_void_p(samples)))

    def binner_size(self, which="greens"):
        """-> (elements per walker, levels, pushes so far)"""
        n, L, T = C.c_size_t(), C.c_int32(), C.c_int64()
        self._c(lib().dqmc_binner_size(self._h, self._bin(which), C.byref(n), C.byref(L), C.byref(T)))
        return n.value, L.value, T.value

    def binner_reliable_level(self, which="greens"):
        lv = C.c_int32()
        self._c(lib().dqmc_binner_reliable_level(self._h, self._bin(which), C.byref(lv)))
        return lv.value

    def binner_level(self, which, walker, level):
        """-> (x_sum, x2_sum, count) of one level of one walker's binners (inspection)"""
        E = self.binner_size(which)[0]
        xs, x2, cnt = np.zeros(E), np.zeros(E), C.c_int64()
        self._c(lib().dqmc_binner_get_level(self._h, self._bin(which), walker, level, dptr(xs), dptr(x2), C.byref(cnt)))
        return xs, x2, cnt.value

    def binned_raw(self, which="greens", level=None):
        """-> dict of flat arrays in the section's element order: mean, std_error (binning, at `level` or the reliable
        one), std_error_walkers (cross-walker), tau; count (pushes per walker) and reliable_level"""
        E, _, T = self.binner_size(which)
        out = {k: np.zeros(E) for k in ("mean", "std_error", "std_error_walkers", "tau")}
        self._c(lib().dqmc_binner_finish(self._h, self._bin(which), -1 if level is None else level,
                                         *[dptr(out[k]) for k in ("mean", "std_error", "std_error_walkers", "tau")]))
        out["count"] = T
        out["reliable_level"] = self.binner_reliable_level(which)
        return out

    def _bin_fields(self, which):
        """[(name, offset, size, shape or None)] of a section, in the layouts of include/dqmc_hip.h"""
        n, B = self.N, self.nb
        nd, K, Kcc = getattr(self, "_ndirs", 0), getattr(self, "_K", 0), getattr(self, "_Kcc", 0)
        if which == "greens":
            sizes = [("G", B * n * n, None), ("occupation", B * n, None)]
        elif which == "correlations":
            sizes = [(k, nd, None) for k in ("CDC", "SDCx", "SDCy", "SDCz")] + [(k, n, None) for k in ("Mx", "My", "Mz")]
        elif which == "pairing":
            sizes = [("PC", nd * K * K, (nd, K, K))]
        elif which == "susceptibilities":
            sizes = [(k, nd, None) for k in ("CDS", "SDSx", "SDSy", "SDSz")]
            if K:
                sizes.append(("PS", nd * K * K, (nd, K, K)))
            if Kcc:
                sizes.append(("CCS", nd * Kcc, (nd, Kcc)))
        elif which == "time_displaced":  # [b][r][d] / [r][d], d fastest: C order
            p = self.time_displaced_plan()
            sizes = []
            if p["what"] & _lib.TD_GREENS:
                sizes += [(k, B * p["rows"] * nd, (B, p["rows"], nd)) for k in ("Gl0", "G0l")]
            if p["what"] & _lib.TD_DENSITY:
                sizes += [(k, p["rows"] * nd, (p["rows"], nd)) for k in ("CDC", "SDCx", "SDCy", "SDCz")]
        elif which in _lib.BIN_MOMENTUM:  # q fastest: C order
            nq = 0 if self._mom is None else self._mom[0].shape[0]
            if which == "momentum_correlations":
                sizes = [(k, nq, None) for k in ("Sc", "Sx", "Sy", "Sz")]
            elif which == "momentum_susceptibilities":
                sizes = [(k, nq, None) for k in ("chi_c", "chi_x", "chi_y", "chi_z")]
            else:
                p = self.time_displaced_plan()
                sizes = []
                if p["what"] & _lib.TD_GREENS:
                    sizes += [(k, B * p["rows"] * nq, (B, p["rows"], nq)) for k in ("Gl0_C", "Gl0_S", "G0l_C", "G0l_S")]
                if p["what"] & _lib.TD_DENSITY:
                    sizes += [(k, p["rows"] * nq, (p["rows"], nq)) for k in ("CDCk", "SDCxk", "SDCyk", "SDCzk")]
            if self.sign_weighting():
                sizes.append(("s", 1, None))
        elif which == "thermodynamics":
            sizes = [(k, 1, None) for k in _lib.THERMO_FIELDS]
            if self.sign_weighting():
                sizes.append(("s", 1, None))
        else:
            sizes = [("x", self.binner_size("user")[0], None)]
        out, off = [], 0
        for name, size, shape in sizes:
            out.append((name, off, size, shape))
            off += size
        return out

    def _bin_shape(self, which, flat):
        """one flat section vector -> {field: array shaped like the existing getters}"""
        n, B, res = self.N, self.nb, {}
        for name, off, size, shape in self._bin_fields(which):
            v = flat[off:off + size]
            if name == "G":
                v = self._blocks(v)
            elif name == "occupation":
                v = [v[b * n:(b + 1) * n] for b in range(B)]
            elif which in ("time_displaced", "momentum_time_displaced"):
                v = v.reshape(shape)
            elif which == "thermodynamics":  # scalars
                v = v[0]
            elif shape is not None:
                v = v.reshape(shape, order="F")
            res[name] = v
        return res

    def _bin_dict(self, which, raw):
        res = {}
        for key, suffix in (("mean", ""), ("std_error", "_std_error"), ("std_error_walkers", "_std_error_walkers"),
                            ("tau", "_tau")):
            for name, v in self._bin_shape(which, raw[key]).items():
                res[name + suffix] = v
        return res

    def binned(self, which="greens", level=None):
        """mean(m), std_error(m), tau(m) of a binned section over the walkers of this handle, shaped like the existing
        getters: greens -> G, occupation (lists of blocks); correlations -> CDC, SDCx, SDCy, SDCz, Mx, My, Mz; pairing
        -> PC[dir12, dir1, dir2]; susceptibilities -> CDS, SDSx, SDSy, SDSz, PS, CCS; user -> x.  Every field X comes with
        X_std_error (binning error at `level`, default the reliable level), X_std_error_walkers (the cross-walker
        error, independent of the binning) and X_tau; plus count (samples per walker) and reliable_level."""
        if which in _lib.BIN_MOMENTUM or which == "thermodynamics":
            return self._binned_momentum(which, level)
        if which in _lib.BIN_RESPONSE:
            return self._binned_response(which, level)
        raw = self.binned_raw(which, level)
        res = self._bin_dict(which, raw)
        if which == "time_displaced":
            res["tau"] = self._td_tau()
        res["count"] = raw["count"]
        res["reliable_level"] = raw["reliable_level"]
        return res

    def binner_moments(self, which="greens", level=None, out=None):
        """dqmc_binner_export_moments: the additive moments [sum mean_w][sum mean_w^2][sum varN_w(level)][sum varN_w(0)]
        [W] as a float64 device tensor of 4 E + 1 entries (`out`, or a new torch tensor on this handle's device).  A
        multi-rank host all-reduces (sum) the whole tensor and hands it to finish_moments."""
        E = self.binner_size(which)[0]
        if out is None:
            import torch
            out = torch.empty(4 * E + 1, dtype=torch.float64, device="cuda:%d" % self._device_id)
        if out.numel() != 4 * E + 1 or not out.is_contiguous() or str(out.dtype) != "torch.float64":
            raise ValueError("out must be a contiguous float64 device tensor of %d entries" % (4 * E + 1))
        self._c(lib().dqmc_binner_export_moments(self._h, self._bin(which), -1 if level is None else level,
                                                 C.c_void_p(out.data_ptr())))
        return out

    def finish_moments(self, buf, which=None):
        """finish_moments(buf), and with `which` the result shaped like binned(which)"""
        raw = finish_moments(buf)
        if which is None:
            return raw
        res = self._bin_dict(which, raw)
        res["n_walkers"] = raw["n_walkers"]
        return res

    # ---- equal-time correlations (charge_density_correlation, spin_density_correlation, magnetization)
    def set_pair_directions(self, iterator):
        """hand the EachSitePairByDistance table of the lattice to the device"""
        self._set_pair_directions(iterator.dir_of, iterator.ndirections())
        self._dirs = np.array(iterator.directions, dtype=np.float64)  # r_d of every direction: set_momenta's tables

    def _set_pair_directions(self, dir_of, n_dirs):
        tab = np.asfortranarray(np.asarray(dir_of).astype(np.int32))  # [src, trg] -> dir_of[src + n*trg]
        self._ndirs = int(n_dirs)
        self._c(lib().dqmc_set_pair_directions(self._h, tab.ctypes.data_as(C.POINTER(C.c_int32)), self._ndirs))
        self._dirs = None
        self._momenta_dropped()  # (the engine turns momenta off with the old directions)
        self._tables["pair_directions"] = (np.array(tab, dtype=np.int32), self._ndirs)

    def accumulate_correlations(self):
        self._c(lib().dqmc_accumulate_correlations(self._h))

    def correlations_raw(self):
        """the raw sums [cdc][sdc_x][sdc_y][sdc_z][mx][my][mz][count] (layout of include/dqmc_hip.h)"""
        return self._section("correlations")

    def correlations(self, _raw=None):
        """-> dict of means: CDC, SDCx, SDCy, SDCz per direction; Mx, My, Mz per site; count"""
        out = self._section("correlations") if _raw is None else _raw
        nd, N, cnt = self._ndirs, self.N, out[-1]
        names = ["CDC", "SDCx", "SDCy", "SDCz"]
        res = {k: out[i * nd:(i + 1) * nd] / cnt for i, k in enumerate(names)}
        for i, k in enumerate(["Mx", "My", "Mz"]):
            res[k] = out[4 * nd + i * N:4 * nd + (i + 1) * N] / cnt
        res["count"] = cnt
        return res

    # ---- pairing_correlation (measurements.jl:199-214) over EachLocalQuadByDistance{K}
    def set_local_targets(self, iterator):
        """hand the (dir, trg) lists of EachLocalQuadByDistance{K} to the device; the pair
        directions of the same lattice are set with it"""
        self.set_pair_directions(iterator.pairs_by_dir)
        self._set_local_targets(iterator.trg_of, iterator.K)

    def _set_local_targets(self, trg_of, K):
        tab = np.asfortranarray(np.asarray(trg_of).astype(np.int32))  # [src, k] -> trg_of[src + n*k]
        self._K = int(K)
        self._channels = None  # (the engine turns the pair channels off with the old targets)
        for k in ("response_pairing", "response_pairing_susceptibility"):
            self._binner_dropped(k)
        self._c(lib().dqmc_set_local_targets(self._h, tab.ctypes.data_as(C.POINTER(C.c_int32)), self._K))
        self._tables["local_targets"] = (np.array(tab, dtype=np.int32), self._K)

    def accumulate_pairing(self):
        self._c(lib().dqmc_accumulate_pairing(self._h))

    def pairing(self, _raw=None):
        """-> (mean of output[dir12, dir1, dir2] as pushed by finish!, sample count)"""
        out = self._section("pairing") if _raw is None else _raw
        cnt = out[-1]
        return out[:-1].reshape((self._ndirs, self._K, self._K), order="F") / cnt, cnt

    # ---- unequal-time Green's functions (src/flavors/DQMC/unequal_time_stack.jl)
    def ut_build_stack(self):
        """build_stack(mc, mc.ut_stack)"""
        self._c(lib().dqmc_ut_build_stack(self._h))

    def ut_stack(self, which, idx, walker=0):
        """(U, D, T) blocks of slot idx (0-based) of the forward / backward / inverse stack"""
        sel = {"forward": 0, "backward": 1, "inverse": 2}[which]
        U = np.zeros(self.nb * self.N * self.N); T = np.zeros_like(U); D = np.zeros(self.nb * self.N)
        self._c(lib().dqmc_ut_get_stack(self._h, walker, sel, idx, dptr(U), dptr(D), dptr(T)))
        return self._blocks(U), [D[b * self.N:(b + 1) * self.N] for b in range(self.nb)], self._blocks(T)

    def _ut_result(self, which, walker):
        out = np.zeros(self.nb * self.N * self.N)
        self._c(lib().dqmc_ut_get(self._h, walker, which, dptr(out)))
        return self._blocks(out)

    def calculate_greens_kl(self, slice1, slice2, walker=0):
        """calculate_greens(mc, slice1, slice2): the effective G(slice1 <- slice2)"""
        self._c(lib().dqmc_ut_greens(self._h, slice1, slice2, 1))
        return self._ut_result(0, walker)

    def greens_kl(self, slice1, slice2, walker=None):
        """greens(mc, k, l) = <c_i(k dtau) c_j^dagger(l dtau)>; walker=None returns every walker"""
        self._c(lib().dqmc_ut_greens(self._h, slice1, slice2, 0))
        if walker is None:
            return [self._ut_result(0, w) for w in range(self.n_walkers)]
        return self._ut_result(0, walker)

    def greens_iterator(self, l=0, recalculate=None, walker=0):
        """GreensIterator(mc, :, l, recalculate): yields G(k <- l) for k = l..slices"""
        recalculate = 4 * self.p.safe_mult if recalculate is None else recalculate
        self._c(lib().dqmc_greens_iterator_begin(self._h, l, recalculate))
        yield self._ut_result(0, walker)
        k = C.c_int32()
        while True:
            self._c(lib().dqmc_greens_iterator_next(self._h, C.byref(k)))
            if k.value < 0:
                return
            yield self._ut_result(0, walker)

    def combined_greens_iterator(self, recalculate=None, walker=0):
        """CombinedGreensIterator(mc, recalculate): yields (G0l, Gl0, Gll) for l = 1..slices"""
        recalculate = 4 * self.p.safe_mult if recalculate is None else recalculate
        self._c(lib().dqmc_combined_iterator_begin(self._h, recalculate))
        l = C.c_int32()
        while True:
            self._c(lib().dqmc_combined_iterator_next(self._h, C.byref(l)))
            if l.value < 0:
                return
            yield tuple(self._ut_result(i, walker) for i in range(3))

    def accumulate_susceptibilities(self, recalculate=None):
        """charge_density_/spin_density_/pairing_susceptibility: one pass of the CombinedGreensIterator
        with the packed kernels summed on the device"""
        recalculate = 4 * self.p.safe_mult if recalculate is None else recalculate
        self._c(lib().dqmc_accumulate_susceptibilities(self._h, recalculate))
        self._sus_layout = True

    def susceptibilities(self, _raw=None):
        """-> dict of means: CDS, SDSx, SDSy, SDSz per direction, PS[dir12, dir1, dir2] if local targets
        are set, CCS[dir12, dir_ii] if current targets are set, count"""
        out = self._section("susceptibilities") if _raw is None else _raw
        nd, cnt = self._ndirs, out[-1]
        res = {k: out[i * nd:(i + 1) * nd] / cnt for i, k in enumerate(["CDS", "SDSx", "SDSy", "SDSz"])}
        K = getattr(self, "_K", 0)
        if K:
            res["PS"] = out[4 * nd:4 * nd + nd * K * K].reshape((nd, K, K), order="F") / cnt
        Kcc = getattr(self, "_Kcc", 0)
        if Kcc:
            off = 4 * nd + nd * K * K
            res["CCS"] = out[off:off + nd * Kcc].reshape((nd, Kcc), order="F") / cnt
        res["count"] = cnt
        return res

    # ---- time-displaced recording (include/dqmc_hip.h): G(r, tau) and the tau-resolved charge / spin correlations
    def set_time_displaced(self, every=1, what=("greens", "density")):
        """from now on every accumulate_susceptibilities pass also records rows at l = 0, every, ..., slices (every = 0:
        off).  `what`: "greens" (Gl0, G0l summed per direction) and / or "density" (CDC, SDCx, SDCy, SDCz), or the
        DQMC_TD_* mask itself.  Needs set_pair_directions; starts the recorded sums at zero."""
        if isinstance(what, str):
            what = (what,)
        if not isinstance(what, int):
            bits = {"greens": _lib.TD_GREENS, "density": _lib.TD_DENSITY}
            for k in what:
                if k not in bits:
                    raise ValueError("unknown time-displaced part %r" % (k,))
            what = sum(bits[k] for k in set(what))
        self._c(lib().dqmc_set_time_displaced(self._h, int(every), int(what)))
        self._td_args = (int(every), int(what)) if int(every) else None
        self._binner_dropped("momentum_time_displaced")  # (the engine disables it: enable it again)
        self._tcov = None  # (and the tau-tau' covariance)

    def time_displaced_plan(self):
        """-> dict(rows, every, what, fast): fast = 1: the Green's rows take the one-lane-per-direction kernel of a Latin
        square table (the Bravais lattices); 2: its injective form over a table with holes (every source and every target
        meets a direction at most once, n_dirs <= 2 n: HoneycombLattice); 0: the pair lists (all zero when recording is
        off)"""
        out = (C.c_int32 * 4)()
        self._c(lib().dqmc_time_displaced_plan(self._h, out))
        return dict(zip(("rows", "every", "what", "fast"), (int(v) for v in out)))

    def time_displaced_size(self):
        return self._section_size("time_displaced")

    def time_displaced_raw(self):
        """the accumulator as the device holds it: the sums in the layout of include/dqmc_hip.h, then the sample count"""
        return self._section("time_displaced")

    def _td_tau(self):
        p = self.time_displaced_plan()
        return np.arange(p["rows"]) * p["every"] * self.p.delta_tau

    def time_displaced(self, _raw=None):
        """-> dict of means over the samples: tau [R]; Gl0, G0l [n_blocks, R, n_dirs]; CDC, SDCx, SDCy, SDCz [R, n_dirs]
        (whichever are recorded); count"""
        raw = self.time_displaced_raw() if _raw is None else _raw
        cnt = raw[-1]
        res = {"tau": self._td_tau()}
        for name, v in self._bin_shape("time_displaced", raw[:-1]).items():
            res[name] = v / cnt
        res["count"] = cnt
        return res

    # ---- momentum-space observables (include/dqmc_hip.h): S(q), chi(q), G(k, tau), n(k)
    def _binner_dropped(self, which):
        self._binned = getattr(self, "_binned", set()) - {which}
        self._bin_caps.pop(which, None)

    def _momenta_dropped(self):
        self._mom = None
        self._ctd = 0  # (the engine turns the imaginary-time current recording off with the tables)
        self._tcov = None  # (and the tau-tau' covariance of the momentum sample)
        for k in tuple(_lib.BIN_MOMENTUM) + tuple(_lib.BIN_RESPONSE):  # (the response binners use the tables)
            self._binner_dropped(k)

    def set_momenta(self, qs="all", iterator=None):
        """the wave vectors of the momentum-space observables: "all" (momentum_grid of the lattice), integer labels
        [n_q, dim] into that grid (an integer array or tuples: (L/2, L/2) is (pi, pi) on a square lattice), or cartesian
        vectors [n_q, dim] (a float array); None or an empty list turns them off.  The phase tables C[d, q] = cos(q . r_d),
        S[d, q] = sin(q . r_d) are built from the `directions` of the iterator given to set_pair_directions (on the
        _set_pair_directions path, which has none, pass the iterator here).  Means need nothing more:
        structure_factors(), static_susceptibilities(), momentum_time_displaced(); error bars come from the momentum
        binners: enable_binning(("momentum_correlations", ...)), binned(...).  Disables the momentum binners."""
        from .lattices import momentum_grid
        if iterator is not None:
            self._dirs = np.array(iterator.directions, dtype=np.float64)
        if qs is None or (not isinstance(qs, str) and len(qs) == 0):
            self._c(lib().dqmc_set_momenta(self._h, 0, None, None))
            self._momenta_dropped()
            return
        if self._dirs is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "set_momenta: call set_pair_directions(iterator) first, or pass the iterator")
        if self._dirs.shape[0] != getattr(self, "_ndirs", 0):
            raise ValueError("set_momenta: the iterator has %d directions, the engine's table %d"
                             % (self._dirs.shape[0], getattr(self, "_ndirs", 0)))
        dim = self._dirs.shape[1]
        if isinstance(qs, str):
            if qs != "all":
                raise ValueError("qs must be 'all', integer labels or cartesian vectors")
            q = momentum_grid(self.model.l)[0]
        else:
            a = np.asarray(qs)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2 or a.shape[1] != dim:
                raise ValueError("qs must have shape [n_q, %d]" % dim)
            if np.issubdtype(a.dtype, np.integer):
                A = np.array(_lat_vectors(self.model.l), dtype=np.float64)
                q = a.astype(np.float64) @ (2.0 * np.pi * np.linalg.inv(A).T)
            else:
                q = a.astype(np.float64)
        phase = self._dirs @ q.T  # [n_dirs, n_q]
        self._set_momenta(q, np.cos(phase).reshape(-1, order="F"), np.sin(phase).reshape(-1, order="F"))

    def _set_momenta(self, q, cos_tab, sin_tab):
        """the engine call: tables [n_dirs x n_q] flat, d fastest"""
        q = np.ascontiguousarray(q, dtype=np.float64)
        cos_tab, sin_tab = np.ascontiguousarray(cos_tab, dtype=np.float64), np.ascontiguousarray(sin_tab, dtype=np.float64)
        nd = getattr(self, "_ndirs", 0)
        if cos_tab.size != nd * q.shape[0] or sin_tab.size != cos_tab.size:
            raise ValueError("the phase tables must hold n_dirs x n_q = %d x %d entries" % (nd, q.shape[0]))
        self._c(lib().dqmc_set_momenta(self._h, q.shape[0], dptr(cos_tab), dptr(sin_tab)))
        self._momenta_dropped()
        self._mom = (q, cos_tab, sin_tab)

    def momenta(self):
        """-> the wave vectors [n_q, dim] of set_momenta (cartesian), or None"""
        return None if self._mom is None else self._mom[0].copy()

    def momenta_plan(self):
        """-> dict(n_q, n_dirs, tile_rows, tile_cols) of the engine, all zero when momenta are off"""
        out = (C.c_int32 * 4)()
        self._c(lib().dqmc_momenta_plan(self._h, out))
        return dict(zip(("n_q", "n_dirs", "tile_rows", "tile_cols"), (int(v) for v in out)))

    def _phase_tables(self):
        if self._mom is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_momenta first")
        q, c, s = self._mom
        return c.reshape((self._ndirs, q.shape[0]), order="F"), s.reshape((self._ndirs, q.shape[0]), order="F")

    def _means(self, which):
        return self.signed(which) if self.sign_weighting() else getattr(self, which)()

    def structure_factors(self):
        """-> dict(Sc, Sx, Sy, Sz [n_q], count): sum_d cos(q . r_d) X[d] of the means CDC, SDCx, SDCy, SDCz - a host
        transform of the accumulated sums (of signed("correlations") with sign weighting on)"""
        Ct, _ = self._phase_tables()
        m = self._means("correlations")
        res = {k: m[src] @ Ct for k, src in (("Sc", "CDC"), ("Sx", "SDCx"), ("Sy", "SDCy"), ("Sz", "SDCz"))}
        res["count"] = m["count"]
        return res

    def static_susceptibilities(self):
        """-> dict(chi_c, chi_x, chi_y, chi_z [n_q], count): the same transform of the means CDS, SDSx, SDSy, SDSz"""
        Ct, _ = self._phase_tables()
        m = self._means("susceptibilities")
        res = {k: m[src] @ Ct for k, src in (("chi_c", "CDS"), ("chi_x", "SDSx"), ("chi_y", "SDSy"), ("chi_z", "SDSz"))}
        res["count"] = m["count"]
        return res

    def momentum_time_displaced(self):
        """-> dict of the transforms of time_displaced(): Gk_l0, Gk_0l (complex [n_blocks, R, n_q]: sum_d e^{-i q . r_d}
        X[d]) and nk = 1 - Re Gk_l0[:, 0, :] if the Green's rows are recorded, CDCk, SDCxk, SDCyk, SDCzk [R, n_q] (cosine
        part) if the density rows are; tau, count.

        On a lattice with a basis (HoneycombLattice) Gk_l0 and Gk_0l are the sublattice trace G_AA(k) + G_BB(k), formed
        from the same-sublattice directions only, and Gk_l0_AB / Gk_0l_AB the complex off-diagonal part G_AB(k), formed
        from the A -> B directions only (source on A; the B -> A directions hold its conjugate partner G_BA).
        Normalisation: the device divides every direction's sum by n = 2 L^2, but a honeycomb direction class has one
        pair per cell, n / 2 of them, so the host multiplies by 2: G_ab(k) = (1 / L^2) sum over the cells of both sites
        e^{-i k . (r_i - r_j)} G[i, j], i on a, j on b, with the true site positions.  nk = 2 - Re tr G(k) at tau = 0 is
        the occupation of both bands together.  The density transforms CDCk .. are the full sums over all directions,
        sum_d cos(q . r_d) X[d] = (1 / n) sum_ij, as on every lattice."""
        if self._basis_classes() is not None:
            return self._momentum_time_displaced_basis()
        Ct, St = self._phase_tables()
        m = self._means("time_displaced")
        res = {"tau": m["tau"], "count": m["count"]}
        for k, src in (("Gk_l0", "Gl0"), ("Gk_0l", "G0l")):
            if src in m:
                res[k] = m[src] @ Ct - 1j * (m[src] @ St)
        if "Gk_l0" in res:
            res["nk"] = 1.0 - res["Gk_l0"][:, 0, :].real
        for src in ("CDC", "SDCx", "SDCy", "SDCz"):
            if src in m:
                res[src + "k"] = m[src] @ Ct
        return res

    # ---- lattices with a basis: direction classes, sublattice-resolved G(k), staggered (q = 0, signed) transforms
    def _basis_classes(self):
        """None on a lattice without a `sublattice` array; else [n_dirs] of 0 (same sublattice), 1 (source on sublattice
        0, target on 1: A -> B) or 2 (B -> A), read off the table of set_pair_directions"""
        sub = getattr(self.model.l, "sublattice", None)
        if sub is None or "pair_directions" not in self._tables:
            return None
        dir_of, nd = self._tables["pair_directions"]
        sub = np.asarray(sub)
        kind = np.where(sub[:, None] == sub[None, :], 0, np.where(sub[:, None] == 0, 1, 2))  # [src, trg]
        cls = np.full(nd, -1, dtype=np.int64)
        cls[np.asarray(dir_of).reshape(-1)] = kind.reshape(-1)
        if (cls < 0).any() or not np.array_equal(cls[np.asarray(dir_of)], kind):
            raise ValueError("the direction table mixes sublattice classes in one direction")
        return cls

    def _momentum_time_displaced_basis(self):
        cls = self._basis_classes()
        Ct, St = self._phase_tables()
        m = self._means("time_displaced")
        res = {"tau": m["tau"], "count": m["count"]}
        same, ab = (cls == 0).astype(np.float64), (cls == 1).astype(np.float64)
        for k, src in (("Gk_l0", "Gl0"), ("Gk_0l", "G0l")):
            if src in m:
                res[k] = 2.0 * ((m[src] * same) @ Ct - 1j * ((m[src] * same) @ St))
                res[k + "_AB"] = 2.0 * ((m[src] * ab) @ Ct - 1j * ((m[src] * ab) @ St))
        if "Gk_l0" in res:
            res["nk"] = 2.0 - res["Gk_l0"][:, 0, :].real
        for src in ("CDC", "SDCx", "SDCy", "SDCz"):
            if src in m:
                res[src + "k"] = m[src] @ Ct
        return res

    def sublattice_signs(self):
        """-> [n_dirs] of +1 (same-sublattice direction) / -1 (inter-sublattice): lattices.sublattice_sign of the table of
        set_pair_directions"""
        cls = self._basis_classes()
        if cls is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "sublattice_signs: a lattice with a sublattice array (HoneycombLattice) "
                                 "and set_pair_directions first")
        return np.where(cls == 0, 1.0, -1.0)

    def staggered_structure_factors(self):
        """-> dict(Sc, Sx, Sy, Sz, count): the q = 0 transform with the sublattice signs, sum_d sign_d X[d] of the means
        CDC, SDCx, SDCy, SDCz = (1 / n) sum_ij (+1 same sublattice, -1 else) <O_i O_j>: the antiferromagnetic S_AF of the
        four channels (the device's direction sums are divided by n = 2 L^2 whatever the pair count of a direction, so
        this is the sum over all pairs over n; on the honeycomb an inter-sublattice direction holds n / 2 pairs and a
        per-pair mean would carry a factor 2).  A host transform of the accumulated sums; for error bars hand the
        signs to the momentum binner: set_staggered_momentum(), then binned("momentum_correlations")."""
        sg = self.sublattice_signs()
        m = self._means("correlations")
        res = {k: float(m[src] @ sg) for k, src in (("Sc", "CDC"), ("Sx", "SDCx"), ("Sy", "SDCy"), ("Sz", "SDCz"))}
        res["count"] = m["count"]
        return res

    def staggered_static_susceptibilities(self):
        """-> dict(chi_c, chi_x, chi_y, chi_z, count): the same signed q = 0 transform of the means CDS, SDSx, SDSy, SDSz:
        the antiferromagnetic chi_AF of the four channels (normalised as staggered_structure_factors)"""
        sg = self.sublattice_signs()
        m = self._means("susceptibilities")
        res = {k: float(m[src] @ sg) for k, src in (("chi_c", "CDS"), ("chi_x", "SDSx"), ("chi_y", "SDSy"), ("chi_z", "SDSz"))}
        res["count"] = m["count"]
        return res

    def set_staggered_momentum(self):
        """hand the engine one table in the place of set_momenta's: cos = the sublattice signs, sin = 0 (the interface
        takes any tables with n_q <= n_dirs), labelled q = 0.  The momentum binners then carry S_AF / chi_AF with error
        bars: structure_factors() and static_susceptibilities() return them as their one "momentum".  Replaces the
        tables of set_momenta (and disables the momentum binners, as set_momenta does)."""
        sg = self.sublattice_signs()
        dim = len(_lat_vectors(self.model.l)[0])
        self._set_momenta(np.zeros((1, dim)), sg, np.zeros_like(sg))

    # ---- tau-tau' covariance (include/dqmc_hip.h "tau-tau' covariance")
    def set_tau_covariance(self, bin_size, what=("greens", "density")):
        """from now on every accumulate_susceptibilities pass also feeds the tau-tau' covariance accumulator of the
        momentum time-displaced sample: per walker, `bin_size` consecutive samples are averaged into a bin, and the
        shifted first and second moments of the bins are kept over tau for every series - Re Gk_l0 of every (block, q)
        for "greens", CDCk, SDCxk, SDCyk, SDCzk of every q for "density" (or the DQMC_TD_* mask itself).  bin_size = 0
        turns it off.  Needs set_momenta and set_time_displaced with these rows; refused with sign weighting on.  Costs
        n_walkers * S * (R^2 + 3 R) doubles (tau_covariance_plan).  Read with tau_covariance(), tau_covariance_moments()."""
        if isinstance(what, str):
            what = (what,)
        if not isinstance(what, int):
            bits = {"greens": _lib.TD_GREENS, "density": _lib.TD_DENSITY}
            for k in what:
                if k not in bits:
                    raise ValueError("unknown time-displaced part %r" % (k,))
            what = sum(bits[k] for k in set(what))
        self._c(lib().dqmc_set_tau_covariance(self._h, int(bin_size), int(what)))
        self._tcov = (int(bin_size), int(what)) if int(bin_size) else None

    def tau_covariance_plan(self):
        """-> dict(bin_size, series, rows, bytes, n_bins) of the engine, all zero when off"""
        out = (C.c_int64 * 5)()
        self._c(lib().dqmc_tau_covariance_plan(self._h, out))
        return dict(zip(("bin_size", "series", "rows", "bytes", "n_bins"), (int(v) for v in out)))

    def _cov_moments(self, plan, get):
        out = (C.c_int64 * 5)()
        self._c(plan(self._h, out))
        bs, S, R = int(out[0]), int(out[1]), int(out[2])
        W = self.n_walkers
        nb = np.zeros(W, dtype=np.int64)
        shift, S1, S2 = np.zeros((W, S, R)), np.zeros((W, S, R)), np.zeros((W, S, R, R))
        self._c(get(self._h, _lib.i64ptr(nb), dptr(shift), dptr(S1), dptr(S2)))
        return {"nb": nb, "shift": shift, "S1": S1, "S2": S2, "bin_size": bs}

    def tau_covariance_moments(self):
        """the raw per-walker moments -> dict(nb [W] closed bins, shift, S1 [W, S, R], S2 [W, S, R, R], bin_size): what a
        multi-rank run gathers and hands, as a list over its ranks, to tau_covariance_from_moments"""
        return self._cov_moments(lib().dqmc_tau_covariance_plan, lib().dqmc_tau_covariance_get)

    def tau_covariance(self, moments=None):
        """-> dict: the mean over the closed bins of every walker and the covariance of that mean (moments: a list of
        tau_covariance_moments() of several ranks; default this handle's).  Gk_l0_mean [n_blocks, R, n_q] and Gk_l0_cov
        [n_blocks, n_q, R, R] (of Re Gk_l0) if "greens" is on; CDCk, SDCxk, SDCyk, SDCzk _mean [R, n_q] and _cov
        [n_q, R, R] if "density" is; tau [R], n_bins, bin_size.  The means are shaped like momentum_time_displaced()."""
        if self._tcov is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "tau_covariance: call set_tau_covariance first")
        pooled = tau_covariance_from_moments([self.tau_covariance_moments()] if moments is None else moments)
        nq, what = self._mom[0].shape[0], self._tcov[1]
        mean, cov = pooled["mean"], pooled["cov"]
        R = mean.shape[1]
        res, s = {}, 0
        if what & _lib.TD_GREENS:
            n = self.nb * nq
            res["Gk_l0_mean"] = np.moveaxis(mean[s:s + n].reshape(self.nb, nq, R), 1, 2).copy()
            res["Gk_l0_cov"] = cov[s:s + n].reshape(self.nb, nq, R, R).copy()
            s += n
        if what & _lib.TD_DENSITY:
            for name in ("CDCk", "SDCxk", "SDCyk", "SDCzk"):
                res[name + "_mean"] = mean[s:s + nq].T.copy()
                res[name + "_cov"] = cov[s:s + nq].copy()
                s += nq
        res.update(tau=self._td_tau(), n_bins=pooled["n_bins"], bin_size=self._tcov[0])
        return res

    def user_covariance(self, n_series, R, bin_size):
        """a tau-tau' covariance accumulator over `n_series` series of `R` values per walker that the caller computes on
        the device (bin_size = 0: off)"""
        self._c(lib().dqmc_user_covariance(self._h, int(n_series), int(R), int(bin_size)))
        self._ucov = (int(n_series), int(R), int(bin_size)) if int(bin_size) else None

    def user_covariance_push(self, samples):
        """push one sample [n_walkers, n_series, R]: a contiguous float64 device tensor (torch) or a device address"""
        if hasattr(samples, "data_ptr"):
            if self._ucov is None:
                raise _lib.DQMCError(_lib.ERR_STATE, "user_covariance_push: call user_covariance first")
            n = self.n_walkers * self._ucov[0] * self._ucov[1]
            if str(samples.dtype) != "torch.float64" or not samples.is_contiguous() or not samples.is_cuda \
                    or samples.numel() != n:
                raise ValueError("samples must be a contiguous float64 device tensor of n_walkers x %d x %d" % self._ucov[:2])
            import torch
            torch.cuda.current_stream(samples.device).synchronize()  # the engine reads it on its own stream
            samples = samples.data_ptr()
        self._c(lib().dqmc_user_covariance_push(self._h, C.c_void_p(samples)))

    def user_covariance_result(self):
        """the raw per-walker moments of the user accumulator, as tau_covariance_moments()"""
        return self._cov_moments(lib().dqmc_user_covariance_plan, lib().dqmc_user_covariance_get)

    def _sac_covariance_input(self, who, key):
        """(tau_covariance(), checked) for a continuation with the full covariance"""
        if self._tcov is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "%s: covariance=True needs set_tau_covariance" % who)
        plan = self.tau_covariance_plan()
        if not plan["n_bins"]:
            check_covariance_bins(0, plan["rows"], who)
        tc = self.tau_covariance()
        if key + "_cov" not in tc:
            raise _lib.DQMCError(_lib.ERR_STATE, "%s: set_tau_covariance does not hold these rows" % who)
        return tc

    def spectral_function(self, omega, momenta=None, run=None, covariance=False, **sac_args):
        """A(k, omega) from G(k, tau) by stochastic analytic continuation on the device (sac.SAC; the fermion kernel
        with this run's beta, norm 1) -> dict(omega [Nw], A, weight [n_blocks, n_k, Nw], chi2, theta [n_blocks, n_k],
        momenta, sac).  `momenta` picks rows of momenta() (default: all); `run` is the keyword dict of SAC.run, the
        other keywords go to SAC (n_deltas, thetas, seed, cut, ...).  Refused with sign weighting on, whose <s G> / <s>
        errors are not those of a plain mean.
        covariance=False: the data are Re Gk_l0 of momentum_time_displaced(), the errors Gk_l0_std_error_re of
        binned("momentum_time_displaced"); the diagonal form of chi2 is used and correlations between time slices are
        ignored.  Errors below `error_floor` (default 1e-6) are raised to it.  Needs
        enable_binning("momentum_time_displaced").
        covariance=True: the data are Gk_l0_mean of tau_covariance(), the mean of the closed bins, and their
        covariance Gk_l0_cov goes to SAC, which rotates data and kernel into its eigenbasis and drops eigenvalues below
        `cut` (default 1e-10) of the largest.  Needs set_tau_covariance with "greens" and more bins than time slices
        (ERR_STATE otherwise: the matrix is singular by construction)."""
        from .sac import SAC, fermion_kernel
        if self.sign_weighting():
            raise _lib.DQMCError(_lib.ERR_STATE, "spectral_function: not available with sign weighting on")
        if covariance:
            tc = self._sac_covariance_input("spectral_function", "Gk_l0")
            G, cov = tc["Gk_l0_mean"], tc["Gk_l0_cov"]
            check_covariance_bins(tc["n_bins"], G.shape[1], "spectral_function")
            ks = np.arange(G.shape[2]) if momenta is None else np.asarray(momenta, dtype=np.int64).reshape(-1)
            G, cov = G[:, :, ks], cov[:, ks]
            nb, nt, nk = G.shape
            s = SAC(tc["tau"], np.ascontiguousarray(np.moveaxis(G, 1, 2).reshape(nb * nk, nt)),
                    covariance=cov.reshape(nb * nk, nt, nt), kernel=fermion_kernel, omega=omega, beta=self.p.beta,
                    device_id=self._device_id, **sac_args)
            s.run(**(run or {}))
            sp = s.spectrum()
            return {"omega": sp["omega"], "A": sp["A"].reshape(nb, nk, -1), "weight": sp["weight"].reshape(nb, nk, -1),
                    "chi2": sp["chi2"].reshape(nb, nk), "theta": sp["theta"].reshape(nb, nk),
                    "momenta": self.momenta()[ks], "n_bins": tc["n_bins"], "sac": s}
        if not self._binning_enabled("momentum_time_displaced"):
            raise _lib.DQMCError(_lib.ERR_STATE, 'spectral_function: call enable_binning("momentum_time_displaced") first')
        floor = float(sac_args.pop("error_floor", 1e-6))
        b = self.binned("momentum_time_displaced")
        if "Gk_l0" not in b:
            raise _lib.DQMCError(_lib.ERR_STATE, "spectral_function: the Green's rows are not recorded (set_time_displaced)")
        ks = np.arange(b["Gk_l0"].shape[2]) if momenta is None else np.asarray(momenta, dtype=np.int64).reshape(-1)
        G = self.momentum_time_displaced()["Gk_l0"].real[:, :, ks]   # [n_blocks, R, n_k]
        err = np.asarray(b["Gk_l0_std_error_re"])[:, :, ks]
        if not np.all(np.isfinite(err)):
            raise _lib.DQMCError(_lib.ERR_STATE, "spectral_function: the binner has no error yet (too few samples)")
        nb, nt, nk = G.shape
        flat = lambda v: np.ascontiguousarray(np.moveaxis(v, 1, 2).reshape(nb * nk, nt))
        s = SAC(np.asarray(b["tau"], dtype=np.float64), flat(G), error=np.maximum(flat(err), floor), kernel=fermion_kernel,
                omega=omega, beta=self.p.beta, device_id=self._device_id, **sac_args)
        s.run(**(run or {}))
        sp = s.spectrum()
        return {"omega": sp["omega"], "A": sp["A"].reshape(nb, nk, -1), "weight": sp["weight"].reshape(nb, nk, -1),
                "chi2": sp["chi2"].reshape(nb, nk), "theta": sp["theta"].reshape(nb, nk), "momenta": self.momenta()[ks],
                "sac": s}

    def dynamical_structure_factor(self, omega, channel="SDCz", momenta=None, covariance=True, run=None, **sac_args):
        """S(q, omega) of a density channel ("SDCz", "SDCx", "SDCy", "CDC") from C(q, tau) = <channel>k of
        tau_covariance() by stochastic analytic continuation with sac.boson_symmetric_kernel on omega >= 0 -> dict(omega,
        B [n_k, Nw]: the sampled density S(q, omega) (1 + e^{-beta omega}); S = B / (1 + e^{-beta omega}); weight [n_k, Nw]
        (it sums to C(q, 0)); chi2, theta [n_k]; momenta; left_out; n_bins; sac).  Only the recorded slices with
        tau <= beta / 2 are used: C(tau) = C(beta - tau), so the upper half carries the same information and would make
        the covariance singular.  norm = C(q, tau = 0) per momentum; a momentum whose C(q, 0) is not positive (q = 0 of
        the charge channel at fixed filling) has no spectrum to normalise, is left out and listed (as an index into
        momenta()) under left_out.  covariance=True hands SAC the covariance of the kept slices and needs more bins than
        kept slices (ERR_STATE otherwise); covariance=False its diagonal, with errors below `error_floor` (default 1e-6)
        raised to it.  Needs set_tau_covariance with "density"; `momenta`, `run` and the other keywords as for
        spectral_function."""
        from .sac import SAC, boson_symmetric_kernel
        if channel not in ("SDCz", "SDCx", "SDCy", "CDC"):
            raise ValueError("channel must be one of SDCz, SDCx, SDCy, CDC")
        if self.sign_weighting():
            raise _lib.DQMCError(_lib.ERR_STATE, "dynamical_structure_factor: not available with sign weighting on")
        floor = float(sac_args.pop("error_floor", 1e-6))
        tc = self._sac_covariance_input("dynamical_structure_factor", channel + "k")
        Cq, cov = tc[channel + "k_mean"], tc[channel + "k_cov"]  # [R, n_q], [n_q, R, R]
        plan = self.time_displaced_plan()
        keep = np.nonzero(2 * plan["every"] * np.arange(plan["rows"]) <= self.p.slices)[0]  # tau <= beta / 2, in integers
        if covariance:
            check_covariance_bins(tc["n_bins"], keep.size, "dynamical_structure_factor")
        elif tc["n_bins"] < 2:
            raise _lib.DQMCError(_lib.ERR_STATE, "dynamical_structure_factor: fewer than two closed bins")
        ks = np.arange(Cq.shape[1]) if momenta is None else np.asarray(momenta, dtype=np.int64).reshape(-1)
        left_out = np.array([k for k in ks if not Cq[0, k] > 0.0], dtype=np.int64)
        ks = np.array([k for k in ks if Cq[0, k] > 0.0], dtype=np.int64)
        if ks.size == 0:
            raise _lib.DQMCError(_lib.ERR_STATE, "dynamical_structure_factor: no momentum with C(q, 0) > 0")
        data = np.ascontiguousarray(Cq[keep][:, ks].T)
        cv = cov[ks][:, keep][:, :, keep]
        how = {"covariance": cv} if covariance else \
            {"error": np.maximum(np.sqrt(np.einsum("kii->ki", cv)), floor)}
        s = SAC(tc["tau"][keep], data, kernel=boson_symmetric_kernel, omega=omega, beta=self.p.beta, norm=Cq[0, ks],
                device_id=self._device_id, **how, **sac_args)
        s.run(**(run or {}))
        sp = s.spectrum()
        return {"omega": sp["omega"], "B": sp["A"], "S": sp["A"] / (1.0 + np.exp(-self.p.beta * sp["omega"]))[None, :],
                "weight": sp["weight"], "chi2": sp["chi2"], "theta": sp["theta"], "momenta": self.momenta()[ks],
                "left_out": left_out, "n_bins": tc["n_bins"], "sac": s}

    def _binned_momentum(self, which, level=None):
        """binned() of a momentum binner: the keys of structure_factors() / static_susceptibilities() /
        momentum_time_displaced(), each X with X_std_error, X_std_error_walkers and X_tau; for the complex Gk_l0, Gk_0l the
        errors and tau of the real and the imaginary part apart (X_std_error_re, X_std_error_im, ...).  With sign weighting
        on X is <s X> / <s>, X_std_error and X_std_error_walkers both the jackknife of that ratio over the walkers
        (jackknife_ratio, from level 0 of the sample and of its trailing s: at least two walkers), X_tau that of s X."""
        raw = self.binned_raw(which, level)
        if self.sign_weighting():
            E = self.binner_size(which)[0]
            lv0 = np.stack([self.binner_level(which, w, 0)[0] for w in range(self.n_walkers)])
            val, err = jackknife_ratio(lv0[:, :E - 1], lv0[:, E - 1])
            pad = lambda v: np.concatenate([v, [np.nan]])
            raw = dict(raw, mean=pad(val), std_error=pad(err), std_error_walkers=pad(err))
        d = self._bin_dict(which, raw)
        for k in [k for k in d if k == "s" or k.startswith("s_")]:
            del d[k]
        sfx = ("", "_std_error", "_std_error_walkers", "_tau")
        res = {}
        if which == "momentum_time_displaced":
            for k, src in (("Gk_l0", "Gl0"), ("Gk_0l", "G0l")):
                if src + "_C" in d:
                    res[k] = d.pop(src + "_C") - 1j * d.pop(src + "_S")
                    for x in sfx[1:]:
                        res[k + x + "_re"], res[k + x + "_im"] = d.pop(src + "_C" + x), d.pop(src + "_S" + x)
            if "Gk_l0" in res:
                res["nk"] = 1.0 - res["Gk_l0"][:, 0, :].real
                for x in sfx[1:]:
                    res["nk" + x] = res["Gk_l0" + x + "_re"][:, 0, :]
            res["tau"] = self._td_tau()
        res.update(d)
        res["count"] = raw["count"]
        res["reliable_level"] = raw["reliable_level"]
        return res

    # ---- pair structure factors and superfluid stiffness (include/dqmc_hip.h; the reference has no such measurement)
    def set_pair_channels(self, channels="default"):
        """the symmetry channels of the pair structure factors: a dict name -> weights f[k], k < K, over the directions
        of set_local_targets (k = 0 is on-site), at most 8 of them; F[kk, c] = f_c[k1] f_c[k2] goes to the engine.
        "default" (lattices.default_pair_channels): s = e_0 and s* = 1/2 on every nearest neighbour on every lattice (no
        1/sqrt(z): the square lattice's weights are kept as they are elsewhere), and on a SquareLattice d = +1/2 on the
        +-x bonds and -1/2 on the +-y bonds, the sign read from the iterator's directions; on a BilayerSquareLattice s, s*
        and d on the in-plane neighbours and s_perp = 1 on the interlayer direction.  None or {} turns the channels
        off.  Needs set_local_targets(iterator); frees the two pairing response binners."""
        from .lattices import default_pair_channels

        def dropped():  # (only once the engine has taken the call: a refused one keeps the setting and the binners)
            for k in ("response_pairing", "response_pairing_susceptibility"):
                self._binner_dropped(k)
        if channels is None or (not isinstance(channels, str) and len(channels) == 0):
            self._c(lib().dqmc_set_pair_channels(self._h, 0, None))
            dropped()
            self._channels = None
            return
        K = getattr(self, "_K", 0)
        if not K:
            raise _lib.DQMCError(_lib.ERR_STATE, "set_pair_channels: call set_local_targets first")
        if isinstance(channels, str):
            if channels != "default":
                raise ValueError("channels must be 'default' or a dict name -> weights")
            if self._dirs is None:
                raise _lib.DQMCError(_lib.ERR_STATE, "set_pair_channels('default'): set_local_targets(iterator) first")
            channels = default_pair_channels(self.model.l, self._dirs, K)
        if len(channels) > 8:
            raise ValueError("at most 8 pair channels")
        ch = {}
        for name, f in channels.items():
            f = np.asarray(f, dtype=np.float64)
            if f.shape != (K,) or not np.all(np.isfinite(f)):
                raise ValueError("channel %r must hold K = %d finite weights" % (name, K))
            ch[str(name)] = f
        F = np.ascontiguousarray(np.concatenate([np.outer(f, f).reshape(-1, order="F") for f in ch.values()]))
        self._c(lib().dqmc_set_pair_channels(self._h, len(ch), dptr(F)))
        dropped()
        self._channels = ch

    def pair_channels(self):
        """-> {name: weights [K]} of set_pair_channels, or None"""
        ch = getattr(self, "_channels", None)
        return None if ch is None else {k: v.copy() for k, v in ch.items()}

    def response_plan(self):
        """-> dict(n_ch, K, K_cc, n_q) of the engine, zeros where unset"""
        out = (C.c_int32 * 4)()
        self._c(lib().dqmc_response_plan(self._h, out))
        return dict(zip(("n_ch", "K", "K_cc", "n_q"), (int(v) for v in out)))

    def _channel_names(self):
        ch = getattr(self, "_channels", None)
        if ch is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_pair_channels first")
        return list(ch)

    def _pair_transform(self, X):
        """X[dir12, k1, k2] -> {name: sum_d e^{-i q . r_d} sum_{k1 k2} f[k1] f[k2] X[d, k1, k2]}"""
        Ct, St = self._phase_tables()
        res = {}
        for name, f in self._channels.items():
            z = np.einsum("dab,a,b->d", X, f, f)
            res[name] = z @ Ct - 1j * (z @ St)
        return res

    def pair_structure_factors(self):
        """-> {channel: P_c(q) complex [n_q]} and count: the host transform of the pairing mean (of signed("pairing")
        with sign weighting on), P_c(q) = sum_d e^{-i q . r_d} sum_{k1 k2} f_c[k1] f_c[k2] PC[d, k1, k2]"""
        self._channel_names()
        if self.sign_weighting():
            m = self.signed("pairing")
            X, cnt = m["PC"], m["count"]
        else:
            X, cnt = self.pairing()
        res = self._pair_transform(X)
        res["count"] = cnt
        return res

    def pair_susceptibilities(self):
        """-> {channel: complex [n_q]} and count: the same transform of the mean PS of susceptibilities()"""
        self._channel_names()
        m = self._means("susceptibilities")
        if "PS" not in m:
            raise _lib.DQMCError(_lib.ERR_STATE, "the susceptibility section has no pairing part: set_local_targets first")
        res = self._pair_transform(m["PS"])
        res["count"] = m["count"]
        return res

    def _kbond(self, G):
        """the bond kinetic energy of the current-target columns from Green's blocks G (include/dqmc_hip.h)"""
        trg, K = self._tables["current_targets"][0], self._Kcc
        N, fac = self.N, (2.0 if self.nb == 1 else 1.0)
        out = np.zeros(K)
        for k in range(K):
            src = np.nonzero(trg[:, k] >= 0)[0]
            t = trg[src, k]
            for b in range(self.nb):
                T = self._cc_T[b * N * N:(b + 1) * N * N].reshape((N, N), order="F")
                out[k] += fac * np.sum(T[t, src] * ((src == t) - G[b][src, t])) / N
        return out

    def current_response(self):
        """-> dict(Lambda complex [K_cc, n_q], count, and kbond [K_cc] if greens was accumulated): Lambda[k, q] =
        sum_d e^{-i q . r_d} CCS[d, k] of the mean CCS of susceptibilities() (the engine's sums as they are: see
        superfluid_stiffness for the sign); kbond is linear in G and comes from the mean G of the greens accumulator."""
        if not getattr(self, "_Kcc", 0):
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_current_targets first")
        Ct, St = self._phase_tables()
        m = self._means("susceptibilities")
        ccs = m["CCS"]
        res = {"Lambda": (ccs.T @ Ct) - 1j * (ccs.T @ St), "count": m["count"]}
        if self._section("greens")[-1] > 0:
            res["kbond"] = self._kbond(self._means_greens())
        return res

    def _means_greens(self):
        return self.signed("greens")["G"] if self.sign_weighting() else self.unpack_accumulators(self._section("greens"))["G"]

    def _stiffness_indices(self, axis):
        """(k+, k-, q_L, q_T): the current-target columns along +-axis and the smallest momenta along / across it"""
        if self._dirs is None or self._mom is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "superfluid_stiffness: set_current_targets(iterator) and set_momenta first")
        A = np.array(_lat_vectors(self.model.l), dtype=np.float64)
        dim = A.shape[0]
        if not 0 <= axis < dim:
            raise ValueError("axis must be 0 .. %d" % (dim - 1))
        self._no_interlayer_current(axis)
        a = A[axis] / np.linalg.norm(A[axis])  # (A_i: the vectors the lattice is periodic under, along the bonds)
        nrm = np.linalg.norm(self._dirs[:self._Kcc], axis=1)
        par = [k for k in range(self._Kcc) if nrm[k] > 0 and np.isclose(abs(self._dirs[k] @ a), nrm[k])]
        ks = [k for k in par if np.isclose(nrm[k], min(nrm[j] for j in par))]
        if len(ks) != 2:
            raise ValueError("superfluid_stiffness: the current targets do not hold the two bonds along axis %d" % axis)
        kp, km = (ks if self._dirs[ks[0]] @ a > 0 else ks[::-1])
        B = 2.0 * np.pi * np.linalg.inv(A).T  # rows B_j with A_i . B_j = 2 pi delta_ij: the smallest momenta
        qL, qT = B[axis], B[(axis + 1) % dim]
        q = self._mom[0]
        idx, missing = [], []
        for name, want in (("q_L", qL), ("q_T", qT)):
            hit = [i for i in range(q.shape[0]) if np.allclose(q[i], want, atol=1e-9)]
            if not hit:
                missing.append("%s = %s" % (name, np.array2string(want, precision=6)))
            idx.append(hit[0] if hit else -1)
        if missing:
            raise ValueError("superfluid_stiffness: set_momenta's list lacks " + " and ".join(missing))
        return kp, km, idx[0], idx[1]

    @staticmethod
    def _stiffness_of(k_axis, lam_L, lam_T):
        return {"k_axis": k_axis, "Lambda_L": lam_L, "Lambda_T": lam_T, "rho_s": (-k_axis - lam_T) / 4.0,
                "drude": -k_axis - lam_L}

    def superfluid_stiffness(self, axis=0):
        """-> dict(k_axis, Lambda_L, Lambda_T, rho_s, drude): k_axis = kbond[+axis] + kbond[-axis]; Lambda_L / Lambda_T =
        Re Lambda_axis at the smallest momentum along / perpendicular to the axis (both must be in set_momenta's list:
        ValueError otherwise); rho_s = (-k_axis - Lambda_T) / 4, drude = -k_axis - Lambda_L.  Sign convention: Lambda_axis
        here is the current-current response whose longitudinal limit tends to -k_axis > 0, i.e. MINUS the cosine
        transform of the engine's CCS[., k = +axis]: the reference's cc_kernel sums <J J> of J = T c+c - h.c. without the
        factor i of the current j = i J, so it carries i^2 = -1 (fixed on free fermions: tests/response_ref.py).
        With the response_current binner on and at least two walkers every key X also has X_std_error: the cross-walker
        error of the per-walker values formed from level 0 of that binner (jackknife_ratio with sign weighting on)."""
        self._nearest_neighbour_current("superfluid_stiffness")
        kp, km, iL, iT = self._stiffness_indices(axis)
        cr = self.current_response()
        if "kbond" not in cr:
            raise _lib.DQMCError(_lib.ERR_STATE, "superfluid_stiffness: accumulate greens as well (kbond comes from its mean)")
        lam = -cr["Lambda"][kp].real
        res = self._stiffness_of(cr["kbond"][kp] + cr["kbond"][km], lam[iL], lam[iT])
        W = self.n_walkers
        if self._binning_enabled("response_current") and W >= 2 and self.binner_size("response_current")[2] > 0:
            E, _, T = self.binner_size("response_current")
            nq, K = self._mom[0].shape[0], self._Kcc
            lv0 = np.stack([self.binner_level("response_current", w, 0)[0] for w in range(W)])
            sel = lambda v: np.stack([v[:, 2 * K * nq + kp] + v[:, 2 * K * nq + km], -v[:, kp * nq + iL], -v[:, kp * nq + iT]], axis=1)
            if self.sign_weighting():
                val, err = jackknife_ratio(sel(lv0), lv0[:, E - 1])
                # (rho_s and drude are linear in the three: their jackknife is that of the combination)
                comb = np.stack([(-sel(lv0)[:, 0] - sel(lv0)[:, 2]) / 4.0, -sel(lv0)[:, 0] - sel(lv0)[:, 1]], axis=1)
                _, err2 = jackknife_ratio(comb, lv0[:, E - 1])
                errs = dict(zip(("k_axis", "Lambda_L", "Lambda_T", "rho_s", "drude"), list(err) + list(err2)))
            else:
                x = sel(lv0) / T
                per = np.stack([x[:, 0], x[:, 1], x[:, 2], (-x[:, 0] - x[:, 2]) / 4.0, -x[:, 0] - x[:, 1]], axis=1)
                e = np.sqrt(((per - per.mean(axis=0)) ** 2).sum(axis=0) / (W * (W - 1)))
                errs = dict(zip(("k_axis", "Lambda_L", "Lambda_T", "rho_s", "drude"), e))
            for k, v in errs.items():
                res[k + "_std_error"] = v
        return res

    def _binned_response(self, which, level=None):
        """binned() of a response binner: response_pairing / response_pairing_susceptibility -> {channel: complex [n_q]};
        response_current -> Lambda complex [K_cc, n_q] and kbond [K_cc]; every X with X_std_error, X_std_error_walkers,
        X_tau, those of a complex X split into _re / _im.  With sign weighting as _binned_momentum."""
        raw = self.binned_raw(which, level)
        if self.sign_weighting():
            E = self.binner_size(which)[0]
            lv0 = np.stack([self.binner_level(which, w, 0)[0] for w in range(self.n_walkers)])
            val, err = jackknife_ratio(lv0[:, :E - 1], lv0[:, E - 1])
            pad = lambda v: np.concatenate([v, [np.nan]])
            raw = dict(raw, mean=pad(val), std_error=pad(err), std_error_walkers=pad(err))
        nq = self._mom[0].shape[0]
        if which == "response_current":
            names, rows = ["Lambda"], self._Kcc
        else:
            names, rows = self._channel_names(), 1
        n = len(names) * rows * nq
        res = {}
        for key, x in (("mean", ""), ("std_error", "_std_error"), ("std_error_walkers", "_std_error_walkers"), ("tau", "_tau")):
            v = raw[key]
            c, s = v[:n].reshape(len(names), rows, nq), v[n:2 * n].reshape(len(names), rows, nq)
            for i, name in enumerate(names):
                ci, si = (c[i], s[i]) if which == "response_current" else (c[i, 0], s[i, 0])
                if key == "mean":
                    res[name] = ci - 1j * si
                else:
                    res[name + x + "_re"], res[name + x + "_im"] = ci, si
            if which == "response_current":
                res["kbond" + x] = v[2 * n:2 * n + self._Kcc]
        res["count"] = raw["count"]
        res["reliable_level"] = raw["reliable_level"]
        return res

    # ---- scalar thermodynamics (include/dqmc_hip.h "thermodynamics"; the reference has no such measurement)
    def set_thermodynamics(self, on=True, hopping=None):
        """configure the thermodynamics section: the model's hopping_matrix() (or `hopping`, one n x n matrix per block)
        goes to the engine, which keeps it as a neighbour list.  From then on accumulate_thermodynamics() and
        run(measurements=(..., "thermodynamics")) add one sample per walker of n_up, n_dn, n, D, m2, E_kin, E_int, E, N2,
        Mz2 (per site; include/dqmc_hip.h).  on=False drops the section.  Either way its sums and its binner go."""
        self._binner_dropped("thermodynamics")
        if not on:
            self._c(lib().dqmc_set_thermodynamics(self._h, None))
            self._thermo = False
            return
        blocks = self.model.hopping_matrix() if hopping is None else hopping
        if isinstance(blocks, np.ndarray) and blocks.ndim == 2:
            blocks = [blocks]
        if len(blocks) != self.nb or any(np.shape(b) != (self.N, self.N) for b in blocks):
            raise ValueError("hopping must be %d matrices of %d x %d" % (self.nb, self.N, self.N))
        T = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, order="F") for b in blocks]))
        self._c(lib().dqmc_set_thermodynamics(self._h, dptr(T)))
        # (what a checkpoint writes down: the hopping only where it is not the model's own, as for the current targets)
        self._thermo = True if hopping is None else [float(x) for x in T]

    def accumulate_thermodynamics(self):
        self._c(lib().dqmc_accumulate_thermodynamics(self._h))

    def _thermo_derived(self, m):
        """kappa = beta (<N2> - N <n>^2), chi_s = beta <Mz2> / 4 of means m [..., 10]"""
        beta = self.p.beta
        return beta * (m[..., 8] - self.N * m[..., 2] ** 2), beta * m[..., 9] / 4.0

    def thermodynamics(self):
        """-> dict of the ten means n_up, n_dn, n, D, m2, E_kin, E_int, E, N2, Mz2 (per site), the derived
        kappa = beta (<N2> - N <n>^2) and chi_s = beta <Mz2> / 4, count, sign_sum and mean_sign.  The sums are divided by
        the section's sum of signs, which is the sample count while sign weighting is off and makes the means <x s> / <s>
        while it is on (signed("thermodynamics") returns the same dict).  With the section's binner on and at least two
        walkers every key X also has X_std_error, the jackknife over the walkers (kappa and chi_s included: they are no
        linear functions of the sums).  ValueError when the sum of signs is 0."""
        raw = self._section("thermodynamics")
        NE = self._NE
        S, cnt = raw[NE], raw[NE + 1]
        if S == 0:
            raise ValueError("thermodynamics(): the sum of signs is 0 over %d samples" % cnt)
        m = raw[:NE] / S
        res = dict(zip(_lib.THERMO_FIELDS, m))
        res["kappa"], res["chi_s"] = self._thermo_derived(m)
        res.update(count=cnt, sign_sum=S, mean_sign=S / cnt)
        if self._binning_enabled("thermodynamics") and self.n_walkers >= 2:
            lv0 = np.stack([self.binner_level("thermodynamics", w, 0)[0] for w in range(self.n_walkers)])
            T = self.binner_size("thermodynamics")[2]
            sx, s = lv0[:, :NE], (lv0[:, NE] if self.sign_weighting() else np.full(self.n_walkers, float(T)))
            W, tot, St = self.n_walkers, sx.sum(axis=0), s.sum()
            if T and St != 0 and not np.any(St - s == 0):
                r = (tot[None, :] - sx) / (St - s)[:, None]  # the means with walker w left out
                k, c = self._thermo_derived(r)
                full = np.concatenate([r, k[:, None], c[:, None]], axis=1)
                err = np.sqrt((W - 1) / W * ((full - full.mean(axis=0)) ** 2).sum(axis=0))
                for name, e in zip(_lib.THERMO_FIELDS + ("kappa", "chi_s"), err):
                    res[name + "_std_error"] = e
        return res

    # ---- current_current_susceptibility (measurements.jl:257-317) over EachLocalQuadBySyncedDistance{K}
    # ---- Renyi-2 entanglement entropy from walker pairs (include/dqmc_hip.h "entanglement"; the reference has no such measurement)
    def set_entanglement(self, subsystems):
        """configure the entanglement measurement: `subsystems` is a list of site sequences (0-based, distinct, taken in
        the order given, at most 128 sites each and 64 lists; lattices.strip_subsystem makes strips) or a dict name ->
        sites; None or an empty list turns it off and frees its memory.  From then on accumulate_entanglement() and
        run(measurements=(..., "entanglement")) add one sample: Grover's x(w, w') of every pair of this object's walkers
        and every subsystem.  Needs at least two walkers; refused while sign weighting is on (the signed estimator is
        not implemented).  Multi-rank runs: each rank pairs its own walkers only and there is no reduced("entanglement");
        the ranks' purities combine as count-weighted means, purity = sum_r count_r purity_r / sum_r count_r, S2 = -log of
        that."""
        if not subsystems:
            self._c(lib().dqmc_set_entanglement(self._h, 0, None, None))
            self._ent = None
            return
        names = None
        if isinstance(subsystems, dict):
            names, subsystems = [str(k) for k in subsystems], list(subsystems.values())
        lists = [[int(a) for a in np.asarray(sub).reshape(-1)] for sub in subsystems]
        ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(a) for a in lists])]), dtype=np.int32)
        flat = np.ascontiguousarray([a for sub in lists for a in sub] or [0], dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._c(lib().dqmc_set_entanglement(self._h, len(lists), ptr.ctypes.data_as(i32), flat.ctypes.data_as(i32)))
        self._ent = (names, lists)

    def accumulate_entanglement(self):
        self._c(lib().dqmc_accumulate_entanglement(self._h))

    def _entanglement_raw(self):
        n = C.c_size_t()
        self._c(lib().dqmc_entanglement_size(self._h, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        self._c(lib().dqmc_get_entanglement(self._h, dptr(out), n.value))
        return out

    def entanglement_sample(self):
        """the last sample, [n_sub, W, W]: x(w, w') in the strictly upper triangle, 0 elsewhere"""
        if self._ent is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_entanglement first")
        W, ns = self.n_walkers, len(self._ent[1])
        out = np.zeros(ns * W * W)
        self._c(lib().dqmc_get_entanglement_sample(self._h, dptr(out), out.size))
        return out.reshape((ns, W, W))

    def entanglement(self):
        """-> {"purity": [n_sub], "S2": [n_sub], "S2_std_error": [n_sub] (three walkers and more), "pair_sums":
        [n_sub, W, W], "count", "failures"} (entanglement_from_pair_sums); "names" with a dict given to
        set_entanglement.  failures counts the pairs whose sample was set to 0 (a singular or non-finite M)."""
        raw = self._entanglement_raw()
        W, ns = self.n_walkers, len(self._ent[1])
        sums, cnt = raw[:-2].reshape((ns, W, W)), int(raw[-2])
        res = entanglement_from_pair_sums(sums, cnt) if cnt else {}
        res.update(pair_sums=sums, count=cnt, failures=int(raw[-1]))
        if self._ent[0] is not None:
            res["names"] = list(self._ent[0])
        return res

    # ---- current response in imaginary time (include/dqmc_hip.h "current response in imaginary time"; the reference has no such measurement)
    def set_current_time_displaced(self, every=1):
        """record the current-current correlator per imaginary time and momentum inside every
        accumulate_susceptibilities() / run(measurements=(..., "susceptibilities")) from now on: rows r = 0 .. slices /
        every at tau_r = r every delta_tau, per walker, for the targets of set_current_targets and the momenta of
        set_momenta (both needed, and prepare(): ERR_STATE otherwise).  `every` must divide slices (ERR_INVALID, and the
        setting stays); 0 or None turns it off and frees its memory.  set_pair_directions, set_current_targets and
        set_momenta turn it off.  Every call starts with zero sums.  Read with current_time_displaced(),
        current_matsubara(), drude_weight(), dc_conductivity().  Multi-rank runs: each rank records its own walkers and
        there is no reduced(...) of it; rank results combine count-weighted, X = sum_r count_r X_r / sum_r count_r (with
        sign weighting: weighted with each rank's sum of signs)."""
        self._c(lib().dqmc_set_current_time_displaced(self._h, int(every or 0)))
        self._ctd = int(every or 0)

    def current_time_displaced_plan(self):
        """-> dict(R, every, K_cc, n_q) of the engine, all zero while the recording is off"""
        out = (C.c_int32 * 4)()
        self._c(lib().dqmc_current_time_displaced_plan(self._h, out))
        return dict(zip(("R", "every", "K_cc", "n_q"), (int(v) for v in out)))

    def _current_tau_raw(self):
        """the per-walker sums [n_walkers, P] as the engine holds them"""
        n = C.c_size_t()
        self._c(lib().dqmc_current_time_displaced_size(self._h, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        self._c(lib().dqmc_get_current_time_displaced(self._h, dptr(out)))
        return out.reshape((self.n_walkers, -1))

    def _current_tau(self):
        """(CurrentTauSums of the engine's sums, tau [R])"""
        p = self.current_time_displaced_plan()
        if not p["every"]:
            raise _lib.DQMCError(_lib.ERR_STATE, "call set_current_time_displaced first")
        ct = CurrentTauSums(self._current_tau_raw(), p["R"], p["K_cc"], p["n_q"], could_leave_out=self.sign_weighting())
        return ct, np.arange(p["R"]) * (p["every"] * self.p.delta_tau)

    def current_time_displaced(self):
        """-> dict(tau [R], Lambda_cos, Lambda_sin [R, K_cc, n_q], kbond [K_cc], count, left_out): Lambda_cos / Lambda_sin
        are MINUS the engine's cosine / sine sums (the sign of superfluid_stiffness: Lambda(q, tau) = Lambda_cos - i
        Lambda_sin >= 0 on the diagonal), means over walkers and calls, <x s> / <s> with sign weighting on; count: samples
        kept, left_out: samples of walkers whose sign came out 0.  Lambda_cos, Lambda_sin and kbond come with
        X_std_error, the delete-one-walker jackknife of the ratio (two walkers and more, three with sign weighting on,
        where a walker can be left out).  ValueError when the sum of signs is 0."""
        ct, tau = self._current_tau()
        res = ct.estimate(lambda C_, S_, kb: {"Lambda_cos": -C_, "Lambda_sin": -S_, "kbond": kb})
        res.update(tau=tau, count=ct.count, left_out=ct.left_out)
        return res

    def current_matsubara(self, n_max=None):
        """-> dict(omega [n_max + 1], Lambda complex [n_max + 1, K_cc, n_q], Lambda_std_error_re / _im): the trapezoid
        rule on the recorded grid, Lambda(q, i omega_m) = every delta_tau sum_r w_r cos(omega_m tau_r) Lambda(q, tau_r),
        w_0 = w_{R-1} = 1/2, else 1, omega_m = 2 pi m / beta, Lambda(q, tau) = Lambda_cos - i Lambda_sin of
        current_time_displaced().  n_max <= (R - 1) / 2 (the default).  Errors: the jackknife through the transform."""
        ct, tau = self._current_tau()
        top = (ct.R - 1) // 2
        n_max = top if n_max is None else int(n_max)
        if not 0 <= n_max <= top:
            raise ValueError("n_max must be 0 .. (R - 1) / 2 = %d" % top)
        beta = self.p.slices * self.p.delta_tau
        omega = 2.0 * np.pi * np.arange(n_max + 1) / beta
        res = ct.estimate(lambda C_, S_, kb: {"Lambda": matsubara_trapezoid(-C_ + 1j * S_, tau, omega)})
        res["omega"] = omega
        return res

    def _nearest_neighbour_current(self, who):
        """superfluid_stiffness, drude_weight and dc_conductivity take the current along an axis and its kinetic energy from
        the two nearest-neighbour bonds along it: with tp != 0 the diagonal bonds carry current along both axes as well,
        and a number without them would be wrong"""
        from .lattices import HoneycombLattice
        if isinstance(self.model.l, HoneycombLattice):
            raise NotImplementedError("%s: a HoneycombLattice has no +- pair of bonds along a cartesian axis (the inverse of "
                                      "an A -> B bond starts on the other sublattice); current_response() with K = 7 holds "
                                      "the six bond directions" % who)
        if getattr(self.model, "tp", 0.0) != 0.0:
            raise NotImplementedError("%s: the current along an axis is taken from the nearest-neighbour bonds only; with "
                                      "tp != 0 the diagonal bonds carry current as well (not implemented).  "
                                      "current_response() and current_time_displaced() with K = 9 hold the diagonal bonds"
                                      % who)

    def _no_interlayer_current(self, axis):
        """a BilayerSquareLattice has one interlayer direction, its own inverse: there is no +- pair of bonds along z to
        take a current from, and no smallest momentum along it"""
        from .lattices import BilayerSquareLattice
        if isinstance(self.model.l, BilayerSquareLattice) and axis == 2:
            raise ValueError("axis 2 of a BilayerSquareLattice: the interlayer current response is not implemented (axis 0 or 1)")

    def _axis_bonds(self, axis):
        """(k+, k-, index of q = 0): the current-target columns along +-axis as superfluid_stiffness takes them"""
        if self._dirs is None or self._mom is None:
            raise _lib.DQMCError(_lib.ERR_STATE, "set_current_targets(iterator) and set_momenta first")
        A = np.array(_lat_vectors(self.model.l), dtype=np.float64)
        if not 0 <= axis < A.shape[0]:
            raise ValueError("axis must be 0 .. %d" % (A.shape[0] - 1))
        self._no_interlayer_current(axis)
        a = A[axis] / np.linalg.norm(A[axis])
        nrm = np.linalg.norm(self._dirs[:self._Kcc], axis=1)
        par = [k for k in range(self._Kcc) if nrm[k] > 0 and np.isclose(abs(self._dirs[k] @ a), nrm[k])]
        ks = [k for k in par if np.isclose(nrm[k], min(nrm[j] for j in par))]
        if len(ks) != 2:
            raise ValueError("the current targets do not hold the two bonds along axis %d" % axis)
        kp, km = (ks if self._dirs[ks[0]] @ a > 0 else ks[::-1])
        q = self._mom[0]
        hit = [i for i in range(q.shape[0]) if np.allclose(q[i], 0.0, atol=1e-9)]
        if not hit:
            raise ValueError("set_momenta's list lacks q = 0")
        return kp, km, hit[0]

    def drude_weight(self, axis=0, m=(1, 2, 3)):
        """-> dict(k_axis, omega_m, Lambda_m, D_over_pi_m, each with X_std_error): Scalapino-White-Zhang's D / pi = -k_axis
        - Lambda_axis,axis(q = 0, i omega_m -> 0) at the Matsubara indices `m` (extrapolate m -> 0), k_axis = kbond[+axis]
        + kbond[-axis] of the recording's own sums, Lambda_m the real part of current_matsubara() at q = 0 (which must be
        in set_momenta's list).  This is the limit q -> 0 first; superfluid_stiffness()["drude"] takes omega = 0 first and
        is fixed to -k_axis by gauge invariance."""
        self._nearest_neighbour_current("drude_weight")
        kp, km, i0 = self._axis_bonds(axis)
        ct, tau = self._current_tau()
        ms = np.atleast_1d(np.asarray(m, dtype=np.int64))
        if ms.size == 0 or ms.min() < 0 or ms.max() > (ct.R - 1) // 2:
            raise ValueError("m must lie in 0 .. (R - 1) / 2 = %d" % ((ct.R - 1) // 2))
        omega = 2.0 * np.pi * ms / (self.p.slices * self.p.delta_tau)

        def f(C_, S_, kb):
            lam = matsubara_trapezoid(-C_[:, kp, i0], tau, omega)
            k_axis = kb[kp] + kb[km]
            return {"k_axis": k_axis, "Lambda_m": lam, "D_over_pi_m": -k_axis - lam}
        res = ct.estimate(f)
        res["omega_m"] = omega
        return res

    def dc_conductivity(self, axis=0):
        """-> dict(sigma_dc, sigma_dc_std_error, Lambda_half): Trivedi-Randeria's proxy (beta^2 / pi) Lambda_axis,axis(q = 0,
        tau = beta / 2).  ValueError unless slice slices / 2 is a recorded row."""
        self._nearest_neighbour_current("dc_conductivity")
        kp, km, i0 = self._axis_bonds(axis)
        ct, tau = self._current_tau()
        M, every = self.p.slices, self.current_time_displaced_plan()["every"]
        if M % 2 or (M // 2) % every:
            raise ValueError("dc_conductivity: tau = beta / 2 (slice %g) is not a recorded row (slices = %d, every = %d)"
                             % (M / 2.0, M, every))
        r, beta = (M // 2) // every, M * self.p.delta_tau
        return ct.estimate(lambda C_, S_, kb: {"Lambda_half": -C_[r, kp, i0], "sigma_dc": beta * beta / np.pi * -C_[r, kp, i0]})

    def set_current_targets(self, iterator, hopping=None):
        """hand the targets of EachLocalQuadBySyncedDistance{K} and mc.s.hopping_matrix (default: the model's
        hopping_matrix(), one n x n matrix per block) to the device; the pair directions of the same lattice are
        set with it.  From then on accumulate_susceptibilities also sums CCS[dir12, dir_ii]."""
        self.set_pair_directions(iterator.pairs_by_dir)
        self._set_current_targets(iterator.trg_of, iterator.K, hopping)

    def _set_current_targets(self, trg_of, K, hopping):
        blocks = self.model.hopping_matrix() if hopping is None else hopping
        if isinstance(blocks, np.ndarray) and blocks.ndim == 2:
            blocks = [blocks]
        if len(blocks) != self.nb or any(np.shape(b) != (self.N, self.N) for b in blocks):
            raise ValueError("hopping must be %d matrices of %d x %d" % (self.nb, self.N, self.N))
        self._cc_T = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, order="F")
                                                          for b in blocks]))
        tab = np.asfortranarray(np.asarray(trg_of).astype(np.int32))  # [src, k] -> trg_of[src + n*k]
        self._c(lib().dqmc_set_current_targets(self._h, tab.ctypes.data_as(C.POINTER(C.c_int32)), int(K), dptr(self._cc_T)))
        self._Kcc = int(K)
        self._binner_dropped("response_current")  # (the engine disables it: enable it again)
        self._ctd = 0  # (and turns the imaginary-time current recording off)
        # (the hopping goes into a checkpoint only where it is not the model's own)
        self._tables["current_targets"] = (np.array(tab, dtype=np.int32), self._Kcc,
                                           None if hopping is None else [float(x) for x in self._cc_T])

    def current_targets_fast_path(self):
        """True when the lattice took the LDS kernel for the current-current sums (see include/dqmc_hip.h)"""
        f = C.c_int32()
        self._c(lib().dqmc_current_targets_fast_path(self._h, C.byref(f)))
        return bool(f.value)

    def current_targets_plan(self):
        """-> dict(fast, C, umax, nchunks, chunks_per_wg, n_wg, threads, lds_bytes): the launch plan of the LDS kernel
        (all zero when no targets are set or the general kernel is taken; see include/dqmc_hip.h)"""
        out = (C.c_int32 * 8)()
        self._c(lib().dqmc_current_targets_plan(self._h, out))
        names = ("fast", "C", "umax", "nchunks", "chunks_per_wg", "n_wg", "threads", "lds_bytes")
        return dict(zip(names, (int(v) for v in out)))

    # ---- instrumentation
    def qr_fallbacks(self):
        """cooperative-QR launches that timed out and were redone by the single-workgroup kernel"""
        n = C.c_int64()
        self._c(lib().dqmc_qr_fallbacks(self._h, C.byref(n)))
        return n.value

    def kron_hopping(self):
        """True when slice products and wraps apply the hopping exponentials in factored form (16 x 16 Kronecker factors
        at n = 256, 8 x 8 at n = 512, the triangular 16 x 16 lattice's three factors, the t-t' square 16 x 16 lattice's four,
        the 16 x 16 x 2 bilayer's 2 x 2 (x) 16 x 16 (x) 16 x 16, the 32 x 8 rectangular lattice's 8 x 8 (x) 32 x 32;
        include/dqmc_hip.h)"""
        f = C.c_int32(0)
        self._c(lib().dqmc_kron_hopping(self._h, C.byref(f)))
        return bool(f.value)

    def udt_one_launch_sites(self):
        """bit mask of the udt_AVX_pivot! call sites served by the one-launch pre-pivoted factorisation (0: none)"""
        w = C.c_int32(0)
        self._c(lib().dqmc_udt_one_launch_sites(self._h, C.byref(w)))
        return int(w.value)

    def launch_plan(self):
        """dqmc_launch_plan: what the handle decided about its co-resident launch forms at creation, as a dict: units,
        units_padded, cus, udt_sites, udt_blocks (0: one-launch UDT not admitted), qr_coop_blocks, qr_coop (1 / 0),
        sweep_fused (1 / 0), wrap_blocks and wrap_one_launch (each a pair: without / with a pending sweep chunk; the wrap
        is never one launch on the triangular three-factor and the t-t' four-factor paths)"""
        out = (C.c_int32 * 12)()
        self._c(lib().dqmc_launch_plan(self._h, out))
        v = [int(x) for x in out]
        names = ("units", "units_padded", "cus", "udt_sites", "udt_blocks", "qr_coop_blocks", "qr_coop", "sweep_fused")
        plan = dict(zip(names, v))
        plan["wrap_blocks"] = (v[8], v[9])
        plan["wrap_one_launch"] = (v[10], v[11])
        return plan

    def device_errors(self):
        """device error word (0 unless a bounded wait inside a kernel ran out)"""
        w = C.c_int32(0)
        self._c(lib().dqmc_device_errors(self._h, C.byref(w)))
        return int(w.value)

    def timing_enable(self, on=True):
        self._c(lib().dqmc_timing_enable(self._h, int(on)))

    def timing(self):
        ms = np.zeros(len(_lib.K_FAMILIES))
        n = np.zeros(len(_lib.K_FAMILIES), dtype=np.int64)
        self._c(lib().dqmc_timing_get(self._h, dptr(ms), i64ptr(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.K_FAMILIES)}


def jackknife_ratio(sx, s):
    """The ratio estimate <O s> / <s> and its jackknife error over W independent walkers.  sx [W, E]: each walker's sum
    of s x, s [W]: its sum of s.  ratio = sum_w sx_w / sum_w s_w; leaving walker w out gives r_w = (sum sx - sx_w) /
    (sum s - s_w), and std_error = sqrt((W - 1) / W sum_w (r_w - mean r)^2).  ValueError below two walkers and when the
    sum of signs, or one with a walker left out, is 0."""
    sx, s = np.asarray(sx, dtype=np.float64), np.asarray(s, dtype=np.float64)
    W = s.shape[0]
    if W < 2:
        raise ValueError("the jackknife over walkers needs at least two walkers")
    S = s.sum()
    if S == 0 or np.any(S - s == 0):
        raise ValueError("the sum of signs is 0 (over all walkers, or with one left out): the ratio is undefined")
    tot = sx.sum(axis=0)
    r = (tot[None, :] - sx) / (S - s)[:, None]
    return tot / S, np.sqrt((W - 1) / W * ((r - r.mean(axis=0)) ** 2).sum(axis=0))


def matsubara_trapezoid(x, tau, omega):
    """sum_r h w_r cos(omega_m tau_r) x[r] over the uniform grid tau [R] (h its spacing, w_0 = w_{R-1} = 1/2, else 1) for
    every omega_m: x [R, ...] -> [len(omega), ...]"""
    x, tau, omega = np.asarray(x), np.asarray(tau, dtype=np.float64), np.atleast_1d(np.asarray(omega, dtype=np.float64))
    if tau.size < 2 or x.shape[0] != tau.size:
        raise ValueError("matsubara_trapezoid needs at least two rows, one per tau")
    w = np.ones(tau.size)
    w[0] = w[-1] = 0.5
    kern = (tau[1] - tau[0]) * w[None, :] * np.cos(omega[:, None] * tau[None, :])  # [m, r]
    return np.tensordot(kern, x, axes=(1, 0))


class CurrentTauSums:
    """The per-walker sums of the imaginary-time current recording (include/dqmc_hip.h), [W, P] with P = 2 R K n_q + K + 3:
    per walker [C: R x K x n_q][S: R x K x n_q][kbond: K][sum of s_w][samples kept][samples left out].  estimate(f) gives
    f of the ratio estimates (sum over walkers of the sums / sum of signs; without sign weighting the sum of signs is the
    number of samples) and, through f, the delete-one-walker jackknife error of every entry of its result.
    `could_leave_out`: a walker's samples can be left out (sign weighting), the jackknife then needs three walkers."""

    def __init__(self, sums, R, K, n_q, could_leave_out=False):
        sums = np.asarray(sums, dtype=np.float64)
        self.R, self.K, self.n_q = int(R), int(K), int(n_q)
        self.E = 2 * self.R * self.K * self.n_q + self.K
        if sums.ndim != 2 or sums.shape[1] != self.E + 3:
            raise ValueError("sums must be [n_walkers, 2 R K n_q + K + 3]")
        self.W = sums.shape[0]
        self.sx, self.s = sums[:, :self.E], sums[:, self.E]
        self.count, self.left_out = int(sums[:, self.E + 1].sum()), int(sums[:, self.E + 2].sum())
        self.min_walkers = 3 if could_leave_out else 2

    def _split(self, v):
        n = self.R * self.K * self.n_q
        shape = (self.R, self.K, self.n_q)
        return v[:n].reshape(shape), v[n:2 * n].reshape(shape), v[2 * n:]

    def estimate(self, f):
        """f(C [R, K, n_q], S [R, K, n_q], kbond [K]) -> dict of arrays / scalars; -> the dict at the ratio estimate, each
        real X with X_std_error, each complex X with X_std_error_re / X_std_error_im (where the jackknife has enough
        walkers).  ValueError when the sum of signs, or one with a walker left out, is 0."""
        S = self.s.sum()
        if S == 0:
            raise ValueError("current_time_displaced: the sum of signs is 0 over %d samples: <O s> / <s> is undefined" % self.count)
        tot = self.sx.sum(axis=0)
        res = {k: np.asarray(v) for k, v in f(*self._split(tot / S)).items()}
        if self.W >= self.min_walkers:
            if np.any(S - self.s == 0):
                raise ValueError("the sum of signs is 0 with one walker left out: the ratio is undefined")
            loo = [f(*self._split((tot - self.sx[w]) / (S - self.s[w]))) for w in range(self.W)]
            for k in list(res):
                r = np.stack([np.asarray(l[k]) for l in loo])
                d = r - r.mean(axis=0)
                fac = (self.W - 1) / self.W
                if np.iscomplexobj(r):
                    res[k + "_std_error_re"] = np.sqrt(fac * (d.real ** 2).sum(axis=0))
                    res[k + "_std_error_im"] = np.sqrt(fac * (d.imag ** 2).sum(axis=0))
                else:
                    res[k + "_std_error"] = np.sqrt(fac * (d ** 2).sum(axis=0))
        return res


def entanglement_from_pair_sums(pair_sums, count):
    """Tr rho_A^2 and S2 = -log Tr rho_A^2 from the pair sums of DQMC.entanglement(): pair_sums [n_sub, W, W] (or [W, W])
    holds sum over `count` samples of x(w, w') in its strictly upper triangle, which alone is read.  purity = sum over
    pairs / (count W (W - 1) / 2).  With three walkers and more, S2_std_error is the delete-one-walker jackknife of
    -log(mean): leaving walker w out drops its W - 1 pairs, S2_w = -log of the mean over the other (W - 1)(W - 2) / 2
    pairs, std_error = sqrt((W - 1) / W sum_w (S2_w - mean S2_w)^2).  A purity <= 0 gives S2 = nan."""
    ps = np.asarray(pair_sums, dtype=np.float64)
    single = ps.ndim == 2
    ps = ps[None] if single else ps
    W = ps.shape[-1]
    if ps.ndim != 3 or ps.shape[1] != W or W < 2:
        raise ValueError("pair_sums must be [n_sub, W, W] with W >= 2")
    if int(count) < 1:
        raise ValueError("entanglement_from_pair_sums needs at least one sample")
    up = np.triu(ps, 1)
    tot = up.sum(axis=(1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        purity = tot / (count * W * (W - 1) / 2.0)
        res = {"purity": purity, "S2": -np.log(purity)}
        if W >= 3:
            mine = up.sum(axis=2) + up.sum(axis=1)  # [n_sub, W]: the pairs walker w is part of
            s2 = -np.log((tot[:, None] - mine) / (count * (W - 1) * (W - 2) / 2.0))
            res["S2_std_error"] = np.sqrt((W - 1) / W * ((s2 - s2.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    return {k: v[0] for k, v in res.items()} if single else res


def check_covariance_bins(n_bins, n_tau, who="spectral_function"):
    """a covariance of `n_tau` time slices estimated from `n_bins` bins has rank n_bins - 1 at most: it can be inverted
    only with n_bins > n_tau.  A condition, not a tolerance: ERR_STATE otherwise."""
    if not int(n_bins) > int(n_tau):
        raise _lib.DQMCError(_lib.ERR_STATE, "%s: %d closed bins for %d time slices: the covariance is singular by "
                             "construction; it needs more bins than slices" % (who, int(n_bins), int(n_tau)))


def tau_covariance_from_moments(list_of_moments):
    """Pools the per-walker moments of DQMC.tau_covariance_moments() / user_covariance_result(), one dict per rank (or a
    single dict): nb [W], shift, S1 [W, S, R], S2 [W, S, R, R].  Per walker the bins have the mean c + S1 / nb and the
    scatter M2 = S2 - S1 S1^T / nb about it (the sums are of deviations from the shift c, so nothing large cancels);
    walkers and ranks are chains at the same parameters, so their bins pool into one sample of n_bins = sum nb_w with the
    pairwise update of Chan, Golub and LeVeque, in float64 and in the order given: n = n_a + n_b, delta = mean_b - mean_a,
    mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta delta^T n_a n_b / n.
    -> dict(mean [S, R], n_bins, cov [S, R, R] = M2 / (n_bins (n_bins - 1)), the covariance of the mean (nan below two
    bins), M2 [S, R, R])."""
    if isinstance(list_of_moments, dict):
        list_of_moments = [list_of_moments]
    n, mean, M2 = 0, None, None
    for m in list_of_moments:
        nb = np.asarray(m["nb"], dtype=np.int64).reshape(-1)
        c, S1, S2 = (np.asarray(m[k], dtype=np.float64) for k in ("shift", "S1", "S2"))
        if S1.ndim != 3 or c.shape != S1.shape or S2.shape != S1.shape + S1.shape[-1:] or nb.size != S1.shape[0]:
            raise ValueError("moments must hold nb [W], shift and S1 [W, S, R], S2 [W, S, R, R]")
        if mean is not None and mean.shape != S1.shape[1:]:
            raise ValueError("the moments of every rank must have the same series and rows")
        for w in range(nb.size):
            k = int(nb[w])
            if k < 1:
                continue
            mw = c[w] + S1[w] / k
            Mw = S2[w] - S1[w][:, :, None] * S1[w][:, None, :] / k
            if mean is None:
                n, mean, M2 = k, mw, Mw
                continue
            delta = mw - mean
            tot = n + k
            mean = mean + delta * (k / tot)
            M2 = M2 + Mw + delta[:, :, None] * delta[:, None, :] * (n * k / tot)
            n = tot
    if mean is None:
        raise ValueError("tau_covariance_from_moments: no closed bin")
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = M2 / (n * (n - 1.0)) if n > 1 else np.full_like(M2, np.nan)
    return {"mean": mean, "n_bins": n, "cov": cov, "M2": M2}


def finish_moments(buf):
    """Reduced binner moments (DQMC.binner_moments summed over ranks: [sum mean_w][sum mean_w^2][sum varN_w(level)]
    [sum varN_w(0)][W]) -> dict of flat arrays mean, std_error, std_error_walkers, tau and n_walkers, with the formulas of
    include/dqmc_hip.h: mean = S1/W, std_error = sqrt(Vl)/W, tau = (Vl/V0 - 1)/2, std_error_walkers =
    sqrt((S2 - S1^2/W) / (W (W - 1)))."""
    if hasattr(buf, "detach"):
        buf = buf.detach().cpu().numpy()
    buf = np.asarray(buf, dtype=np.float64)
    E, W = (buf.size - 1) // 4, buf[-1]
    if buf.ndim != 1 or buf.size != 4 * E + 1 or W < 1:
        raise ValueError("not a binner moment buffer")
    s1, s2, vl, v0 = (buf[i * E:(i + 1) * E] for i in range(4))
    with np.errstate(invalid="ignore", divide="ignore"):
        between = np.maximum(s2 - s1 * s1 / W, 0.0) / (W * (W - 1)) if W >= 2 else np.full(E, np.nan)
        return dict(mean=s1 / W, std_error=np.sqrt(np.where(vl < 0, 0.0, vl)) / W, std_error_walkers=np.sqrt(between),
                    tau=0.5 * (vl / v0 - 1.0), n_walkers=int(W))


# ---------------------------------------------------------------------------
# batched linalg primitives (src/linalg), host arrays in/out
def _batch(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    return a


def _pack(mats):
    return np.ascontiguousarray(np.concatenate([m.reshape(-1, order="F") for m in mats]))


def _unpack(flat, batch, n):
    return np.stack([flat[i * n * n:(i + 1) * n * n].reshape((n, n), order="F") for i in range(batch)])


def vmul(A, B, transa=False, transb=False, device_id=0):
    """vmul!(C, A, B) and its adjoint/transpose variants (general.jl:7-56)"""
    A, B = _batch(A), _batch(B)
    batch, n = A.shape[0], A.shape[1]
    a, b = _pack(A), _pack(B)
    c = np.zeros_like(a)
    check(lib().dqmc_vmul(device_id, n, batch, int(transa), int(transb), dptr(a), dptr(b), dptr(c)))
    return _unpack(c, batch, n)


def udt_AVX_pivot(X, apply_pivot=True, device_id=0):
    """udt_AVX_pivot!(U, D, T, pivot, temp, Val(apply)) (UDT.jl:192-306) -> U, D, T, pivot(1-based)"""
    X = _batch(X)
    batch, n = X.shape[0], X.shape[1]
    t = _pack(X)
    u = np.zeros_like(t)
    d = np.zeros(batch * n)
    piv = np.zeros(batch * n, dtype=np.int64)
    check(lib().dqmc_udt_pivot(device_id, n, batch, dptr(u), dptr(d), dptr(t), i64ptr(piv), int(apply_pivot)))
    return _unpack(u, batch, n), d.reshape(batch, n), _unpack(t, batch, n), piv.reshape(batch, n)


def logdet_matrices(A, D, n, strideA=None, strideD=None, device_id=0):
    """logdet_kernel (csrc/logdet.hip) on the caller's matrices: A flat, unit u column-major at u * strideA, D flat at
    u * strideD -> logabsdet [batch], sign [batch], and A and D as the device left them"""
    strideA = n * n if strideA is None else int(strideA)
    strideD = n if strideD is None else int(strideD)
    a = np.array(A, dtype=np.float64).reshape(-1)
    d = np.array(D, dtype=np.float64).reshape(-1)
    batch = a.size // strideA
    if batch < 1 or a.size != batch * strideA or d.size != batch * strideD:
        raise ValueError("A and D must hold batch * strideA and batch * strideD numbers")
    lad = np.zeros(batch)
    sg = np.zeros(batch, dtype=np.int32)
    check(lib().dqmc_logdet_matrices(device_id, n, batch, dptr(a), strideA, dptr(d), strideD, dptr(lad),
                                     sg.ctypes.data_as(C.POINTER(C.c_int32))))
    return lad, sg, a, d


def rdivp(A, T, pivot, device_id=0):
    """rdivp!(A, T, O, pivot) (general.jl:138-166)"""
    A, T = _batch(A), _batch(T)
    batch, n = A.shape[0], A.shape[1]
    a, t = _pack(A), _pack(T)
    piv = np.ascontiguousarray(np.asarray(pivot, dtype=np.int64).reshape(-1))
    check(lib().dqmc_rdivp(device_id, n, batch, dptr(a), dptr(t), i64ptr(piv)))
    return _unpack(a, batch, n)


def calculate_greens_AVX(Ul, Dl, Tl, Ur, Dr, Tr, device_id=0):
    """calculate_greens_AVX! (stack.jl:337-393)"""
    Ul, Tl, Ur, Tr = _batch(Ul), _batch(Tl), _batch(Ur), _batch(Tr)
    batch, n = Ul.shape[0], Ul.shape[1]
    dl = np.ascontiguousarray(np.asarray(Dl, dtype=np.float64).reshape(-1))
    dr = np.ascontiguousarray(np.asarray(Dr, dtype=np.float64).reshape(-1))
    g = np.zeros(batch * n * n)
    check(lib().dqmc_calculate_greens(device_id, n, batch, dptr(_pack(Ul)), dptr(dl), dptr(_pack(Tl)),
                                      dptr(_pack(Ur)), dptr(dr), dptr(_pack(Tr)), dptr(g)))
    return _unpack(g, batch, n)


def mfma_f64_peak(iters=20000, device_id=0):
    t = C.c_double()
    check(lib().dqmc_mfma_f64_peak(device_id, iters, C.byref(t)))
    return t.value


def device_count():
    return lib().dqmc_device_count()
