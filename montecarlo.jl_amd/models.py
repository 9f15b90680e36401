"""Hubbard models as the DQMC stack sees them (src/models/HubbardModel/*.jl).

The structs carry exactly the fields the hot path reads (U, t, mu, l, flv); the
performance-critical methods (interaction_matrix_exp!, propose_local,
accept_local!) live on the device behind dqmc_sweep_spatial / dqmc_propagate."""
import numpy as np

from .lattices import BilayerSquareLattice, Chain, CubicLattice, RectangularLattice, SquareLattice


def _check_tp(tp, l):
    """next-nearest-neighbour hopping is defined on the square and rectangular lattices only (the ones with an nnn table)"""
    tp = float(tp)
    if tp != 0.0 and not isinstance(l, (SquareLattice, RectangularLattice)):
        raise ValueError("tp != 0 needs a SquareLattice or RectangularLattice, not %s" % type(l).__name__)
    return tp


def _check_t_perp(t_perp, t, l):
    """the interlayer hopping of a BilayerSquareLattice (None: t); no other lattice has one"""
    if isinstance(l, BilayerSquareLattice):
        return float(t) if t_perp is None else float(t_perp)
    if t_perp is not None:
        raise ValueError("t_perp needs a BilayerSquareLattice, not %s" % type(l).__name__)
    return None


def _add_hopping(T, l, t, t_perp):
    """-t at T[trg, src] for every directed nearest-neighbour pair (+=: coinciding neighbours count twice); on a
    BilayerSquareLattice -t_perp on the perp row of neighs (the fifth target of every source)"""
    if t_perp is None:
        for src, trg in l.neighbors(True):
            T[trg - 1, src - 1] += -t
        return
    for k, (src, trg) in enumerate(l.neighbors(True)):
        T[trg - 1, src - 1] += -(t_perp if k % 5 == 4 else t)


def _add_tp(T, l, tp):
    """-tp at T[trg, src] for the four diagonal neighbours of every source (+=, as the nearest neighbours are added: at
    L = 2 the coinciding diagonals count twice)"""
    for src, trg in l.next_neighbors(True):
        T[trg - 1, src - 1] += -tp


def choose_lattice(dims, L):
    """HubbardModel.jl:23-31"""
    if dims == 1:
        return Chain(L)
    if dims == 2:
        return SquareLattice(L)
    return CubicLattice(dims, L)


class HubbardModelAttractive:
    """HubbardModelAttractive.jl:26-39; U is stored positive.  `tp` is the next-nearest-neighbour hopping t' of
    H = -t sum_<ij> - t' sum_<<ij>> - mu sum n + U-term on a SquareLattice (an extension; tp = 0: the reference's matrices).
    `t_perp` is the interlayer hopping of a BilayerSquareLattice (None there: t; any value on another lattice: ValueError)."""
    flv = 1
    kind = 0

    def __init__(self, L=None, dims=None, l=None, U=1.0, t=1.0, mu=0.0, tp=0.0, t_perp=None):
        if U < 0:
            raise ValueError("U must be positive.")  # @assert U >= 0.
        self.l = l if l is not None else choose_lattice(dims, L)
        self.U, self.t, self.mu = float(U), float(t), float(mu)
        self.tp = _check_tp(tp, self.l)
        self.t_perp = _check_t_perp(t_perp, self.t, self.l)

    def hopping_matrix(self):
        """HubbardModelAttractive.jl:78-91"""
        N = len(self.l)
        T = np.diag(np.full(N, -self.mu))
        _add_hopping(T, self.l, self.t, self.t_perp)
        if self.tp != 0.0:
            _add_tp(T, self.l, self.tp)
        return [T]


class HubbardModelRepulsive:
    """HubbardModelRepulsive.jl:24-41; two spin blocks (BlockDiagonal, :68-69).  The reference fixes mu at 0; here `mu`
    dopes the model: -mu on the diagonal of both blocks, as in the attractive model (mu = 0: the reference's matrices).
    `tp`: the next-nearest-neighbour hopping t' on a SquareLattice, `t_perp`: the interlayer hopping of a
    BilayerSquareLattice, both as in the attractive model."""
    flv = 2
    kind = 1

    def __init__(self, L=None, dims=None, l=None, U=1.0, t=1.0, mu=0.0, tp=0.0, t_perp=None):
        if U < 0:
            raise ValueError("U must be positive.")
        self.l = l if l is not None else choose_lattice(dims, L)
        self.U, self.t, self.mu = float(U), float(t), float(mu)
        self.tp = _check_tp(tp, self.l)
        self.t_perp = _check_t_perp(t_perp, self.t, self.l)

    def hopping_matrix(self):
        """HubbardModelRepulsive.jl:87-100: BlockDiagonal(T, copy(T)), with -mu on the diagonal"""
        N = len(self.l)
        T = np.zeros((N, N))
        if self.mu != 0.0:
            T[np.diag_indices(N)] = -self.mu
        _add_hopping(T, self.l, self.t, self.t_perp)
        if self.tp != 0.0:
            _add_tp(T, self.l, self.tp)
        return [T, T.copy()]


def HubbardModel(*args, U, **kwargs):
    """HubbardModel.jl:14-20: U > 0 repulsive, else attractive with U -> -U"""
    if U > 0.0:
        return HubbardModelRepulsive(*args, U=U, **kwargs)
    return HubbardModelAttractive(*args, U=-U, **kwargs)


def rand_conf(rng, n_sites, slices):
    """rand(DQMC, m, nslices) (HubbardModel.jl:46-48): Int8 ±1, filled column-major."""
    flat = rng.integers(0, 2, size=n_sites * slices, dtype=np.int8) * 2 - 1
    return np.asfortranarray(flat.reshape((n_sites, slices), order="F").astype(np.int8))
