"""The classical MC flavor (src/flavors/MC/MC.jl) with the IsingModel (src/models/Ising/IsingModel.jl,
measurements.jl), `n_walkers` independent Markov chains batched on one device (csrc/ising.hip).

Walker w draws from the Philox4x32-10 stream keyed by `seed + first_walker + w`: draws 0..N-1 give the initial
configuration (rand(MC, m)), the Metropolis uniforms follow.  The Wolff cluster move (`cluster_moves=True`) draws from a
domain of its own of the same key (include/dqmc_hip.h, dqmc_mc_global_move), and so does replica exchange
(`n_replicas`, `exchange_rate`; dqmc_mc_set_exchange).  The host holds the model, the loop control
and finish!; every site update runs on the device."""
import ctypes as C
import math
import time

import numpy as np

from . import checkpoint as _ckpt
from ._lib import (DQMCError, ERR_INVALID, ERR_STATE, MC_UPDATE_KINDS, McBinned, McExchangeStats, McFss, McFssBinned,
                   McGlobalStats, McParams, McStats, McUpdateStats, lib)
from .configurations import CompressedConf
from .lattices import Chain, CubicLattice, SquareLattice, _lattice_vectors, _positions

IsingTc = 1.0 / (0.5 * math.log(1.0 + math.sqrt(2.0)))  # IsingModel.jl:7


def _choose_lattice(dims, L):
    """choose_lattice(IsingModel, dims, L) (IsingModel.jl:26-35)"""
    if dims == 1:
        return Chain(L)
    if dims == 2:
        return SquareLattice(L)
    return CubicLattice(dims, L)


class IsingModel:
    """IsingModel(; dims, L) (IsingModel.jl:17-22); any project lattice may be given as `l`."""

    def __init__(self, dims=None, L=None, l=None):
        if l is None:
            if dims is None or L is None:
                raise ValueError("IsingModel needs dims and L, or a lattice l")
            l = _choose_lattice(dims, L)
        self.l = l
        self.L = L if L is not None else getattr(l, "L", len(l))
        self.dims = dims if dims is not None else getattr(l, "dim", 2 if hasattr(l, "lattice") else 1)

    def __len__(self):
        return len(self.l)

    def energy(self, conf):
        """energy(mc, m, conf) (IsingModel.jl:149-186): -sum over the undirected bonds table, for any integer spins"""
        c = np.asarray(conf).reshape(-1, order="F").astype(np.int64)
        b = np.asarray(self.l.bonds, dtype=np.int64)[:, :2] - 1
        return float(-np.sum(c[b[:, 0]] * c[b[:, 1]]))

    def propose_local(self, i, conf):
        """propose_local(mc, m, i, conf) (IsingModel.jl:85-101): delta_E = 2 conf[i] sum_{j in neighs[:, i]} conf[j],
        i 1-based"""
        c = np.asarray(conf).reshape(-1, order="F").astype(np.int64)
        return 2.0 * float(c[i - 1]) * float(np.sum(c[np.asarray(self.l.neighs)[:, i - 1] - 1]))


def reciprocal_vectors(l):
    """the smallest wave vectors of the lattice, one per lattice dimension: the columns b_j of B with A^T B = 2 pi I,
    A's columns the lattice vectors (a_i . b_j = 2 pi delta_ij), returned as rows"""
    A = np.array(_lattice_vectors(l), dtype=float).T
    return (2.0 * np.pi * np.linalg.inv(A.T)).T.copy()


def _llround(x):
    """half away from zero, as C's llround; int64"""
    x = np.asarray(x, dtype=np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def q30_tables(l, k_vectors):
    """(cos_q30, sin_q30, k): int32 [n_k][N] with llround(cos(k . r_i) 2^30) and the sine likewise, r_i =
    lattices._positions(l) in the site order of mc.conf (include/dqmc_hip.h, "finite-size-scaling observables")"""
    r = np.array(_positions(l), dtype=float)
    k = np.array(k_vectors, dtype=float).reshape(-1, r.shape[1]) if len(k_vectors) else np.zeros((0, r.shape[1]))
    if len(k) > 8:
        raise ValueError("FSS: at most 8 wave vectors")
    ph = k @ r.T

    return (np.ascontiguousarray(_llround(np.cos(ph) * 2.0 ** 30).astype(np.int32)),
            np.ascontiguousarray(_llround(np.sin(ph) * 2.0 ** 30).astype(np.int32)), k)


def greedy_colouring(l):
    """the default colouring of update="checkerboard" (dqmc_mc_set_update): in site order, the smallest colour not used
    by an already-coloured neighbour j < i; int32 [N].  Two colours on the bipartite lattices (even chains, even square
    and cubic lattices), three or four on odd ones and on the triangular lattice.  A site that lists itself as a
    neighbour (the 1-site chain) cannot be coloured: ValueError."""
    nb = np.asarray(l.neighs, dtype=np.int64) - 1
    N = nb.shape[1]
    colour = np.full(N, -1, dtype=np.int32)
    for i in range(N):
        if np.any(nb[:, i] == i):
            raise ValueError("greedy_colouring: site %d lists itself as a neighbour" % i)
        used = {int(colour[j]) for j in nb[:, i] if j < i}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return colour


def _binder(M2, M4):
    """U4 = 1 - <M4> / (3 <M2>^2) and its gradient with respect to (M2, M4)"""
    return 1.0 - M4 / (3.0 * M2 * M2), (2.0 * M4 / (3.0 * M2 ** 3), -1.0 / (3.0 * M2 * M2))


def _xi(M2, S, N, knorm):
    """xi = sqrt(S(0) / S(k) - 1) / (2 sin(|k| / 2)) with S(0) = <M2> / N and its gradient with respect to (M2, S);
    NaN where S(0) < S(k)"""
    c = 1.0 / (2.0 * math.sin(0.5 * knorm))
    with np.errstate(invalid="ignore", divide="ignore"):
        root = float(np.sqrt(np.float64(M2) / (N * np.float64(S)) - 1.0))
        g = np.float64(c) / (2.0 * np.float64(root))
        return c * root, (float(g / (N * S)), float(-g * M2 / (N * S * S)))


def _delta_var(grad, vx, vy, cov):
    """first-order variance of f(x, y) from the variances of the means and their covariance"""
    var = grad[0] * grad[0] * vx + grad[1] * grad[1] * vy + 2.0 * grad[0] * grad[1] * cov
    return max(var, 0.0) if var == var else var


def pool_walkers(method, betas, walker, walkers, per_walker, derived_tau=None):
    """The binned results of one walker, or of several chains of equal beta pooled (MC.binned's docstring has the
    formulas).  `walkers` None: the single `walker`, not pooled.  per_walker(w) gives (obs, count, level) of walker w,
    obs = {name: entry or [entry, ..]} with entry = (mean, variance of the mean at `level`, the same at level 0, or None
    for a derived observable, which is no time series); it is asked only once the walkers have passed the checks, which
    raise ValueError under the calling `method`'s name.  Returns {name: pooled or [pooled, ..], "count", "level"} (count
    and level of the first walker; they are the same for all), pooled = {mean, std_error, tau}, where a derived
    observable gets tau = derived_tau, or no tau key for derived_tau None; pooling adds std_error_walkers (NaN for one
    walker) to every entry and n_walkers to the result.  Needs no handle."""
    pooled = walkers is not None
    ws = [int(w) for w in walkers] if pooled else [walker]
    if not ws:
        raise ValueError("%s: no walker given" % method)
    if any(betas[w] != betas[ws[0]] for w in ws):
        raise ValueError("%s: the pooled walkers must share one beta" % method)
    per = [per_walker(w) for w in ws]
    W = float(len(ws))

    def pool(entries):
        means = np.array([e[0] for e in entries])
        vl = float(np.sum([e[1] for e in entries]))
        mean = float(means.sum() / W)
        o = {"mean": mean, "std_error": (math.sqrt(max(vl, 0.0)) if vl == vl else vl) / W}
        if entries[0][2] is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                o["tau"] = float(0.5 * (np.float64(vl) / np.sum([e[2] for e in entries]) - 1.0))
        elif derived_tau is not None:
            o["tau"] = derived_tau
        if pooled:
            o["std_error_walkers"] = (math.sqrt(float(((means - mean) ** 2).sum()) / (W * (W - 1.0)))
                                      if W >= 2 else float("nan"))
        return o

    out = {"count": per[0][1], "level": per[0][2]}
    for name, first in per[0][0].items():
        if isinstance(first, list):
            out[name] = [pool([p[0][name][k] for p in per]) for k in range(len(first))]
        else:
            out[name] = pool([p[0][name] for p in per])
    if pooled:
        out["n_walkers"] = len(ws)
    return out


class _MCBase:
    """What MC and qstate.QStateMC share: the handle of one engine's ABI family (`_abi`: "dqmc_mc_" / "dqmc_qs_", whose
    create, destroy, last_error, seed, set_beta, rand_conf, sweep, reset_accumulators, synchronize, the exchange calls
    and the binner calls have one shape), the temperatures, the colouring argument, replica exchange, the binner's
    sections and the run! loop.  A subclass has stats(walker) with acc_local and prop_local, and names the ctypes
    struct of its exchange stats (`_ExchangeStats`)."""
    _abi = None
    _ExchangeStats = None

    def _call(self, name, *args):
        self._c(getattr(lib(), self._abi + name)(self._h, *args))

    @staticmethod
    def _resolve_beta(beta, T):
        if (beta is None) == (T is None):
            raise ValueError("MC needs exactly one of beta and T")
        if T is not None:
            beta = (1.0 / np.asarray(T, dtype=float)) if np.ndim(T) else 1.0 / float(T)
        return np.asarray(beta, dtype=float)

    def _init_common(self, model, beta, n_walkers, seed, first_walker, thermalization, sweeps, measure_rate, print_rate,
                     series_capacity):
        betas = np.broadcast_to(beta, (n_walkers,)).copy()
        if not np.all(np.isfinite(betas)) or np.any(betas < 0):
            raise ValueError("beta must be finite and >= 0")
        if measure_rate < 1:
            raise ValueError("measure_rate must be >= 1")
        self.model = model
        self.N = len(model.l)
        self.n_walkers = n_walkers
        self.betas = betas
        self.beta = float(betas[0]) if np.all(betas == betas[0]) else betas
        self.seeds = [seed + first_walker + w for w in range(n_walkers)]
        self._seed0, self._first_walker = seed, first_walker  # (what a checkpoint's preamble writes down)
        self._binning = None  # the capacity enable_binning was last given (0: the default); None: no binner
        self.thermalization, self.sweeps, self.measure_rate = thermalization, sweeps, measure_rate
        self.print_rate = print_rate
        self.last_sweep = 0
        self.series_capacity = series_capacity
        self._neighs = np.asfortranarray(np.asarray(model.l.neighs, dtype=np.int64))
        self._bonds = np.asfortranarray(np.asarray(model.l.bonds, dtype=np.int64)[:, :2])

    def _create(self, params):
        """the handle for `params`, every walker seeded, at its beta and with a random configuration (init!, MC.jl:61,74)"""
        h = C.c_void_p()
        self._h = None
        rc = getattr(lib(), self._abi + "create")(C.byref(params), C.byref(h))
        if rc != 0:
            msg = getattr(lib(), self._abi + "last_error")(None)
            raise DQMCError(rc, msg.decode() if msg else "")
        self._h = h
        for w in range(self.n_walkers):
            self._call("seed", w, self.seeds[w])
            self._call("set_beta", w, float(self.betas[w]))
        self._call("rand_conf", -1)

    def _colours(self, colouring, what):
        """(int32 [N], n_colours) of a colouring argument; None: greedy_colouring(lattice)"""
        col = greedy_colouring(self.model.l) if colouring is None else colouring
        col = np.ascontiguousarray(np.asarray(col).reshape(-1), dtype=np.int32)
        if col.size != self.N:
            raise DQMCError(ERR_INVALID, "%s: expected %d colours" % (what, self.N))
        return col, (int(col.max()) + 1 if col.size else 0)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(lib(), self._abi + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        if rc != 0:
            msg = getattr(lib(), self._abi + "last_error")(self._h)
            raise DQMCError(rc, msg.decode() if msg else "")

    # ---- state
    def seed(self, walker, seed):
        """key the walker's streams with `seed`, every cursor at 0 (the configuration stays)"""
        self._call("seed", walker, seed)
        self.seeds[walker] = seed

    def set_beta(self, walker, beta):
        self._call("set_beta", walker, float(beta))
        self.betas[walker] = float(beta)

    def rand_conf(self, walker=-1):
        self._call("rand_conf", walker)

    def reset_accumulators(self):
        self._call("reset_accumulators")

    def synchronize(self):
        self._call("synchronize")

    # ---- replica exchange
    def set_exchange(self, n_replicas, rate):
        """dqmc_*_set_exchange: ladders of n_replicas consecutive walkers (0 or 1: none), a round after every rate-th
        sweep (0: none; the q-state engine runs it behind its cluster move and before its measurement); resets the
        exchange cursor, the replica labels and the exchange counters"""
        self._call("set_exchange", int(n_replicas), int(rate))
        self.n_replicas, self.exchange_rate = int(n_replicas), int(rate)

    def exchange(self):
        """one exchange round by hand (dqmc_*_exchange), counted in the exchange stats, no measurement"""
        self._call("exchange")

    def exchange_stats(self, walker=0):
        """prop_exchange and acc_exchange of the pair (walker, walker + 1), the label `replica` of the configuration
        now in the slot, and `rounds` (the exchange cursor)"""
        st = self._ExchangeStats()
        self._call("get_exchange_stats", walker, C.byref(st))
        return st

    def replicas(self):
        """the replica labels of all slots: replicas()[w] is the ladder-local index of the slot in which the
        configuration now in slot w started"""
        return np.array([self.exchange_stats(w).replica for w in range(self.n_walkers)], dtype=np.int64)

    # ---- the binner: the main section and, with the `prefix` of their calls ("fss_", "scaling_", "stiffness_"), the
    # sections of the measurements that have one
    def enable_binning(self, capacity=None):
        """a logarithmic binner (LogBinner) per walker over the engine's main elements - MC: [E, E2, |M|, M2], QStateMC:
        [E, E2, |M|, M2, M2, M4] - (capacity None: 100000 measurements), pushed on the device where the measurement is
        taken; enabling again starts anew.  A sweep() whose measurements would pass the capacity raises before
        anything runs."""
        self._call("binner_enable", 0 if capacity is None else int(capacity))
        self._binning = 0 if capacity is None else int(capacity)

    def binner_size(self):
        """(levels, pushes so far)"""
        L, T = C.c_int32(), C.c_int64()
        self._call("binner_size", C.byref(L), C.byref(T))
        return L.value, T.value

    def binner_reliable_level(self):
        lv = C.c_int32()
        self._call("binner_reliable_level", C.byref(lv))
        return lv.value

    def _section_level(self, prefix, n_elem, n_pairs, walker, level):
        """(x_sum[n_elem], x2_sum[n_elem], xy_sum[n_pairs], count) of one level of one walker of a section"""
        xs, x2, xy, n = np.zeros(max(n_elem, 1)), np.zeros(max(n_elem, 1)), np.zeros(max(n_pairs, 1)), C.c_int64()
        dp = C.POINTER(C.c_double)
        self._call(prefix + "binner_get_level", walker, level, xs.ctypes.data_as(dp), x2.ctypes.data_as(dp),
                   xy.ctypes.data_as(dp), C.byref(n))
        return xs[:n_elem], x2[:n_elem], xy[:n_pairs], n.value

    def _section_finish(self, prefix, Struct, walker, level):
        """the section's dqmc_*_binned (`Struct`) of one walker at `level` (None: the reliable level)"""
        out = Struct()
        self._call(prefix + "binner_finish", walker, -1 if level is None else int(level), C.byref(out))
        return out

    # ---- the loop
    def sweep(self, n=1):
        """n x sweep(mc) with run!'s measurement rule, continuing from last_sweep"""
        if n > 0:
            self._call("sweep", n, self.last_sweep + 1, self.thermalization, self.measure_rate)
            self.last_sweep += n

    def _print_mark(self):
        """run(verbose=True): what _print_more needs from before the first print window"""
        return None

    def _print_more(self, mark):
        """run(verbose=True): the lines behind the local acceptance rate; returns the next window's mark"""
        return mark

    # ---- checkpoint and resume (include/dqmc_hip.h "checkpoint and resume of the classical MC flavor"; the file:
    # checkpoint.py, the container of DQMC.save with a "flavor" key in the preamble)
    _flavor = None  # "mc_ising" / "mc_qstate"

    def state_size(self):
        n = C.c_size_t()
        self._call("state_size", C.byref(n))
        return n.value

    def state(self):
        """dqmc_*_state_export: the engine's state as a numpy.uint8 array - configurations, Philox keys, every cursor, the
        running energy and magnetization, the sums, counters, series, replica labels and every binner level.  Between any
        two calls; the chains are left exactly as they were."""
        buf = np.empty(self.state_size(), dtype=np.uint8)
        self._call("state_export", buf.ctypes.data, buf.size)
        return buf

    def set_state(self, blob):
        """dqmc_*_state_import into this object, which must be configured as the exporting one was (walkers, lattice,
        model tables, betas, colouring, update, cluster and exchange settings, binner, FSS / scaling, stiffness):
        ERR_INVALID naming the first field that differs otherwise, and the object stays as it was.  Afterwards the chains
        continue bit for bit as the exporting object's would have."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        self._call("state_import", blob.ctypes.data, blob.size)

    @staticmethod
    def _lattice_entry(l):
        from .dqmc import DQMC
        args = DQMC._lattice_args(type(l).__name__)
        if args is None:
            raise ValueError("save(): %s is not a lattice a checkpoint can name" % type(l).__name__)
        return {"class": type(l).__name__, "args": [int(getattr(l, a)) for a in args]}

    @staticmethod
    def _lattice_from_entry(entry):
        from . import lattices as _lat
        from .dqmc import DQMC
        if DQMC._lattice_args(entry["class"]) is None:
            raise _ckpt.CheckpointError("the checkpoint names an unknown lattice")
        return getattr(_lat, entry["class"])(*entry["args"])

    def _preamble(self):
        """everything load() needs to build and configure the object again; `mc` holds the constructor's keywords"""
        return {"format": 1, "flavor": self._flavor, "model": self._model_entry(self.model),
                "lattice": self._lattice_entry(self.model.l),
                "mc": dict(self._settings(), beta=[float(b) for b in self.betas], n_walkers=int(self.n_walkers),
                           seed=int(self._seed0), first_walker=int(self._first_walker),
                           thermalization=int(self.thermalization), sweeps=int(self.sweeps),
                           measure_rate=int(self.measure_rate), print_rate=int(self.print_rate),
                           series_capacity=int(self.series_capacity)),
                "seeds": [int(s) for s in self.seeds], "last_sweep": int(self.last_sweep)}

    def save(self, path):
        """save(filename, mc) (FileIO.jl) for what lives on the device: one file (checkpoint.py) with a JSON preamble -
        flavor, model, lattice, the constructor's keywords as they stand now, the seeds and the run loop's last sweep - and
        the blob of state().  Written to a temporary file in the same directory and moved into place, so `path` always
        holds a whole checkpoint.  Between any two sweep() calls: the classical flavor has no measurement point."""
        _ckpt.write(path, self._preamble(), self.state())

    @classmethod
    def check_flavor(cls, pre):
        """CheckpointError naming the flavor found unless the preamble is one of this class"""
        found = pre.get("flavor", "dqmc")
        if found != cls._flavor:
            raise _ckpt.CheckpointError("the checkpoint holds a run of flavor %r, %s.load reads flavor %r"
                                        % (found, cls.__name__, cls._flavor))
        if pre.get("format") != 1:
            raise _ckpt.CheckpointError("checkpoint preamble format %r, this package reads format 1" % (pre.get("format"),))

    @classmethod
    def load(cls, path, device_id=0):
        """load(filename): an object constructed and configured as the saved one - the settings applied in the order the
        constructor applies them - with its state imported (set_state, whose configuration check guards the
        reconstruction) on device `device_id`.  seed and first_walker are the saved ones, so the files of the ranks of a
        sharded run give back distinct walkers.  last_sweep is the saved one; run() continues behind it."""
        pre, blob = _ckpt.read(path)
        cls.check_flavor(pre)
        model = cls._model_from_entry(pre["model"], cls._lattice_from_entry(pre["lattice"]))
        kw = dict(pre["mc"])
        kw["beta"] = np.array(kw["beta"], dtype=np.float64)
        mc = cls(model, device_id=device_id, **cls._keywords(kw))
        try:
            mc.set_state(blob)
        except BaseException:
            mc.close()
            raise
        mc.seeds = [int(s) for s in pre["seeds"]]
        mc.last_sweep = int(pre["last_sweep"])
        return mc

    @staticmethod
    def _keywords(kw):
        """the constructor's keywords from the "mc" entry of a preamble (JSON lists back to what the constructor takes)"""
        return kw

    def _run(self, verbose, recorder, sweeps, thermalization, checkpoint=None, checkpoint_every=None):
        if checkpoint is not None and (checkpoint_every is None or int(checkpoint_every) < 1):
            raise ValueError("run(checkpoint=path) needs checkpoint_every >= 1")
        every = int(checkpoint_every) if checkpoint is not None else 0
        if sweeps is not None:
            self.sweeps = sweeps
        if thermalization is not None:
            self.thermalization = thermalization
        total = self.thermalization + self.sweeps
        t0 = time.time()
        mark = self._print_mark() if verbose else None
        while self.last_sweep < total:
            stop = total
            if recorder is not None and getattr(recorder, "rate", None):
                nxt = max(self.last_sweep + 1, self.thermalization + 1)
                r = recorder.rate
                stop = min(total, ((nxt + r - 1) // r) * r)
            elif verbose and self.print_rate:
                stop = min(total, (self.last_sweep // self.print_rate + 1) * self.print_rate)
            if every:  # a sweep call also ends at every multiple of checkpoint_every: the results do not depend on the cuts
                stop = min(stop, (self.last_sweep // every + 1) * every)
            self.sweep(stop - self.last_sweep)
            i = self.last_sweep
            if recorder is not None and i > self.thermalization:
                recorder.push(self, i)
            if verbose and self.print_rate and i % self.print_rate == 0:
                st = self.stats(0)
                print("\t%d\n\t\tsweep dur: %.3fs\n\t\tacc rate (local) : %.1f%%" %
                      (i, (time.time() - t0) / self.print_rate, 100.0 * st.acc_local / max(st.prop_local, 1)))
                t0 = time.time()
                mark = self._print_more(mark)
            if every and (i % every == 0 or i == total):
                self.save(checkpoint)
        return True


class MC(_MCBase):
    """MC(model; beta | T, ...) (MC.jl:16-80) for `n_walkers` chains.  `beta` may be a sequence of n_walkers values
    (one temperature per walker).

    `cluster_moves=True` runs a Wolff cluster move per walker after every sweep whose index is a multiple of
    `global_rate`, as run! does with global_moves (MC.jl:233-236), on a stream of its own (dqmc_mc_global_move).
    `global_moves=True` is refused: the reference's global_move cannot run as written (IsingModel.jl:137 assigns to an
    undefined `model`) and its rand(1:N) draws have no place in the walker streams; `cluster_moves` is its defined
    counterpart.

    `binning=True` gives every walker a logarithmic binner over E, E2, |M| and M2, pushed on the device where the
    measurement is taken (enable_binning); `binned()` then answers mean, std_error and tau, and the errors of C and
    chi.

    `n_replicas=R` (R >= 2, n_walkers a multiple of it) makes every R consecutive walkers a ladder for replica exchange
    (parallel tempering, an extension the reference does not have; dqmc_mc_set_exchange defines it), and
    `exchange_rate=k` runs one exchange round after every k-th sweep: after that sweep's cluster move, before its
    measurement.  A `beta` or `T` sequence of length R is tiled over the ladders.  Walker w stays at beta_w with its
    stream, sums, series and binner; an accepted exchange swaps the configurations (spins, E, M and the replica label)
    of two neighbouring walkers, so measurements(w) and binned(w) remain "at beta_w".  `exchange_rate=0` leaves the
    sweeps as they are without exchange; `exchange()` then still runs a round by hand.

    `fss=True` (or a list of at most 8 wave vectors) also measures M^4 and the structure factor S(k) wherever E and |M|
    are measured (set_fss): `fss()` gives the Binder cumulant U4 and the second-moment correlation length xi, and with
    `binning=True` `binned_fss()` gives their error bars.

    `update="checkerboard"` sweeps every walker with a whole workgroup, colour class by colour class (set_update;
    `colouring=None`: greedy_colouring(lattice)): another Markov chain than the reference's sequential sweep(mc), with
    the same stationary distribution, on a Philox domain of its own, and much faster per sweep where the walkers are
    few and the lattice is large.  `update="sequential"` (the default) is the reference's sweep.

    With a q-state model (qstate.PottsModel, ClockModel, QStateModel) MC(...) returns a qstate.QStateMC: the engine of
    dqmc_qs_* with its own kernels.  With an IsingModel nothing changes."""
    _abi = "dqmc_mc_"
    _flavor = "mc_ising"
    _ExchangeStats = McExchangeStats

    def __new__(cls, model, *args, **kwargs):
        if cls is MC and getattr(model, "is_qstate", False):
            from .qstate import QStateMC
            return QStateMC(model, *args, **kwargs)  # (not an MC: __init__ below does not run)
        return super().__new__(cls)

    def __init__(self, model, beta=None, T=None, n_walkers=1, seed=123, first_walker=0, thermalization=0, sweeps=1000,
                 measure_rate=1, print_rate=1000, global_moves=False, global_rate=5, device_id=0, series_capacity=0,
                 cluster_moves=False, binning=False, binning_capacity=None, n_replicas=0, exchange_rate=0,
                 fss=False, update="sequential", colouring=None):
        if global_moves:
            raise NotImplementedError(
                "MC(global_moves=True): the reference's Wolff global_move cannot run (IsingModel.jl:137 uses the "
                "undefined `model`) and its rand(1:N) draws have no defined place in the walkers' Philox streams; "
                "MC(cluster_moves=True, global_rate=...) runs the cluster move on a stream of its own")
        if cluster_moves and (int(global_rate) != global_rate or global_rate < 1):
            raise ValueError("MC(cluster_moves=True): global_rate must be an integer >= 1")
        beta = self._resolve_beta(beta, T)
        if int(n_replicas) != n_replicas or int(exchange_rate) != exchange_rate:
            raise ValueError("MC: n_replicas and exchange_rate must be integers")
        if n_replicas >= 2 and beta.ndim == 1 and len(beta) == n_replicas and n_walkers % n_replicas == 0:
            beta = np.tile(beta, n_walkers // n_replicas)  # one ladder's temperatures, the same in every ladder
        self._init_common(model, beta, n_walkers, seed, first_walker, thermalization, sweeps, measure_rate, print_rate,
                          series_capacity)
        self.global_moves, self.global_rate = global_moves, global_rate
        self.cluster_moves = bool(cluster_moves)
        self.n_replicas, self.exchange_rate = int(n_replicas), int(exchange_rate)
        self._create(McParams(n_sites=self.N, z=self._neighs.shape[0], n_walkers=n_walkers, device_id=device_id,
                              n_bonds=self._bonds.shape[0], series_capacity=series_capacity,
                              neighs=self._neighs.ctypes.data_as(C.POINTER(C.c_int64)),
                              bonds=self._bonds.ctypes.data_as(C.POINTER(C.c_int64))))
        if self.cluster_moves:
            self._c(lib().dqmc_mc_set_global_rate(self._h, int(global_rate)))
        if self.n_replicas or self.exchange_rate:
            self.set_exchange(self.n_replicas, self.exchange_rate)
        self.update, self.colouring = "sequential", None
        if update != "sequential" or colouring is not None:
            self.set_update(update, colouring)
        self.k_vectors = None
        if fss is not False and fss is not None:
            self.set_fss(fss)
        if binning:
            self.enable_binning(binning_capacity)

    # ---- state
    def conf(self, walker=0):
        out = np.zeros(self.N, dtype=np.int8)
        self._c(lib().dqmc_mc_get_conf(self._h, walker, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_conf(self, walker, conf):
        c = np.ascontiguousarray(np.asarray(conf).reshape(-1, order="F"), dtype=np.int8)
        if c.size != self.N:
            raise DQMCError(ERR_INVALID, "set_conf: expected %d spins" % self.N)
        self._c(lib().dqmc_mc_set_conf(self._h, walker, c.ctypes.data_as(C.c_void_p)))

    def conf_bits(self, walker=0):
        """compress(mc, m, conf) = BitArray(conf .== 1) as CompressedConf (shape (N, 1), decompress gives conf(w))"""
        out = np.zeros((self.N + 63) // 64, dtype=np.uint64)
        self._c(lib().dqmc_mc_get_conf_bits(self._h, walker, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return CompressedConf(out, (self.N, 1))

    def stats(self, walker=0):
        st = McStats()
        self._c(lib().dqmc_mc_get_stats(self._h, walker, C.byref(st)))
        return st

    def energy(self, walker=0):
        """model.energy[] of the walker, tracked on the device"""
        return float(self.stats(walker).energy)

    def uniforms_used(self, walker=0):
        return int(self.stats(walker).uniforms_used)

    # ---- the loop
    def run(self, verbose=False, recorder=None, sweeps=None, thermalization=None, checkpoint=None, checkpoint_every=None):
        """run!(mc) (MC.jl:190-315) for every walker, resuming after last_sweep; a recorder gets
        push(mc, i) after each sweep i > thermalization (of walker 0, ConfigRecorder keeps every rate-th).
        `checkpoint=path` saves the run (save()) after every sweep whose index is a multiple of `checkpoint_every` and
        after the last one; the sweep calls are cut there, which changes no bit of the results.  A ConfigRecorder's
        configurations are the caller's and are not part of the file."""
        return self._run(verbose, recorder, sweeps, thermalization, checkpoint, checkpoint_every)

    # ---- checkpoint and resume (state, set_state, save, load: _MCBase)
    @staticmethod
    def _model_entry(m):
        if type(m) is not IsingModel:
            raise ValueError("save(): %s is not a model a checkpoint can name" % type(m).__name__)
        return {"class": "IsingModel", "dims": int(m.dims), "L": int(m.L)}

    @staticmethod
    def _model_from_entry(entry, l):
        if entry.get("class") != "IsingModel":
            raise _ckpt.CheckpointError("the checkpoint names an unknown model")
        return IsingModel(dims=entry["dims"], L=entry["L"], l=l)

    def _settings(self):
        return {"cluster_moves": bool(self.cluster_moves), "global_rate": int(self.global_rate),
                "n_replicas": int(self.n_replicas), "exchange_rate": int(self.exchange_rate), "update": self.update,
                "colouring": None if self.colouring is None else [int(c) for c in self.colouring],
                "fss": False if self.k_vectors is None else np.asarray(self.k_vectors, dtype=np.float64).tolist(),
                "binning": self._binning is not None, "binning_capacity": self._binning or None}

    def _print_mark(self):
        if not self.cluster_moves:
            return None
        g = self.global_stats(0)
        return g.acc_global, g.prop_global

    def _print_more(self, mark):
        if not self.cluster_moves:
            return mark
        g = self.global_stats(0)  # MC.jl:265-271: this print window, then overall
        print("\t\tacc rate (global): %.1f%%\n\t\tacc rate (global, overall): %.1f%%" %
              (100.0 * (g.acc_global - mark[0]) / max(g.prop_global - mark[1], 1),
               100.0 * g.acc_global / max(g.prop_global, 1)))
        return g.acc_global, g.prop_global

    def global_move(self, walker=-1):
        """global_move(mc, m, conf) (IsingModel.jl:104-140): one Wolff cluster move of one walker (walker < 0: every
        walker), counted in the global stats, no measurement"""
        self._c(lib().dqmc_mc_global_move(self._h, walker))

    def global_stats(self, walker=0):
        """prop_global, acc_global, sum_cluster_size and moves_drawn (the move cursor) of one walker"""
        st = McGlobalStats()
        self._c(lib().dqmc_mc_get_global_stats(self._h, walker, C.byref(st)))
        return st

    # ---- replica exchange (set_exchange, exchange, exchange_stats, replicas: _MCBase)
    def exchange_fused(self):
        """True: sweep() runs its exchange rounds inside the sweep kernel (64 % n_replicas == 0)"""
        f = C.c_int32()
        self._c(lib().dqmc_mc_exchange_fused(self._h, C.byref(f)))
        return bool(f.value)

    # ---- the local update
    def set_update(self, kind, colouring=None):
        """dqmc_mc_set_update: "sequential" (the reference's sweep(mc), the default) or "checkerboard" with `colouring`
        (an integer per site, at most 16 colours, no two neighbours alike; None: greedy_colouring(lattice)).  Between
        sweeps at any time; configurations, sums and cursors stay."""
        if kind not in MC_UPDATE_KINDS:
            raise ValueError("set_update: kind must be one of %s" % (MC_UPDATE_KINDS,))
        if kind == "sequential":
            self._c(lib().dqmc_mc_set_update(self._h, 0, None, 0))
            self.colouring = None
        else:
            col, n = self._colours(colouring, "set_update")
            self._c(lib().dqmc_mc_set_update(self._h, 1, col.ctypes.data_as(C.POINTER(C.c_int32)), n))
            self.colouring = col
        self.update = kind

    def update_stats(self, walker=0):
        """kind, n_colours and sweeps_drawn (the walker's checkerboard sweep cursor)"""
        st = McUpdateStats()
        self._c(lib().dqmc_mc_get_update(self._h, walker, C.byref(st)))
        return st

    # ---- results
    def analysis(self, walker=0):
        """MCAnalysis (MC.jl:1-11) of one walker"""
        st = self.stats(walker)
        g = self.global_stats(walker)
        x = self.exchange_stats(walker)
        return {"acc_rate": st.acc_local / st.prop_local if st.prop_local else 0.0, "prop_local": int(st.prop_local),
                "acc_rate_exchange": x.acc_exchange / x.prop_exchange if x.prop_exchange else 0.0,
                "prop_exchange": int(x.prop_exchange), "acc_exchange": int(x.acc_exchange),
                "acc_local": int(st.acc_local),
                "acc_rate_global": g.acc_global / g.prop_global if g.prop_global else 0.0,
                "prop_global": int(g.prop_global), "acc_global": int(g.acc_global)}

    def measurements(self, walker=0):
        """finish! of IsingMagnetizationMeasurement and IsingEnergyMeasurement (measurements.jl:13-94) on the sums:
        {"Magn": {M, M2, m, chi}, "Energy": {E, E2, e, C}} (means over the walker's measurements)"""
        st = self.stats(walker)
        n = st.n_meas
        if n == 0:
            raise DQMCError(ERR_INVALID, "measurements: no measurement has been taken")
        beta, invN = float(self.betas[walker]), 1.0 / self.N
        E, E2, M, M2 = st.sum_E / n, st.sum_E2 / n, st.sum_absM / n, st.sum_M2 / n
        return {"Magn": {"M": M, "M2": M2, "m": M * invN, "chi": beta * invN * (M2 - M * M)},
                "Energy": {"E": E, "E2": E2, "e": E * invN, "C": beta * beta * invN * (E2 - E * E)},
                "n_meas": int(n)}

    # ---- error bars (enable_binning, binner_size, binner_reliable_level: _MCBase)
    def binner_level(self, walker, level):
        """(x_sum[4], x2_sum[4], xy_sum[2], count) of one level of one walker: elements [E, E2, |M|, M2], pairs
        (E, E2) and (|M|, M2)"""
        return self._section_level("", 4, 2, walker, level)

    def binner_finish(self, walker=0, level=None):
        """dqmc_mc_binned of one walker at `level` (None: the reliable level)"""
        return self._section_finish("", McBinned, walker, level)

    def _binned_walker(self, walker, level):
        """per observable (mean, variance of the mean at `level`, the same at level 0 or None) of one walker"""
        b = self.binner_finish(walker, level)
        beta, invN = float(self.betas[walker]), 1.0 / self.N
        E, E2, M, M2 = b.mean
        vE, vE2, vM, vM2 = b.varN

        def fluct(scale, x, x2, vx, vx2, cov):  # scale (<x2> - <x>^2) and the delta method on the binned covariance
            var = scale * scale * (vx2 - 4.0 * x * cov + 4.0 * x * x * vx)
            return scale * (x2 - x * x), (max(var, 0.0) if var == var else var), None

        obs = {"E": (E, vE, b.varN0[0]), "E2": (E2, vE2, b.varN0[1]),
               "e": (E * invN, vE * invN * invN, b.varN0[0] * invN * invN),
               "C": fluct(beta * beta * invN, E, E2, vE, vE2, b.covN[0]),
               "M": (M, vM, b.varN0[2]), "M2": (M2, vM2, b.varN0[3]),
               "m": (M * invN, vM * invN * invN, b.varN0[2] * invN * invN),
               "chi": fluct(beta * invN, M, M2, vM, vM2, b.covN[1])}
        return obs, int(b.count), int(b.level)

    def binned(self, walker=0, level=None, walkers=None):
        """mean(obs), std_error(obs) and tau(obs) of the Observables of IsingEnergyMeasurement /
        IsingMagnetizationMeasurement (measurements.jl:13-94) from the device binner at `level` (None: the reliable
        one): {"Energy": {E, E2, e, C}, "Magn": {M, M2, m, chi}, "count", "level"}, each observable {mean, std_error,
        tau}.  C and chi get their error by the delta method on the binned covariance of (E, E2) and (|M|, M2) and
        have no tau.  `walkers=[...]` pools chains of equal beta: mean = sum_w mean_w / W, std_error =
        sqrt(sum_w var_w) / W (C and chi formed per walker first), tau from the summed variances, plus
        std_error_walkers = sqrt(sum_w (mean_w - mean)^2 / (W (W - 1))), which needs no binning."""
        p = pool_walkers("binned", self.betas, walker, walkers, lambda w: self._binned_walker(w, level))
        out = {"Energy": {k: p.pop(k) for k in ("E", "E2", "e", "C")},
               "Magn": {k: p.pop(k) for k in ("M", "M2", "m", "chi")}}
        out.update(p)
        return out

    # ---- finite-size scaling
    def set_fss(self, k_vectors=True):
        """dqmc_mc_set_fss: from now on every measurement also takes M^4 and S(k) = |sum_i s_i e^{i k . r_i}|^2 / N at
        the given wave vectors (True: reciprocal_vectors(lattice), the smallest ones, one per lattice dimension; a
        list of at most 8 vectors of the lattice's dimension, possibly empty: M^4 only; None or False: off).  Resets
        the FSS sums and, if binning is on, restarts the binner with every section empty."""
        if k_vectors is None or k_vectors is False:
            self._c(lib().dqmc_mc_set_fss(self._h, -1, None, None))
            self.k_vectors = None
            return
        ks = reciprocal_vectors(self.model.l) if k_vectors is True else k_vectors
        cq, sq, k = q30_tables(self.model.l, ks)
        i32 = C.POINTER(C.c_int32)
        self._c(lib().dqmc_mc_set_fss(self._h, len(k), cq.ctypes.data_as(i32), sq.ctypes.data_as(i32)))
        self.k_vectors = k

    def fss_sums(self, walker=0):
        """dqmc_mc_fss of one walker: n_meas, n_k, sum_M4, sum_S[8]"""
        out = McFss()
        self._c(lib().dqmc_mc_get_fss(self._h, walker, C.byref(out)))
        return out

    def _fss_derived(self, M2, M4, S):
        U4, _ = _binder(M2, M4)
        xi = np.array([_xi(M2, S[k], self.N, float(np.linalg.norm(self.k_vectors[k])))[0] for k in range(len(S))])
        out = {"M2": M2, "M4": M4, "S": np.array(S, dtype=float), "U4": U4, "xi": xi}
        L = getattr(self.model.l, "L", None)
        if L is not None:
            out["xi_over_L"] = xi / float(L)
        return out

    def fss(self, walker=0):
        """the plain means of one walker: M4, S (one per wave vector), the Binder cumulant U4 = 1 - <M4>/(3 <M2>^2)
        and the second-moment correlation length xi_k = sqrt(S(0)/S_k - 1) / (2 sin(|k|/2)) with S(0) = <M2>/N (the
        usual definition for unit lattice spacing; NaN where S(0) < S_k), xi_over_L where the lattice has an L.
        <M2> is the one of measurements(): the two counts must agree (after switching FSS on mid-run,
        reset_accumulators() first)."""
        f, st = self.fss_sums(walker), self.stats(walker)
        if f.n_k < 0:
            raise DQMCError(ERR_STATE, "fss: FSS is off (MC(fss=True) or set_fss)")
        if f.n_meas == 0:
            raise DQMCError(ERR_INVALID, "fss: no measurement has been taken")
        if f.n_meas != st.n_meas:
            raise DQMCError(ERR_STATE, "fss: %d FSS measurements but %d of M2 (FSS was switched on mid-run: "
                                       "reset_accumulators() first)" % (f.n_meas, st.n_meas))
        n = float(f.n_meas)
        out = self._fss_derived(st.sum_M2 / n, f.sum_M4 / n, [f.sum_S[k] / n for k in range(f.n_k)])
        out["n_meas"] = int(f.n_meas)
        return out

    def fss_binner_level(self, walker, level):
        """(x_sum[2 + n_k], x2_sum[2 + n_k], xy_sum[1 + n_k], count) of one level of one walker of the binner's FSS
        section: elements [M2, M4, S_0 ..], pairs (M2, M4), (M2, S_0) .."""
        nk = 0 if self.k_vectors is None else len(self.k_vectors)
        return self._section_level("fss_", 2 + nk, 1 + nk, walker, level)

    def fss_binner_finish(self, walker=0, level=None):
        """dqmc_mc_fss_binned of one walker at `level` (None: the reliable level)"""
        return self._section_finish("fss_", McFssBinned, walker, level)

    def _binned_fss_walker(self, walker, level):
        """{name: (mean, variance of the mean at `level`, the same at level 0 or None)} of one walker; S, xi as lists"""
        b = self.fss_binner_finish(walker, level)
        nk = b.n_k
        M2, M4 = b.mean[0], b.mean[1]
        U4, gU = _binder(M2, M4)
        obs = {"M2": (M2, b.varN[0], b.varN0[0]), "M4": (M4, b.varN[1], b.varN0[1]),
               "U4": (U4, _delta_var(gU, b.varN[0], b.varN[1], b.covN[0]), None), "S": [], "xi": []}
        for k in range(nk):
            S = b.mean[2 + k]
            xi, g = _xi(M2, S, self.N, float(np.linalg.norm(self.k_vectors[k])))
            obs["S"].append((S, b.varN[2 + k], b.varN0[2 + k]))
            obs["xi"].append((xi, _delta_var(g, b.varN[0], b.varN[2 + k], b.covN[1 + k]), None))
        return obs, int(b.count), int(b.level)

    def binned_fss(self, walker=0, level=None, walkers=None):
        """mean, std_error and tau of M2, M4 and each S_k from the binner's FSS section at `level` (None: the reliable
        one), and mean and std_error of U4 and each xi_k (xi_over_L where the lattice has an L) by the delta method on
        the binned covariances of (M2, M4) and (M2, S_k): {"M2", "M4", "U4": {...}, "S", "xi": [{...} per k], "count",
        "level"}.  `walkers=[...]` pools chains of equal beta under the rules of binned(): U4 and xi are formed per
        walker first, std_error = sqrt(sum_w var_w) / W, plus std_error_walkers."""
        out = pool_walkers("binned_fss", self.betas, walker, walkers, lambda w: self._binned_fss_walker(w, level))
        L = getattr(self.model.l, "L", None)
        if L is not None:
            out["xi_over_L"] = [{key: v / float(L) for key, v in o.items()} for o in out["xi"]]
        return out

    def series(self, walker=0):
        """per-measurement (E, |M|) of the walker as recorded (at most series_capacity entries)"""
        cap = self.series_capacity
        e = np.zeros(max(cap, 1), dtype=np.int32)
        m = np.zeros(max(cap, 1), dtype=np.int32)
        n = C.c_int64()
        self._c(lib().dqmc_mc_get_series(self._h, walker, e.ctypes.data_as(C.POINTER(C.c_int32)),
                                         m.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
        return e[:n.value].copy(), m[:n.value].copy()
