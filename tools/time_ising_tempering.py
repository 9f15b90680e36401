"""Cost and effect of the Ising flavor's replica exchange (csrc/ising.hip: the round fused into the sweep kernels,
ising_exchange_kernel), one JSON line per measurement.

Rates: 2D square L = 8 and 64 with 256 and 4096 walkers, betas of a ladder spread over 0.8 .. 1.2 beta_c, site updates per
second of one `sweep` call after a warm-up, handles taking turns (two turns each, the faster one):
- exchange off (driven through the C ABI alone, so that `--parent-lib` can time another build of the library, such as
  the parent commit's, in the same call);
- fused: R = 8, a round after every sweep (exchange_rate = 1) and after every tenth;
- stand-alone: R = 128 (a ladder of two waves), the same two rates: every round is a launch of its own.

Effect: L = 8 and 32, 256 walkers as 32 ladders of R = 8 across T_c, 1000 sweeps with a round after each: swaps per try of
every pair, and round trips (slot 0 -> slot R - 1 -> slot 0) per replica per 1000 sweeps, from the labels after every sweep.

    python tools/time_ising_tempering.py [--out FILE] [--parent-lib PATH] [--scale S]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BETA_C = 0.5 * np.log(1.0 + np.sqrt(2.0))


def ladder(R):
    return np.linspace(0.8 * BETA_C, 1.2 * BETA_C, R)


class RawHandle:
    """an exchange-off handle on any build of the library, through the entry points every build has"""

    def __init__(self, mc_amd, libpath, L, W, betas, seed):
        from montecarlo_jl_amd import _lib
        self.lib = C.CDLL(libpath)
        self.lib.dqmc_mc_set_beta.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        self.lib.dqmc_mc_seed.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
        self.lib.dqmc_mc_rand_conf.argtypes = [C.c_void_p, C.c_int32]
        self.lib.dqmc_mc_sweep.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32]
        self.lib.dqmc_mc_destroy.argtypes = [C.c_void_p]
        l = mc_amd.SquareLattice(L)
        self.neighs = np.asfortranarray(np.asarray(l.neighs, dtype=np.int64))
        self.bonds = np.asfortranarray(np.asarray(l.bonds, dtype=np.int64)[:, :2])
        p = _lib.McParams(n_sites=len(l), z=self.neighs.shape[0], n_walkers=W, device_id=0, n_bonds=self.bonds.shape[0],
                          series_capacity=0, neighs=self.neighs.ctypes.data_as(C.POINTER(C.c_int64)),
                          bonds=self.bonds.ctypes.data_as(C.POINTER(C.c_int64)))
        self.h = C.c_void_p()
        assert self.lib.dqmc_mc_create(C.byref(p), C.byref(self.h)) == 0
        for w in range(W):
            assert self.lib.dqmc_mc_seed(self.h, w, seed + w) == 0
            assert self.lib.dqmc_mc_set_beta(self.h, w, float(betas[w])) == 0
        assert self.lib.dqmc_mc_rand_conf(self.h, -1) == 0
        self.last_sweep = 0

    def sweep(self, n):
        assert self.lib.dqmc_mc_sweep(self.h, n, self.last_sweep + 1, 10 ** 12, 1) == 0
        self.last_sweep += n

    def close(self):
        self.lib.dqmc_mc_destroy(self.h)


def timed(handles, n, turns=2):
    """seconds of sweep(n) per handle: the handles take turns, the faster turn of each"""
    best = [float("inf")] * len(handles)
    for _ in range(turns):
        for i, h in enumerate(handles):
            t0 = time.perf_counter()
            h.sweep(n)
            best[i] = min(best[i], time.perf_counter() - t0)
    return best


def round_trips(labels, R):
    """labels: [sweep][ladder][slot]; completed trips slot 0 -> slot R - 1 -> slot 0 per replica"""
    n_lad = labels.shape[1]
    state = np.zeros((n_lad, R), dtype=np.int8)  # per replica: 0 = not yet at slot 0, 1 = left slot 0, 2 = reached the top
    trips = 0
    rows = np.arange(n_lad)
    for lab in labels:
        bottom, top = lab[:, 0], lab[:, R - 1]
        trips += int(np.sum(state[rows, bottom] == 2))
        state[rows, bottom] = 1
        at_top = state[rows, top] == 1
        state[rows[at_top], top[at_top]] = 2
    return trips / (n_lad * R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of libdqmc_hip.so to time with exchange off")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every sweep count")
    args = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    from montecarlo_jl_amd import _lib
    src_hash = mc_amd.lib().dqmc_build_source_hash().decode()
    lines = []

    def emit(line):
        line["source_hash"] = src_hash
        print(json.dumps(line), flush=True)
        lines.append(line)

    for L, W, n in ((8, 256, 20000), (8, 4096, 20000), (64, 256, 400), (64, 4096, 400)):
        n = max(10, int(n * args.scale))
        N = L * L
        model = mc_amd.IsingModel(dims=2, L=L)
        kw = dict(n_walkers=W, seed=L, thermalization=10 ** 12)
        names, handles = ["off"], [RawHandle(mc_amd, _lib.LIB_PATH, L, W, np.tile(ladder(8), W // 8), L)]
        if args.parent_lib:
            names.append("off_parent")
            handles.append(RawHandle(mc_amd, args.parent_lib, L, W, np.tile(ladder(8), W // 8), L))
        for R, form in ((8, "fused"), (128, "standalone")):
            for k in (1, 10):
                mc = mc_amd.MC(model, beta=ladder(R), n_replicas=R, exchange_rate=k, **kw)
                assert mc.exchange_fused() == (form == "fused")
                names.append("%s_R%d_k%d" % (form, R, k))
                handles.append(mc)
        for h in handles:
            h.sweep(max(10, n // 10))  # warm-up
        secs = timed(handles, n)
        line = {"shape": "square L=%d" % L, "n_sites": N, "n_walkers": W, "sweeps": n}
        for name, s in zip(names, secs):
            line["site_updates_per_s_" + name] = N * W * n / s
            line["sweep_us_" + name] = 1e6 * s / n
        for name in names[1:]:
            line["over_off_" + name] = line["sweep_us_" + name] / line["sweep_us_off"] - 1.0
        for h in handles:
            h.close()
        emit(line)

    for L in (8, 32):
        R, W, n = 8, 256, max(20, int(1000 * args.scale))
        mc = mc_amd.MC(mc_amd.IsingModel(dims=2, L=L), beta=ladder(R), n_walkers=W, seed=7 + L, thermalization=10 ** 12,
                       n_replicas=R, exchange_rate=1)
        mc.sweep(200)
        mc.set_exchange(R, 1)  # counters, labels and cursor from here
        labels = np.zeros((n, W // R, R), dtype=np.int64)
        for i in range(n):
            mc.sweep(1)
            labels[i] = mc.replicas().reshape(-1, R)
        xs = [mc.exchange_stats(w) for w in range(W)]
        rate = [float(np.sum([xs[w].acc_exchange for w in range(i, W, R)]) /
                      max(1, np.sum([xs[w].prop_exchange for w in range(i, W, R)]))) for i in range(R - 1)]
        emit({"shape": "square L=%d" % L, "n_walkers": W, "n_replicas": R, "betas_over_beta_c": [0.8, 1.2], "sweeps": n,
              "swap_rate_per_pair": [round(r, 4) for r in rate],
              "round_trips_per_replica_per_1000_sweeps": 1000.0 * round_trips(labels, R) / n})
        mc.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
