"""Cost of the Ising flavor's finite-size-scaling measurement (csrc/ising_fss.inl: ising_fss_kernel behind every measured
sweep), one JSON line per measurement.  2D square L = 8 and 64, 256 walkers at beta_c, measure_rate 1 and 10, n_k = 2
(the two smallest wave vectors), site updates per second of one `sweep` call after a warm-up:

- FSS off on this build against another build of the library (`--parent-lib`, such as the parent commit's), both driven
  through the C ABI alone and alternated in one call, `--repeats` turns each.  Acceptance: this build's median lies
  within the spread (min .. max) of the parent's own repeats.
- FSS on, without and with binning: the added time per measurement against FSS off on this build.

    python tools/time_ising_fss.py [--out FILE] [--parent-lib PATH] [--scale S] [--repeats R]"""
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
W, N_K = 256, 2


class RawHandle:
    """a handle on any build of the library through the entry points every build has; fss / binning only on this build"""

    def __init__(self, mc_amd, libpath, L, rate, seed, fss=False, binning=False):
        from montecarlo_jl_amd import _lib, mc
        self.lib = C.CDLL(libpath)
        self.lib.dqmc_mc_set_beta.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        self.lib.dqmc_mc_seed.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
        self.lib.dqmc_mc_rand_conf.argtypes = [C.c_void_p, C.c_int32]
        self.lib.dqmc_mc_sweep.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32]
        self.lib.dqmc_mc_binner_enable.argtypes = [C.c_void_p, C.c_int64]
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
            assert self.lib.dqmc_mc_set_beta(self.h, w, float(BETA_C)) == 0
        assert self.lib.dqmc_mc_rand_conf(self.h, -1) == 0
        if fss:
            cq, sq, k = mc.q30_tables(l, mc.reciprocal_vectors(l))
            assert len(k) == N_K
            i32 = C.POINTER(C.c_int32)
            self.lib.dqmc_mc_set_fss.argtypes = [C.c_void_p, C.c_int32, i32, i32]
            assert self.lib.dqmc_mc_set_fss(self.h, N_K, cq.ctypes.data_as(i32), sq.ctypes.data_as(i32)) == 0
        if binning:
            assert self.lib.dqmc_mc_binner_enable(self.h, 1 << 30) == 0
        self.rate, self.last_sweep = rate, 0

    def sweep(self, n):
        assert self.lib.dqmc_mc_sweep(self.h, n, self.last_sweep + 1, 0, self.rate) == 0
        self.last_sweep += n

    def close(self):
        self.lib.dqmc_mc_destroy(self.h)


def timed(handles, n, repeats):
    """seconds of sweep(n): [handle][turn], the handles taking turns"""
    out = [[] for _ in handles]
    for _ in range(repeats):
        for i, h in enumerate(handles):
            t0 = time.perf_counter()
            h.sweep(n)
            out[i].append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of libdqmc_hip.so to alternate with (FSS off)")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the number of sweeps per timing")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    mc_amd = g.load_package()
    from montecarlo_jl_amd import _lib
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for L in (8, 64):
        N = L * L
        n = max(10, int(args.scale * (20000 if L == 8 else 400)))  # a multiple of 10: the same measurements per turn
        n -= n % 10
        for rate in (1, 10):
            names = ["off", "fss", "fss_binned"]
            handles = [RawHandle(mc_amd, _lib.LIB_PATH, L, rate, 1000),
                       RawHandle(mc_amd, _lib.LIB_PATH, L, rate, 1000, fss=True),
                       RawHandle(mc_amd, _lib.LIB_PATH, L, rate, 1000, fss=True, binning=True)]
            if args.parent_lib:
                names.append("parent_off")
                handles.append(RawHandle(mc_amd, args.parent_lib, L, rate, 1000))
            for h in handles:
                h.sweep(n)  # warm-up
            t = dict(zip(names, timed(handles, n, args.repeats)))
            for h in handles:
                h.close()
            visits = float(n) * N * W
            rec = {"L": L, "walkers": W, "measure_rate": rate, "n_k": N_K, "sweeps": n, "repeats": args.repeats,
                   "updates_per_s": {k: [visits / x for x in v] for k, v in t.items()},
                   "median_updates_per_s": {k: visits / float(np.median(v)) for k, v in t.items()}}
            meas = n // rate
            for k in ("fss", "fss_binned"):
                rec["added_us_per_measurement_" + k] = 1e6 * (float(np.median(t[k])) - float(np.median(t["off"]))) / meas
            if args.parent_lib:
                p = rec["updates_per_s"]["parent_off"]
                m = rec["median_updates_per_s"]["off"]
                rec["parent_spread"] = [min(p), max(p)]
                rec["off_within_parent_spread"] = bool(m >= min(p))  # (faster than the parent's best is no regression)
                rec["off_vs_parent_median"] = m / rec["median_updates_per_s"]["parent_off"]
            emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
