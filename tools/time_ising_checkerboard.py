"""Sequential against checkerboard sweeps of the Ising flavor (csrc/ising_sweep.inl: one lane per chain; csrc/ising_cb.inl:
one workgroup per chain), one JSON line per measurement.

Rates: 2D square L = 8, 32, 64, 128 with 16, 64, 256 and 4096 walkers at T_c, microseconds per sweep of the whole handle
(all walkers advance one sweep) for one `sweep` call after a warm-up, no measurements; the handles take turns in one
process (two turns each, the faster one).  `--parent-lib` adds the sequential sweep of another build of the library, such
as the parent commit's, driven through the C ABI alone, to the same turns.

Mixing: tau_int of |M| in sweeps for both updates at T_c (L = 8, 16, 32; 64 walkers pooled, from the device binner), so
that sweeps per second can be turned into effective samples per second: the two chains need not mix alike.

    python tools/time_ising_checkerboard.py [--out FILE] [--parent-lib PATH] [--scale S] [--no-tau]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_ising_tempering import RawHandle, timed  # noqa: E402

SWEEPS = {8: 2000, 32: 400, 64: 100, 128: 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="another build of libdqmc_hip.so to time in sequential mode")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every sweep count")
    ap.add_argument("--no-tau", action="store_true")
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

    beta = 1.0 / mc_amd.IsingTc
    for L in (8, 32, 64, 128):
        for W in (16, 64, 256, 4096):
            n = max(4, int(SWEEPS[L] * args.scale))
            model = mc_amd.IsingModel(dims=2, L=L)
            kw = dict(beta=beta, n_walkers=W, seed=L, thermalization=10 ** 12)
            names = ["sequential", "checkerboard"]
            handles = [mc_amd.MC(model, **kw), mc_amd.MC(model, update="checkerboard", **kw)]
            if args.parent_lib:
                names.append("sequential_parent")
                handles.append(RawHandle(mc_amd, args.parent_lib, L, W, [beta] * W, L))
            for h in handles:
                h.sweep(max(2, n // 10))  # warm-up
            secs = timed(handles, n)
            line = {"shape": "square L=%d" % L, "n_sites": L * L, "n_walkers": W, "sweeps": n, "T": "T_c"}
            for name, s in zip(names, secs):
                line["sweep_us_" + name] = 1e6 * s / n
                line["site_updates_per_s_" + name] = L * L * W * n / s
            line["sequential_over_checkerboard"] = line["sweep_us_sequential"] / line["sweep_us_checkerboard"]
            if args.parent_lib:
                line["sequential_over_parent"] = line["sweep_us_sequential"] / line["sweep_us_sequential_parent"] - 1.0
            for h in handles:
                h.close()
            emit(line)

    for L in () if args.no_tau else (8, 16, 32):
        W, therm, n = 64, 2000, max(1024, int(32768 * args.scale))
        line = {"shape": "square L=%d" % L, "n_walkers": W, "T": "T_c", "thermalization": therm, "sweeps": n}
        for kind in ("sequential", "checkerboard"):
            mc = mc_amd.MC(mc_amd.IsingModel(dims=2, L=L), beta=beta, n_walkers=W, seed=17 + L, thermalization=therm,
                           sweeps=n, binning=True, binning_capacity=n, update=kind)
            mc.run()
            b = mc.binned(walkers=range(W))
            line["tau_int_absM_" + kind] = b["Magn"]["M"]["tau"]
            line["absM_per_site_" + kind] = b["Magn"]["m"]["mean"]
            line["binning_level_" + kind] = b["level"]
            mc.close()
        emit(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
