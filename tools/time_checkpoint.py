"""Cost of a checkpoint at the benchmark shape (attractive 16 x 16, beta = 8, 32 walkers: n = 256, config 3 of bench.py).

  python tools/time_checkpoint.py [--reps 3] [--out FILE]

Times DQMC.state() (dqmc_state_export: device to host) and DQMC.set_state() (dqmc_state_import: host to device, then the
rebuild of the stack and G from the fields) for two cases: the Green's-function binner on at its default capacity (the
binner's 0.84 GB of levels dominate the blob) and no binner (the fields, cursors, counters and the Green's sums).  Prints
one JSON line per case: bytes, milliseconds (the median of `reps`), and for scale the time of one sweep.  Needs the GPU."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (before the library opens the device: imported later it reports no HIP device)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mc_amd = g.load_package()
    if mc_amd.device_count() < 1:
        raise SystemExit("time_checkpoint.py needs the GPU")
    lines = []
    for case, binner in (("greens_binner_default_capacity", True), ("no_binner", False)):
        mc = mc_amd.DQMC(mc_amd.HubbardModelAttractive(16, 2), beta=8.0, delta_tau=0.1, n_walkers=32, seed=1)
        mc.prepare()
        if binner:
            mc.enable_binning(("greens",))
        mc.update_until_measure()
        mc.accumulate_greens()
        t0 = time.perf_counter()
        mc.sweep(1)
        t_sweep = time.perf_counter() - t0
        t_exp, t_imp = [], []
        blob = mc.state()  # (the first call pays for the pages of the host buffer)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            blob = mc.state()
            t_exp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            mc.set_state(blob)
            t_imp.append(time.perf_counter() - t0)
        # the rebuild alone: an import of the same blob moves the bytes and rebuilds; prepare() is a rebuild of like size
        t0 = time.perf_counter()
        mc.prepare()
        t_prep = time.perf_counter() - t0
        lines.append(dict(case=case, bytes=int(blob.size), export_ms=1e3 * median(t_exp), import_ms=1e3 * median(t_imp),
                          export_GBps=blob.size / median(t_exp) / 1e9, prepare_ms=1e3 * t_prep, sweep_ms=1e3 * t_sweep,
                          reps=a.reps, source_hash=mc_amd.lib().dqmc_build_source_hash().decode()))
        mc.close()
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
