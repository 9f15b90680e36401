"""Cost of the device-side binning at the benchmark shape (attractive 16 x 16, beta = 8, 32 walkers: n = 256).

  python tools/time_binner.py [--pushes 1024] [--out FILE]

Times `pushes` calls of accumulate_greens without and with the Green's section binner on one handle (the difference is
the push kernel, launches included), a device-to-device copy of the same number of bytes in the same process, and one
sweep, and prints one JSON line: bytes moved per push (counted from the cascade lengths: the sample, x_sum and x2_sum
read and written on every level touched, the compressor read on completed levels and written on the last), achieved
bandwidth, the ratio to the copy, and the cost of one binned accumulate_greens in sweeps.  Needs the GPU."""
import argparse
import json
import os
import sys
import time

import torch  # (before the library opens the device: imported later it reports no HIP device)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def push_bytes(t, n_values, top):
    """bytes binner_push_kernel moves for push index t over n_values = W * E binners"""
    lmax = 0
    while (t >> lmax) & 1:
        lmax += 1
    return 8 * n_values * (1 + 4 * (lmax + 1) + lmax + (1 if lmax < top else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=1024)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mc_amd = g.load_package()
    if mc_amd.device_count() < 1:
        raise SystemExit("time_binner.py needs the GPU")
    W = 32
    mc = mc_amd.DQMC(mc_amd.HubbardModelAttractive(16, 2), beta=8.0, delta_tau=0.1, n_walkers=W, seed=1)
    mc.prepare()
    mc.sweep(1)

    def timed(fn, reps):
        mc.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        mc.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    timed(mc.accumulate_greens, 16)                                  # warm-up
    t_off = timed(mc.accumulate_greens, a.pushes)
    mc.enable_binning(("greens",))
    E, L, _ = mc.binner_size("greens")
    timed(mc.accumulate_greens, 16)
    mc.reset_accumulators()
    t_on = timed(mc.accumulate_greens, a.pushes)
    assert mc.binner_size("greens")[2] == a.pushes
    nbytes = sum(push_bytes(t, W * E, L - 1) for t in range(a.pushes)) / a.pushes
    # a copy moves its bytes twice (read + write): same traffic = nbytes / 2 copied
    src = torch.empty(int(nbytes // 16), dtype=torch.float64, device="cuda:0").normal_()
    dst = torch.empty_like(src)
    timed(lambda: dst.copy_(src), 16)
    t_copy = timed(lambda: dst.copy_(src), a.pushes)
    t_sweep = timed(lambda: mc.sweep(1), a.sweeps)
    t_push = t_on - t_off
    res = dict(shape="attractive 16x16 beta=8, n=256, W=%d" % W, pushes=a.pushes, elements_per_walker=E, levels=L,
               state_bytes=8 * (3 * L - 1) * W * E, bytes_per_push=nbytes,
               accumulate_greens_us=1e6 * t_off, binned_accumulate_greens_us=1e6 * t_on, push_us=1e6 * t_push,
               push_TBps=nbytes / t_push / 1e12, copy_us=1e6 * t_copy, copy_TBps=2 * src.numel() * 8 / t_copy / 1e12,
               push_over_copy=t_push / t_copy, sweep_ms=1e3 * t_sweep,
               binned_accumulate_greens_in_sweeps=t_on / t_sweep, source_hash=mc_amd.lib().dqmc_build_source_hash().decode())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    mc.close()


if __name__ == "__main__":
    main()
