"""In-kernel timeline of the wrap launch that applies a sweep's pending last chunk (kron_wrap_kernel<true>, or
kron_chain_kernel<true> under DQMC_WRAP_TWO_LAUNCH=1; config 3 shape): build the library with `make -C montecarlo.jl_amd/csrc XFLAGS=-DKR_STAMPS` (add -DKR_NO_XCD_GROUPS for the unit
placement without XCD grouping, -DKR_PROBE_PRODUCTS for the timing probe of the product form of the solves: wrong values) in a copy of the tree, run with DQMC_HIP_LIB=<that library> python tools/kr_stamps.py.
Stamps per workgroup (wave 0): 0 start, 2 image + R0 in LDS (first barrier passed), 3 solves done, 4 product D = C R^
issued, 5 update added to X_0, 6 the wrap step done, 7 result stored (one launch: P' stored write-through and drained),
and in the one-launch form 9 hand-off over (barrier, arrival, the unit's 16 workgroups in, acquire, barrier), 10 second
step done and stored; 1 / 8 the 100 MHz clock at start / end."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
gpu = g.load_package()
L = gpu.lib()
WG = 32 * 16
buf = torch.zeros(16 * WG, dtype=torch.int64, device="cuda:0")
L.dqmc_debug_kr_stamps.argtypes = [C.c_void_p]
assert L.dqmc_debug_kr_stamps(C.c_void_p(buf.data_ptr())) == 0
mc = gpu.DQMC(gpu.HubbardModelAttractive(16, 2), beta=8.0, delta_tau=0.1, safe_mult=10, n_walkers=32, seed=123)
mc.prepare()
mc.update_until_measure()
one_launch = "DQMC_WRAP_TWO_LAUNCH" not in os.environ
names = ["barrier 1 (image, R0)", "solves", "C fetch + product", "update into X_0", "wrap step", "store"]
stamps = [2, 3, 4, 5, 6, 7]
if one_launch:
    names += ["hand-off wait", "second step + store"]
    stamps += [9, 10]
last = stamps[-1]
for rep in range(3):
    buf.zero_()
    for _ in range(3):  # (the stamps of the last folded wrap of the call remain)
        mc.update()
    mc.sweep(1)
    torch.cuda.synchronize()
    t = buf.cpu().numpy().astype(np.int64).reshape(WG, 16)
    t = t[t[:, 0] != 0]
    cyc = (t[:, last] - t[:, 0]).astype(float)
    ns = (t[:, 8] - t[:, 1]) * 10.0
    ghz = np.median(cyc / ns)
    start = (t[:, 1] - t[:, 1].min()) * 10.0 / 1000
    print("rep %d: %d workgroups, %.2f GHz, workgroup start spread %.2f us, launch (first start -> last end) %.2f us"
          % (rep, len(t), ghz, start.max(), ((t[:, 8].max() - t[:, 1].min()) * 10.0) / 1000))
    print("  workgroup lifetime: median %.2f us, max %.2f us" % (np.median(cyc) / ghz / 1000, cyc.max() / ghz / 1000))
    prev = t[:, 0]
    for k, name in zip(stamps, names):
        d = (t[:, k] - prev) / ghz / 1000
        print("  %-24s median %6.2f us  p90 %6.2f us  max %6.2f us" % (name, np.median(d), np.percentile(d, 90), d.max()))
        prev = t[:, k]
mc.close()
