"""Two-layer square 16 x 16 x 2 attractive Hubbard model (t_perp = 1.3), beta = 8, 16 walkers: walker-sweeps/s, per-family
device ms per sweep (dqmc_timing_get: HIP events around every launch) and the ten-step chain launch with the factored
path (bilayer.hip) and with DQMC_NO_KRON=1, alternating, REPS runs each.  One JSON line per run;
`python tools/time_bilayer.py [sweeps] [out.jsonl] [reps]`.

The chain launch is timed through dqmc_build_stack, whose gemm family holds, per stack interval, the safe_mult = 10 slice
products and the products of the UDT step behind them: the latter are the same launches on both paths, the former one
launch of bilayer_chain_kernel on the factored path and ten GEMMs on the dense one.  One such GEMM is timed through
dqmc_wrap_greens, which on the dense path at n = 512 is two of them (wrap_gemm_ms = half a wrap; on the factored path a
wrap is two one-step chain launches: wrap_ms).  So, per repetition,
  dense_products_ms = 10 wrap_gemm_ms,   chain_ms = factored interval - (dense interval - dense_products_ms)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

m = g.load_package()
NS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
W, L, BETA, TPERP = 16, 16, 8.0, 1.3
lines = []
for rep in range(REPS):
    pair = []
    for dense in (False, True):
        if dense:
            os.environ["DQMC_NO_KRON"] = "1"
        mc = m.DQMC(m.HubbardModelAttractive(l=m.BilayerSquareLattice(L), t_perp=TPERP), beta=BETA, n_walkers=W, seed=11)
        os.environ.pop("DQMC_NO_KRON", None)
        assert mc.kron_hopping() == (not dense)
        assert mc.p.safe_mult == 10
        mc.prepare()
        mc.sweep(1)
        mc.synchronize()
        t0 = time.perf_counter()
        mc.sweep(NS)
        mc.synchronize()
        dt = (time.perf_counter() - t0) / NS
        mc.timing_enable(True)
        mc.sweep(NS)
        mc.synchronize()
        tm = mc.timing()
        mc.timing_enable(False)
        mc.timing_enable(True)  # (a fresh count: the stack build alone)
        mc.build_stack()
        mc.synchronize()
        bs = mc.timing()
        mc.timing_enable(False)
        intervals = mc.p.slices // mc.p.safe_mult
        NWRAP = 8
        mc.timing_enable(True)
        for k in range(NWRAP):
            mc.wrap_greens(2 + k, 1)
        mc.synchronize()
        wr = mc.timing()
        mc.timing_enable(False)
        assert wr["gemm"][1] == 2 * NWRAP
        rec = dict(lattice="bilayer %dx%dx2" % (L, L), model="attractive", t_perp=TPERP, beta=BETA, walkers=W,
                   kron_hopping=mc.kron_hopping(), env="DQMC_NO_KRON=1" if dense else "default", sweeps_timed=NS,
                   ms_per_sweep=dt * 1e3, walker_sweeps_per_s=W / dt, device_errors=mc.device_errors(),
                   qr_fallbacks=mc.qr_fallbacks(), device_ms_per_sweep={k: v[0] / NS for k, v in tm.items()},
                   launches_per_sweep={k: v[1] // NS for k, v in tm.items()},
                   build_stack_gemm_ms_per_interval=bs["gemm"][0] / intervals,
                   build_stack_gemm_launches_per_interval=bs["gemm"][1] / intervals,
                   wrap_ms=wr["gemm"][0] / NWRAP,
                   build_commit=m.lib().dqmc_build_commit().decode() if hasattr(m.lib(), "dqmc_build_commit") else None)
        pair.append(rec)
        mc.close()
    pair[1]["wrap_gemm_ms"] = pair[1]["wrap_ms"] / 2.0
    pair[1]["dense_products_ms"] = 10.0 * pair[1]["wrap_gemm_ms"]
    pair[0]["chain_ms"] = pair[0]["build_stack_gemm_ms_per_interval"] - (pair[1]["build_stack_gemm_ms_per_interval"]
                                                                         - pair[1]["dense_products_ms"])
    for rec in pair:
        print(json.dumps(rec), flush=True)
        lines.append(rec)
if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
