"""Rectangular 32 x 8 attractive Hubbard model, beta = 8, 32 walkers: walker-sweeps/s, per-family device ms per sweep
(dqmc_timing_get: HIP events around every launch), the gemm family of one stack interval and one wrap with the factored
path (rect.hip) and with DQMC_NO_KRON=1 (slab.hip), alternating, REPS runs each.  One JSON line per run;
`python tools/time_rect.py [sweeps] [out.jsonl] [reps]`.

The gemm family of dqmc_build_stack holds, per stack interval, the safe_mult = 10 slice products and the products of the
UDT step behind them: the latter are the same launches on both paths, the former one launch of rect_chain_kernel on the
factored path and one of slab_chain_kernel on the dense one, so the difference of the two interval figures is the
difference of the two chain launches.  A wrap (dqmc_wrap_greens) is two one-step rect launches on the factored path and
one slab launch on the dense one: wrap_ms, with wrap_launches saying which."""
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
W, LX, LY, BETA = 32, 32, 8, 8.0
lines = []
for rep in range(REPS):
    for dense in (False, True):
        if dense:
            os.environ["DQMC_NO_KRON"] = "1"
        mc = m.DQMC(m.HubbardModelAttractive(l=m.RectangularLattice(LX, LY)), beta=BETA, n_walkers=W, seed=11)
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
        rec = dict(lattice="rectangular %dx%d" % (LX, LY), model="attractive", beta=BETA, walkers=W,
                   kron_hopping=mc.kron_hopping(), env="DQMC_NO_KRON=1" if dense else "default", sweeps_timed=NS,
                   ms_per_sweep=dt * 1e3, walker_sweeps_per_s=W / dt, device_errors=mc.device_errors(),
                   qr_fallbacks=mc.qr_fallbacks(), device_ms_per_sweep={k: v[0] / NS for k, v in tm.items()},
                   launches_per_sweep={k: v[1] // NS for k, v in tm.items()},
                   build_stack_gemm_ms_per_interval=bs["gemm"][0] / intervals,
                   build_stack_gemm_launches_per_interval=bs["gemm"][1] / intervals,
                   wrap_ms=wr["gemm"][0] / NWRAP, wrap_launches=wr["gemm"][1] / NWRAP,
                   build_commit=m.lib().dqmc_build_commit().decode() if hasattr(m.lib(), "dqmc_build_commit") else None)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        mc.close()
if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
