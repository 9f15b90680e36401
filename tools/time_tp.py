"""t-t' square 16 x 16 repulsive Hubbard model (t' = -0.25, mu = -0.4), beta = 8, 32 walkers: walker-sweeps/s and per-family
device ms per sweep (dqmc_timing_get: HIP events around every launch) with the four-factor path (ttp.hip) and with
DQMC_NO_KRON=1, alternating, REPS runs each.  One JSON line per run; `python tools/time_tp.py [sweeps] [out.jsonl] [reps]`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

m = g.load_package()
NS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 2
W, L, BETA, TP, MU = 32, 16, 8.0, -0.25, -0.4
lines = []
for rep in range(REPS):
    for dense in (False, True):
        if dense:
            os.environ["DQMC_NO_KRON"] = "1"
        mc = m.DQMC(m.HubbardModelRepulsive(L, 2, tp=TP, mu=MU), beta=BETA, n_walkers=W, seed=11)
        os.environ.pop("DQMC_NO_KRON", None)
        assert mc.kron_hopping() == (not dense)
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
        rec = dict(lattice="square %dx%d" % (L, L), model="repulsive", tp=TP, mu=MU, beta=BETA, walkers=W,
                   kron_hopping=mc.kron_hopping(), env="DQMC_NO_KRON=1" if dense else "default", sweeps_timed=NS,
                   ms_per_sweep=dt * 1e3, walker_sweeps_per_s=W / dt, device_errors=mc.device_errors(),
                   qr_fallbacks=mc.qr_fallbacks(), device_ms_per_sweep={k: v[0] / NS for k, v in tm.items()},
                   launches_per_sweep={k: v[1] // NS for k, v in tm.items()},
                   build_commit=m.lib().dqmc_build_commit().decode() if hasattr(m.lib(), "dqmc_build_commit") else None)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        mc.close()
if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
