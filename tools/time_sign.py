"""Cost of sign weighting at 16 x 16 with 32 walkers (beta = 8, dtau = 0.1, the shape of bench config 3): the time of one
measurement pass (accumulate_greens, synchronised) with weighting on against off, on the same handle and build, with
the time of one local sweep beside it.  Between two passes one sweep runs, so the kept determinant signs are stale as
they are inside a run and a weighted pass of the repulsive model pays its slice chain.  The attractive model's sign is +1
by construction: its weighted pass runs no chain and is listed as the control.  One JSON line per model;
`python tools/time_sign.py [passes] [U] [out.jsonl]`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

m = g.load_package()
NP = int(sys.argv[1]) if len(sys.argv) > 1 else 5
U = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
OUT = sys.argv[3] if len(sys.argv) > 3 else None
W, L, BETA = 32, 16, 8.0
lines = []
for name, cls in (("repulsive", m.HubbardModelRepulsive), ("attractive", m.HubbardModelAttractive)):
    mc = m.DQMC(cls(L, 2, U=U), beta=BETA, n_walkers=W, seed=11)
    mc.prepare()
    mc.sweep(1)
    t_pass, t_sweep = {}, 0.0
    for on in (False, True, False, True):  # off, on, off, on: drift shows as a difference between the two rounds
        mc.reset_accumulators()
        mc.set_sign_weighting(on)
        mc.accumulate_greens()  # warm-up: first launches of the kernels
        for _ in range(NP):
            t0 = time.perf_counter()
            mc.sweep(1)
            t1 = time.perf_counter()
            mc.accumulate_greens()
            mc.synchronize()
            t2 = time.perf_counter()
            t_sweep += t1 - t0
            t_pass.setdefault(on, []).append(t2 - t1)
    ms = {on: 1e3 * sum(v) / len(v) for on, v in t_pass.items()}
    ms_sweep = 1e3 * t_sweep / (4 * NP)
    extra = ms[True] - ms[False]
    rec = dict(config="%s %dx%d beta %g U %g" % (name, L, L, BETA, U), walkers=W, passes_timed=2 * NP,
               ms_per_pass_off=ms[False], ms_per_pass_on=ms[True], ms_extra=extra, ms_per_local_sweep=ms_sweep,
               extra_over_sweep=extra / ms_sweep, share_at_measure_rate_10=extra / (10 * ms_sweep),
               mean_sign=mc.mean_sign("greens"), sign_failures=int(mc.sign_failures().sum()),
               device_errors=mc.device_errors(), build_commit=m.lib().dqmc_build_commit().decode())
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    mc.close()
if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
