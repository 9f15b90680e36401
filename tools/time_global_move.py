"""Global moves at bench config 3 (attractive 16 x 16, beta = 8, dtau = 0.1, 32 walkers): moves per second and the
acceptance rate of both kinds, with the time of one local sweep of the same handle beside it, and the time of one
dqmc_logdet.  Between two moves one local sweep runs, so the cache of the current field's logabsdet is cold as it is
inside a run.  One JSON line per kind; `python tools/time_global_move.py [moves] [U] [out.jsonl]`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

m = g.load_package()
NM = int(sys.argv[1]) if len(sys.argv) > 1 else 5
U = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
OUT = sys.argv[3] if len(sys.argv) > 3 else None
W, L, BETA = 32, 16, 8.0
lines = []
for kind in ("site", "all"):
    mc = m.DQMC(m.HubbardModelAttractive(L, 2, U=U), beta=BETA, n_walkers=W, seed=11)
    mc.prepare()
    mc.sweep(1)
    mc.global_move(kind)  # warm-up: first launches of the kernels
    t_move = t_sweep = 0.0
    for _ in range(NM):
        t0 = time.perf_counter()
        mc.sweep(1)
        t1 = time.perf_counter()
        mc.global_move(kind)
        t2 = time.perf_counter()
        t_sweep += t1 - t0
        t_move += t2 - t1
    t0 = time.perf_counter()
    mc.logdet()
    t_logdet = time.perf_counter() - t0
    st = [mc.global_stats(w) for w in range(W)]
    prop, acc = sum(s["prop_global"] for s in st), sum(s["acc_global"] for s in st)
    rec = dict(config="attractive %dx%d beta %g U %g" % (L, L, BETA, U), walkers=W, kind=kind, moves_timed=NM,
               ms_per_move=t_move / NM * 1e3, walker_moves_per_s=W * NM / t_move, ms_per_local_sweep=t_sweep / NM * 1e3,
               ms_per_logdet=t_logdet * 1e3, prop_global=prop, acc_global=acc, acceptance=acc / prop if prop else None,
               device_errors=mc.device_errors(), build_commit=m.lib().dqmc_build_commit().decode())
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    mc.close()
if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
