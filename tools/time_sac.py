"""Rate of the SAC flavor (csrc/sac.hip), one JSON line per measurement.

Device: 256 problems x 8 replicas, Nt = 40, Nd = 256, Nw = 2000 on the fermion kernel (beta = 10, two-peak spectra with
noise 1e-3, different per problem), an exchange round after every sweep and a refresh after every 16th: moves per second
of `sweep` calls after a warm-up call, three turns, every one reported.  Host: the numpy restatement (tests/sac_ref.py)
of one of those problems on one core, moves per second over a few sweeps.

    python tools/time_sac.py [--out FILE] [--problems P] [--sweeps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NT, ND, NW, R, BETA = 40, 256, 2000, 8, 10.0
THETAS = [4.0 * 0.6 ** r for r in range(R)]


def problems(P, seed=1):
    import sac_ref
    rng = np.random.RandomState(seed)
    tau, omega = np.linspace(0.0, BETA, NT), np.linspace(-8.0, 8.0, NW)
    K = sac_ref.fermion_kernel(tau, omega, BETA)
    G = np.zeros((P, NT))
    for p in range(P):
        c = rng.uniform(-3.0, 3.0, 2)
        A = 0.4 * np.exp(-0.5 * ((omega - c[0]) / 0.4) ** 2) + 0.6 * np.exp(-0.5 * ((omega - c[1]) / 0.4) ** 2)
        G[p] = K @ (A / A.sum()) + 1e-3 * rng.standard_normal(NT)
    return tau, omega, K, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--sweeps", type=int, default=1000)
    ap.add_argument("--host-sweeps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    import sac_ref
    if pkg.device_count() < 1:
        raise RuntimeError("time_sac: no HIP device visible")
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    tau, omega, K, G = problems(a.problems)
    s = pkg.SAC(tau, G, error=1e-3, kernel=K, omega=omega, n_deltas=ND, thetas=THETAS, seed=11, window=NW // 20)
    s.set_exchange(1)
    s.sweep(a.sweeps, 0, 16)  # warm-up: code objects, first touches
    for turn in range(3):
        t = time.perf_counter()
        s.sweep(a.sweeps, 0, 16)  # complete on return (dqmc_sac_sweep synchronises)
        dt = time.perf_counter() - t
        moves = a.sweeps * ND * R * a.problems
        emit({"what": "device", "problems": a.problems, "replicas": R, "Nt": NT, "Nd": ND, "Nw": NW, "sweeps": a.sweeps,
              "turn": turn, "seconds": dt, "moves_per_second": moves / dt})
    st = s.stats(0, R - 1)
    emit({"what": "device_state", "acceptance_coldest": st.acc / st.prop, "max_drift": st.max_drift})
    lad = sac_ref.Ladder(s.g[0], s.w[0], s.Kt[0], 1.0, THETAS, [s.chain_seed(0, r) for r in range(R)],
                         [sac_ref.default_positions(ND, NW)] * R, NW // 20)
    lad.set_exchange(1)
    s.close()
    t = time.perf_counter()
    lad.sweep(a.host_sweeps, 1, 0, 16)
    dt = time.perf_counter() - t
    emit({"what": "host_numpy_one_core", "problems": 1, "replicas": R, "sweeps": a.host_sweeps, "seconds": dt,
          "moves_per_second": a.host_sweeps * ND * R / dt})


if __name__ == "__main__":
    main()
