"""In-kernel timeline of the elimination kernel (walker 0): build with `make -C montecarlo.jl_amd/csrc -f diag.mk lu4_stamps`,
run with DQMC_HIP_LIB=montecarlo.jl_amd/libdqmc_hip_lu4stamps.so python tools/lu4_stamps.py

Stamp map (cycles of s_memtime; the buffer holds 2048 words):
  0..63                  pivot: decision of site s begins
  64 (1 + J) + s         wave J: flag of site s seen and the next site's flag / payload requested
  320 + 8 J + k          phases of wave J;  360 / 361  kernel start / end;  400 + 8 J + k  prologue
  512 + 64 (J - 1) + s   helper J: flag of site s seen (before the next site is requested)
  704 + 64 (J - 1) + s   helper J: strip MFMAs of site s issued
  896 + 48 (J - 1) + 3 (4 I0 + r0) + k   helper J, panel r0 of block I0: k = 0 panel end entered, 1 tile (J, J) issued,
                         2 strips of the waves between waited for and every k = 4 MFMA issued
A stamp is s_memtime, a wait for it (which drains the LDS requests in flight as well) and a store: every figure of a build
with stamps in the site loop is inflated, and two such builds compare with each other, not with the product."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
gpu = g.load_package()
L = gpu.lib()
buf = torch.zeros(2048, dtype=torch.int64, device="cuda:0")
L.dqmc_debug_lu4_stamps.argtypes = [C.c_void_p]
assert L.dqmc_debug_lu4_stamps(C.c_void_p(buf.data_ptr())) == 0
model = gpu.HubbardModelAttractive(16, 2)
mc = gpu.DQMC(model, beta=8.0, delta_tau=0.1, safe_mult=10, n_walkers=32, seed=123)
mc.prepare()
mc.sweep(1)


def med(x):
    return int(np.median(x)) if len(x) else 0


def helper_sites(t, J, I0):
    """Per-site split of helper J in block I0, sites with c = 1..14 that are not the first of a panel (steady state):
    wait = flag seen - previous site's MFMAs issued; request = next site requested - flag seen;
    mfma = strip MFMAs issued - next site requested; lag = flag seen - the pivot's decision stamp."""
    seen, req, done = t[512 + 64 * (J - 1):][:64], t[64 * (1 + J):][:64], t[704 + 64 * (J - 1):][:64]
    w, r, m, lag, tot = [], [], [], [], []
    for c in range(1, 15):
        s = 16 * I0 + c
        if c % 4 == 0 or not (seen[s] and done[s - 1]):
            continue
        w.append(seen[s] - done[s - 1]); r.append(req[s] - seen[s]); m.append(done[s] - req[s])
        lag.append(seen[s] - t[s]); tot.append(done[s] - done[s - 1])
    return w, r, m, lag, tot


def panel_ends(t, J, I0):
    p = t[896 + 48 * (J - 1) + 12 * I0:][:12].reshape(4, 3)
    last = t[704 + 64 * (J - 1) + 16 * I0:][:16]
    rows = []
    for r0 in range(4):
        if not p[r0, 0]:
            continue
        ls = last[4 * r0 + 3] if r0 < 3 else t[512 + 64 * (J - 1) + 16 * I0 + 15]  # site 15: no MFMAs, its flag
        rows.append((int(p[r0, 0] - ls), int(p[r0, 1] - p[r0, 0]), int(p[r0, 2] - p[r0, 1])))
    return rows


for rep in range(3):
    buf.zero_()
    mc.update()
    torch.cuda.synchronize()
    t = buf.cpu().numpy().astype(np.int64)
    t0 = t[360]
    rel = lambda x: (x - t0) if x else 0  # (0: this stamp is not in the build)
    piv = t[:64]
    print("kernel start->end: %d cycles" % (t[361] - t0))
    for J in range(4):
        b = 320 + 8 * J
        print(" wave %d: prologue done %d, start %d, tiles loaded %d, block ends %s, done %d" % (J, rel(t[b + 7]), rel(t[b]), rel(t[b + 1]), [int(rel(x)) if x else 0 for x in t[b + 2:b + 6]], rel(t[b + 6])))
    if t[400]:
        for J in range(4):
            b = 400 + 8 * J
            print(" wave %d prologue: entered %d, loads issued %d, loads arrived %d, solves done %d, barrier passed %d" % ((J,) + tuple(int(rel(t[b + k])) for k in range(5))))
    if not piv[1]:  # STAMP_LEVEL=2: no stamps in the site loop
        continue
    print(" pivot step stamps (rel):", [int(rel(x)) for x in piv[::4]])
    d = np.diff(piv)
    print(" pivot step deltas: block0 %s" % d[:15].tolist())
    print("                    block1 %s" % d[16:31].tolist())
    print("   pivot site, median of the deltas inside a block: %s" % [med(d[16 * I:16 * I + 15]) for I in range(4)])
    print("   block transitions:", int(piv[16] - piv[15]), int(piv[32] - piv[31]), int(piv[48] - piv[47]))
    for J in (1, 2, 3):  # hand-over to wave J: last decision of block J-1 -> its payload seen by J -> J's block end -> J decides
        sl = 16 * J - 1
        hJ = t[64 * (1 + J):64 * (2 + J)]
        print(" hand-over %d->%d: payload of site %d seen +%d, panel/strips done +%d, first decision +%d (cycles after that site's decision stamp)" % (
            J - 1, J, sl, hJ[sl] - piv[sl], t[320 + 8 * J + 2 + (J - 1)] - piv[sl], piv[sl + 1] - piv[sl]))
    for J in (1, 2, 3):
        h = t[64 * (1 + J):64 * (2 + J)]
        lag = [int(h[s] - piv[s]) for s in range(0, 16 * J, 3)]
        print(" helper %d lag behind the pivot's decision stamp:" % J, lag)
        print(" helper %d own site-to-site deltas, block 0:" % J, np.diff(h[:16]).tolist())
    for I0 in range(3):  # the helpers of block I0; J = I0 + 1 pivots next
        for J in range(I0 + 1, 4):
            w, r, m, lag, tot = helper_sites(t, J, I0)
            print(" block %d helper %d%s, per site (median; sites inside a panel): wait for flag %d, next request %d, select + strip MFMAs %d, site %d;"
                  " flag seen %d after the decision began (min %d, max %d); waits %s" % (
                      I0, J, " (next pivot)" if J == I0 + 1 else "", med(w), med(r), med(m), med(tot), med(lag),
                      min(lag) if lag else 0, max(lag) if lag else 0, [int(x) for x in w]))
            print("   panel ends (last site's MFMAs -> entered, entered -> tile (J, J) issued, -> strips of others and all issued): %s" % panel_ends(t, J, I0))
mc.close()
