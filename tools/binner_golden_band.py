"""Scatter of a single run's binned std_error at the attractive 4 x 4 golden run shape (beta = 1, 10 + 1000 sweeps,
measure_rate = 10), from the CPU oracle over seeds: the band of tests/test_gpu_binner.py::
test_binned_errors_against_the_published_ones.  python tools/binner_golden_band.py N_SEEDS (no GPU; imports the package
for rand_conf only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
from oracle import oracle as O, ref_test_oracle as R
from logbinner_ref import LogBinnerRef
import __graft_entry__ as g
mc_amd=g.load_package()
O.build()
L=4
def chain(seed):
    o=O.OracleDQMC(L,"attractive",beta=1.0)
    rng=np.random.Generator(np.random.Philox(key=seed))
    o.set_conf(mc_amd.rand_conf(rng,16,10)); o.seed(seed); o.prepare()
    bG,bC=LogBinnerRef(16),LogBinnerRef(16)
    for i in range(1,1011):
        o.sweeps(1)
        if i>10 and i%10==0:
            G=o.greens()
            bG.push(np.diag(G[0])); bC.push(R.equal_time_correlations(G,L,True)["CDC"])
    assert bG.reliable_level()==1
    return bG.std_error(), bC.std_error()
t0=time.time(); res=[chain(7000+s) for s in range(int(sys.argv[1]))]
print("time",time.time()-t0)
for k,name in ((0,"G"),(1,"CDC")):
    se=np.array([r[k] for r in res]); pooled=np.sqrt((se**2).mean(0))
    ratio=np.median(se/pooled,axis=1)
    print(name,"pooled",pooled.round(5)); print(name,"ratio per seed: mean %.4f sd %.4f min %.4f max %.4f"%(ratio.mean(),ratio.std(ddof=1),ratio.min(),ratio.max()))
    print(np.sort(ratio).round(3))
