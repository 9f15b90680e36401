"""The prologue of the elimination workgroup inside a fused sweep launch (sweep_lu.hip, lu4_wave with PRO): the previous
chunk of 64 sites is still pending, so every wave first stages that chunk's images, solves for its T' rows and adds its
share of T R0 to its tiles.  Attractive model (one block per walker): images and the R0 block are staged in LDS by all
four waves together (one memory round trip), wave 0 leaves its T' tiles in LDS and goes on to the decisions, waves 1..3
make the products of block row 0 from there and send each other the tiles to their right as deltas.  Repulsive model (two
blocks): operands in registers, all four waves meet at two barriers.

Compared with the oracle after every propagate / sweep_spatial as in test_gpu_sweep_handover.py (run_case): HS field bit
for bit, uniforms consumed and acceptance counters equal, G within 1e-10.  beta = 1 with safe_mult = 5 gives 10 time
slices in two stack blocks; every case goes up and back through all of them (2 x slices + 3 updates: both directions,
both wraps), which visits more than three slices in each direction.  Shapes, the smallest that reach each form:
  16 x 16 attractive   four chunks: three fused launches per slice, the products of all four waves
  ... with recorded uniforms u = 0 (every proposal accepted: dense previous chunks) and u = 1 - 2^-53 (only p > 1
                       is accepted, about 0.17 at U = 1: sparse previous chunks)
  Chain(128)           two chunks: ONE fused launch per slice, its prologue right behind the stand-alone elimination
  Chain(192)           three chunks, fused launches off the 256 grid (64-column flush workgroups beside them)
  16 x 16 repulsive    the two-barrier prologue
  16 x 16 attractive, default against DQMC_SWEEP_SPLIT=1 in a fresh handle: the same chunks with the flush between the
                       eliminations, no prologue at all
U = 1 throughout (at U = 8 engine and oracle differ by 1.45e-10 whatever the sweep kernels do)."""
import os

import numpy as np
import pytest
import torch  # (at import time, before the library opens the device)

from conftest import relerr
from test_gpu_sweep_handover import make_model, run_case, sweep_fused_rule

pytestmark = pytest.mark.gpu
NUPD = 2 * 10 + 3  # beta = 1, delta_tau = 0.1: 10 slices


def test_early_prologue_matches_oracle(gpu, O):
    """16 x 16 attractive, 2 walkers, seeded stream: chunks 1..3 of every slice run the early prologue"""
    worst, rate, _ = run_case(gpu, O, ("square", 16), "attractive", 2, NUPD, fused=True)
    assert 0.5 < rate < 1.0  # (0.91 in the oracle at U = 1: most sites of a previous chunk have x != 0)


def test_early_prologue_dense_previous_chunks(gpu, O):
    """recorded uniforms u = 0: every proposal accepted, every x of the pending chunk nonzero"""
    _, rate, _ = run_case(gpu, O, ("square", 16), "attractive", 2, NUPD, uniforms=np.zeros(256 * (NUPD + 2)), fused=True)
    assert rate == 1.0


def test_early_prologue_sparse_previous_chunks(gpu, O):
    """recorded uniforms just below 1: only proposals with p > 1 are accepted (they consume no uniform), so most rows of
    the pending chunk's T' are zero"""
    uni = np.full(256 * (NUPD + 2), 1.0 - 2.0 ** -53)
    _, rate, _ = run_case(gpu, O, ("square", 16), "attractive", 2, NUPD, uniforms=uni, fused=True)
    assert 0.1 < rate < 0.25


@pytest.mark.parametrize("n", [128, 192])
def test_early_prologue_on_chains(gpu, O, n):
    """Chain(128): two chunks, one fused launch per slice; Chain(192): three chunks, n % 128 != 0"""
    run_case(gpu, O, ("chain", n), "attractive", 2, NUPD, fused=True)


def test_two_barrier_prologue_matches_oracle(gpu, O):
    """16 x 16 repulsive, 2 walkers (two blocks per walker: no LDS for the staged images, all waves meet at barriers)"""
    run_case(gpu, O, ("square", 16), "repulsive", 2, NUPD, fused=True)


def _handle(gpu, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # kernel switches are read when a handle is created
    try:
        return gpu.DQMC(make_model(gpu, ("square", 16), "attractive"), beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2,
                        seed=31)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_fused_against_split_launches(gpu):
    """16 x 16 attractive, same seeds: the default handle (fused launches) against a fresh one with DQMC_SWEEP_SPLIT=1
    (elimination, flush, elimination, ...): HS fields and counters equal, G within 1e-12 after every call"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert sweep_fused_rule(256, 2, 1, cus)
    mcs = [_handle(gpu, {}), _handle(gpu, {"DQMC_SWEEP_SPLIT": "1"})]
    for mc in mcs:
        mc.prepare()
    worst = 0.0
    for step in range(NUPD):
        for mc in mcs:
            mc.propagate()
            mc.sweep_spatial()
        for w in range(2):
            assert np.array_equal(mcs[0].conf(w), mcs[1].conf(w)), (step, w)
            assert mcs[0].uniforms_used(w) == mcs[1].uniforms_used(w)
            for a, b in zip(mcs[0].greens_eff(w), mcs[1].greens_eff(w)):
                worst = max(worst, relerr(a, b))
    print("16 x 16 attractive: worst rel |G_fused - G_split| = %.3g" % worst)
    for w in range(2):
        a, b = mcs[0].analysis(w), mcs[1].analysis(w)
        assert (a.prop_local, a.acc_local) == (b.prop_local, b.acc_local)
    for mc in mcs:
        mc.close()
    assert worst < 1e-12
