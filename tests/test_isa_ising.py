"""ISA budget of the Ising kernels (ising.hip), in the style of test_isa_kron3.py: no flat memory operations, no scratch,
at most three load -> s_waitcnt vmcnt(0) pairs in a row (the cold prologue that brings a walker's words into LDS), and
the site loop reads its row of the neighbour table with scalar loads, no per-lane gather."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_guard import _load_shipped, _runs_and_flat  # noqa: E402


@pytest.fixture(scope="module")
def ising_kernels():
    hits = {n: v for n, v in _load_shipped().items() if "dqmc_mc::ising_" in n and "(" in n}
    assert sum("ising_sweep_kernel<" in n for n in hits) == 8, sorted(hits)
    assert any("ising_rand_conf_kernel" in n for n in hits) and any("ising_observables_kernel" in n for n in hits)
    return hits


def test_ising_kernels_budget(ising_kernels):
    for name, ins in ising_kernels.items():
        run, flat = _runs_and_flat(ins)
        assert run <= 3, (name, "consecutive load -> s_waitcnt vmcnt(0) pairs", run)
        assert flat == 0, (name, "flat memory operations", flat)
        assert not any(t.startswith(("scratch_", "buffer_store", "buffer_load")) for t in ins), (name, "scratch")
        assert not any(t.startswith("v_mfma") for t in ins), name


def test_ising_sweep_reads_the_neighbour_row_with_scalar_loads(ising_kernels):
    """the only loads of the sweep kernel are its prologue's and epilogue's: a walker's words, counters, sums and
    thresholds (one per array, a few more where the compiler splits the word loop), none per site"""
    for name, ins in ising_kernels.items():
        if "ising_sweep_kernel<" not in name:
            continue
        vec = sum(t.startswith("global_load") for t in ins)
        z = int(name.split("ising_sweep_kernel<")[1].split(">")[0])
        assert vec <= 24 + z, (name, "vector loads", vec)
        assert any(t.startswith("s_load_dwordx4") and "0x0" in t for t in ins), name
