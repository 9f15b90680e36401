"""ISA budget of the binning kernels (binner.hip), in the style of test_isa_ising.py: both kernels are in the shipped
code object, and they are plain streaming code - no flat memory operations, no scratch, no MFMA, no LDS, no atomics,
and every store to memory is a vector store."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_guard import _load_shipped, _runs_and_flat  # noqa: E402


@pytest.fixture(scope="module")
def binner_kernels():
    hits = {n: v for n, v in _load_shipped().items() if "dqmc::binner_" in n and "(" in n}
    # one push kernel per sample source (plain, Green's function, correlations) and the finish kernel
    assert sum("binner_push_kernel<" in n for n in hits) == 3, sorted(hits)
    assert sum("binner_finish_kernel" in n for n in hits) == 1, sorted(hits)
    return hits


def test_binner_kernels_are_plain_streaming_code(binner_kernels):
    for name, ins in binner_kernels.items():
        _, flat = _runs_and_flat(ins)
        assert flat == 0 and not any(t.startswith("flat_") for t in ins), (name, "flat memory operations")
        assert not any(t.startswith(("scratch_", "buffer_store", "buffer_load")) for t in ins), (name, "scratch")
        assert not any(t.startswith("v_mfma") for t in ins), (name, "MFMA")
        assert not any(t.startswith("ds_") for t in ins), (name, "LDS")
        assert not any("atomic" in t for t in ins), (name, "atomics")
        stores = [t for t in ins if "store" in t.split()[0]]
        assert stores and all(t.startswith("global_store_dword") for t in stores), (name, sorted(set(t.split()[0] for t in stores)))


def test_binner_kernels_move_doubles(binner_kernels):
    """every load and store of the state is a whole double per lane (dwordx2), contiguous across the wave"""
    for name, ins in binner_kernels.items():
        mem = [t.split()[0] for t in ins if t.startswith(("global_load", "global_store"))]
        assert mem and all(m in ("global_load_dwordx2", "global_store_dwordx2", "global_load_dwordx4",
                                 "global_store_dwordx4") for m in mem), (name, sorted(set(mem)))
