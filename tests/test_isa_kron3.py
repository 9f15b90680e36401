"""ISA budget of the three-factor Kronecker chain kernel (kron3.hip), in the style of test_isa_kron.py: no flat memory
operations, at most one load -> s_waitcnt vmcnt(0) pair in a row, no MFMA source-C write-after-read, MFMAs present."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_guard import _load_shipped, _runs_and_flat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kron3_kernels():
    hits = {n: v for n, v in _load_shipped().items() if "kron3_chain_kernel" in n and "(" in n}
    assert hits, "kron3_chain_kernel is not in the shipped library"
    return hits


def test_kron3_chain_kernel_budget(kron3_kernels):
    for name, ins in kron3_kernels.items():
        run, flat = _runs_and_flat(ins)
        assert run <= 1, (name, "consecutive load -> s_waitcnt vmcnt(0) pairs", run)
        assert flat == 0, (name, "flat memory operations", flat)
        # one step of each parity: 64 + 16 MFMAs per pair
        assert sum(t.startswith("v_mfma_f64_16x16x4") for t in ins) >= 80


def test_kron3_chain_kernel_has_no_mfma_source_c_hazard(kron3_kernels):
    import scan_mfma_war as W
    for name, ins in kron3_kernels.items():
        assert not W.hazards(["\t" + t for t in ins]), name
