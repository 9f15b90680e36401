"""ISA budget of the t-t' square-lattice chain kernel (ttp.hip), in the style of test_isa_triangular.py: no flat memory
operations, at most one load -> s_waitcnt vmcnt(0) pair in a row, no MFMA source-C write-after-read, 16 MFMAs per column
per step, at most three LDS passes per step, no scratch, and registers and LDS for two workgroups per CU."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_isa_guard import _load_shipped, _runs_and_flat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "montecarlo.jl_amd", "libdqmc_hip.so")
COLUMNS_PER_WAVE = 4  # TP_NC of ttp.hip


@pytest.fixture(scope="module")
def ttp_kernels():
    hits = {n: v for n, v in _load_shipped().items() if "ttp_chain_kernel" in n and "(" in n}
    assert hits, "ttp_chain_kernel is not in the shipped library"
    return hits


def test_ttp_chain_kernel_budget(ttp_kernels):
    for name, ins in ttp_kernels.items():
        run, flat = _runs_and_flat(ins)
        assert run <= 1, (name, "consecutive load -> s_waitcnt vmcnt(0) pairs", run)
        assert flat == 0, (name, "flat memory operations", flat)
        assert not any(t.startswith(("scratch_", "buffer_store", "buffer_load")) for t in ins), name
        # one step (the loop body, the only place with MFMAs): 4 products x 4 k-blocks x 4 columns per wave
        assert sum(t.startswith("v_mfma_f64_16x16x4") for t in ins) == 16 * COLUMNS_PER_WAVE
        assert not any(t.startswith("v_mfma") and not t.startswith("v_mfma_f64_16x16x4") for t in ins)
        assert sum(t.startswith("s_barrier") for t in ins) <= 5  # three per step, two around the staging image
        # LDS: per step three passes of 16 writes and 16 reads (4 columns x 4 registers); the staging image adds 16 writes
        # and 8 reads in each of its two store forms
        writes = sum(t.startswith("ds_write") for t in ins)
        reads = sum(t.startswith("ds_read") for t in ins)
        assert writes <= 3 * 16 + 16 and reads <= 3 * 16 + 2 * 8, (writes, reads)
        assert not any(t.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")) for t in ins)  # S -> R goes through a tile


def test_ttp_chain_kernel_has_no_mfma_source_c_hazard(ttp_kernels):
    import scan_mfma_war as W
    for name, ins in ttp_kernels.items():
        assert not W.hazards(["\t" + t for t in ins]), name


def test_ttp_chain_kernel_resources():
    """no spills, no scratch, and VGPRs and LDS that let two workgroups (8 waves) share a CU"""
    import shutil
    import tempfile
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(LIB) and os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("library or llvm tools missing")
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(LIB, os.path.join(tmp, "lib.so"))
        subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True, timeout=120)
        notes = ""
        for f in sorted(os.listdir(tmp)):
            if "gfx950" in f:
                notes += subprocess.run([readelf, "--notes", f], cwd=tmp, check=True, capture_output=True, text=True,
                                        timeout=120).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    metas = [m for m in re.split(r"\n  - \.", notes)[1:] if re.search(r"\.name:\s+_ZN4dqmc16ttp_chain_kernel", m)]
    assert len(metas) == 1, "ttp_chain_kernel metadata not found"
    meta = metas[0]
    get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0
    assert get("private_segment_fixed_size") == 0
    assert get("vgpr_count") <= 256  # two waves per SIMD
    assert 2 * get("group_segment_fixed_size") <= 160 * 1024
