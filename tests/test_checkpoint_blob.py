"""Checkpoint and resume, the parts that need no GPU: the file container of DQMC.save / DQMC.load (checkpoint.py), the
plain C++ blob code (csrc/state_blob.cpp) under the host sanitizers, and the three ABI symbols."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")


@pytest.fixture(scope="module")
def ckpt(mc_amd):
    from montecarlo_jl_amd import checkpoint
    return checkpoint


PREAMBLE = {"format": 1, "last_sweep": 4, "model": {"class": "HubbardModelAttractive", "U": 1.0, "mu": 0.1 + 0.2}}


# ---- the file container
def test_preamble_and_blob_split_and_rejoin(ckpt, tmp_path):
    blob = np.random.Generator(np.random.Philox(key=1)).integers(0, 256, size=1000, dtype=np.uint8)
    data = b"".join(bytes(p) for p in ckpt.join(PREAMBLE, blob))
    pre, back = ckpt.split(data)
    assert pre == PREAMBLE and pre["model"]["mu"] == 0.1 + 0.2  # doubles survive the JSON
    assert back.dtype == np.uint8 and np.array_equal(back, blob)
    p = tmp_path / "run.ckpt"
    ckpt.write(p, PREAMBLE, blob)
    assert p.read_bytes() == data
    pre, back = ckpt.read(p)
    assert pre == PREAMBLE and np.array_equal(back, blob)
    assert os.listdir(tmp_path) == ["run.ckpt"]  # no temporary stays


def test_integer_tables_survive_the_preamble(ckpt):
    import json
    tab = np.asfortranarray(np.arange(-1, 23, dtype=np.int32).reshape(4, 6))
    back = ckpt.unpack_table(json.loads(json.dumps(ckpt.pack_table(tab))))
    assert back.dtype == np.int32 and back.shape == (4, 6) and np.array_equal(back, tab)


def test_incomplete_files_are_refused(ckpt):
    blob = np.arange(64, dtype=np.uint8)
    parts = [bytes(p) for p in ckpt.join(PREAMBLE, blob)]
    whole = b"".join(parts)
    head = ckpt._HEAD
    n_text = len(parts[1])
    cases = {
        "a bare blob": bytes(blob),
        "a bare preamble": parts[1],
        "the preamble without a blob": head.pack(ckpt.MAGIC, ckpt.VERSION, n_text, 0) + parts[1],
        "the blob without a preamble": head.pack(ckpt.MAGIC, ckpt.VERSION, 0, blob.size) + bytes(blob),
        "one byte short": whole[:-1],
        "one byte long": whole + b"\0",
        "the head alone": parts[0],
        "nothing": b"",
        "another magic": b"X" + whole[1:],
        "another version": head.pack(ckpt.MAGIC, ckpt.VERSION + 1, n_text, blob.size) + parts[1] + bytes(blob),
        "a preamble that is no JSON": head.pack(ckpt.MAGIC, ckpt.VERSION, 4, blob.size) + b"{{{{" + bytes(blob),
        "a preamble that is no object": head.pack(ckpt.MAGIC, ckpt.VERSION, 2, blob.size) + b"[]" + bytes(blob),
    }
    for name, data in cases.items():
        with pytest.raises(ckpt.CheckpointError):
            ckpt.split(data)
            pytest.fail("accepted: " + name)
    for bad in (({}, blob), (PREAMBLE, np.zeros(0, dtype=np.uint8))):
        with pytest.raises(ckpt.CheckpointError):
            ckpt.join(*bad)


def test_atomic_write_keeps_the_old_file_when_the_write_raises(ckpt, tmp_path):
    p = tmp_path / "run.ckpt"
    ckpt.write(p, PREAMBLE, np.arange(10, dtype=np.uint8))
    old = p.read_bytes()

    def parts():
        yield b"half of a new file"
        raise OSError("disk full")
    with pytest.raises(OSError, match="disk full"):
        ckpt.write_atomic(p, parts())
    assert p.read_bytes() == old
    assert os.listdir(tmp_path) == ["run.ckpt"]
    # and a first write that fails leaves nothing
    q = tmp_path / "other.ckpt"
    with pytest.raises(OSError):
        ckpt.write_atomic(q, parts())
    assert sorted(os.listdir(tmp_path)) == ["run.ckpt"]


# ---- the plain C++ blob code under the host sanitizers
def test_blob_code_under_address_and_undefined_sanitizers(tmp_path):
    """state_blob.cpp with tests/checkpoint_blob_check.cpp (its own main), g++ -fsanitize=address,undefined, run as a child
    process on the CPU: a valid header validates, every truncation, a trailing byte and 400 single-byte corruptions from a
    fixed seed are refused, and neither sanitizer reports anything (a report aborts the program).  The sanitizer runtimes
    are linked into the program, which runs in the environment the test inherits"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the blob code"
    exe = str(tmp_path / "blob_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "checkpoint_blob_check.cpp"),
                    os.path.join(CSRC, "state_blob.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and "400 corruptions refused of 400" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_blob_code_has_no_hip_in_it():
    for f in ("state_blob.h", "state_blob.cpp"):
        txt = open(os.path.join(CSRC, f)).read()
        assert "hip" not in re.sub(r"//.*", "", txt).lower(), f


# ---- the ABI surface
def test_state_symbols_and_signatures(mc_amd):
    from montecarlo_jl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (dqmc_state_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert decl == {"dqmc_state_size": "dqmc_handle *h, size_t *n_bytes",
                    "dqmc_state_export": "dqmc_handle *h, void *host_out, size_t n_bytes",
                    "dqmc_state_import": "dqmc_handle *h, const void *host_in, size_t n_bytes"}
    L = C.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(L, name)
    S = _lib.SIGNATURES
    assert S["dqmc_state_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)])
    assert S["dqmc_state_export"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])
    assert S["dqmc_state_import"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])


def test_null_handle_is_invalid(mc_amd):
    from montecarlo_jl_amd import _lib
    lib = _lib.lib()
    n = C.c_size_t(7)
    buf = np.zeros(16, dtype=np.uint8)
    assert lib.dqmc_state_size(None, C.byref(n)) == _lib.ERR_INVALID and n.value == 7
    assert lib.dqmc_state_export(None, buf.ctypes.data, buf.size) == _lib.ERR_INVALID
    assert lib.dqmc_state_import(None, buf.ctypes.data, buf.size) == _lib.ERR_INVALID
    assert not buf.any()


def test_dqmc_object_has_the_entry_points(mc_amd):
    for name in ("state", "set_state", "save", "load", "state_size"):
        assert callable(getattr(mc_amd.DQMC, name))
    import inspect
    sig = inspect.signature(mc_amd.DQMC.run)
    assert "checkpoint" in sig.parameters and "checkpoint_every" in sig.parameters
    assert list(inspect.signature(mc_amd.DQMC.load).parameters) == ["path", "device_id"]
