"""The checkpoint blob of the classical MC flavor (csrc/mc_blob.cpp), no GPU: the plain C++ blob code under the host
sanitizers, as tests/test_checkpoint_blob.py does for the DQMC blob."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")


def test_mc_blob_code_under_address_and_undefined_sanitizers(tmp_path):
    """mc_blob.cpp + state_blob.cpp with tests/mc_blob_check.cpp (its own main), g++ -fsanitize=address,undefined, run as a
    child process on the CPU: an Ising and a q-state shape with every section on and off round-trip through layout, write
    and validate; every refusal of validate's list, every cut at a record boundary and one byte short, flipped header,
    payload and checksum bytes, each configuration field changed in turn (named), and every state value out of range are
    refused; neither sanitizer reports anything (a report aborts the program).  The sanitizer runtimes are linked into the
    program, which runs in the environment the test inherits"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the blob code"
    exe = str(tmp_path / "mc_blob_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "mc_blob_check.cpp"), os.path.join(CSRC, "mc_blob.cpp"),
                    os.path.join(CSRC, "state_blob.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
    for shape in ("ising all on", "ising all off", "qstate all on", "qstate all off"):
        m = re.search(r"^%s: (\d+) records, (\d+) bytes, (\d+) flipped bytes refused of (\d+), (\d+) fields named$" % shape,
                      out.stdout, flags=re.M)
        assert m, out.stdout[-2000:]
        assert m.group(3) == m.group(4) and int(m.group(4)) > 500 and int(m.group(5)) >= 30
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_mc_blob_code_has_no_hip_in_it():
    for f in ("mc_blob.h", "mc_blob.cpp", "state_blob.h", "state_blob.cpp"):
        txt = open(os.path.join(CSRC, f)).read()
        assert "hip" not in re.sub(r"//.*", "", txt).lower(), f
        assert not re.search(r"#\s*include\s*[<\"][^>\"]*hip", txt), f


def test_mc_blob_reuses_the_dqmc_hash():
    """one FNV-1a 64 in the tree: mc_blob.cpp calls dqmc_blob::fnv1a64 and defines no hash loop of its own"""
    txt = open(os.path.join(CSRC, "mc_blob.cpp")).read()
    assert "dqmc_blob::fnv1a64" in txt
    assert "0x100000001b3" not in txt.lower() and "1099511628211" not in txt  # the FNV prime
