"""The factored hopping forms' host code (csrc/hopping_forms.h: the form table, kron_split, build_hop_image and the two
host-factor gates) without a GPU: tests/hopping_forms_check.cpp under the host sanitizers, and the device images it builds
against the hashes recorded from the code the header replaced."""
import json
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlo.jl_amd", "csrc")


def test_hopping_forms_under_address_and_undefined_sanitizers(tmp_path):
    """g++ -fsanitize=address,undefined, run as a child process on the CPU (the sanitizer runtimes are linked into the
    program).  Every gate form takes Kronecker products of its own shape (nb = 1, 2; non-symmetric factors that differ per
    block and matrix) and builds the image the four creation blocks of engine.cpp built before the table (FNV-1a 64 of its
    bytes: tests/golden/hopping_forms.json, recorded from those functions on the same inputs); it rejects one entry off by
    1e-12, E[0] <= 0 or NaN, an Inf and the products of another shape, and takes a one-ulp change.  The host-factor forms take
    commuting circulant factors, build the setters' image, and reject a transposed factor.  -ffp-contract=off: the inputs
    are the same bits on a target whose compiler would otherwise fuse the generator's multiply-adds."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host code"
    exe = str(tmp_path / "hopping_forms_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "hopping_forms_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok") and "FAILED" not in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    got = dict(re.findall(r"^hash (\S+) ([0-9a-f]{16})$", out.stdout, re.M))
    with open(os.path.join(ROOT, "tests", "golden", "hopping_forms.json")) as f:
        want = json.load(f)
    assert len(want) == 10 and got == want


def test_hopping_forms_header_has_no_hip_in_it():
    txt = open(os.path.join(CSRC, "hopping_forms.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()
