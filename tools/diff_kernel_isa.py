"""Instruction-for-instruction comparison of the gfx950 code two versions of one HIP source file build: each file is
compiled device-only with the library's flags, its code object disassembled, and every function of the two listed as
SAME / DIFFERENT / NEW / GONE (instruction text without addresses; branch targets are relative, so code that merely
moved compares equal).  Needs no GPU.  Used to show that a change left existing kernels as they were:

    git show HEAD:montecarlo.jl_amd/csrc/ising.hip > /tmp/parent/ising.hip    (next to a copy of kernels.h, and of
                                                                                include/ two levels up)
    python tools/diff_kernel_isa.py /tmp/parent/ising.hip montecarlo.jl_amd/csrc/ising.hip [--diff NAME_FRAGMENT]

Exit status 1 if a function present in both differs."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output"]


def functions(src, extra):
    """{mangled name: [instruction text]} of the code object `src` compiles to"""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "dev.hsaco")
        subprocess.run([os.environ.get("HIPCC", "hipcc")] + FLAGS + extra + ["-c", src, "-o", obj], check=True)
        out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True, capture_output=True,
                             text=True).stdout
    funcs, cur = {}, None
    for line in out.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.startswith("\t") and line.strip() != "...":  # ("...": padding between functions)
            funcs[cur].append(line.split("//")[0].strip())
    for code in funcs.values():  # the s_nop fill behind a function's last instruction depends on what follows it
        while code and code[-1] == "s_nop 0":
            code.pop()
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--flag", action="append", default=[], help="extra compiler flag for both (repeatable)")
    ap.add_argument("--diff", default=None, help="print the instruction diff of functions whose name contains this")
    args = ap.parse_args()
    a, b = functions(args.old, args.flag), functions(args.new, args.flag)
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    changed = 0
    for n, d in zip(names, dem):
        d = d.split("(")[0]
        if n not in a:
            print("NEW       %5d  %s" % (len(b[n]), d))
        elif n not in b:
            print("GONE      %5d  %s" % (len(a[n]), d))
        else:
            same = a[n] == b[n]
            changed += not same
            print("%s %5d  %s" % ("SAME     " if same else "DIFFERENT", len(b[n]), d))
            if not same and args.diff and args.diff in d:
                print("\n".join(difflib.unified_diff(a[n], b[n], lineterm="", n=1)))
    sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
