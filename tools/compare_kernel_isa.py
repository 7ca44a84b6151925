#!/usr/bin/env python3
"""Do the uniform kernels of decode_wave.hip / encode_wave.hip compile to what they compiled to at another revision?

    python tools/compare_kernel_isa.py <git revision> [file.hip ...]

Both versions of every file are compiled for gfx950 to assembly (device side only, the Makefile's flags); every kernel of
the old revision is paired with the kernel of the same name in the working tree -- a trailing `false` template argument
that the tree added (RAGGED) is ignored, k_decode_word64_t<false> is k_decode_word64 -- and their opcode sequences, VGPR
counts and scratch sizes are compared.  Prints one line per file and the kernels that differ; exit status 1 if any does.
The revision must be one from before the RAGGED template parameter existed (norm() below maps the tree's mangled names
back to the old ones by dropping that argument).  No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "ryg_rans_amd/csrc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_Z\w*k_(?:de|en)code\w*):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.S | re.M):
        ops = [ln.split()[0] for ln in m.group(2).split("\n")
               if ln.strip() and not ln.strip().startswith((";", ".")) and not ln.strip().endswith(":")]
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        res = tuple(re.findall(r"\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\S+)", meta))
        out[m.group(1)] = (ops, res)
    return out


def norm(name):
    return name.replace("17k_decode_word64_tILb0EEEv", "15k_decode_word64E").replace("Lb0E", "")


def compile_asm(srcdir, fn, out):
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [fn, "-o", out], cwd=srcdir, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def main():
    rev = sys.argv[1]
    files = sys.argv[2:] or ["decode_wave.hip", "encode_wave.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, CSRC)
        os.makedirs(old)
        os.makedirs(os.path.join(tmp, "include"))
        listed = subprocess.run(["git", "ls-tree", "--name-only", rev, CSRC + "/", "include/ryg_rans_amd.h"], cwd=ROOT, check=True,
                                capture_output=True, text=True).stdout.split()
        for path in listed:
            blob = subprocess.run(["git", "show", "%s:%s" % (rev, path)], cwd=ROOT, check=True, capture_output=True).stdout
            open(os.path.join(tmp, path), "wb").write(blob)
        for fn in files:
            a = kernels(compile_asm(old, fn, os.path.join(tmp, "old.s")))
            b = {norm(k): v for k, v in kernels(compile_asm(os.path.join(ROOT, CSRC), fn, os.path.join(tmp, "new.s"))).items()
                 if "Lb1E" not in k}
            differ = [k for k in a if b.get(k) != a[k]]
            print("%s: %d kernels at %s, %d with the same opcode sequence, VGPR count and scratch size in the tree"
                  % (fn, len(a), rev, len(a) - len(differ)))
            for k in differ:
                print("   differs or missing:", k)
            bad += len(differ)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
