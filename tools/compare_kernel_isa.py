#!/usr/bin/env python3
"""Do the kernels of a set of files compile to what they compiled to at another revision?

    python tools/compare_kernel_isa.py <git revision> [file.hip ...]
    python tools/compare_kernel_isa.py <git revision> --old lanes.hip --new decode_lanes.hip encode_lanes.hip

The files of the old side are compiled as they were at the revision, those of the new side as they are in the working tree
(device side only, for gfx950, the Makefile's flags), and the kernels of each side are pooled: a kernel may have moved from
one file to another.  Kernels are paired by their exact mangled name; of every pair the opcode sequence, next_free_vgpr,
private_segment_fixed_size (scratch) and group_segment_fixed_size (static LDS) are compared, and kernels that only one side
has are reported.  Prints one table row per kernel and a summary; exit status 1 unless every kernel is on both sides and
equal.  Without --old / --new both sides take the files named (default: decode_wave.hip encode_wave.hip).  No GPU needed.

--new-default-false: the kernel templates of the tree gained a trailing `bool = false` template argument since the revision
(a RAGGED form, say).  A kernel of the tree whose last template argument is `false` is then paired under the name it had
without that argument; the instantiations with `true` stay what they are, kernels only the tree has.

--kernels REGEX: compare the kernels whose names contain REGEX instead of the coders (k_compact, say, with
container_kernels.hip).

--ranges: behind the table, for every kernel whose opcode sequence DIFFERS, the index ranges of the opcodes that differ
(old range -> new range, indices into the kernel's opcode list as counted in the `instructions` column)."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "ryg_rans_amd/csrc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
FIELDS = ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")


KERNELS = r"k_(?:de|en)code"  # --kernels: which kernels are compared, a regex that their names contain


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_Z\w*(?:%s)\w*):[^\n]*\n(.*?)\n\.Lfunc_end" % KERNELS, asm, re.S | re.M):
        ops = [ln.split()[0] for ln in m.group(2).split("\n")
               if ln.strip() and not ln.strip().startswith((";", ".")) and not ln.strip().endswith(":")]
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
        res = tuple(re.search(r"\.amdhsa_%s\s+(\S+)" % f, meta).group(1) for f in FIELDS)
        out[m.group(1)] = (ops, res)
    return out


def compile_asm(job):
    srcdir, fn, out = job
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [fn, "-o", out], cwd=srcdir, check=True, stderr=subprocess.DEVNULL)
    return kernels(open(out).read())


def main():
    global KERNELS
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", help="git revision of the old side")
    ap.add_argument("files", nargs="*", help="files of both sides (in %s)" % CSRC)
    ap.add_argument("--old", nargs="+", help="files of the old side, at the revision")
    ap.add_argument("--new", nargs="+", help="files of the new side, in the working tree")
    ap.add_argument("--new-default-false", action="store_true",
                    help="pair a kernel of the tree whose last template argument is `false` with the old kernel without that argument")
    ap.add_argument("--ranges", action="store_true", help="print the index ranges of the differing opcodes of every DIFFERS row")
    ap.add_argument("--kernels", default=KERNELS, help="regex the compared kernels' names contain (default: %(default)s)")
    args = ap.parse_args()
    KERNELS = args.kernels
    both = args.files or ["decode_wave.hip", "encode_wave.hip"]
    old_files, new_files = args.old or both, args.new or both
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, CSRC)
        os.makedirs(old)
        os.makedirs(os.path.join(tmp, "include"))
        listed = subprocess.run(["git", "ls-tree", "--name-only", args.rev, CSRC + "/", "include/ryg_rans_amd.h"], cwd=ROOT,
                                check=True, capture_output=True, text=True).stdout.split()
        for path in listed:
            blob = subprocess.run(["git", "show", "%s:%s" % (args.rev, path)], cwd=ROOT, check=True, capture_output=True).stdout
            open(os.path.join(tmp, path), "wb").write(blob)
        jobs = [(old, fn, os.path.join(tmp, "old_%d.s" % i)) for i, fn in enumerate(old_files)] + \
               [(os.path.join(ROOT, CSRC), fn, os.path.join(tmp, "new_%d.s" % i)) for i, fn in enumerate(new_files)]
        with ThreadPoolExecutor(max_workers=4) as pool:
            found = list(pool.map(compile_asm, jobs))
    a, b, where = {}, {}, {}
    for ks in found[:len(old_files)]:
        a.update(ks)
    for fn, ks in zip(new_files, found[len(old_files):]):
        if args.new_default_false:  # (Itanium mangling: I<args>Lb0EE..Ev -- drop the Lb0E in front of the closing E's and the return type)
            ks = {re.sub(r"Lb0E(E+v)", r"\1", k, count=1): v for k, v in ks.items()}
        b.update(ks)
        where.update((k, fn) for k in ks)
    rev = subprocess.run(["git", "rev-parse", "--short", args.rev], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    print("old: %s at %s; new: %s in the tree\n" % (" ".join(old_files), rev, " ".join(new_files)))
    print("| kernel | now in | instructions | %s | verdict |" % " | ".join(FIELDS))
    print("|---|---|---|---|---|---|---|")
    same, differing = 0, []
    for k in sorted(set(a) | set(b)):
        if k not in b:
            verdict = "ONLY AT THE REVISION"
        elif k not in a:
            verdict = "ONLY IN THE TREE"
        elif a[k] != b[k]:
            verdict = "DIFFERS (%d instructions, %s at the revision)" % (len(a[k][0]), " / ".join(a[k][1]))
            differing.append(k)
        else:
            verdict = "same"
            same += 1
        ops, res = b.get(k) or a[k]
        print("| `%s` | %s | %d | %s | %s |" % (k, where.get(k, "-"), len(ops), " | ".join(res), verdict))
    for k in differing if args.ranges else []:
        ops = difflib.SequenceMatcher(None, a[k][0], b[k][0], autojunk=False).get_opcodes()
        print("\n`%s`: %s" % (k, ", ".join("%s [%d, %d) -> [%d, %d)" % op for op in ops if op[0] != "equal") or "the opcodes are equal"))
    print("\n%d kernels at the revision, %d in the tree, %d on both sides with the same opcode sequence, VGPR count, scratch "
          "size and static LDS size" % (len(a), len(b), same))
    sys.exit(0 if same == len(a) == len(b) else 1)


if __name__ == "__main__":
    main()
