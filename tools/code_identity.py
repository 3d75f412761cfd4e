#!/usr/bin/env python
"""Do two builds carry the same device code?  `python tools/code_identity.py <objdir_a> <objdir_b>`  (CPU only)

For every device code object (`*-gfx950.out`, what `-save-temps=obj` leaves in `humanoid-gym_amd/lib/obj`) of the two directories: the
bytes of `.text` and of `.rodata` (`llvm-objcopy -O binary --only-section=...`) compared, their sizes, and the number of kernels
(`llvm-readelf -s`, as build.py's kernel_sizes reads it).  One line per code object; for one that differs, the per-kernel code sizes of
both sides.  Bytes and sizes only -- nothing is disassembled.  Whole-file hashes do not serve: two builds of the same source differ in
the `__hip_cuid_<hash>` symbol, and renaming a kernel template moves the symbol table while the code stays what it was.

Exit status 1 if any section differs, a kernel count differs, or a code object exists on one side only.
"""
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
OBJCOPY = os.environ.get("LLVM_OBJCOPY", os.path.join(LLVM, "llvm-objcopy"))
READELF = os.environ.get("LLVM_READELF", os.path.join(LLVM, "llvm-readelf"))
SUFFIX = "-gfx950.out"
SECTIONS = (".text", ".rodata")


def section(path, name, tmp):
    out = os.path.join(tmp, "section.bin")
    if os.path.exists(out):
        os.remove(out)
    subprocess.check_call([OBJCOPY, "-O", "binary", "--only-section=" + name, path, out])
    with open(out, "rb") as f:
        return f.read()


def kernels(path):
    """[(symbol, bytes of code)] of the functions defined in a code object, in symbol-table order."""
    out = subprocess.run([READELF, "-s", "-W", path], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND":
            found.append((p[7], int(p[2])))
    return found


def main(dir_a, dir_b):
    objs = [{f for f in os.listdir(d) if f.endswith(SUFFIX)} for d in (dir_a, dir_b)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(objs[0] | objs[1]):
            name = f.split("-hip-amdgcn")[0]
            if f not in objs[0] or f not in objs[1]:
                print("%-24s ONLY IN %s" % (name, dir_a if f in objs[0] else dir_b))
                bad += 1
                continue
            pa, pb = os.path.join(dir_a, f), os.path.join(dir_b, f)
            cols, differs = [], False
            for s in SECTIONS:
                a, b = section(pa, s, tmp), section(pb, s, tmp)
                same = a == b
                differs |= not same
                cols.append("%s %s %s" % (s, "identical" if same else "DIFFERS", len(a) if same else "%d / %d" % (len(a), len(b))))
            ka, kb = kernels(pa), kernels(pb)
            differs |= len(ka) != len(kb)
            cols.append("kernels %s" % (len(ka) if len(ka) == len(kb) else "%d / %d DIFFERS" % (len(ka), len(kb))))
            print("%-24s %s" % (name, "   ".join(cols)))
            if differs:
                bad += 1
                for side, ks in ((dir_a, ka), (dir_b, kb)):
                    print("    %s" % side)
                    for sym, size in ks:
                        print("    %8d  %s" % (size, sym))
    print("%d code objects, %d differ" % (len(objs[0] | objs[1]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
