#!/usr/bin/env python3
"""One line per device symbol of the library's object files: digest of its instruction text, instruction count, symbol.

    python tools/kernel_isa.py [OBJECT_OR_DIR ...] > listing.txt        (default: 0g-halo2_amd/csrc)
    python tools/kernel_isa.py --diff parent.txt branch.txt             (compared by symbol; exit 1 on any difference)

For every *.o the gfx950 code object is extracted (llvm-objdump --offloading) and disassembled without addresses and
encodings; branch targets print as relative offsets, so a kernel that moved to another file or another place in its
file keeps its digest, and a kernel whose instructions changed does not.  A change of the host code around the
kernels leaves the listing as it was: that is what the comparison is for (tools/isa_blocks.py, the neighbour, reads
the instruction mix of one kernel's blocks)."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def objdump():
    for c in (os.environ.get("LLVM_OBJDUMP"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm/bin/llvm-objdump"),
              shutil.which("llvm-objdump")):
        if c and os.path.exists(c):
            return c
    sys.exit("kernel_isa: no llvm-objdump (set LLVM_OBJDUMP or ROCM_PATH)")


def symbols(obj, tool):
    """(digest, instruction count, symbol) of every device symbol in the gfx950 code object(s) of `obj`"""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([tool, "--offloading", os.path.basename(local)], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for co in sorted(glob.glob(local + ".*gfx950*")):
            text = subprocess.run([tool, "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                                  text=True).stdout
            name, body = None, []
            for ln in text.split("\n") + ["<end>:"]:
                m = re.match(r"^<(.+)>:$", ln)
                if m:
                    if name is not None:
                        out.append((hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body), name))
                    name, body = m.group(1), []
                elif name is not None and ln.startswith("\t") and ln.strip() != "...":  # ("...": zero padding up to the next symbol)
                    body.append(re.sub(r"\s*//.*$", "", ln).strip())
    return out


def listing(paths):
    tool = objdump()
    objs = []
    for p in paths:
        objs += sorted(glob.glob(os.path.join(p, "*.o"))) if os.path.isdir(p) else [p]
    if not objs:
        sys.exit("kernel_isa: no object files (build the library first)")
    for obj in objs:
        stem = os.path.splitext(os.path.basename(obj))[0]
        for digest, count, name in symbols(obj, tool):
            print(f"{digest} {count:7d} {stem:12s} {name}")


def read(path):
    table = {}
    for ln in open(path):
        f = ln.split(None, 3)
        if len(f) == 4:
            table[f[3].strip()] = (f[0], int(f[1]), f[2])
    return table


def diff(a_path, b_path):
    a, b = read(a_path), read(b_path)
    bad = 0
    for s in sorted(set(a) | set(b)):
        if s not in b:
            print(f"missing  {s} (was in {a[s][2]})")
        elif s not in a:
            print(f"added    {s} (in {b[s][2]})")
        elif a[s][:2] != b[s][:2]:
            print(f"changed  {s}: {a[s][0]} {a[s][1]} ({a[s][2]}) -> {b[s][0]} {b[s][1]} ({b[s][2]})")
        else:
            continue
        bad += 1
    moved = sum(1 for s in a if s in b and a[s][2] != b[s][2])
    print(f"{len(a)} / {len(b)} device symbols, {moved} in another file, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    listing(sys.argv[1:] or [os.path.join(ROOT, "0g-halo2_amd", "csrc")])
