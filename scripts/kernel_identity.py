#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of one .hip file, kernel by kernel.

  python scripts/kernel_identity.py PARENT.o BRANCH.o [NAME.hip] > table

The gfx950 code object is taken out of each object file's .hip_fatbin section (llvm-objcopy --dump-section,
clang-offload-bundler --unbundle) and the .text bytes of every kernel symbol (a FUNC symbol with a .kd descriptor) are
compared, matched by demangled name. A kernel only one side has is listed as "new" / "gone"."""
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj: str, work: str) -> dict:
    """demangled kernel name -> its .text bytes"""
    fat, co, text = (os.path.join(work, n) for n in ("fatbin", "gfx950.co", "text.bin"))
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(work, "rest.o"))
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, text)
    blob = open(text, "rb").read()
    base = None
    for line in run(f"{LLVM}/llvm-readelf", "-SW", co).splitlines():
        parts = line.replace("[", " ").replace("]", " ").split()
        if len(parts) > 4 and parts[1] == ".text":
            base = int(parts[3], 16)
    funcs, descriptors = {}, set()
    for line in run(f"{LLVM}/llvm-readelf", "-sW", co).splitlines():
        p = line.split()
        if len(p) < 8 or not p[0].rstrip(":").isdigit():
            continue
        value, size, kind, name = int(p[1], 16), int(p[2]), p[3], p[7]
        if name.endswith(".kd"):
            descriptors.add(name[:-3])
        elif kind == "FUNC":
            funcs[name] = (value, size)
    out = {}
    names = sorted(n for n in funcs if n in descriptors)
    # (binutils' c++filt does not know DF16_, _Float16: demangled as Dh, another builtin type, and so printed as __fp16)
    demangled = run("c++filt", *[n.replace("DF16_", "Dh") for n in names]).splitlines() if names else []
    for name, plain in zip(names, demangled):
        value, size = funcs[name]
        out[plain.split("(")[0].replace("void ", "")] = blob[value - base:value - base + size]
    return out


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    label = sys.argv[3] if len(sys.argv) > 3 else os.path.basename(branch)
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        ka, kb = kernels(parent, a), kernels(branch, b)
    print(f"{'file':<14} {'kernel':<100} {'bytes parent':>12} {'bytes branch':>12}  result")
    differ = 0
    for name in sorted(set(ka) | set(kb)):
        if name not in ka:
            result = "new"
        elif name not in kb:
            result = "gone"
        else:
            result = "equal" if ka[name] == kb[name] else "DIFFERENT"
        differ += result in ("gone", "DIFFERENT")
        print(f"{label:<14} {name:<100} {len(ka.get(name, b'')) or '-':>12} {len(kb.get(name, b'')) or '-':>12}  {result}")
    print(f"\n{len(ka)} kernels in the parent, {len(kb)} in the branch, {sum(n not in ka for n in kb)} new, {differ} gone or different")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
