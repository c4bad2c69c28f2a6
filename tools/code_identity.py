#!/usr/bin/env python3
"""Are the kernels of two builds of libmoka_hip.so the same machine code?  (What a refactor of the launch rules has to show.)

    python tools/code_identity.py OLD.so NEW.so [--drop KERNEL:INDEX ...]

For every kernel of the gfx950 code objects: the bytes of its function and its 64-byte kernel descriptor (bytes 16..23, the code-entry
offset, masked: it moves with the layout) are hashed and compared by demangled name.  ``--drop moka_wgrad_kernel:1`` maps OLD names to NEW
ones by removing template argument 1 (from 0) of that kernel.  Prints the kernels only one side has and those that differ; exit status 1
if a kernel both sides have differs.  Hashes bytes and inspects nothing else.  Needs the ROCm LLVM object tools, no GPU."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def run(tool, *args, **kw):
    path = os.path.join(LLVM, tool)
    return subprocess.run([path if os.path.exists(path) else shutil.which(tool), *args], check=True, capture_output=True, text=True, **kw).stdout


def kernels(lib):
    """{demangled name without blanks and arguments: (sha256 of the code, sha256 of the masked descriptor, code bytes)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        run("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "discard"))
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, s in enumerate(starts):                    # one bundle per translation unit
            bundle, co = os.path.join(tmp, f"b{i}"), os.path.join(tmp, f"c{i}.co")
            with open(bundle, "wb") as f:
                f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
            elf = open(co, "rb").read()
            sections = {}                                 # index -> (address, file offset)
            for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", run("llvm-readelf", "-S", "--wide", co), re.M):
                sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
            code, kd = {}, {}
            for line in run("llvm-readelf", "-s", "--wide", co).splitlines():
                f = line.split()
                if len(f) < 8 or f[4] != "GLOBAL" or not f[6].isdigit():
                    continue
                addr, off = sections[int(f[6])]
                blob = elf[int(f[1], 16) - addr + off:][:int(f[2])]
                if f[3] == "FUNC":
                    code[f[7]] = blob
                elif f[3] == "OBJECT" and f[7].endswith(".kd"):
                    kd[f[7][:-3]] = blob[:16] + bytes(8) + blob[24:]
            names = sorted(code)
            dem = run("llvm-cxxfilt" if os.path.exists(os.path.join(LLVM, "llvm-cxxfilt")) else "c++filt", input="\n".join(names)).splitlines()
            for n, d in zip(names, dem):
                key = re.sub(r"^void ", "", d).split("(")[0].replace(" ", "")
                out[key] = (hashlib.sha256(code[n]).hexdigest(), hashlib.sha256(kd[n]).hexdigest(), len(code[n]))
    return out


def renamed(name, drops):
    m = re.match(r"(\w+)<(.*)>$", name)
    if not m or m.group(1) not in drops:
        return name
    args = m.group(2).split(",")
    return f"{m.group(1)}<{','.join(a for i, a in enumerate(args) if i not in drops[m.group(1)])}>"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop", action="append", default=[], metavar="KERNEL:INDEX")
    a = ap.parse_args()
    drops = {}
    for d in a.drop:
        k, _, i = d.partition(":")
        drops.setdefault(k, set()).add(int(i))
    old_raw, new = kernels(a.old), kernels(a.new)
    old = {renamed(k, drops): v for k, v in old_raw.items()}
    if len(old) != len(old_raw):
        sys.exit("--drop maps two kernels of OLD to one name: the dropped argument still has more than one value there")
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k][:2] != new[k][:2]]
    for side, only in (("old", sorted(set(old) - set(new))), ("new", sorted(set(new) - set(old)))):
        print(f"only in {side}: {len(only)} kernels, {sum((old if side == 'old' else new)[k][2] for k in only)} code bytes")
        for k in only:
            print("   ", k)
    print(f"kernel code bytes: old {sum(v[2] for v in old.values())} ({len(old)} kernels), new {sum(v[2] for v in new.values())} ({len(new)} kernels)")
    print(f"in both: {len(both)} kernels, {len(both) - len(differ)} with identical code and descriptor")
    for k in differ:
        print("    DIFFERS:", k, "(code)" if old[k][0] != new[k][0] else "(descriptor)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
