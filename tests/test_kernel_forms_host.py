"""The kernel-form table of the buffer-contract tests (tests/kernel_forms.py) lists exactly the kernel instances of the built
library: every instance is reached by a contract row, and no name is stale.  Reads the gfx950
code objects out of moka_amd/libmoka_hip.so with the ROCm LLVM tools (no GPU needed)."""
import os
import re
import shutil
import subprocess

import pytest

from tests.kernel_forms import PRODUCT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def _instances(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "discard")], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    names = set()
    for i, s in enumerate(starts):                        # one bundle per translation unit
        bundle, co = os.path.join(tmp, f"b{i}"), os.path.join(tmp, f"c{i}.co")
        with open(bundle, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        out = subprocess.run([_tool("llvm-readelf"), "-s", "--wide", co], check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL":
                names.add(f[7])
    dem = subprocess.run([_tool("llvm-cxxfilt") or _tool("c++filt")], input="\n".join(sorted(names)), check=True,
                         capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"^void ", "", d).split("(")[0].replace(" ", "") for d in dem if d.strip()}


def test_every_kernel_instance_of_the_library_is_sorted(tmp_path):
    lib = os.path.join(ROOT, "moka_amd", "libmoka_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    tools = ["llvm-objcopy", "clang-offload-bundler", "llvm-readelf"]
    if not all(_tool(t) for t in tools) or not (_tool("llvm-cxxfilt") or _tool("c++filt")):
        pytest.skip("the ROCm LLVM object tools are not installed")
    inst = _instances(lib, str(tmp_path))
    assert len(inst) > 50
    unsorted = inst - PRODUCT
    assert not unsorted, f"kernel instances that no contract row reaches (tests/kernel_forms.py does not list them): {sorted(unsorted)}"
    stale = PRODUCT - inst
    assert not stale, f"names in tests/kernel_forms.py that the library no longer has: {sorted(stale)}"
