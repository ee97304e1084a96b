#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel:  compare_device_code.py LIBDIR_A LIBDIR_B NAME.hip [NAME.hip ...]

For every NAME.hip.o of both directories the device code object is taken out of the host object (.hip_fatbin section ->
clang-offload-bundler), and for every kernel symbol (and its descriptor NAME.kd) the bytes are compared.  Per symbol, not per
file: the order of the instantiations inside an object follows the host code that names them.  One line per file; exit
status 1 if any file differs."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"))),
                    "llvm", "bin")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def kernels(obj, tmp):
    """{symbol: bytes} for the functions and kernel descriptors of the gfx950 code object inside a host object"""
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "copy.o"))
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb, "--output=" + co,
         "--targets=hipv4-amdgcn-amd-amdhsa--gfx950")
    data = open(co, "rb").read()
    sections = {}   # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", tool("llvm-readelf", "-SW", co), flags=re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in tool("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit() and (f[3] == "FUNC" or f[7].endswith(".kd")):
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            out[f[7]] = data[start:start + int(f[2])]
            if f[3] == "OBJECT":  # bytes 16 .. 23 of a descriptor: the distance to the kernel's code, which moves with the order
                out[f[7]] = out[f[7]][:16] + out[f[7]][24:]
    return out


def main(a, b, names):
    bad = 0
    for name in names:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ka, kb = kernels(os.path.join(a, name + ".o"), ta), kernels(os.path.join(b, name + ".o"), tb)
        n = sum(1 for k in ka if not k.endswith(".kd"))
        diff = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
        bad += bool(diff)
        print(f"{name}: {n} kernels, " + ("identical" if not diff else "DIFFERENT: " + ", ".join(diff[:8])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
