#!/usr/bin/env python3
"""One sha256 per translation unit of the gfx950 DEVICE code inside totsu_amd/csrc/*.o.

A host-only change leaves every digest as it was; a digest that moves means a kernel changed.  To compare two commits, build
both from the same directory path and diff the two outputs.  (If only the ORDER in which kernels are emitted changed, compare
the sorted per-symbol `llvm-objdump -d` of the code objects instead.)

    python tools/device_code_digest.py [--objs DIR] [--keep DIR]
"""
import argparse
import glob
import hashlib
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, outdir):
    stem = os.path.join(outdir, os.path.basename(obj)[:-2])
    dump = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + stem + ".fatbin", obj],
                          stderr=subprocess.PIPE, text=True)
    if dump.returncode != 0:
        if "not found" in dump.stderr:
            return None                 # a host-only translation unit
        raise RuntimeError(dump.stderr)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + stem + ".fatbin",
                           "--targets=" + TARGET, "--output=" + stem + ".co"])
    os.remove(stem + ".fatbin")
    return stem + ".co"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--objs", metavar="DIR", default=os.path.join(ROOT, "totsu_amd", "csrc"), help="where the *.o files are")
    ap.add_argument("--keep", metavar="DIR", help="keep the extracted X.co code objects here")
    args = ap.parse_args()
    outdir = args.keep or tempfile.mkdtemp(prefix="devcode_")
    os.makedirs(outdir, exist_ok=True)
    try:
        for obj in sorted(glob.glob(os.path.join(args.objs, "*.o"))):
            co = code_object(obj, outdir)
            if co is None:
                print("%-64s %s" % ("(no device code)", os.path.basename(obj)))
                continue
            with open(co, "rb") as f:
                print(hashlib.sha256(f.read()).hexdigest(), os.path.basename(obj))
    finally:
        if not args.keep:
            shutil.rmtree(outdir, ignore_errors=True)


if __name__ == "__main__":
    main()
