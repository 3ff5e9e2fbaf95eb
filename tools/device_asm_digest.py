"""Digest of the gfx950 device code of the HIP translation units -- the gate of a refactor that claims "the device code is the same":
run it at the parent commit and at the branch, and every touched unit must show the same digest and the same numbers twice.  No GPU.

    python tools/device_asm_digest.py [--root DIR] [--jobs N] [--keep DIR] [unit.hip ...]

For each .hip unit of the Makefile's HIP_UNITS (or those named), in that order: compile the device side to assembly with the Makefile's
HIPFLAGS (hipcc $(HIPFLAGS) -x hip --cuda-device-only -S) into a temporary directory, drop the lines that carry the per-translation-unit
__hip_cuid_ symbol (a hash of the file, which changes with every edit), and print the unit's name and the SHA-256 of the rest, then per
kernel of the metadata block its .vgpr_count, .sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size.  It hashes text and
reads metadata numbers; it does not look at the instruction stream.  --root names another checkout of the repository (the parent commit
exported to a directory): the compile runs inside its hisparse_amd/csrc with a relative file name, so the text does not depend on where
the checkout lies."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def make_var(root, name):
    """the value of a Makefile variable, expanded by make itself"""
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", root, "--eval", "print-%: ; @echo $($*)", f"print-{name}"], check=True,
                         capture_output=True, text=True).stdout
    return out.split()


def kernels_of(text):
    """[(name, {field: value})] from the amdhsa.kernels list of the assembly's metadata block, in the order of the block"""
    block = text.split(".amdgpu_metadata", 1)[1].split(".end_amdgpu_metadata", 1)[0] if ".amdgpu_metadata" in text else ""
    found, cur = [], None
    for line in block.splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)      # a kernel's own keys: its arguments' keys are indented further
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
            found.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'\"")
    return [(k.get("name", "?"), {f: k.get(f, "0") for f in FIELDS}) for k in found]


def digest(root, hipcc, flags, unit, tmp):
    csrc = os.path.join(root, "hisparse_amd", "csrc")
    out = os.path.join(tmp, unit + ".s")
    run = subprocess.run([hipcc, *flags, "-x", "hip", "--cuda-device-only", "-S", "-o", out, unit], cwd=csrc, capture_output=True, text=True)
    if run.returncode != 0:
        return unit, None, run.stderr
    with open(out) as f:
        text = "".join(line for line in f if "__hip_cuid_" not in line)
    with open(out, "w") as f:      # what --keep leaves: the hashed text, ready for diff
        f.write(text)
    return unit, hashlib.sha256(text.encode()).hexdigest(), kernels_of(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=ROOT, help="the checkout to digest (default: the one this file lies in)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", metavar="DIR", help="leave each unit's hashed text there as <unit>.s, for a diff when two digests differ")
    ap.add_argument("units", nargs="*", help="file names under hisparse_amd/csrc (default: every .hip unit of HIP_UNITS)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    hipcc = make_var(root, "HIPCC")[0]
    flags = make_var(root, "HIPFLAGS")
    units = args.units or [u for u in make_var(root, "HIP_UNITS") if u.endswith(".hip")]
    failed = False
    with tempfile.TemporaryDirectory() as scratch, ThreadPoolExecutor(max(1, args.jobs)) as pool:
        tmp = scratch
        if args.keep:
            tmp = os.path.abspath(args.keep)
            os.makedirs(tmp, exist_ok=True)
        for unit, sha, kernels in pool.map(lambda u: digest(root, hipcc, flags, u, tmp), units):
            if sha is None:
                failed = True
                print(f"{unit}  DID NOT COMPILE\n{kernels}")
                continue
            print(f"{unit}  sha256 {sha}")
            for name, k in kernels:
                print(f"    {name}  vgpr {k['vgpr_count']}  sgpr {k['sgpr_count']}  lds {k['group_segment_fixed_size']}  private {k['private_segment_fixed_size']}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
