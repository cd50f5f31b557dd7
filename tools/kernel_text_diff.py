#!/usr/bin/env python3
"""Are the GPU kernels of two builds of the library the same machine code?

    python tools/kernel_text_diff.py OLD.so NEW.so

Unbundles both libraries (llvm-objdump --offloading), pairs their gfx950 code
objects by the kernels they define, and compares for each pair the raw bytes of
the .text section and for each kernel the resource figures of its
amdhsa.kernels metadata.  One line per kernel; exit status 1 on any difference.
Whole code objects are not compared: the order of read-only data and the
per-unit ID symbol differ between builds of the same source.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
          "sgpr_spill_count", "vgpr_spill_count", "kernarg_segment_size")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    """{kernel names of a code object: (its .text bytes, {kernel: {field: value}})}"""
    d = tempfile.mkdtemp(dir=tmp)
    shutil.copy(lib, os.path.join(d, "lib.so"))
    run("llvm-objdump", "--offloading", "lib.so", cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "amdgcn" not in f or not f.endswith("gfx950"):
            continue
        path = os.path.join(d, f)
        notes = run("llvm-readelf", "--notes", path)
        # the entries of amdhsa.kernels: list items at the list's own indentation
        kernels = {}
        for item in re.split(r"^  - ", notes.split("amdhsa.kernels:")[-1].split("\namdhsa.target")[0], flags=re.M)[1:]:
            meta = dict(re.findall(r"^ {4}\.(\w+):\s+(\S+)$", "    " + item, flags=re.M))  # (not the .args' fields)
            kernels[meta["name"]] = {k: meta.get(k) for k in FIELDS}
        if not kernels:
            continue
        run("llvm-objcopy", "-O", "binary", "--only-section=.text", path, path + ".text")
        with open(path + ".text", "rb") as fh:
            out[tuple(sorted(kernels))] = (fh.read(), kernels)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old, new = code_objects(sys.argv[1], tmp), code_objects(sys.argv[2], tmp)
    bad = 0
    for names in sorted(set(old) | set(new)):
        if names not in old or names not in new:
            bad += 1
            print(f"{'only in ' + ('OLD' if names in old else 'NEW'):<24} code object of {', '.join(names)}")
            continue
        (t0, k0), (t1, k1) = old[names], new[names]
        text = "same" if t0 == t1 else f"DIFFERS ({len(t0)} -> {len(t1)} B)"
        for n in names:
            diff = [f"{f} {k0[n][f]} -> {k1[n][f]}" for f in FIELDS if k0[n][f] != k1[n][f]]
            bad += (t0 != t1) + bool(diff)
            print(f".text {text:<18} metadata {'; '.join(diff) if diff else 'same':<6} {n}")
    print(f"{sum(len(n) for n in old)} kernels in OLD, {sum(len(n) for n in new)} in NEW: "
          + ("identical" if not bad else f"{bad} differences"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
