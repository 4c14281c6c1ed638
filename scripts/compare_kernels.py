#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel: the instruction text and the resource figures of the code-object notes.

    python scripts/compare_kernels.py OLD NEW

OLD and NEW are device-only gfx950 objects, or directories of them, built with the Makefile's flags plus
`--offload-device-only --no-gpu-bundle-output -c`.  Kernels are matched by symbol name across all objects of a side, so a kernel may
move from one unit to another.  One line per kernel: `same`, `DIFF` with what differs, or the side it is missing from.  The
instruction text is the llvm-objdump disassembly without the address comments, cut after the kernel's last end-of-program
instruction (what follows is alignment padding that depends on the neighbours in the unit).  Exit status 1 if a kernel differs or
is missing from one side.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

NOTE_FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
               ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def tool(name):
    for cand in (shutil.which(name), f"/opt/rocm/llvm/bin/{name}", f"/opt/rocm/lib/llvm/bin/{name}"):
        if cand and os.access(cand, os.X_OK):
            return cand
    sys.exit(f"{name} not found")


def objects(path):
    return sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]


def kernel_notes(obj):
    """{kernel name: {field: value}} from the amdhsa.kernels list of the code-object notes"""
    text = subprocess.run([tool("llvm-readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout
    kernels, cur = [], None
    for line in text.splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)
        if m:
            cur = {m.group(1): m.group(2)}
            kernels.append(cur)
            continue
        m = re.match(r"^    (\.\w+):\s*(.*)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
        elif not line.startswith("   "):
            cur = None
    return {k[".name"].strip("'\""): {f: k.get(f) for f in NOTE_FIELDS} for k in kernels if ".name" in k}


def kernel_text(obj):
    """{symbol: instruction lines} of the text section"""
    text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", obj], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for name, lines in out.items():
        ends = [i for i, l in enumerate(lines) if l.startswith("s_endpgm")]
        if ends:
            del lines[ends[-1] + 1:]
    return out


def side(path):
    kernels = {}
    for obj in objects(path):
        notes, text = kernel_notes(obj), kernel_text(obj)
        for name, fields in notes.items():
            kernels[name] = (text.get(name, []), fields, os.path.basename(obj))
    return kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = side(sys.argv[1]), side(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"only in {'OLD' if name in old else 'NEW'}  {name}")
            bad += 1
            continue
        (t0, f0, u0), (t1, f1, u1) = old[name], new[name]
        what = []
        if t0 != t1:
            first = next((i for i, (a, b) in enumerate(zip(t0, t1)) if a != b), min(len(t0), len(t1)))
            what.append(f"text: {len(t0)} -> {len(t1)} instructions, first difference at {first}")
        what += [f"{f} {f0[f]} -> {f1[f]}" for f in NOTE_FIELDS if f0[f] != f1[f]]
        bad += bool(what)
        print(f"{'DIFF' if what else 'same'}  {name}  ({u0} -> {u1}, {len(t1)} instructions)" + "".join(f"\n      {w}" for w in what))
    print(f"{len(set(old) & set(new))} kernels on both sides, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
