#!/usr/bin/env python3
"""Do the device functions two source trees have in common compile to the same code?  For the .hip files named of each
tree, taken together: the tools/kernel_resources.py rows (registers, scratch, spills, LDS, occupancy) and the gfx950 assembly
of every function body (``hipcc --offload-device-only -S`` with the flags each file is built with), basic-block labels
renumbered (a new function earlier in the file shifts every later ``.LBB<function>_<block>``).  The files may differ between
the trees -- a translation unit that was split is compared as the union of its parts.  Prints the differences and nothing
else: empty output = identical.  A function that two files of one tree define with different code is a difference; functions
only the second tree has are counted on stderr.

usage: tools/kernel_code_diff.py <old tree> <new tree> [csrc file ...] [-- csrc file of the new tree ...]
       no file: ste_kernels.hip in both trees; no `--`: the same files in both trees, e.g.
       tools/kernel_code_diff.py A B ste_kernels.hip -- ste_kernels.hip ste_forward_quad.hip ste_smooth.hip ste_sample.hip
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import __graft_entry__ as entry  # noqa: E402  (the compiler flags, per file)


def resource_rows(tree, names):
    rows = {}
    for name in names:
        out = subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py"),
                              os.path.join(tree, "ship-track-estimators_amd", "csrc", name)],
                             capture_output=True, text=True, check=True).stdout
        rows.update({ln[:60].rstrip(): ln for ln in out.splitlines() if ln.startswith("ste::")})
    return rows


def function_bodies(tree, names, tmp):
    out = {}
    for name in names:
        src = os.path.join(tree, "ship-track-estimators_amd", "csrc", name)
        asm = os.path.join(tmp, name + ".s")
        subprocess.run([entry._hipcc()] + entry.HIPCC_FLAGS + entry.HIPCC_FILE_FLAGS.get(name, []) +
                       ["--offload-device-only", "-S", src, "-o", asm], check=True)
        mine, cur = {}, None
        for ln in open(asm):
            m = re.match(r"^(_Z\S+):", ln)
            if m:
                cur = mine.setdefault(m.group(1), [])
                continue
            if cur is None:
                continue
            if ln.startswith(".Lfunc_end") or re.match(r"\s*\.size\s", ln):
                cur = None
                continue
            ln = ln.split(";")[0].rstrip()
            cur.append(re.sub(r"\.L(BB|CPI|tmp|func_end)?\d+_", r".L\1N_", ln))
        for k, body in mine.items():  # an out-of-line device function may be in several code objects: with the same code
            if out.setdefault(k, body) != body:
                print(f"defined differently by two files of {tree} (the second is {name}): {k}")
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or ["ste_kernels.hip"]
    cut = names.index("--") if "--" in names else None
    na, nb = (names, names) if cut is None else (names[:cut], names[cut + 1:])
    ra, rb = resource_rows(old, na), resource_rows(new, nb)
    for k in sorted(ra):
        if ra[k] != rb.get(k):
            print(f"resources: {k}\n  - {ra[k]}\n  + {rb.get(k)}")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a"))
        os.makedirs(os.path.join(tmp, "b"))
        fa = function_bodies(old, na, os.path.join(tmp, "a"))
        fb = function_bodies(new, nb, os.path.join(tmp, "b"))
    for k in sorted(fa):
        if k not in fb:
            print(f"missing in {new}: {k}")
        elif fa[k] != fb[k]:
            print(f"assembly: {k}")
            print("\n".join(list(difflib.unified_diff(fa[k], fb[k], lineterm="", n=1))[:40]))
    print(f"[kernel_code_diff] {len(fa)} functions compared, {len(set(fb) - set(fa))} only in {new}, "
          f"{len(set(rb) - set(ra))} new resource rows", file=sys.stderr)


if __name__ == "__main__":
    main()
