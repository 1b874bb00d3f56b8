#!/usr/bin/env python3
"""Do the device functions two source trees have in common compile to the same code?  For one .hip file of each tree:
the tools/kernel_resources.py rows (registers, scratch, spills, LDS, occupancy) and the gfx950 assembly of every function
body (``hipcc --offload-device-only -S`` with the flags the library is built with), basic-block labels renumbered (a new
function earlier in the file shifts every later ``.LBB<function>_<block>``).  Prints the differences and nothing else:
empty output = identical.  Functions only the second tree has are counted on stderr.

usage: tools/kernel_code_diff.py <old tree> <new tree> [csrc file, default ste_kernels.hip]
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


def resource_rows(tree, name):
    out = subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py"),
                          os.path.join(tree, "ship-track-estimators_amd", "csrc", name)],
                         capture_output=True, text=True, check=True).stdout
    return {ln[:60].rstrip(): ln for ln in out.splitlines() if ln.startswith("ste::")}


def function_bodies(tree, name, tmp):
    src = os.path.join(tree, "ship-track-estimators_amd", "csrc", name)
    asm = os.path.join(tmp, name + ".s")
    subprocess.run([entry._hipcc()] + entry.HIPCC_FLAGS + entry.HIPCC_FILE_FLAGS.get(name, []) +
                   ["--offload-device-only", "-S", src, "-o", asm], check=True)
    out, cur = {}, None
    for ln in open(asm):
        m = re.match(r"^(_Z\S+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end") or re.match(r"\s*\.size\s", ln):
            cur = None
            continue
        ln = ln.split(";")[0].rstrip()
        cur.append(re.sub(r"\.L(BB|CPI|tmp|func_end)?\d+_", r".L\1N_", ln))
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = sys.argv[1], sys.argv[2]
    name = sys.argv[3] if len(sys.argv) > 3 else "ste_kernels.hip"
    ra, rb = resource_rows(old, name), resource_rows(new, name)
    for k in sorted(ra):
        if ra[k] != rb.get(k):
            print(f"resources: {k}\n  - {ra[k]}\n  + {rb.get(k)}")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a"))
        os.makedirs(os.path.join(tmp, "b"))
        fa = function_bodies(old, name, os.path.join(tmp, "a"))
        fb = function_bodies(new, name, os.path.join(tmp, "b"))
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
