#!/usr/bin/env python3
"""Compare the kernels of two hipcc device-assembly files (the library's flags plus -S --cuda-device-only), kernel by kernel.

Per kernel symbol, two things are compared as text: the instructions up to s_endpgm (comments and directives dropped,
.LBB labels renumbered in order of appearance, the kernel's own name replaced) and the .amdhsa_* block.  One line per kernel:
identical, differs (with what: code, or the metadata lines that changed), or only in one file.

usage: tools/isa_diff.py <old.s> <new.s> [<old-mangled-name>=<new-mangled-name> ...]     (pairs: kernels that were renamed)
exit status 1 if any kernel differs or is in one file only.
"""
import re
import sys


def kernels(path):
    """{mangled name: (instruction lines, .amdhsa_ lines)} of every kernel in the file"""
    out = {}
    for f in re.split(r"\n\s*\.globl\s+", open(path).read())[1:]:
        name, rest = f.split("\n", 1)
        name = name.strip()
        m = re.search(r"\n\s*\.amdhsa_kernel\s+%s\n(.*?)\n\s*\.end_amdhsa_kernel" % re.escape(name), rest, re.S)
        if not m:
            continue  # a global that is no kernel
        code, labels = [], {}
        for ln in rest.split("\n"):
            t = ln.split(";", 1)[0].strip().replace(name, "<self>")
            if not t or (t.startswith(".") and not t.startswith(".LBB")) or t == "<self>:":
                continue
            t = re.sub(r"\.LBB[0-9]+_[0-9]+", lambda g: labels.setdefault(g.group(0), ".L%d" % len(labels)), t)
            code.append(t)
            if t.startswith("s_endpgm"):
                break
        meta = [ln.split(";", 1)[0].strip().replace(name, "<self>") for ln in m.group(1).split("\n")]
        out[name] = (code, [t for t in meta if t])
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
renamed = dict(a.split("=", 1) for a in sys.argv[3:])
bad = 0
for name in sorted(old):
    other = renamed.get(name, name)
    if other not in new:
        print("only in old   %s" % name)
        bad += 1
        continue
    (c0, m0), (c1, m1) = old[name], new.pop(other)
    what = (["code"] if c0 != c1 else []) + ["%s -> %s" % (a, b) for a, b in zip(m0, m1) if a != b]
    if len(m0) != len(m1):
        what.append("metadata length")
    bad += bool(what)
    label = name if other == name else "%s = %s" % (name, other)
    n0, n1 = (sum(not t.endswith(":") for t in c) for c in (c0, c1))  # labels are compared, not counted
    print("%-13s %6d / %6d instructions  %s%s" % ("differs" if what else "identical", n0, n1, label,
                                                  "   [" + "; ".join(what) + "]" if what else ""))
for name in sorted(new):
    print("only in new   %s" % name)
    bad += 1
sys.exit(1 if bad else 0)
