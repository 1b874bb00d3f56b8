#!/usr/bin/env python3
"""Every `s_waitcnt` with a vmcnt field in the step loop of one kernel of a hipcc -S / -save-temps .s file.

gfx9 counts loads and stores in ONE in-order counter, so `s_waitcnt vmcnt(N)` lets the N youngest vector-memory
operations stay in flight and waits for everything older.  A wait whose N is smaller than the number of stores the wave has
issued since the load it is meant for also waits for those stores' acknowledgements ("Store drain").

For each wait: its basic block (and where in the block), N, and what lies behind it, walking back through the block and
on through the blocks in front of it inside the loop (across the back edge too; where paths meet, the path with the most
stores is reported, as the compiler has to assume it):
  stores   store instructions met before the nearest older vector-memory instruction that is not a store; a range where
           the paths differ (the covariance layout and the optional position output are run-time choices: 14 stores per
           row packed, 20 full, 2 more with positions)
  then     what ended the walk: `load` (a global/scratch/buffer/flat load: block[index]) or `call` (s_swappc: anything may
           be pending)
A wait with N < stores sits behind stores that are younger than every load it can be meant for, and waits for their
acknowledgements too: it is marked.  Waits on lgkmcnt / expcnt alone are only counted.

usage: tools/isa_waits.py <file.s> <mangled-name-substring>
"""
import re
import sys

from isa_loop_hist import step_loops

VMEM = ("global_", "scratch_", "buffer_", "flat_")


def vmem_kind(op):
    if not op.startswith(VMEM):
        return None
    return "store" if "_store" in op else "load"  # atomics with return count as loads; the loops have none


def waits_of(blocks, order, succ, comp):
    inloop = set(comp)
    # edges into each block, as (block, index to walk back from): a branch leaves from where it stands (the loop finder's
    # blocks run from label to label, branches inside them), the fall-through from the block's end
    preds = {b: [] for b in comp}
    for i, a in enumerate(order):
        if a not in inloop:
            continue
        fall = True
        for j, t in enumerate(blocks[a]):
            op = t.split()[0]
            if op.startswith("s_cbranch") or op == "s_branch":
                if t.split()[-1] in inloop:
                    preds[t.split()[-1]].append((a, j))
                fall = fall and op != "s_branch"
        if fall and i + 1 < len(order) and order[i + 1] in inloop:
            preds[order[i + 1]].append((a, len(blocks[a])))
    rows, other, memo = [], 0, {}

    def back(cb, ci, path):
        """(fewest stores, most stores, then, joins) walking back from instruction ci of block cb; where paths join, every
        path is followed and `then` is what ended the one with the most stores.  None: once round the loop without a load."""
        stores = 0
        for j in range(ci - 1, -1, -1):
            op = blocks[cb][j].split()[0]
            k = vmem_kind(op)
            if k == "store":
                stores += 1
            elif k == "load":
                return stores, stores, f"load {cb}[{j}]", 0
            elif op.startswith("s_swappc"):
                return stores, stores, f"call {cb}[{j}]", 0
        found = []
        for e in preds[cb]:
            if e[0] in path:
                continue
            if e not in memo:
                memo[e] = back(e[0], e[1], path + (e[0],))
            if memo[e] is not None:
                found.append(memo[e])
        if not found:
            return None
        worst = max(found, key=lambda r: r[1])
        return stores + min(r[0] for r in found), stores + worst[1], worst[2], worst[3] + (len(preds[cb]) > 1)

    for b in comp:
        for i, t in enumerate(blocks[b]):
            if not t.startswith("s_waitcnt"):
                continue
            m = re.search(r"vmcnt\((\d+)\)", t)
            if not m:
                other += 1
                continue
            rows.append((b, i, len(blocks[b]), int(m.group(1))) + (back(b, i, (b,)) or (0, 0, "nothing in the loop", 0)))
    return rows, other


if __name__ == "__main__":
    for name, blocks, order, succ, comp in step_loops(open(sys.argv[1]).read(), sys.argv[2]):
        rows, other = waits_of(blocks, order, succ, comp)
        print(name, "loop blocks:", len(comp), "instructions (static):", sum(len(blocks[b]) for b in comp))
        print(f"  {'block':14s} {'at':>11s} {'vmcnt':>5s} {'stores':>7s}  then")
        for b, i, n, vm, smin, smax, then, joins in rows:
            mark = "  <-- drains stores" if vm < smin else "  <- drains stores on some paths" if vm < smax else ""
            st = str(smin) if smin == smax else f"{smin}-{smax}"
            print(f"  {b:14s} {i:5d}/{n:<5d} {vm:5d} {st:>7s}  {then}{f' (across {joins} joins)' if joins else ''}{mark}")
        print(f"  ({len(rows)} waits with vmcnt, {other} on other counters alone)")
