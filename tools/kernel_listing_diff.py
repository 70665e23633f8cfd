#!/usr/bin/env python3
"""Which kernels differ between two builds' gfx950 listings (raptor_amd/csrc/_obj/*.s, kept by raptor_amd.build)?

    python tools/kernel_listing_diff.py OLD_DIR NEW_DIR

Per kernel symbol the instruction stream (label to .Lfunc_end) and the .amdhsa_kernel descriptor block are compared as text, with
comments dropped and what only numbers a function within its file (.Lfunc_begin7, .LBB7_3, .Ltmp12) renamed by order of appearance: adding a kernel to a
source must leave every other kernel's text as it was.  Prints the kernels that are new, gone or changed; exit status 1 if any
pre-existing kernel changed or went.
"""
import os
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if f".amdhsa_kernel {name}\n" not in text:
            continue
        desc = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), text, re.S).group(1)
        names = {}

        def local(mm):
            return names.setdefault(mm.group(0), f".L{len(names)}")
        body = re.sub(r"[ \t]*;[^\n]*", "", body)                  # comments name basic blocks by the function's number
        body = re.sub(r"\.L(?:BB|tmp|func_begin|func_end)\d+(?:_\d+)?", local, body)
        out[name] = body + "\n--descriptor--\n" + desc
    return out


def main(old_dir, new_dir):
    bad = 0
    for f in sorted(os.listdir(old_dir)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(new_dir, f)):
            continue
        old, new = kernels(os.path.join(old_dir, f)), kernels(os.path.join(new_dir, f))
        same = [k for k in old if k in new and old[k] == new[k]]
        changed = [k for k in old if k in new and old[k] != new[k]]
        gone = [k for k in old if k not in new]
        added = [k for k in new if k not in old]
        print(f"{f}: {len(same)} kernels unchanged, {len(changed)} changed, {len(gone)} gone, {len(added)} new")
        for k in changed:
            print("  CHANGED", k)
        for k in gone:
            print("  GONE   ", k)
        for k in added:
            print("  new    ", k)
        bad += len(changed) + len(gone)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
