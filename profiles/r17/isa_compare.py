#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of kernels.hip function by function.

usage: isa_compare.py parent.s tree.s

A function is the text between its `<name>:` label (after `.type <name>,@function`) and its `.Lfunc_end*` label.  Comments, `.loc` /
`.file` / `.cfi` lines and blank lines are dropped, local label numbers (.LBB<f>_<n>, .Lfunc_*<n>, .Ltmp<n>) are replaced by the order
in which the function first mentions them.  The compiler's per-compile `__hip_cuid_*` symbol is not a function and is not compared.
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    want = set()
    for line in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+([A-Za-z_0-9.$]+),@function", line)
        if m:
            want.add(m.group(1))
            continue
        m = re.match(r"([A-Za-z_0-9.$]+):", line)
        if name is None and m and m.group(1) in want:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            out[name] = normalise(body)
            name = None
            continue
        body.append(line)
    return out


def normalise(lines):
    labels = {}

    def lab(m):
        return labels.setdefault(m.group(0), "L%d" % len(labels))

    res = []
    for line in lines:
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).strip()
        if not line or re.match(r"\.(loc|file|cfi_\w+)\b", line):
            continue
        res.append(re.sub(r"\.L(BB\d+_\d+|func_\w+?\d+|tmp\d+|JTI\d+_\d+)", lab, line))
    return res


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = [n for n in a if n in b and a[n] == b[n]]
    differ = [n for n in a if n in b and a[n] != b[n]]
    print("functions: parent %d, tree %d; identical %d, different %d, only in parent %d, only in tree %d"
          % (len(a), len(b), len(same), len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    for n in differ:
        print("DIFFERENT", n)
    for n in sorted(set(a) - set(b)):
        print("ONLY PARENT", n)
    for n in sorted(set(b) - set(a)):
        print("ONLY TREE", n)
    print("order of functions identical:", list(a) == list(b))
    return 0 if not differ and set(a) == set(b) else 1


if __name__ == "__main__":
    sys.exit(main())
