#!/usr/bin/env python3
"""Compares the kernels of two `hipcc --offload-device-only -S` outputs body by body.

    python tools/isa_diff.py parent.s new.s

A body runs from a `_Z...:` label to its `.Lfunc_end`.  Comments and `.p2align` / `.loc` / `.cfi` lines are dropped and
`.LBB*` / `.Ltmp*` labels renumbered in order of appearance, so that two bodies compare equal exactly when they hold the
same instructions in the same order.  Exit status 0: same kernel names and every body identical."""
import re
import subprocess
import sys

LABEL = re.compile(r"\.L(BB|tmp)[0-9_]+")


def bodies(path):
    out, name, body, labels = {}, None, None, {}
    for line in open(path):
        line = re.split(r"\s*(;|//)", line, 1)[0].strip()
        m = re.fullmatch(r"(_Z\w+):", line)
        if m and name is None:
            name, body, labels = m.group(1), [], {}
        elif name is not None and line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif name is not None and line and not line.startswith((".p2align", ".loc", ".cfi")):
            body.append(LABEL.sub(lambda l: labels.setdefault(l.group(0), ".L%s%d" % (l.group(1), len(labels))), line))
    return out


def instructions(body):
    return sum(1 for l in body if not l.startswith(".") and not l.endswith(":"))


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    for n in sorted(set(a) - set(b)): print("only in %s: %s" % (sys.argv[1], n))
    for n in sorted(set(b) - set(a)): print("only in %s: %s" % (sys.argv[2], n))
    both = [n for n in a if n in b]
    differ = [n for n in both if a[n] != b[n]]
    pretty = demangle(differ)
    for n in differ: print("differs: %s  (%d -> %d instructions)" % (pretty[n], instructions(a[n]), instructions(b[n])))
    print("kernels %d / %d, names %s, identical %d, different %d" %
          (len(a), len(b), "equal" if set(a) == set(b) else "NOT equal", len(both) - len(differ), len(differ)))
    return 0 if set(a) == set(b) and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
