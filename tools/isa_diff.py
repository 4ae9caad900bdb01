#!/usr/bin/env python3
"""Compare two device assembly files function by function.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o old/x.s    (parent)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o new/x.s    (change)
    tools/isa_diff.py old/x.s new/x.s [--renamed OLD=NEW ...]

A refactor that is meant to leave the device code alone is checked by this:
per function (kernels and out-of-line device functions) it prints the
instruction counts of both sides, the VGPR / SGPR / scratch / LDS figures the
compiler writes beside each function, and `identical: yes` or `identical: NO`.

What is compared is the instruction stream only: mnemonics and operands in
order.  Set aside: directives (the kernel descriptor included), comments,
blank lines, and the per-compilation `__hip_cuid_*` object.  Labels are not
instructions either; a branch's target is compared as the index of the
instruction it lands on, so a function that only moved inside the file (its
`.LBB<n>_` prefix changed) still compares equal and a retargeted branch does
not.  There is no "same up to register numbering": a renumbered stream is NO.

--renamed OLD=NEW (symbol names as they stand in the files, i.e. mangled)
pairs a function whose name changed and rewrites OLD to NEW wherever the old
side's instructions name it (a call's `OLD@rel32`).

Exit status 1 on any NO, on any differing figure, and on any function present
on one side only that no --renamed pairs; 0 otherwise.  Host only: it reads
two text files.
"""
import argparse
import re
import sys

FIGURES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")
_LABEL = re.compile(r"^([.\w$]+):")
_FIG = re.compile(r"^;\s*(\w+)\s*[:=]\s*(\d+)")
_LOCAL = re.compile(r"\.L[\w$.]+")


class Func:
    def __init__(self, name):
        self.name = name
        self.ins = []      # instruction texts, comments stripped
        self.labels = {}   # local label -> index of the next instruction
        self.fig = {}

    def stream(self, rename):
        out = []
        for text in self.ins:
            text = _LOCAL.sub(lambda m: "@%d" % self.labels[m.group(0)] if m.group(0) in self.labels
                              else m.group(0), text)
            for old, new in rename.items():
                text = re.sub(r"(?<![\w$.])%s(?![\w$.])" % re.escape(old), new, text)
            out.append(text)
        return out


def parse(path):
    """{name: Func} in file order, for every symbol of `.type ...,@function`."""
    funcs, names = {}, set()
    cur = last = None
    want_fig = False
    with open(path) as f:
        for raw in f:
            line = raw.strip()
            if not line:
                continue
            if line.startswith(".type"):
                m = re.match(r"\.type\s+([^,\s]+)\s*,\s*@function", line)
                if m:
                    names.add(m.group(1))
                continue
            if line.startswith(";"):
                if line.startswith("; Kernel info:") or line.startswith("; Function info:"):
                    want_fig = last is not None
                elif want_fig:
                    m = _FIG.match(line)
                    if m and m.group(1) in FIGURES:
                        last.fig[m.group(1)] = int(m.group(2))
                continue
            m = _LABEL.match(line)
            if m:
                lab = m.group(1)
                if lab in names and lab not in funcs:
                    cur = last = funcs[lab] = Func(lab)
                    want_fig = False
                elif lab.startswith(".Lfunc_end"):
                    cur = None
                elif cur is not None:
                    cur.labels[lab] = len(cur.ins)
                continue
            if line.startswith(".") or cur is None:
                continue  # directive, or data outside any function
            cur.ins.append(" ".join(line.split(";", 1)[0].split()))
    return funcs


def fig_text(f):
    return " ".join("%s=%s" % (k, f.fig.get(k, "-")) for k in FIGURES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    rename = dict(r.split("=", 1) for r in args.renamed)
    old, new = parse(args.old), parse(args.new)
    bad = 0
    print("# %s -> %s" % (args.old, args.new))
    for name, fo in old.items():
        to = rename.get(name, name)
        fn = new.get(to)
        if fn is None:
            print("%s\n  only in %s" % (name, args.old))
            bad += 1
            continue
        so, sn = fo.stream(rename), fn.stream({})
        same = so == sn
        figs = fo.fig == fn.fig
        print(name if to == name else "%s -> %s" % (name, to))
        print("  instructions: %d -> %d" % (len(so), len(sn)))
        if figs:
            print("  figures: %s (same)" % fig_text(fo))
        else:
            print("  figures: %s -> %s (DIFFER)" % (fig_text(fo), fig_text(fn)))
        print("  identical: %s" % ("yes" if same else "NO"))
        if not same:
            for k, (a, b) in enumerate(zip(so, sn)):
                if a != b:
                    print("  first difference at instruction %d:\n    - %s\n    + %s" % (k, a, b))
                    break
        bad += (not same) or (not figs)
    paired = set(rename.get(n, n) for n in old)
    for name in new:
        if name not in paired:
            print("%s\n  only in %s" % (name, args.new))
            bad += 1
    print("# %d functions, %d not identical or unpaired" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
