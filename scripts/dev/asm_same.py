#!/usr/bin/env python3
"""Did a change of the source move the generated code?  Two device assembly files (build_native keeps them: build/<variant>/*.device.s) go
in; per function SAME or DIFF of its instruction stream -- comments and directives stripped, the block labels (.LBB..) kept without the
function's ordinal in its file (.LBB7_3 -> .LBB_3: a function that moved to another translation unit keeps its stream) -- and per kernel
the resource metadata.  Exit status 1 on any DIFF.  A translation unit split in two: hold the old file against the two new ones concatenated.
usage: asm_same.py OLD.s NEW.s [OLDNAME=NEWNAME ...]     a rename is a regular expression and its replacement, applied to OLD's text:
       '10tree_stageILi(\\d+)ELi1E=19tree_stage_dynamicsILi\\1E'"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "soft-grip_amd"))
import devasm  # noqa: E402


def parse(text):
    funcs = {name: [re.sub(r"\.LBB\d+_", ".LBB_", t) for _, t in body] for name, body in devasm.functions(text).items()}
    kernels = {name: tuple(str(rec[k]) for k in devasm.META) for name, rec in devasm.kernels(text).items()}
    return funcs, kernels


def main(argv):
    old, new = open(argv[1]).read(), open(argv[2]).read()
    for r in argv[3:]:
        a, b = r.split("=", 1)
        old = re.sub(a, b, old)
    (fo, ko), (fn, kn) = parse(old), parse(new)
    bad = 0
    for name in sorted(set(fo) | set(fn)):
        a, b = fo.get(name), fn.get(name)
        if a == b:
            print("SAME %6d instructions  %s" % (sum(1 for s in a if not s.endswith(":")), name))
            continue
        bad += 1
        if a is None or b is None:
            print("DIFF only in %s  %s" % ("NEW" if a is None else "OLD", name))
        else:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("DIFF %d -> %d lines, first at line %d of the stream  %s" % (len(a), len(b), first, name))
    for name in sorted(set(ko) | set(kn)):
        same = ko.get(name) == kn.get(name)
        bad += not same
        print("%s metadata %s  %s" % ("SAME" if same else "DIFF", " ".join("%s=%s" % (k, v) for k, v in zip(devasm.META.values(), kn.get(name) or ko.get(name))) if same
                                       else "%s -> %s" % (ko.get(name), kn.get(name)), name))
    print("%d functions, %d kernels: %s" % (len(set(fo) | set(fn)), len(set(ko) | set(kn)), "all SAME" if not bad else "%d DIFF" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
