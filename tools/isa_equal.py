#!/usr/bin/env python
"""Are two objects the same device code?  Disassembles every gfx950 kernel of both (as tools/isa_census.py does), drops the
addresses and the address comments, pairs the kernels by mangled name and compares the instruction text line by line -- the
instrument of a refactor that must leave a fenced kernel's code alone.
    python tools/isa_equal.py OLD.o NEW.o [--kernel SUBSTR] [--rename OLD=NEW]...
--rename (repeatable) replaces the substring OLD by NEW in OLD.o's kernel names before pairing: for a refactor that renames a
kernel or changes its template parameters.
Prints per kernel `identical`, or the number of differing lines with the first few; exit 1 on any difference or unpaired kernel."""
import difflib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_census import disassemble      # noqa: E402

SHOWN = 4


def kernels(obj, pat):
    """-> {mangled name: [instruction text]} (branch targets are function-relative in the text: they survive a move of the function)"""
    return {name: [body for _, body, _ in ins] for name, ins in disassemble(obj).items() if pat in name}


def main():
    args = sys.argv[1:]
    pat = ""
    if "--kernel" in args:
        i = args.index("--kernel")
        pat = args[i + 1]
        del args[i:i + 2]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    if len(args) != 2 or any(len(r) != 2 for r in renames):
        sys.exit(__doc__)
    old, new = kernels(args[0], pat), kernels(args[1], pat)
    for src, dst in renames:
        old = {name.replace(src, dst): body for name, body in old.items()}
    bad = 0
    if not old and not new:
        print("no kernel matched %r in either object" % pat)
        bad = 1
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%s: only in %s" % (name, args[1] if name in new else args[0]))
            bad += 1
            continue
        if old[name] == new[name]:
            print("%s: identical (%d instructions)" % (name, len(old[name])))
            continue
        delta = [d for d in list(difflib.unified_diff(old[name], new[name], lineterm="", n=0))[2:] if d[0] in "+-"]
        print("%s: %d lines differ (%d -> %d instructions)" % (name, len(delta), len(old[name]), len(new[name])))
        for d in delta[:SHOWN]:
            print("    " + d)
        bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
