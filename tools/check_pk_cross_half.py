#!/usr/bin/env python
"""Build-time scan for packed float32 instructions whose LOW result reads the HIGH half of a source (round 6):

    v_pk_add_f32 v[4:5], v[0:1], v[2:3] op_sel:[0,1] op_sel_hi:[1,0]      <- low result = v0 + v3

conv_wino3's first-forward defect was traced to exactly this form (the low result came out as `a.lo + 0` in a few fresh processes);
the same subtraction as plain v_sub_f32 never failed, and why the packed form fails there is not known.  So no new kernel may carry
it: an op_sel bit of 1 on any source of a v_pk_*_f32 instruction refuses the build, except in an object whose file name, or a kernel
whose mangled name, EQUALS an --allow entry (counted, not refused: the objects that carried the form -- mostly as a horizontal add
lo + hi -- before the scan existed, csrc/Makefile; an exact match, so a new object or kernel is never exempt by a similar name).
    python tools/check_pk_cross_half.py [--report] [--allow NAME ...] <file.o|file.so> ...     (--report: print, never fail)"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_store_hazard as ch

PK_F32 = re.compile(r"^\s*(v_pk_\w+_f32)\s")
OP_SEL = re.compile(r"\bop_sel:\[([01](?:,[01])*)\]")


def scan_text(text, where, allow=()):
    """-> (refused, allowed): the cross-half packed f32 instructions of an objdump listing, as 'where: function: instruction'."""
    refused, allowed, fn = [], [], "?"
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            fn = m.group(1)
            continue
        body = ln.split("//")[0]
        if not PK_F32.match(body):
            continue
        sel = OP_SEL.search(body)
        if sel and "1" in sel.group(1).split(","):
            hit = "%s: %s: %s" % (where, fn[:70], body.strip())
            (allowed if where in allow or fn in allow else refused).append(hit)
    return refused, allowed


def main(argv):
    report = "--report" in argv
    allow, paths, i = [], [], 0
    while i < len(argv):
        if argv[i] == "--allow":
            allow.append(argv[i + 1])
            i += 2
            continue
        if not argv[i].startswith("--"):
            paths.append(argv[i])
        i += 1
    tmp = tempfile.mkdtemp(prefix="pkcross")
    refused, allowed, nobj, npk = [], [], 0, 0
    try:
        for p in paths:
            local = os.path.join(tmp, os.path.basename(p))
            shutil.copy(p, local)
            subprocess.run([ch.OBJDUMP, "--offloading", local], capture_output=True, text=True)
            for co in sorted(glob.glob(local + ".*gfx950*")):
                text = subprocess.run([ch.OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
                nobj += 1
                npk += sum(1 for ln in text.splitlines() if PK_F32.match(ln.split("//")[0]))
                r, a = scan_text(text, os.path.basename(p), allow)
                refused += r
                allowed += a
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for b in refused:
        print("PACKED F32 CROSS-HALF  " + b)
    if report:
        for b in allowed[:8]:
            print("allowed  " + b)
    print("check_pk_cross_half: %d code object(s), %d packed f32 instruction(s), %d cross-half refused, %d in allowed kernels" % (
        nobj, npk, len(refused), len(allowed)))
    if not nobj:
        print("check_pk_cross_half: no device code found -- refusing")
        return 1
    return 1 if refused and not report else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
