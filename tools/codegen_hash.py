#!/usr/bin/env python3
"""Hash of each kernel's machine code in a device assembly listing (hipcc --offload-device-only -S).

    python tools/codegen_hash.py PARENT.s BRANCH.s [--only k_solve]

One line per kernel symbol: sha256 (first 16 hex digits) of its instructions in the first listing beside the second, and
whether they agree.  A kernel's text is the instructions and labels between its label and its `.Lfunc_end`; comments,
assembler directives (the kernel descriptor: kernarg size, register counts — `make resource-usage` reports those) and the
compiler's per-function label numbers (`.LBB12_3` -> `.LBB_3`) are dropped, so that a new kernel in front of an old one
does not change the old one's hash.  This is how profiles/diag_codegen.txt was made.
"""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        t = line.strip()
        if name is None:
            m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", t)
            if m and not t.startswith(".L"):
                name, body = m.group(1), []
            continue
        if t.startswith(".Lfunc_end"):
            out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body)
            name = None
            continue
        if not t or t.startswith(";") or (t.startswith(".") and not t.endswith(":")):
            continue        # comments and assembler directives (the kernel descriptor's .amdhsa_* lines among them)
        t = re.sub(r";.*$", "", t).strip()
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"\.Ltmp\d+", ".Ltmp", t)
        if t:
            body.append(t)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def main(argv):
    only = None
    if "--only" in argv:
        i = argv.index("--only")
        only = argv[i + 1]
        del argv[i:i + 2]
    a, b = kernels(argv[1]), kernels(argv[2])
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    same = diff = 0
    for n in names:
        if only and only not in pretty[n]:
            continue
        ha, hb = a.get(n), b.get(n)
        if ha and hb:
            verdict = "same" if ha[0] == hb[0] else "DIFFERENT"
            same += verdict == "same"
            diff += verdict != "same"
        else:
            verdict = "new" if hb else "gone"
        print(f"{ha[0] if ha else '-':16s} {hb[0] if hb else '-':16s} {(hb or ha)[1]:6d}  {verdict:9s} {re.sub(r'^void ', '', pretty[n])}")
    print(f"# kernels in both listings: {same} with identical code, {diff} different")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(list(sys.argv)))
