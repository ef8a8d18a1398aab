#!/usr/bin/env python3
"""Compare two device-assembly listings of the same translation unit kernel by kernel.

    hipcc $HIPFLAGS -I../../include -I. --offload-device-only -S surfdisp_kernels.hip -o parent.s     (in either tree)
    isa_identity.py parent.s candidate.s

Lines that hold the compiler's random __hip_cuid symbol are dropped; everything else is compared.  Prints the number of
differing lines of the whole listing, then per function its instruction count on either side and whether the bodies
are equal.  Exit status 1 when any line differs.
"""
import difflib
import re
import subprocess
import sys


def lines_of(path):
    return [l.rstrip("\n") for l in open(path) if "__hip_cuid" not in l]


def functions(lines):
    """name -> body lines (label line to its .Lfunc_end)"""
    out, name, body = {}, None, []
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if name is None and m and not l.startswith(".L"):
            name, body = m.group(1), []
        elif name is not None:
            if l.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(l)
    return out


def ninstr(body):
    return sum(1 for l in body if l.startswith("\t") and not l.lstrip().startswith((".", ";")))


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = lines_of(sys.argv[1]), lines_of(sys.argv[2])
    ndiff = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0)
                if l[:1] in "+-" and not l.startswith(("+++", "---"))) if a != b else 0
    fa, fb = functions(a), functions(b)
    names = sorted(set(fa) | set(fb))
    dm = demangle(names)
    print(f"lines {len(a)} / {len(b)}, differing lines {ndiff}, functions {len(fa)} / {len(fb)}")
    print(f"{'instr A':>8} {'instr B':>8}  body       function")
    for n in names:
        ia = ninstr(fa[n]) if n in fa else -1
        ib = ninstr(fb[n]) if n in fb else -1
        same = "equal" if fa.get(n) == fb.get(n) else "DIFFERENT"
        print(f"{ia:8d} {ib:8d}  {same:9s}  {dm[n]}")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
