#!/usr/bin/env python3
"""CPU: the host-side layout answers of two builds of the library, compared.

    host_layout.py parent.so candidate.so     each library in a process of its own; prints the verdict, exit status 1 on a difference
    host_layout.py --dump                     the table of the library SURFDISP_LIB_PATH names (what the two processes run)

Per (B, Lmax, P): the seven *_workspace_bytes functions and surfdisp_group_kernels_shift_offset; per (B, Lmax, P, kind):
surfdisp_get_team2 for both wave types x {none, PHASE_ONLY, INDEPENDENT, PIPELINED}.  None of these calls needs a device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = (1, 3, 100, 4096, 16384, 25600, 65536, 131072)
LS = (2, 5, 10, 24, 64, 96, 200)
PS = (1, 4, 20, 200)
INVALID = ((0, 10, 20), (100, 1, 20), (100, 10, 0))
SIZES = ("surfdisp_workspace_bytes", "surfdisp_kernels_workspace_bytes", "surfdisp_group_kernels_workspace_bytes",
         "surfdisp_ellip_kernels_workspace_bytes", "surfdisp_atten_workspace_bytes", "surfdisp_eigen_workspace_bytes",
         "surfdisp_thickness_kernels_workspace_bytes", "surfdisp_group_kernels_shift_offset")


def dump():
    sys.path.insert(0, ROOT)
    from pysurfinv_amd import _lib
    L = _lib.lib()
    flags = (0, _lib.PHASE_ONLY, _lib.INDEPENDENT, _lib.PIPELINED)
    shapes = [(B, Lm, P) for B in BS for Lm in LS for P in PS]
    for B, Lm, P in shapes + list(INVALID):
        sizes = " ".join(str(int(getattr(L, f)(B, Lm, P))) for f in SIZES)
        teams = " ".join(str(L.surfdisp_get_team2(B, Lm, P, wave | f)) for wave in (1, 2) for f in flags) \
            if (B, Lm, P) not in INVALID else "-"
        print(f"{B} {Lm} {P} | {sizes} | {teams}")


def main():
    if sys.argv[1:] == ["--dump"]:
        return dump()
    tables = []
    for path in sys.argv[1:3]:
        env = dict(os.environ, SURFDISP_LIB_PATH=os.path.abspath(path))
        tables.append(subprocess.run([sys.executable, os.path.abspath(__file__), "--dump"], env=env, check=True,
                                     capture_output=True, text=True).stdout.splitlines())
    a, b = tables
    ndiff = sum(1 for x, y in zip(a, b) if x != y) + abs(len(a) - len(b))
    print(f"shapes {len(BS)} x {len(LS)} x {len(PS)} + {len(INVALID)} invalid corners = {len(a)} rows; per row {len(SIZES)} sizes / offsets "
          f"and 8 teams (2 wave types x none, PHASE_ONLY, INDEPENDENT, PIPELINED)")
    print(f"differing rows: {ndiff}")
    for x, y in zip(a, b):
        if x != y:
            print("A", x), print("B", y)
    print("first, middle and last row (B Lmax P | forward kernels group ellip atten eigen thickness shift_offset | teams):")
    for r in (a[0], a[len(a) // 2], a[-len(INVALID) - 1]) + tuple(a[-len(INVALID):]):
        print("  " + r)
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
