#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (hipcc <the Makefile's flags> --cuda-device-only -S), kernel by kernel:
the instruction streams with comments and directives ignored, and the resources the compiler reports behind each kernel.

    tools/isa_diff.py parent/dbscan.s result/dbscan.s [--markdown]

Prints one line per kernel: `same`, or `differs` with VGPRs, SGPRs, scratch bytes, LDS bytes and waves per SIMD of both."""
import re
import subprocess
import sys

RES = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; NumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
       ("lds", r"; LDSByteSize: (\d+)"), ("waves", r"; Occupancy: (\d+)"))


def kernels(path):
    """{kernel symbol: (instruction lines, resources)} of one .s file"""
    out, name, body = {}, None, []
    lines = open(path).read().splitlines()
    for idx, line in enumerate(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and name is None and idx and ".type" not in line:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            tail = "\n".join(lines[idx:idx + 60])
            res = {k: int(re.search(p, tail).group(1)) if re.search(p, tail) else -1 for k, p in RES}
            out[name] = (body, res)
            name = None
            continue
        code = line.split(";")[0].strip()
        if not code or (code.startswith(".") and not code.endswith(":")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    return out


def demangle(names):
    if not names:
        return {}
    try:
        res = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, res))
    except Exception:
        return {n: n for n in names}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    md = "--markdown" in sys.argv
    dm = demangle(sorted(set(a) | set(b)))
    differs = 0
    for k in sorted(set(a) | set(b)):
        short = re.sub(r"^void mused::", "", dm[k]).split("(")[0]
        if k not in a or k not in b:
            print(f"{short}: only in {'parent' if k in a else 'result'}")
            continue
        same = a[k][0] == b[k][0]
        differs += not same
        ra, rb = a[k][1], b[k][1]
        cells = " | ".join(f"{ra[x]} / {rb[x]}" for x, _ in RES)
        if md:
            print(f"| `{short}` | {'same' if same else 'differs'} | {len(a[k][0])} / {len(b[k][0])} | {cells} |")
        else:
            print(f"{short}: {'same' if same else 'DIFFERS'}  instr {len(a[k][0])} / {len(b[k][0])}  "
                  + "  ".join(f"{x} {ra[x]} / {rb[x]}" for x, _ in RES))
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
