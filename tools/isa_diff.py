"""Which kernels differ between two gfx950 assembly listings of one source file.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S a.hip -o a.s      (likewise b.s)
    python tools/isa_diff.py a.s b.s

A kernel's text runs from its label to the `.end_amdhsa_kernel` behind it (code and kernel descriptor).  Comments are
stripped, local `.L...` labels map to one token, and the rest is compared as plain text.  Prints one line per kernel
that is missing from either file or differs, with the scratch / VGPR / SGPR / LDS / occupancy figures of both sides, then
a count; exit status 1 if any differ.  --list prints every kernel name with `identical` or `changed`.
"""
import argparse
import re
import sys

_LOCAL = re.compile(r"\.L[A-Za-z0-9_$.]+")
_FIGURES = (("scratch", r"; ScratchSize: (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"),
            ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"))


def kernels(path):
    """{kernel symbol: (normalised text lines, {figure: value})} of one .s file."""
    lines = open(path).read().splitlines()
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        raw = lines[start:end + 1]
        text = []
        for ln in raw:
            ln = ln.split(";", 1)[0].split("//", 1)[0].strip()
            if ln:
                text.append(_LOCAL.sub(".L", ln))
        info = "\n".join(lines[end:end + 60])           # the "; Kernel info:" comment block behind the descriptor
        figures = {}
        for key, pat in _FIGURES:
            m = re.search(pat, info)
            if m:
                figures[key] = int(m.group(1))
        out[name] = (text, figures)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--list", action="store_true", help="every kernel, identical or changed")
    args = ap.parse_args()
    ka, kb = kernels(args.a), kernels(args.b)
    changed = []
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"{name}: only in {args.b if name in kb else args.a}")
            changed.append(name)
        elif ka[name][0] != kb[name][0]:
            changed.append(name)
            print(f"{name}: changed  a={ka[name][1]}  b={kb[name][1]}")
        elif args.list:
            print(f"{name}: identical")
    print(f"{len(set(ka) | set(kb))} kernels, {len(changed)} differ")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
