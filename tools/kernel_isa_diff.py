#!/usr/bin/env python3
"""Compares the kernels of two device assembly files symbol by symbol.

  hipcc <FLAGS of lap_amd/build.py> --cuda-device-only -S csrc/gemm.hip -o before.s       (at the parent)
  hipcc <the same>                                        csrc/gemm.hip -o after.s        (at the change)
  python tools/kernel_isa_diff.py before.s after.s

A kernel is every symbol with an .amdhsa_kernel descriptor; its text is the instructions from its label to its .Lfunc_end plus the
descriptor block (registers, LDS, scratch).  Comments, line / file / cfi directives and blank lines are dropped, and the function
index inside local labels (.LBB<function>_<block>) is removed, since it only counts the functions ahead in the file.  Prints the
number of kernels on each side, how many are identical, and every symbol that differs or exists on one side only; exit status 1
if there is any.
"""
import re
import sys

_SKIP = re.compile(r"^\.(loc|file|cfi_\w+|p2align|Ltmp\d+:)")
_LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def _clean(line):
    line = line.split(";", 1)[0].split("//", 1)[0].strip()
    if not line or _SKIP.match(line):
        return None
    return _LABEL.sub(lambda m: "." + m.group(1), line)


def kernels(path):
    """{symbol: cleaned text lines} of every kernel in an assembly file."""
    lines = open(path, errors="replace").read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    want, out, cur = set(names), {n: [] for n in names}, None
    for l in lines:
        s = l.split(";", 1)[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in want:
                cur = ("code", s[:-1])
            elif s.startswith(".amdhsa_kernel "):
                cur = ("desc", s.split()[1])
            continue
        kind, name = cur
        if (kind == "code" and s.startswith(".Lfunc_end")) or (kind == "desc" and s.startswith(".end_amdhsa_kernel")):
            cur = None
            continue
        c = _clean(l)
        if c is not None:
            out[name].append(c)
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    same = sorted(n for n in a if n in b and a[n] == b[n])
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"kernels: {len(a)} in {argv[1]}, {len(b)} in {argv[2]}")
    print(f"identical: {len(same)}")
    for title, names in (("differ", differ), (f"only in {argv[1]}", only_a), (f"only in {argv[2]}", only_b)):
        print(f"{title}: {len(names)}")
        for n in names:
            extra = f"   ({len(a[n])} -> {len(b[n])} lines)" if title == "differ" else ""
            print(f"  {n}{extra}")
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
