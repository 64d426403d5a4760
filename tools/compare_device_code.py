#!/usr/bin/env python3
"""Compare the device assembly of one translation unit before and after a change that must not alter any kernel.

    hipcc <the Makefile's flags> -save-temps=obj -c -o OLD_DIR/ba_api.o ba_api.hip      (and the same into NEW_DIR)
    tools/compare_device_code.py OLD_DIR/ba_api-hip-amdgcn-amd-amdhsa-gfx950.s NEW_DIR/ba_api-hip-amdgcn-amd-amdhsa-gfx950.s

Per symbol: the text of every @function symbol from its label to its .Lfunc_end, and every .amdhsa_kernel ... .end_amdhsa_kernel
descriptor.  Only the numbers that say where in the module a function sits are normalised (.LBB<n>_, .Lfunc_begin/end<n>, .Ltmp<n>,
.LJTI<n>_, BB<n>_ where a loop comment repeats a label, and the padding between a label and its comment), so a move that reorders the kernels compares equal and nothing else does.  Prints one line; exit status 1 on any
difference.  Keep the .s files outside the repository.
"""
import re
import sys

POSITION = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+")
LOOP_NOTE = re.compile(r"\bBB\d+(?=_\d)")      # the same label number in the assembler's loop comments ("in Loop: Header=BB32_3")
LABEL_PAD = re.compile(r"^(\.LBB#_\d+:) +;", re.M)      # the comment behind a label starts at a fixed column: a function number that gains a digit moves it


def symbols(path):
    """{name: text} for function bodies ('name') and kernel descriptors ('name [descriptor]')."""
    lines = open(path).read().split("\n")
    functions = [m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l and not l[0].isspace() and ":" in l}
    out = {}
    for name in functions:
        i = start[name]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[name] = LABEL_PAD.sub(r"\1 ;", LOOP_NOTE.sub("BB#", POSITION.sub(r".\1#", "\n".join(lines[i:j + 1]))))
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            out[m.group(1) + " [descriptor]"] = "\n".join(lines[i:j + 1])
            i = j
        i += 1
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
    bad = sorted(set(old) ^ set(new)) + sorted(n for n in set(old) & set(new) if old[n] != new[n])
    for name in bad:
        print(("only in OLD: " if name not in new else "only in NEW: " if name not in old else "differs: ") + name)
    kernels = sum(1 for n in new if n.endswith(" [descriptor]"))
    print(f"{sys.argv[2].split('/')[-1]}: {len(new) - kernels} functions, {kernels} kernels, "
          + ("all bodies and descriptors identical" if not bad else f"{len(bad)} DIFFER"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
