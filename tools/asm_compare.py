#!/usr/bin/env python3
"""Compare the device assembly (hipcc --cuda-device-only -S) of two builds of one source file function by function.

usage: asm_compare.py [--rename OLD=NEW]... [--subset] A.s B.s   (or two directories of *.s files with the same names)
  --rename OLD=NEW   replace OLD by NEW in A's text first: a kernel whose template parameter list changed carries a new mangled name
  --subset           B may lack functions of A (retired template instantiations); what B has must be A's, nothing may be new

A refactor that only moves host code or changes the order in which templates are instantiated leaves every kernel's instructions
alone but may reorder the functions of the file, which renumbers the local labels (.LBB<function>_<block>), and the compilation-unit
id symbol (__hip_cuid_<hash>) follows the path of the source.  So: bodies are keyed by symbol name, function numbers are taken out
of local labels, assembler comments are dropped (they repeat those numbers), the cuid hash is masked, the kernel descriptors
(.amdhsa_kernel blocks) belong to their kernel's entry, and the kernel metadata blocks are compared as a set.  Prints one line per file; exit
status 1 if anything differs."""
import os
import re
import sys
from collections import Counter


def functions(path, renames=()):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    for old, new in renames:
        text = text.replace(old, new)
    text = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)(\d+)(_?)", lambda m: "." + m.group(1) + ("_" if m.group(3) else ""), text)
    out, rest = {}, []
    name, body = None, []
    for line in text.split("\n"):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if "; -- End function" in line:
                out[name] = "\n".join(body)
                name = None
            else:          # (comments carry block numbers of the form BB<function>_<block> and alignment padding: dropped)
                body.append(line if line.lstrip().startswith(";;#") else line.split(";")[0].rstrip())
        else:
            rest.append(line)
    rest = "\n".join(rest)
    # kernel descriptors (.amdhsa_kernel NAME ... .end_amdhsa_kernel): hipcc of ROCm 7.2 emits them between the function markers, so they are part of
    # the body compared above; one found outside is keyed by kernel name in the same way
    for m in re.finditer(r"[ \t]*\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel\n", rest, flags=re.S):
        out["descriptor of " + m.group(1)] = m.group(0)
    rest = re.sub(r"[ \t]*\.amdhsa_kernel \S+\n.*?\.end_amdhsa_kernel\n", "", rest, flags=re.S)
    kernels, _, trailer = rest.partition("amdhsa.target:")          # the kernel list of the metadata ends where the target line begins
    meta = sorted(("  - .agpr_count:" + b) for b in kernels.split("  - .agpr_count:")[1:])
    head = kernels.split("  - .agpr_count:")[0] + trailer
    # outside the functions: section / .globl lines of each function (order follows the functions) and file-level data
    head = "\n".join(sorted(head.split("\n")))
    return out, meta, head


def compare(a, b, renames=(), subset=False):
    fa, ma, ha = functions(a, renames)
    fb, mb, hb = functions(b)
    problems = []
    if subset:          # A keeps only what B also has; anything of B that A lacks still shows below
        fa = {k: v for k, v in fa.items() if k in fb}
        ma = [m for m in ma if m in mb]
        ha = "\n".join(sorted((Counter(ha.split("\n")) & Counter(hb.split("\n"))).elements()))
    if set(fa) != set(fb):
        problems.append(f"symbols differ: only A {sorted(set(fa) - set(fb))[:3]} only B {sorted(set(fb) - set(fa))[:3]}")
    problems += [f"body differs: {k}" for k in sorted(set(fa) & set(fb)) if fa[k] != fb[k]]
    if ma != mb:
        problems.append("kernel metadata differs")
    if ha != hb:
        problems.append("file-level lines differ")
    same_order = list(fa) == list(fb)
    return problems, len(fb), same_order


def main():
    args = sys.argv[1:]
    renames, subset = [], False
    while args and args[0].startswith("--"):
        if args[0] == "--subset":
            subset = True
            args = args[1:]
        else:
            assert args[0] == "--rename", __doc__
            renames.append(tuple(args[1].split("=", 1)))
            args = args[2:]
    a, b = args
    pairs = [(os.path.join(a, f), os.path.join(b, f)) for f in sorted(os.listdir(a)) if f.endswith(".s")] if os.path.isdir(a) else [(a, b)]
    bad = 0
    for x, y in pairs:
        problems, n, same_order = compare(x, y, renames, subset)
        status = "IDENTICAL" if not problems else "DIFFERENT"
        print(f"{status}  {os.path.basename(x)}: {n} functions, {'same order' if same_order else 'order differs'}" + "".join("\n    " + p for p in problems[:8]))
        bad += bool(problems)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
