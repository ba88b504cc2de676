#!/usr/bin/env python3
"""The table of profiles/parity_gates.txt from the per-assertion log of the sliced parity gates.

    SAT_PARITY_LOG=gates.log python -m pytest tests/test_gpu_kernels.py tests/test_gpu_dit_head_dim.py tests/test_gpu_dit_options.py -m gpu
    python tools/parity_gates_table.py gates.log

tests/util.py writes one line per assert_close_sliced call (test id, assertion name, whole-tensor rel-L2, worst slice and its index, number of
slices, F_ref, gate).  Assertions are grouped by test function, operand format and assertion name with the tile variant and the shape
taken out; every group is shown at the ONE parametrisation whose worst slice comes closest to its gate -- all figures of a row, the
whole-tensor one included, are that parametrisation's, and its test id and logged name close the row."""
import collections
import re
import sys


def main(paths):
    groups = collections.defaultdict(list)
    for path in paths:
        for line in open(path):
            f = line.rstrip("\n").split("\t")
            if len(f) < 8:
                continue
            kv = dict(x.split("=", 1) for x in f[2:8])
            fn = f[0].split("::")[-1]
            base, _, params = fn.partition("[")
            params = params.rstrip("]")
            fmt = "f16" if re.search(r"(^|-)f16($|-)", params) else "bf16" if re.search(r"(^|-)bf16($|-)", params) else "-"
            if base == "test_fp16_range_policy":
                fmt = "f16"
            cls = re.sub(r" v\d+| \d+x\d+(x\d+)*( kv\d+ sk\d+)?|, \d+ keys", "", f[1])
            groups[(f[0].split("::")[0].split("/")[-1], base, cls, fmt)].append((float(kv["worst"]) / float(kv["gate"]), params, kv, f[1]))
    print(f"{'file::test':74s} {'assertion (variant and shape taken out)':80s} {'fmt':5s} {'cases':>5s} {'whole':>9s} {'worst slice':>11s} {'at':>16s} "
          f"{'slices':>7s} {'F_ref':>6s} {'gate':>9s} {'worst/gate':>10s}  parametrisation shown: logged name")
    for (file, base, cls, fmt), v in sorted(groups.items()):
        v.sort(key=lambda r: -r[0])
        ratio, params, kv, name = v[0]
        print(f"{file + '::' + base:74s} {cls:80s} {fmt:5s} {len({r[1] for r in v}):5d} {float(kv['whole']):9.2e} {float(kv['worst']):11.2e} {kv['at']:>16s} "
              f"{kv['slices']:>7s} {float(kv['F_ref']):6.2f} {float(kv['gate']):9.2e} {ratio:10.2f}  [{params}]: {name}")


if __name__ == "__main__":
    main(sys.argv[1:])
