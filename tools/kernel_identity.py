"""Are the kernels of one source file the same in two trees?  Compiles the file device-only to assembly in both (the Makefile's flags, each
operand build the Makefile gives the file) and compares kernel by kernel: the instruction stream with symbol names replaced by their
demangled, namespace-free form, and the resource metadata.  A plain diff of two compilations; developer tool, no GPU.

usage: python tools/kernel_identity.py [--rename old=new]... [--define NAME]... <parent tree's csrc> [file.hip]      (default oobleck.hip;
exit code 1 when a kernel differs; --rename: the parent's kernel `old`, named as the table prints it, is compared with the branch's kernel
`new`; --define: -DNAME on every compilation, e.g. SAT_GEMM_EXPERIMENTS for the `make exp` objects or SAT_RING_MFMA_32X32)"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
HIPCC, FILT = "/opt/rocm/bin/hipcc", "c++filt"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--cuda-device-only", "-S"]
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size")


def builds_of(src):
    """the operand builds the Makefile compiles `src` in: bf16 always, fp16 for the files of DUAL, fp32 for those of TRIPLE"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    listed = lambda var: src in re.search(r"^%s\s*=(.*)$" % var, mk, re.M).group(1).split()
    res = {"bf16": []}
    if listed("DUAL"):
        res["fp16"] = ["-DSAT_OPERAND_F16"]
    if listed("TRIPLE"):
        res["fp32"] = ["-DSAT_OPERAND_F32"]
    return res


def plain(names):
    """mangled -> demangled without namespaces and without the parameter list"""
    # (binutils' c++filt predates the DF16_ spelling of _Float16; the parameter list is dropped anyway)
    out = subprocess.run([FILT], input="\n".join(n.replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for m, d in zip(names, out):
        d = re.sub(r"\((anonymous namespace)\)::|\b(bf16|f16|f32)::", "", d)
        res[m] = re.sub(r"^void ", "", d).split("(")[0]
    return res


def kernels(csrc, src, defs, workdir, rename={}):
    """{kernel: (instruction lines, {metadata})} of one compilation"""
    out = os.path.join(workdir, "k.s")
    cmd = [HIPCC, *FLAGS, *defs, os.path.join(csrc, src), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    names = {m: rename.get(d, d) for m, d in plain(sorted(set(re.findall(r"\b_Z\w+", text)))).items()}
    # (basic-block labels carry the function's position in the file, which a renamed kernel need not keep)
    sub = lambda s: re.sub(r"\bL?BB\d+_", "BB_", re.sub(r"\b_Z\w+", lambda m: names[m.group(0)], s))
    meta = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[names[name]] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in META}
    res = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @.*?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        if names[m.group(1)] in meta:
            res[names[m.group(1)]] = ([sub(ln) for ln in m.group(2).split("\n")], meta[names[m.group(1)]])
    assert sorted(res) == sorted(meta), (sorted(res), sorted(meta))
    return res, " ".join(cmd[:-3] + ["<csrc>/" + src])


def main():
    argv, rename, defines = sys.argv[1:], {}, []
    while argv and argv[0] in ("--rename", "--define"):
        if argv[0] == "--rename":
            old, new = argv[1].split("=", 1)
            rename[old] = new
        else:
            defines.append("-D" + argv[1])
        argv = argv[2:]
    parent, src = argv[0], argv[1] if len(argv) > 1 else "oobleck.hip"
    bad = 0
    builds = builds_of(src)
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(2 * len(builds)) as pool:
        # the compilations are independent of each other: all of them at once, each into a directory of its own
        jobs = {}
        for build, defs in builds.items():
            for side, csrc, ren in (("old", parent, rename), ("new", CSRC, {})):
                wd = os.path.join(d, build + side)
                os.mkdir(wd)
                jobs[build, side] = pool.submit(kernels, csrc, src, defs + defines, wd, ren)
        done = {k: j.result() for k, j in jobs.items()}
    for build in builds:
        (old, cmd), (new, _) = done[build, "old"], done[build, "new"]
        print(f"== {build}: {cmd}")
        print(f"{'kernel':44s} {'instr':>6s} " + " ".join(f"{k.replace('_segment', '').replace('_fixed_size', '').replace('_count', ''):>10s}" for k in META) + "  stream  metadata")
        same = sorted(old) == sorted(new)
        for k in sorted(set(old) | set(new)):
            if k not in old or k not in new:
                print(f"{k:44s} only in the {'parent' if k in old else 'branch'}")
                continue
            s, m = old[k][0] == new[k][0], old[k][1] == new[k][1]
            same &= s and m
            n = sum(1 for ln in new[k][0] if ln.startswith("\t") and not ln.startswith(("\t.", "\t;")))
            print(f"{k:44s} {n:6d} " + " ".join(f"{new[k][1][f]:10d}" for f in META) + f"  {'same' if s else 'DIFFERS':7s} {'same' if m else 'DIFFERS: parent ' + str(old[k][1])}")
        print(f"{build}: {len(new)} kernels, identical: {'yes' if same else 'NO'}\n")
        bad += not same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
