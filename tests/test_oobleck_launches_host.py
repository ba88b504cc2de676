"""CPU test of the Oobleck codec's launch path (csrc/oobleck_plan.hip: weight set-up at finalize, workspace, decode / encode, range report,
sat_oobleck_unit; and the launchers of csrc/oobleck.hip in its three builds).  The codec objects are compiled host-only and linked against
tests/host/oobleck_launch_dump.cpp, which is the HIP runtime: allocations and copies work on host memory, and every kernel launch prints its
kernel name with template arguments, grid, block, LDS bytes and every argument, behind a line "build <bf16|f16|f32>" wherever the build changes.
tests/golden/oobleck_launches.json.gz (read it with zcat) holds what the codec of the commit named there did for every case of the driver:
each launch, every arena / workspace offset, every return code and error text.  The driver links against a commit whose codec is still one file as well, which is how the fixture was recorded from the commit before
the plan was split off.  No GPU.

    python tests/test_oobleck_launches_host.py --record <commit> [--csrc <csrc of a checkout of that commit>]
        rewrites the fixture from that csrc (default: the working tree's; a refactor never re-records)"""
import gzip
import io
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host", "oobleck_launch_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "oobleck_launches.json.gz")
HIPCC, CLANG = "/opt/rocm/bin/hipcc", "/opt/rocm/lib/llvm/bin/clang++"
BUILDS = (("bf16", []), ("f16", ["-DSAT_OPERAND_F16"]), ("f32", ["-DSAT_OPERAND_F32"]))


def dump(workdir, extra=(), csrc=CSRC):
    """{case name: [lines]} of the driver linked against the codec of `csrc`, built in `workdir`."""
    cc = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "--cuda-host-only", *extra]
    obj = lambda n: os.path.join(str(workdir), n)
    units = [(obj(f"oobleck_{b}.o"), ["-I", csrc, *defs, "-c", os.path.join(csrc, "oobleck.hip")]) for b, defs in BUILDS]
    kernel_objs = [o for o, _ in units]
    if os.path.exists(os.path.join(csrc, "oobleck_plan.hip")):          # (a commit without it keeps its plan in oobleck.hip)
        units.append((obj("oobleck_plan.o"), ["-I", csrc, "-c", os.path.join(csrc, "oobleck_plan.hip")]))
    # the driver reads ConvArgs from this tree's header, whichever commit's codec it links against: the layout is fixed (oobleck_kernels.h)
    units.append((obj("oobleck_launch_dump.o"), ["-I", CSRC, "-Wall", "-Wno-unused-function", "-x", "hip", "-c", DRIVER]))
    jobs = [subprocess.Popen(cc + args + ["-o", o], stderr=subprocess.PIPE, text=True) for o, args in units]
    for j in jobs:          # the translation units side by side
        err = j.communicate()[1]
        assert j.returncode == 0, err
    # no HIP runtime on the link line: the driver is the runtime.  Each kernel object refers to its device code as __hip_fatbin_<hash>; there is
    # none here, and the address given instead tells the driver which build a kernel was registered by: 1 bf16, 2 fp16, 3 fp32
    defsyms = []
    for i, o in enumerate(kernel_objs):
        syms = re.findall(r"\b__hip_fatbin_\w+", subprocess.run(["nm", "-u", o], check=True, capture_output=True, text=True).stdout)
        assert len(syms) == 1, (o, syms)
        defsyms.append(f"-Wl,--defsym,{syms[0]}={i + 1}")
    assert len(set(defsyms)) == len(BUILDS), defsyms
    link = CLANG if os.path.exists(CLANG) else shutil.which("g++")          # hipcc's own clang: it also links what `extra` asks for (sanitizers)
    exe = obj("oobleck_launch_dump")
    subprocess.run([link] + list(extra) + [o for o, _ in units] + defsyms + ["-lm", "-o", exe], check=True, capture_output=True)
    cases, name = {}, None
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]:
        if ln.startswith("== "):
            name = ln[3:]
            cases[name] = []
        else:
            cases[name].append(ln)
    return cases


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_launches_are_the_recorded_ones(tmp_path):
    """Every case of the fixture: the same lines in the same order."""
    fx = json.load(gzip.open(GOLDEN, "rt"))
    got = dump(tmp_path)
    assert list(got) == list(fx["cases"])
    for name, codes in fx["cases"].items():
        want = [fx["lines"][i] for i in codes]
        first = next((i for i, (w, g) in enumerate(zip(want, got[name])) if w != g), min(len(want), len(got[name])))
        assert got[name] == want, f"{name}: {len(got[name])} lines, recorded {len(want)}; first difference at line {first}:\n  recorded {want[first:first + 1]}\n  got      {got[name][first:first + 1]}"
    # the fixture reaches what it is there for: every case stays in the build of its format; both convolution tiles and ring depths of each build,
    # the fused unit in its four instantiations, both forms of the first convolution, every packing kernel, the range statistics, every error code
    text = "\n".join(fx["lines"])
    launched = {}
    for fmt, build in (("bf16", "bf16"), ("fp16", "f16"), ("fp32", "f32")):
        mine = {name: [fx["lines"][i] for i in codes] for name, codes in fx["cases"].items() if name.endswith("_" + fmt)}
        assert len(mine) >= 7, fmt
        for name, lines in mine.items():
            assert {ln for ln in lines if ln.startswith("build ")} == {"build " + build}, name
        launched[fmt] = {ln.split()[1] for lines in mine.values() for ln in lines if ln.startswith("launch ")}
    tiles16 = {"conv_pipe_kernel<128,128,4,2,3>", "conv_pipe_kernel<128,128,4,2,2>", "conv_pipe_kernel<256,64,8,1,3>", "conv_pipe_kernel<256,64,8,1,2>"}
    fused = {"ru_fused_kernel<128,4,2,2,0>", "ru_fused_kernel<128,4,2,2,1>", "ru_fused_kernel<256,2,4,3,0>", "ru_fused_kernel<256,2,4,3,1>"}
    small = {"first_conv_kernel<true>", "first_conv_kernel<false>", "cf_to_cl_kernel", "wn_invnorm_kernel", "wn_pack_conv_kernel", "wn_pack_convT_kernel",
             "wn_pack_nearest_kernel", "wn_fold_f32_kernel", "snake_params_kernel"}
    assert launched["bf16"] == tiles16 | fused | small and launched["fp16"] == tiles16 | fused | small
    assert launched["fp32"] == {"conv_pipe_kernel<128,128,4,2,2>", "conv_pipe_kernel<128,64,4,1,2>"} | small
    for needle in ("sat_ensure_dynamic_lds conv_pipe_kernel<128,128,4,2,2> 131072", "range_stats ws+", "hipDeviceSynchronize"):
        assert needle in text, needle
    assert not any(" unknown" in ln or "unregistered" in ln for ln in fx["lines"] if ln.startswith(("launch ", "range_stats ", "hip", "sat_ensure"))), "a pointer outside every named range"
    assert "build ?" not in fx["lines"]
    for code in (-1, -2, -3, -4, -5):
        assert any(re.match(r"rc \w+ %d$" % code, ln) for ln in fx["lines"]), code
    assert len(fx["cases"]) >= 35 and len(fx["commit"]) >= 7


if __name__ == "__main__":
    import argparse
    import tempfile

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", required=True, metavar="COMMIT")
    ap.add_argument("--csrc", default=CSRC)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        cases = dump(d, csrc=os.path.abspath(args.csrc))
    lines = sorted({ln for v in cases.values() for ln in v})
    index = {ln: i for i, ln in enumerate(lines)}
    # one line of text per distinct output line and per case, gzipped (a few thousand lines of recorded text); no time stamp, so the same lines give the same file
    with open(GOLDEN, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as gz, io.TextIOWrapper(gz, encoding="utf-8") as f:
        about = "tests/host/oobleck_launch_dump.cpp linked against csrc/oobleck*.hip of `commit`; cases[name] indexes lines"
        f.write('{"commit": %s, "about": %s, "lines": [\n' % (json.dumps(args.record), json.dumps(about)) + ",\n".join(map(json.dumps, lines)) + '\n], "cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps([index[ln] for ln in v], separators=(',', ':'))}" for k, v in cases.items()) + "\n}}\n")
