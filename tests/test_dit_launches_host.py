"""CPU test of the DiT plan's launch path (csrc/dit_plan.hip: build, the prepare calls, run_forward).  That file holds no kernel: compiled
host-only and linked against tests/host/dit_launch_dump.cpp -- which defines the HIP runtime calls on host memory and every internal launcher as a
function that prints its arguments -- it runs on the CPU.  tests/golden/dit_launches.json holds what the plan of the commit named there did for
every case of the driver: each launch with every argument, every arena / workspace / context offset, every return code and error text.  No GPU.

    python tests/test_dit_launches_host.py --record <commit>      rewrites the fixture from the working tree's dit_plan.hip (a refactor never does)"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host", "dit_launch_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dit_launches.json")
HIPCC = "/opt/rocm/bin/hipcc"


def dump(workdir, extra=()):
    """{case name: [lines]} of the driver built from the tree's dit_plan.hip in `workdir`."""
    cc = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "--cuda-host-only", "-I", CSRC, *extra]
    plan, drv, exe = (os.path.join(str(workdir), n) for n in ("dit_plan.o", "dit_launch_dump.o", "dit_launch_dump"))
    jobs = [subprocess.Popen(cc + ["-c", os.path.join(CSRC, "dit_plan.hip"), "-o", plan], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(cc + ["-Wall", "-Wno-unused-function", "-x", "hip", "-c", DRIVER, "-o", drv], stderr=subprocess.PIPE, text=True)]
    for j in jobs:          # the two translation units side by side
        err = j.communicate()[1]
        assert j.returncode == 0, err
    # no HIP runtime on the link line: the driver is the runtime
    link = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.run([link] + list(extra) + [plan, drv, "-lm", "-o", exe], check=True, capture_output=True)
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
    fx = json.load(open(GOLDEN))
    got = dump(tmp_path)
    assert list(got) == list(fx["cases"])
    for name, codes in fx["cases"].items():
        want = [fx["lines"][i] for i in codes]
        first = next((i for i, (w, g) in enumerate(zip(want, got[name])) if w != g), min(len(want), len(got[name])))
        assert got[name] == want, f"{name}: {len(got[name])} lines, recorded {len(want)}; first difference at line {first}:\n  recorded {want[first:first + 1]}\n  got      {got[name][first:first + 1]}"
    # the fixture reaches what it is there for: every launcher of the plan, both operand formats, e4m3 in both A-scale forms, fold, fusion, slab, refusals
    text = "\n".join(fx["lines"])
    for needle in ("sat_launch_gemm_f32", "sat_launch_layernorm_fp8", "sat_launch_pack_rows_ln", "sat_launch_quant_rows_fp8", "glue_resid_stats", "glue_add_pos",
                   "glue_input_proj_extra", "glue_adaln_finish", "hipEventRecord", " f16 1 ", " fp8 2 ", " fp8 3 ", "rc sat_dit_forward -5", "rc sat_dit_forward -1",
                   "rc sat_dit_plan_create_sized -2", "rc sat_dit_plan_set_transformer_options -2"):
        assert needle in text, needle
    gemms = [ln for ln in fx["lines"] if ln.startswith("sat_launch_gemm ")]
    assert any(" slab ws+" in ln for ln in gemms) and any(" xa alloc" in ln for ln in gemms) and any(" fold ws+" in ln for ln in gemms)
    assert len(fx["cases"]) >= 30 and len(fx["commit"]) >= 7


if __name__ == "__main__":
    import tempfile

    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    with tempfile.TemporaryDirectory() as d:
        cases = dump(d)
    lines = sorted({ln for v in cases.values() for ln in v})
    index = {ln: i for i, ln in enumerate(lines)}
    with open(GOLDEN, "w") as f:          # one line of text per distinct output line and per case
        about = "tests/host/dit_launch_dump.cpp linked against csrc/dit_plan.hip of `commit`; cases[name] indexes lines"
        f.write('{"commit": %s, "about": %s, "lines": [\n' % (json.dumps(sys.argv[2]), json.dumps(about)) + ",\n".join(map(json.dumps, lines)) + '\n], "cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps([index[ln] for ln in v], separators=(',', ':'))}" for k, v in cases.items()) + "\n}}\n")
