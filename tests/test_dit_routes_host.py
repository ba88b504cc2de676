"""CPU test of the DiT plan's launch path on the routes tests/test_dit_launches_host.py cannot reach: 128-, 32- and 96-channel heads (the staged
route), causal attention, the range report, the block options, the convolutional feed-forward and patch sizes.  csrc/dit_plan.hip, compiled
host-only, is linked against tests/host/dit_routes_dump.cpp, which adds the launchers that tests/host/dit_launch_dump.cpp leaves null.
tests/golden/dit_route_launches.json holds what the plan of the commit named there did for every case of the driver: each launch with every
argument, every arena / workspace / context offset, every return code and error text.  No GPU.

    python tests/test_dit_routes_host.py --record <commit>      rewrites the fixture from csrc/ and include/ of <commit> (git archive) and the
                                                                working tree's driver; the same command on the same commit gives the same bytes"""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = os.path.join("friendly-stable-audio-tools_amd", "csrc")
CSRC = os.path.join(ROOT, CSRC_REL)
HOST = os.path.join(ROOT, "tests", "host")
DRIVER = os.path.join(HOST, "dit_routes_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dit_route_launches.json")
HIPCC = "/opt/rocm/bin/hipcc"

# the launchers dit_launch_dump.cpp leaves null: every one occurs in the fixture
LAUNCHERS = ("sat_launch_attention_hdw", "sat_launch_head_split_hdw", "sat_launch_attention_causal", "sat_launch_attention_hdw_causal",
             "sat_launch_rope_table_hdw", "sat_launch_range_stats", "sat_launch_dwconv_ln_silu", "sat_launch_round_rows", "sat_launch_silu_f32",
             "sat_launch_ff_conv", "sat_launch_pack_conv_taps", "sat_launch_im2col_rows_f32", "sat_launch_split_heads_f32_w",
             "sat_launch_attention_f32_w", "sat_launch_attention_f32_causal", "glue_fold_in_patch", "glue_fold_out_patch", "glue_input_proj_patch",
             "glue_output_proj_patch")
# what a 64-channel plan with cross-attention as two kernels fills: every slot of sat_dit_range_slot_name
SLOTS = ("a_qkv", "q", "k", "v", "attn_out", "a_cross_q", "cross_q", "cross_k", "cross_v", "cross_attn_out", "a_ff", "ff_hidden")
# case -> (the call that refuses, its code, a piece of the error text)
REFUSALS = {
    "refused_hd32_create_sized": ("sat_dit_plan_create_sized", -2, "32 and 96 through sat_dit_plan_create_ex"),
    "refused_hd32_fp8": ("sat_dit_plan_create_ex", -2, "dim_heads 32 does not run with e4m3"),
    "refused_hd128_fp8": ("sat_dit_plan_create_sized", -2, "dim_heads 128 runs with bf16 or fp16 operands only (gemm_dtype 1)"),
    "refused_hd128_fp32": ("sat_dit_plan_create_sized", -2, "dim_heads 128 runs with bf16 or fp16 operands only (gemm_dtype 2)"),
    "refused_block_options_hd128": ("sat_dit_plan_set_block_options", -2, "with dim_heads 128 is not built"),
    "refused_block_options_hd96": ("sat_dit_plan_set_block_options", -2, "with dim_heads 96 is not built"),
    "refused_ff_conv_hd32": ("sat_dit_plan_set_ff_conv", -2, "with dim_heads 32 is not built"),
    "refused_causal_cross": ("sat_dit_plan_set_attention_options", -2, "causal with cross-attention"),
    "refused_causal_fp8": ("sat_dit_plan_set_attention_options", -2, "causal with gemm_dtype fp8"),
    "refused_range_report_conformer": ("sat_dit_range_report", -2, "no rows for the 16-bit buffers of a plan with conformer"),
    "refused_t_len_not_multiple_of_patch": ("sat_dit_forward", -1, "t_len 13 is not a multiple of patch_size 2"),
}


def dump(workdir, plan_csrc=CSRC):
    """{case name: [lines]} of the driver linked against dit_plan.hip of `plan_csrc`, built in `workdir`."""
    cc = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fPIC", "--cuda-host-only"]
    plan, drv, exe = (os.path.join(str(workdir), n) for n in ("dit_plan.o", "dit_routes_dump.o", "dit_routes_dump"))
    jobs = [subprocess.Popen(cc + ["-I", plan_csrc, "-c", os.path.join(plan_csrc, "dit_plan.hip"), "-o", plan], stderr=subprocess.PIPE, text=True),
            subprocess.Popen(cc + ["-I", CSRC, "-I", HOST, "-Wall", "-Wno-unused-function", "-x", "hip", "-c", DRIVER, "-o", drv], stderr=subprocess.PIPE,
                             text=True)]
    for j in jobs:          # the two translation units side by side
        err = j.communicate()[1]
        assert j.returncode == 0, err
    # no HIP runtime on the link line: the driver is the runtime
    link = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.run([link, plan, drv, "-lm", "-o", exe], check=True, capture_output=True)
    cases, name = {}, None
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]:
        if ln.startswith("== "):
            name = ln[3:]
            cases[name] = []
        else:
            cases[name].append(ln)
    return cases


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_route_launches_are_the_recorded_ones(tmp_path):
    """Every case of the fixture: the same lines in the same order."""
    fx = json.load(open(GOLDEN))
    got = dump(tmp_path)
    assert list(got) == list(fx["cases"])
    for name, codes in fx["cases"].items():
        want = [fx["lines"][i] for i in codes]
        first = next((i for i, (w, g) in enumerate(zip(want, got[name])) if w != g), min(len(want), len(got[name])))
        assert got[name] == want, f"{name}: {len(got[name])} lines, recorded {len(want)}; first difference at line {first}:\n  recorded {want[first:first + 1]}\n  got      {got[name][first:first + 1]}"
    # the fixture reaches what it is there for
    recorded = {name: [fx["lines"][i] for i in codes] for name, codes in fx["cases"].items()}
    names = {ln.split()[0] for ln in fx["lines"]}
    for launcher in LAUNCHERS:
        assert launcher in names, launcher
    staged = [ln for ln in fx["lines"] if ln.split()[0] in ("sat_launch_head_split_hdw", "sat_launch_attention_hdw", "sat_launch_attention_hdw_causal")]
    assert any(ln.endswith(" f16 1") for ln in staged) and any(ln.endswith(" f16 0") for ln in staged)
    two_kernels = [ln for ln in recorded["range_fp16_fold_two_kernels"] if ln.startswith("sat_launch_range_stats ")]
    for slot in SLOTS:
        assert any(ln.endswith(" slot " + slot) for ln in two_kernels), slot
    # (the fused to_q + cross-attention launch keeps Q in registers: its slot stays empty)
    fused = [ln for ln in recorded["range_fp16_fold_fused"] if ln.startswith("sat_launch_range_stats ")]
    assert fused and not any(ln.endswith(" slot cross_q") for ln in fused)
    for name, (call, rc, text) in REFUSALS.items():
        lines = recorded[name]
        assert f"rc {call} {rc}" in lines and any(ln.startswith("error:") and text in ln for ln in lines), (name, lines[:6])
    # ... and every other case runs: its forward returns 0
    for name, lines in recorded.items():
        assert name in REFUSALS or "rc sat_dit_forward 0" in lines, name
    assert len(fx["cases"]) >= 50 and len(fx["commit"]) >= 7


if __name__ == "__main__":
    import tempfile

    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    commit = sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", commit, CSRC_REL, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        cases = dump(d, plan_csrc=os.path.join(d, CSRC_REL))
    lines = sorted({ln for v in cases.values() for ln in v})
    index = {ln: i for i, ln in enumerate(lines)}
    with open(GOLDEN, "w") as f:          # one line of text per distinct output line and per case
        about = "tests/host/dit_routes_dump.cpp linked against csrc/dit_plan.hip of `commit`; cases[name] indexes lines"
        f.write('{"commit": %s, "about": %s, "lines": [\n' % (json.dumps(commit), json.dumps(about)) + ",\n".join(map(json.dumps, lines)) + '\n], "cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps([index[ln] for ln in v], separators=(',', ':'))}" for k, v in cases.items()) + "\n}}\n")
