"""CPU tests of the host logic that decides what every DiT GEMM launches: the tile choice (csrc/gemm_tiles.h: sat_gemm_route) and the
persistent schedule of the 8-phase kernel (csrc/ph8_sched.h).  Both headers are plain C++17; tests/host/gemm_host_dump.cpp is compiled
with the host compiler in tmp_path and run as a subprocess.  No GPU."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host", "gemm_host_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_routes.json")
HIPCC = "/opt/rocm/bin/hipcc"


def _host_cxx():
    gxx = shutil.which("g++")
    if gxx:
        return [gxx, "-std=c++17"]
    if os.path.exists(HIPCC):
        return [HIPCC, "-x", "c++", "-std=c++17"]
    return None


needs_cxx = pytest.mark.skipif(_host_cxx() is None, reason="neither g++ nor hipcc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_host") / "gemm_host_dump")
    subprocess.run(_host_cxx() + ["-O2", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, DRIVER, "-o", exe], check=True, capture_output=True)
    return exe


# ---- the cases of the route fixture: generated from the fixture's own "grids" (tests/golden/gemm_routes.json), in this order ----
CASE_FIELDS = ("epi", "M", "N", "K", "fp8", "h8", "ln", "gate", "slab", "heads", "xattn", "variant", "f16", "cus")
POLICY_BITS = {0: 0, 22: 1 << 24, 81: 2 << 24, 82: 3 << 24}


def route_cases(grids):
    """Each grid is a dict of lists (cross product, in CASE_FIELDS order; missing fields are [0]) with `tile`, `policy` and `bit23` combined
    into the variant word.  A case that sat_launch_gemm refuses before it chooses (K not a multiple of 64, or of 128 with e4m3 operands;
    e4m3 operands in the fp16 build; LayerNorm fold with e4m3 operands) is left out."""
    out = []
    for g in grids:
        names = CASE_FIELDS[:11] + ("tile", "policy", "bit23", "f16", "cus")
        for vals in itertools.product(*[g.get(n, [0]) for n in names]):
            c = dict(zip(names, vals))
            if c["K"] % (128 if c["fp8"] else 64) or c["N"] % 128 or (c["fp8"] and (c["f16"] or c["ln"])):
                continue
            c["variant"] = c["tile"] | POLICY_BITS[c["policy"]] | (c["bit23"] << 23)
            out.append(tuple(c[f] for f in CASE_FIELDS))
    return out


def run_routes(exe, cases, splits=False):
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    return subprocess.run([exe, "routes"] + (["splits"] if splits else []), input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


ALPHABET = "".join(chr(c) for c in range(48, 123) if chr(c) not in "\\\"")


@needs_cxx
def test_route_is_the_recorded_choice(driver):
    """Every entry of tests/golden/gemm_routes.json -- what the dispatcher of the commit named there launched, recorded from its own code --
    is reproduced by sat_gemm_route: kernel family and template arguments, or the error code."""
    fx = json.load(open(GOLDEN))
    cases = route_cases(fx["grids"])
    assert len(cases) == len(fx["codes"]) and len(cases) > 50000
    got = run_routes(driver, cases)
    assert len(got) == len(cases)
    want = [fx["results"][ALPHABET.index(ch)] for ch in fx["codes"]]
    wrong = [(dict(zip(CASE_FIELDS, c)), w, g) for c, w, g in zip(cases, want, got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(cases)} differ, first: {wrong[:5]}"
    # the fixture exercises every family, the e4m3 flavours, the 8-phase route and the errors
    kinds = {r.split()[0] for r in fx["results"]}
    assert kinds == {"pipe", "cfg", "ph8", "err"}, kinds


def _route(driver, epi, M, N, K, cus=256, heads=24, slab=1, splits=False, **kw):
    c = dict(dict.fromkeys(CASE_FIELDS, 0), epi=epi, M=M, N=N, K=K, cus=cus, heads=heads, slab=slab, **kw)
    return run_routes(driver, [tuple(c[f] for f in CASE_FIELDS)], splits)[0]


# template arguments of the tiles by id (gemm_tiles.h): BM BN BK WM WN NS . FP8 KG DIL
PIPE = {16: "128 64 64 4 1 3 {e} 0 1 1", 22: "256 256 64 4 4 2 {e} 0 1 0", 30: "256 192 64 4 3 2 {e} 0 1 0", 49: "128 128 64 2 2 2 {e} 0 2 0"}
F32, RESID, SWIGLU, HEADS = 0, 1, 2, 3


@needs_cxx
@pytest.mark.parametrize("m,to_qkv,to_out,cross_q,cross_out,ff_in,ff_out", [
    (2050, 30, 49, 16, 16, "ph8", 49),                  # 1 prompt (CFG: 2 x 1025 rows)
    (16400, "ph8", 22, "ph8", 22, "ph8", "ph8"),        # 8 prompts
    (12290, "ph8", 30, 30, 30, "ph8", "ph8"),           # SA-2.0 (2 x 6145), cross-attention over all rows
], ids=["one_prompt", "eight_prompts", "sa2"])
def test_documented_choices(driver, m, to_qkv, to_out, cross_q, cross_out, ff_in, ff_out):
    """The rows of DESIGN.md 4.1 / 4.2: 16-bit operands, 256 CUs, default policy, slab workspace present."""
    def expect(tile, epi):
        return f"ph8 {epi} 0 1 1 4 4 0 0" if tile == "ph8" else "pipe " + PIPE[tile].format(e=epi)

    mx = m if m == 12290 else m // 2          # cross-attention rows: the conditional half of the CFG batch
    assert _route(driver, HEADS, m, 4608, 1536, ln=1) == expect(to_qkv, HEADS)
    assert _route(driver, RESID, m, 1536, 1536) == expect(to_out, F32)
    assert _route(driver, HEADS, mx, 1536, 1536, ln=1) == expect(cross_q, HEADS)
    assert _route(driver, RESID, mx, 1536, 1536) == expect(cross_out, F32)
    assert _route(driver, SWIGLU, m, 12288, 1536, ln=1) == expect(ff_in, SWIGLU)
    assert _route(driver, RESID, m, 1536, 6144) == expect(ff_out, F32)
    if ff_out == "ph8":
        # "8-phase, split" at the SA-2.0 shape only (K >= 4096 behind a whole round, every remainder tile >= 2 parts): the score's assumption
        # (GemmRoute::splits) and the schedule the launch then builds agree; without slab workspace neither splits
        split = int(m == 12290)
        assert _route(driver, RESID, m, 1536, 6144, splits=True) == expect(ff_out, F32) + f" splits={split} schedule.split={split}"
        assert "split=1" not in _route(driver, RESID, m, 1536, 6144, slab=0, splits=True) and "splits=1" not in _route(driver, RESID, m, 1536, 6144, slab=0, splits=True)


@needs_cxx
def test_schedule_is_an_exact_cover(driver):
    """For cus x M x N x K x output x split mode x balanced rounds x geometry (72 000 schedules) the driver builds the schedule and walks every
    workgroup as the kernel does: xcd_remap is a bijection, every piece lies in the tile space, every (tile, 128-k unit) is covered exactly
    once, unsplit schedules hand out whole tiles only, a workgroup of a split schedule holds at most one partial tile and the workgroups of
    remainder tile j are first .. first + parts - 1 of ph8_tile_parts.  No schedule of the grid is refused."""
    p = subprocess.run([driver, "sched"], capture_output=True, text=True)
    summary = p.stdout.strip().split("\n")[-1].split()
    assert summary[0::2] == ["cases", "split", "refused", "failures"], p.stdout[-2000:]
    cases, split, refused, failures = map(int, summary[1::2])
    assert failures == 0 and p.returncode == 0, p.stdout[-4000:]
    assert refused == 0
    assert cases == 72000 and split > 1000


# ---- the ring tiles' geometry (csrc/gemm_ring_geom.h), which gemm_pipe_kernel and launch_pipe both read ----
def _ring(exe):
    rows = []
    for line in subprocess.run([exe, "ring"], check=True, capture_output=True, text=True).stdout.strip().split("\n"):
        rows.append({k: int(v) for k, v in (f.split("=") for f in line.split())})
    return rows


def _one(rows, tile, epix, f8=0):
    got = [r for r in rows if (r["tile"], r["epix"], r["f8"]) == (tile, epix, f8)]
    assert len(got) == 1, (tile, epix, f8)
    return got[0]


HEADS_QKN, ACT16 = 4, 5


@needs_cxx
def test_ring_geometry_of_every_built_tile(driver):
    """RingGeom of every (ring tile, epilogue, operand flavour) that launch_epi / launch_flavour build.  The values are those of the
    expressions gemm_pipe_kernel and launch_pipe each had of their own before the struct (commit 18f5687): the launch's dynamic LDS bytes,
    the wave-load split, the in-loop DMA pieces, the offsets behind the ring."""
    rows = _ring(driver)
    # 4 tiles x (3 epilogues x 3 flavours + MXFP8 A + qk_norm + plain activation) + tiles 44, 49 (fp32) + tile 256 (heads, qk_norm)
    assert len(rows) == 4 * 12 + 2 + 2 and len({(r["tile"], r["epix"], r["f8"]) for r in rows}) == len(rows)
    for r in rows:
        assert r["LDS"] <= 160 * 1024 and r["XA_LDS"] <= 160 * 1024, r
        assert (r["D"] - 1) * r["LPT"] < 64, r          # the counted vmcnt waits fit the 6-bit immediate
        f32, mxa = r["EPI"] == F32, r["f8"] == 3
        assert r["ORI"] == (0 if f32 or mxa else 1 if r["EPI"] == SWIGLU else 2), r
        assert r["EPI"] == {HEADS_QKN: HEADS, ACT16: SWIGLU}.get(r["epix"], r["epix"]) and r["QKN"] == (r["epix"] in (HEADS_QKN, ACT16)), r
        # the launcher's LDS is the kernel's: NS stages, then the LayerNorm constants where the build has them; the cross-attention tiles behind both
        bm, bn = r["TILE_M"], r["TILE_N"]
        assert r["STAGE_BYTES"] == r["KGROUPS"] * ((bm + bn) * 128 + mxa * bm * 4) and r["LN_OFF"] == r["STAGES"] * r["STAGE_BYTES"], r
        assert r["LDS"] == r["LN_OFF"] + r["LN_CONS"] * (bm + bn) * 8 and r["NT"] == 64 * r["NW"], r
        assert r["XA_LDS"] == (r["XA_OFF"] + 3 * 16384 if r["XA_OK"] else r["LDS"]), r
        assert r["XA_OFF"] % 1024 == 0 and r["XA_OFF"] >= r["LDS"], r
        assert r["WL"] == r["WLG"] * (2 if r["tile"] == 49 else 1) and r["UNIFORM"] == (r["WL"] % r["NW"] == 0), r
        assert r["N_FULL"] == r["WL"] - (r["LPT"] - 1) * r["NW"] and 0 < r["N_FULL"] <= r["NW"], r
        # the fused cross-attention epilogue: the heads builds of the 128 x 64 geometry (tile 256, and tile 16 whose kernel carries it
        # too -- both the kernel's and the launcher's expression said so) with 16-bit operands, and no other
        assert r["XA_OK"] == (r["tile"] in (16, 256) and r["EPI"] == HEADS and r["f8"] == 0), r
        assert r["S16"] == (r["f8"] == 0 and ((f32 and r["NT"] == 512) or (r["epix"] == HEADS and r["NT"] == 768))), r

    t30 = _one(rows, 30, HEADS)          # 256 x 192 on 12 waves: the ragged tile
    assert (t30["WL"], t30["LPT"], t30["N_FULL"], t30["UNIFORM"], t30["NW"]) == (56, 5, 8, 0, 12)
    assert t30["LDS"] == 2 * 57344 + 448 * 8 == 118272 and t30["S16"] == 1 and _one(rows, 30, HEADS_QKN)["S16"] == 0

    t49 = _one(rows, 49, F32)            # two K-groups: the exchange and staging areas fit the ring exactly
    assert t49["STAGE_BYTES"] == 65536 and t49["LDS"] == 131072 == 2 * t49["NW"] * 8192 and t49["KG_STAGING_OFF"] == 65536
    # (every wave issues LPT = 64 wave-loads / 8 waves = 8 pieces in the loop body, all of them in the one 32-k step in front of the
    # mid-iteration barrier: `DIL_PER == 8 && NM == 16` in the 16 x 16 x 32 fragment loop.  4 is DIL_PER of the 32 x 32 x 16 build, below)
    assert (t49["LPT"], t49["NDIL"], t49["DIL_STEPS"], t49["DIL_PER"], t49["S16"], t49["PRE_RESID"]) == (8, 8, 1, 8, 1, 1)

    assert _one(rows, 44, F32)["LDS"] == 4 * 32768 == 131072
    t15 = _one(rows, 15, F32)
    assert t15["LDS"] == 3 * 32768 == 98304 and t15["S16"] == 1 and t15["PRE_RESID"] == 1
    assert all(_one(rows, 15, F32, f8)["S16"] == 0 and _one(rows, 15, F32, f8)["LDS"] == 98304 + (f8 == 3) * 3 * 128 * 4 for f8 in (1, 2, 3))

    t22 = _one(rows, 22, SWIGLU)
    assert t22["LDS"] == 2 * 65536 + 512 * 8 == 135168 and t22["NT"] == 1024 and t22["PRE_RESID"] == 0
    mx = _one(rows, 22, F32, 3)          # MXFP8 A operand: + one scale dword per A row per stage
    assert (mx["STAGE_BYTES"], mx["LDS"], mx["SCALE_WAVES"], mx["MXA"]) == (66560, 133120, 4, 1)

    xa = _one(rows, 256, HEADS)          # cross-attention: ring, LayerNorm constants, rounded up to 1 KiB, three 16-KiB K / V^T tiles
    assert xa["XA_OFF"] == 75776 and xa["XA_LDS"] == 75776 + 3 * 16384 == 124928 and xa["LDS"] == 3 * 24576 + 192 * 8 and xa["DIL_ON"] == 0
    t16 = _one(rows, 16, HEADS)          # the same geometry with the pieces in the MFMA stream (16-bit operands only)
    assert (t16["DIL_ON"], t16["NDIL"], t16["DIL_STEPS"], t16["DIL_PER"]) == (1, 6, 3, 2) and _one(rows, 16, HEADS, 1)["DIL_ON"] == 0
    # LayerNorm constants: 16-bit SwiGLU / heads builds only, (BM + BN) * 8 bytes behind the ring
    for r in rows:
        assert r["LN_CONS"] == (r["EPI"] in (SWIGLU, HEADS) and r["f8"] == 0), r
    assert t30["LDS"] - t30["LN_OFF"] == 448 * 8 and t22["LDS"] - t22["LN_OFF"] == 512 * 8 and t15["LDS"] == t15["LN_OFF"]


@needs_cxx
def test_ring_geometry_of_the_32x32_build(tmp_path):
    """-DSAT_RING_MFMA_32X32 (A/B builds): no tile on the 16 x 16 x 32 MFMA; the K-group tile spreads its pieces over two 16-k steps."""
    exe = str(tmp_path / "gemm_host_dump_32")
    subprocess.run(_host_cxx() + ["-O2", "-Wall", "-Wno-unknown-pragmas", "-DSAT_RING_MFMA_32X32", "-I", CSRC, DRIVER, "-o", exe], check=True, capture_output=True)
    rows = _ring(exe)
    assert not any(r["S16"] for r in rows) and all(r["MB"] == 1 for r in rows)
    t49 = _one(rows, 49, F32)
    assert (t49["NDIL"], t49["DIL_STEPS"], t49["DIL_PER"], t49["LDS"]) == (8, 2, 4, 131072)


@needs_cxx
@pytest.mark.parametrize("header", ["gemm_tiles.h", "ph8_sched.h", "gemm_ring_geom.h"])
def test_headers_compile_alone_with_the_host_compiler(header, tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text(f'#include "{header}"\nint main() {{ return 0; }}\n')
    subprocess.run(_host_cxx() + ["-Wall", "-Wno-unknown-pragmas", "-fsyntax-only", "-I", CSRC, str(src)], check=True, capture_output=True)
