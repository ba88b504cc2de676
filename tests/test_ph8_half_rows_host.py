"""CPU tests of the half-row schedule of the 8-phase GEMM (csrc/ph8_sched.h: ph8_half_rows_ints): every workgroup one full 256 x 256 tile and
at most one half tile (128 rows), the M tail of <= 16 rows on "extended" half tiles.  tests/host/ph8_half_rows_dump.cpp is compiled with the
host compiler and walks every workgroup as the kernel does.  No GPU."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "friendly-stable-audio-tools_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host", "ph8_half_rows_dump.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SWIGLU16, F32OUT, E4M3 = 0, 1, 2


def _host_cxx():
    gxx = shutil.which("g++")
    if gxx:
        return [gxx, "-std=c++17"]
    if os.path.exists(HIPCC):
        return [HIPCC, "-x", "c++", "-std=c++17"]
    return None


pytestmark = pytest.mark.skipif(_host_cxx() is None, reason="neither g++ nor hipcc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ph8_half_rows") / "ph8_half_rows_dump")
    subprocess.run(_host_cxx() + ["-O2", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", CSRC, DRIVER, "-o", exe], check=True, capture_output=True)
    return exe


def run(exe, cases):
    """cases: (cus, M, N, K, kind, off) -> one list of words per case"""
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(out) == len(cases)
    return [line.split() for line in out]


def eligible(cus, M, N, K):
    """The rule, restated: 16-bit SwiGLU is the caller's part.  Tail 0 or <= 16 rows; G < t <= 1.5 G full tiles; S = t - G row tiles are cut in
    two, but with a tail at least one per column (its extended half tile), and 2 S half tiles must not outnumber the G workgroups."""
    if M < 256 or N % 256 or K % 128 or M % 256 > 16:
        return None
    t, tiles_n = (M // 256) * (N // 256), N // 256
    if not (cus < t and 2 * t <= 3 * cus):
        return None
    S = max(t - cus, tiles_n if M % 256 else 0)
    if 2 * S > cus:
        return None
    return cus, t - S, 2 * S, tiles_n if M % 256 else 0


def old_schedule(cus, M, N):
    """ph8_schedule_ints for an unsplit 256 x 256 launch, restated from its rule (balanced rounds included): what the parent answered."""
    tiles_m, tail, tiles_n = -(-M // 256), M % 256, N // 256
    light = int(tail != 0 and tail <= 64 and tiles_m > 1)
    t_full, t_light = (tiles_m - light) * tiles_n, light * tiles_n
    t_all = t_full + t_light
    G = min(cus, t_all)
    if G < t_all <= 2 * G:
        G = (t_all + 1) // 2
    dp = t_full // G
    rem0 = dp * G
    sk = t_all - rem0
    return [G, dp, rem0, sk, sk // G if sk else 0, sk % G if sk else 0, light, 0, tiles_m - light, tiles_n]


CUS = [256, 304, 64, 8]
MS = [256, 257, 272, 273, 511, 512, 528, 768, 1025, 1538, 2048, 2050, 2064, 2065, 2304, 2305, 3075, 4100, 16400]
NS = [256, 512, 1536, 4608, 11008, 12288]
KS = [128, 256, 384, 1536]


def test_flagship_shape(driver):
    """FF-in at one prompt on 256 CUs: 256 full + 256 half tiles, the 48 last ones of their columns extended; no light tile."""
    assert run(driver, [(256, 2050, 12288, 1536, SWIGLU16, 0)]) == [["hr", "256", "256", "256", "48"]]
    assert eligible(256, 2050, 12288, 1536) == (256, 256, 256, 48)


def test_schedule_is_an_exact_cover_within_one_and_a_half_tiles(driver):
    """Over cus x M x N x K: where the rule applies the driver has walked every workgroup (xcd_remap a bijection, every (16-row block with valid
    rows, column tile) covered exactly once, no block without valid rows, at most one full plus one (extended) half tile per workgroup) and
    reports the tile counts of the rule; where it does not apply the launch gets the pre-existing schedule."""
    cases = [(c, m, n, k, SWIGLU16, 0) for c, m, n, k in itertools.product(CUS, MS, NS, KS)]
    assert (256, 2050, 12288, 1536, SWIGLU16, 0) in cases
    got = run(driver, cases)
    n_hr = 0
    for c, g in zip(cases, got):
        want = eligible(*c[:4])
        if want is None:
            assert g == ["old"] + [str(v) for v in old_schedule(c[0], c[1], c[2])], (c, g)
        else:
            assert g == ["hr"] + [str(v) for v in want], (c, g)
            n_hr += 1
    assert n_hr >= 40, n_hr          # the grid does exercise the rule: with and without tail, t - G above and below tiles_n


@pytest.mark.parametrize("case,why", [
    ((256, 2048 + 17, 12288, 1536, SWIGLU16, 0), "tail of 17 rows"),
    ((256, 2048 + 64, 12288, 1536, SWIGLU16, 0), "tail of 64 rows"),
    ((256, 2048 + 255, 12288, 1536, SWIGLU16, 0), "tail of 255 rows"),
    ((256, 2050, 8192, 1536, SWIGLU16, 0), "t = 256 <= G: one round"),
    ((256, 1025, 12288, 1536, SWIGLU16, 0), "t = 192 <= G"),
    ((256, 2306, 12288, 1536, SWIGLU16, 0), "t = 432 > 1.5 G"),
    ((256, 2050, 12288, 1536, F32OUT, 0), "fp32 output"),
    ((256, 2050, 12288, 1536, E4M3, 0), "e4m3 operands"),
    ((256, 2050, 12288, 1536, SWIGLU16, 1), "switched off (variant bit 27)"),
])
def test_refused_cases_get_the_previous_schedule(driver, case, why):
    g = run(driver, [case])[0]
    assert g == ["old"] + [str(v) for v in old_schedule(case[0], case[1], case[2])], (why, g)


def test_previous_schedule_of_the_flagship_is_the_recorded_one(driver):
    """The literal numbers of the balanced rounds this schedule replaces (2 x 216 workgroups, 384 full + 48 light tiles), so that the
    restatement above cannot drift together with the header."""
    g = run(driver, [(256, 2050, 12288, 1536, SWIGLU16, 1)])[0]
    assert g == ["old", "216", "1", "216", "216", "1", "0", "1", "0", "8", "48"]
