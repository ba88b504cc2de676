// Host driver of tests/test_ph8_half_rows_host.py: the half-row schedule of the 8-phase GEMM (csrc/ph8_sched.h: ph8_half_rows_ints) on the CPU.
// Plain C++17, no HIP.  One case per stdin line:  cus M N K kind off
//   kind 0 = SwiGLU epilogue with 16-bit operands, 1 = fp32-output epilogue, 2 = SwiGLU with e4m3 operands; off = the A/B switch
//   (SAT_VARIANT_HALF_ROWS_OFF).  The launcher (launch_ph8, gemm_ph8.hip) asks ph8_half_rows_ints first and ph8_schedule_ints when it refuses.
// Output per case:
//   hr G full half extended            the schedule applies and every check below holds
//   old G dp_rounds rem0 sk_tiles sk_q sk_r light split tiles_m_full tiles_n     refused: what ph8_schedule_ints then answers
//   FAIL <what>
#include <stdio.h>

#include <vector>

#include "gemm_tiles.h"

struct HrPiece {
    int m0, tn;
    bool half, ext;
};

// The walk of workgroup wgi under the half-row schedule: the `sc.hr` branch of the `next_seg` lambda of gemm_ph8_kernel restated -- change both
// together.
static void hr_walk(const Ph8Sched& sc, int wgi, std::vector<HrPiece>& out) {
    if (ph8_hr_has_full(sc, wgi)) {
        int tm, tn;
        ph8_hr_full_of(sc, wgi, tm, tn);
        out.push_back(HrPiece{tm * 256, tn, false, false});
    }
    const int j = ph8_hr_half_index(sc, wgi);
    if (j >= 0) {
        int r0, tn, ext;
        ph8_hr_half_of(sc, j, r0, tn, ext);
        out.push_back(HrPiece{r0, tn, true, ext != 0});
    }
}

static const char* check(const Ph8Sched& sc, int cus, int M, int N, int K, int& n_ext) {
    if (sc.G != cus || sc.tiles_n != N / 256 || sc.nkp != K / 128 || sc.dp_rounds != 0 || sc.sk_tiles != 0 || sc.split != 0) return "header fields";
    const int blocks_m = (M + 15) / 16, tiles_n = sc.tiles_n;
    std::vector<int> cover((size_t)blocks_m * tiles_n, 0), seen(sc.G, 0);
    std::vector<HrPiece> pieces;
    int full = 0, half = 0;
    n_ext = 0;
    for (int bid = 0; bid < sc.G; ++bid) {
        const int wgi = xcd_remap(bid, sc.G);
        if (wgi < 0 || wgi >= sc.G || seen[wgi]++) return "xcd_remap is not a bijection";
        pieces.clear();
        hr_walk(sc, wgi, pieces);
        if (pieces.empty()) return "a workgroup without work";
        int f = 0, h = 0;
        for (const HrPiece& p : pieces) {
            (p.half ? h : f)++;
            if (p.tn < 0 || p.tn >= tiles_n || p.m0 < 0 || p.m0 % 128) return "piece outside the tile space";
            if (!p.half && p.m0 % 256) return "full tile off the 256-row grid";
            // 16-row blocks: 16 of a full tile, 8 of a half tile, + the block at m0 + 128 of an extended one (the kernel gives it to wave row 1)
            const int nb = p.half ? (p.ext ? 9 : 8) : 16;
            for (int b = 0; b < nb; ++b) {
                const int blk = p.m0 / 16 + b;
                if (blk >= blocks_m) return "a block without valid rows";
                ++cover[(size_t)blk * tiles_n + p.tn];
            }
            // what the kernel does NOT mask row by row inside quadrant 0: all 128 / 256 rows of a piece must exist
            if (p.m0 + (p.half ? 128 : 256) > M) return "quadrant-0 rows beyond M";
            n_ext += p.ext;
        }
        if (f > 1 || h > 1) return "more than one full plus one half tile in a workgroup";
        full += f;
        half += h;
    }
    if (full != sc.hr_full || half != sc.hr_half) return "tile counts";
    for (int c : cover)
        if (c != 1) return "a (16-row block, column tile) is not covered exactly once";
    return nullptr;
}

int main() {
    int cus, M, N, K, kind, off;
    while (scanf("%d %d %d %d %d %d", &cus, &M, &N, &K, &kind, &off) == 6) {
        const int Kk = kind == 2 ? K / 2 : K;          // (e4m3: the kernel and its schedule count 16-bit columns, as launch_ph8 does)
        Ph8Sched sc;
        if (ph8_half_rows_ints(M, N, Kk, kind == 0, cus, off != 0, sc)) {
            int n_ext = 0;
            const char* err = check(sc, cus, M, N, Kk, n_ext);
            if (err) printf("FAIL %s\n", err);
            else printf("hr %d %d %d %d\n", sc.G, sc.hr_full, sc.hr_half, n_ext);
        } else {
            if (ph8_schedule_ints(M, N, Kk, 0, kind == 1, 256, 256, 1, cus, true, PH8_BALANCE_TWO_ROUNDS, sc) != 0) {
                printf("FAIL ph8_schedule_ints refused\n");
                continue;
            }
            printf("old %d %d %d %d %d %d %d %d %d %d\n", sc.G, sc.dp_rounds, sc.rem0, sc.sk_tiles, sc.sk_q, sc.sk_r, sc.light, sc.split, sc.tiles_m_full, sc.tiles_n);
        }
    }
    return 0;
}
