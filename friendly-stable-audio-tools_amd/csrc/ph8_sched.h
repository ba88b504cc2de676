// The persistent schedule of the 8-phase GEMM (gemm_ph8.hip): which tiles and K-ranges each workgroup walks.  Pure integer code in
// closed form, shared by the kernels and the host; plain C++17 without a HIP header, so tests/test_gemm_host.py builds every schedule
// of a grid of shapes on the CPU and checks that the walk covers every (tile, 128-k unit) exactly once.
#pragma once

#ifdef __HIPCC__
#define SAT_HD __host__ __device__ __forceinline__
#else
#define SAT_HD inline
#endif

// (internal linkage on purpose: Ph8Sched is a kernel argument, so its name is part of the kernels' symbols)
namespace {

// XCD-aware bijective remap of a linear workgroup id (guide T1): consecutive logical ids
// land on the same XCD (hardware places block b on XCD b % 8), so neighbouring tiles share
// one L2.  Speed only -- never correctness.
SAT_HD int xcd_remap(int bid, int nwg) {
    const int NX = 8;
    int xcd = bid % NX, idx = bid / NX;
    int q = nwg / NX, r = nwg % NX;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

struct Ph8Sched {          // host-computed per launch (ph8_schedule), passed by value
    int G;                  // workgroups (== gridDim.x)
    int tiles_n;
    int tiles_m_full;       // row tiles of the "full" logical tile space
    int light;              // 1: one more row of tiles with <= 64 valid rows ("light": about half the time of a full tile: the W panel still streams)
    int light_first;        // work order: light tiles before the full ones (K-split schedules with whole rounds) instead of behind them
    int dp_rounds;          // whole tiles per workgroup
    int nkp;                // K-pair units (128 k) per tile
    int sk_tiles;           // tiles of the remainder space (the full tiles left over by the whole rounds, and the light tiles)
    int rem0;               // work-order position of the first remainder tile (remainder tile j = position rem0 + j)
    int split;              // 0: remainder tiles stay whole; 1: every remainder tile is cut along K, one workgroup per part
    int sk_q, sk_r;         // split 0: workgroup i takes sk_q (+ 1 if i < sk_r) consecutive remainder tiles
    int cls_n[3], cls_p[3]; // split 1: three consecutive classes of remainder tiles, cls_n[c] tiles of cls_p[c] parts each
    float* sk_slab;         // split 1: [G][65536] raw accumulator images (caller's workspace)
    // the half-row schedule (ph8_half_rows_ints below).  hr = 1: the walk described above is empty (dp_rounds = sk_tiles = 0) and workgroup i takes
    // full tile i (i < hr_full), then half tile i - (G - hr_half) (i >= G - hr_half)
    int hr;
    int hr_full, hr_half;   // full tiles, half tiles (128 rows of one column tile)
    int hr_q, hr_r;         // row tiles cut into two half tiles: the LAST hr_q (+ 1 in the columns < hr_r) of every column
    int hr_ext;             // 1: the last half tile of every column is extended by the 16-row block that holds the M tail
};

// units [b, e) of the remainder space (unit = 128 k of one tile, tile j = units [j nkp, (j + 1) nkp)) that workgroup i works on
SAT_HD void ph8_wg_units(const Ph8Sched& sc, int i, int& b, int& e) {
    if (!sc.split) {
        const int lo = i < sc.sk_r ? i : sc.sk_r, hi = i + 1 < sc.sk_r ? i + 1 : sc.sk_r;
        b = (i * sc.sk_q + lo) * sc.nkp;
        e = ((i + 1) * sc.sk_q + hi) * sc.nkp;
        return;
    }
    int w0 = 0, j0 = 0;
    b = e = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int n = sc.cls_n[c], p = sc.cls_p[c];
        if (i >= w0 && i < w0 + n * p) {
            const int j = j0 + (i - w0) / p, k = (i - w0) % p;
            b = j * sc.nkp + sc.nkp * k / p;
            e = j * sc.nkp + sc.nkp * (k + 1) / p;
        }
        w0 += n * p;
        j0 += n;
    }
}
// split 1: the workgroups first .. first + parts - 1 that hold remainder tile j's K-ranges
SAT_HD void ph8_tile_parts(const Ph8Sched& sc, int j, int& first, int& parts) {
    int w0 = 0, j0 = 0;
    first = 0;
    parts = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int n = sc.cls_n[c], p = sc.cls_p[c];
        if (j >= j0 && j < j0 + n) {
            first = w0 + (j - j0) * p;
            parts = p;
        }
        w0 += n * p;
        j0 += n;
    }
}

// position in the work order -> tile.  Work order: the full tiles (short M: m fastest, the W panel of a column tile stays in one
// XCD's L2; long M: bands of 8 row tiles, n-major inside a band -- 8 A panels + the W panels in flight) with the light row behind
// them, or (light_first) in front of them.
SAT_HD void ph8_tile_of(const Ph8Sched& sc, int id, int& tm, int& tn) {
    const int nl = sc.light ? sc.tiles_n : 0;
    const int lid = sc.light_first ? id : id - sc.tiles_m_full * sc.tiles_n;
    if (lid >= 0 && lid < nl) {
        tm = sc.tiles_m_full;
        tn = lid;
        return;
    }
    const int L = sc.light_first ? id - nl : id;
    const int tiles_m = sc.tiles_m_full, tiles_n = sc.tiles_n;
    if (tiles_m <= 12) {
        tn = L / tiles_m;
        tm = L - tn * tiles_m;
    } else {
        const int band_sz = 8 * tiles_n;
        const int band = L / band_sz;
        const int rem = L - band * band_sz;
        const int gm = tiles_m - band * 8 < 8 ? tiles_m - band * 8 : 8;
        tn = rem / gm;
        tm = band * 8 + (rem - tn * gm);
    }
}

// ---- the half-row schedule: work-order index -> tile.  Column-major like the short-M order above (the W panel of a column stays in one
// XCD's L2): column tn holds tiles_m_full - s(tn) full tiles on top of 2 s(tn) half tiles, s(tn) = hr_q + (tn < hr_r).
SAT_HD void ph8_hr_full_of(const Ph8Sched& sc, int L, int& tm, int& tn) {
    const int fa = sc.tiles_m_full - sc.hr_q - 1, fb = fa + 1;          // full tiles of a column < hr_r, of the others
    const int na = sc.hr_r * fa;
    if (L < na) {
        tn = L / fa;
        tm = L - tn * fa;
    } else {
        const int c = (L - na) / fb;
        tn = sc.hr_r + c;
        tm = L - na - c * fb;
    }
}
// half tile j -> its first row r0 (a multiple of 128), its column tile, and whether it carries the M tail (rows [r0 + 128, M))
SAT_HD void ph8_hr_half_of(const Ph8Sched& sc, int j, int& r0, int& tn, int& ext) {
    const int ha = 2 * (sc.hr_q + 1), hb = 2 * sc.hr_q;                 // half tiles of a column < hr_r, of the others
    const int na = sc.hr_r * ha;
    int k, s;
    if (j < na) {
        tn = j / ha;
        k = j - tn * ha;
        s = sc.hr_q + 1;
    } else {
        const int c = (j - na) / hb;
        tn = sc.hr_r + c;
        k = j - na - c * hb;
        s = sc.hr_q;
    }
    r0 = (sc.tiles_m_full - s) * 256 + k * 128;
    ext = (sc.hr_ext && k == 2 * s - 1) ? 1 : 0;
}
// the (at most two) pieces of workgroup wgi, in the order it walks them: step 0 = its full tile, step 1 = its half tile
SAT_HD bool ph8_hr_has_full(const Ph8Sched& sc, int wgi) { return wgi < sc.hr_full; }
SAT_HD int ph8_hr_half_index(const Ph8Sched& sc, int wgi) { return wgi - (sc.G - sc.hr_half); }          // < 0: none

// The walk of workgroup `wgi` (= xcd_remap(blockIdx.x, G)) over its work is the `next_seg` lambda of gemm_ph8_kernel: dp_rounds
// whole tiles at work-order positions d * G + wgi, then the units [b, e) of ph8_wg_units, cut at tile borders.  It stays in the
// kernel: as a function of this header (state struct + one step returning tm, tn, ub, ue, whole) the compiler emitted different code for every
// gemm_ph8_kernel (profiles/gemm_host_refactor.txt), and this change promises the parent's device code.  tests/host/gemm_host_dump.cpp
// restates it in the same few lines -- change both together.

// Measured policy (profiles/r03_ph8_streamk.txt): split only fp32-output GEMMs with a long reduction (K >= 4096: FF-out) behind at
// least one whole round, and only when every remainder tile gets >= 2 parts (otherwise the whole tiles set the makespan and the slab
// traffic -- 256 KiB per part written and read back at HBM speed, everybody at the same time -- is pure loss): SA-2.0 FF-out -25 %.
// 8 prompts (134 remainder tiles on 256 CUs) and every K = 1536 GEMM stay whole; below one whole round the 128 x 128 tiles of
// gemm_bf16.hip are faster (FF-out at 1 prompt: 60 us against 67).
inline bool ph8_auto_split(int M, int N, int K, bool epi_f32, int cus) {
    const long t_all = (long)((M + 255) / 256) * (N / 256);
    const long rem = t_all % cus;
    return epi_f32 && K >= 4096 && t_all > cus && rem > 0 && 2 * rem <= cus;
}

// `balance` argument of ph8_schedule_ints
enum { PH8_BALANCE_TWO_ROUNDS = 0, PH8_BALANCE_OFF = 1 };

// The schedule of one launch on `cus` compute units.
// split: 0 = the remainder round's tiles stay whole (contiguous shares, light tiles last), 1 = every remainder tile is cut along K
// (the caller then checks GemmArgs::slab against G slabs and sets sk_slab), -1 = the measured policy above, which needs have_slab.
// Returns 0, or the number of workgroups a K-split would need when that is more than the out.G there are.
inline long ph8_schedule_ints(int M, int N, int K, int split, bool epi_f32, int bm, int bn, int wgs_per_cu, int cus, bool have_slab, int balance,
                              Ph8Sched& out) {
    auto lmin = [](long a, long b) { return a < b ? a : b; };
    auto lmax = [](long a, long b) { return a > b ? a : b; };
    if (split < 0) split = (bm == 256 && epi_f32 && have_slab && ph8_auto_split(M, N, K, epi_f32, cus)) ? 1 : 0;
    if (bm != 256 || !epi_f32) split = 0;          // the K-split machinery (slabs, reduce kernel) is built for the 256 x 256 fp32-output tile
    Ph8Sched s{};
    const int tiles_m = (M + bm - 1) / bm, tail = M % bm;
    s.tiles_n = N / bn;
    s.light = (tail != 0 && tail <= bm / 4 && tiles_m > 1) ? 1 : 0;          // only the first quadrant of the first wave row has rows
    s.tiles_m_full = tiles_m - s.light;
    s.nkp = K / 128;
    const long t_full = (long)s.tiles_m_full * s.tiles_n, t_light = s.light ? s.tiles_n : 0;
    const long t_all = t_full + t_light;
    s.G = (int)lmin((long)cus * wgs_per_cu, split ? t_all * s.nkp : t_all);
    // Balanced rounds: a launch of more than one and at most two rounds runs on FEWER workgroups, every one with two tiles (390 tiles:
    // 2 x 195 instead of 256 + 134; FF-in at one prompt: 2 x 216, which is also what the vendor library's stream-K launches for this
    // shape).  The chip is power-limited under MFMA load -- a tile runs faster when fewer CUs are active -- so the idle CUs cost
    // less than a half-empty second round: FF-out at 8 prompts 336 -> 311 us, FF-in at one prompt 85.4 -> 82.6 us.  With many rounds it
    // loses (FF-in at 8 prompts, 12.2 rounds: 479 -> 488 us): profiles/r04_ph8_balanced_rounds.txt.  PH8_BALANCE_OFF switches it off (A/B).
    if (!split && !(balance & PH8_BALANCE_OFF) && t_all > s.G && t_all <= 2L * s.G) s.G = (int)((t_all + 1) / 2);
    s.dp_rounds = (int)((split ? t_all : t_full) / s.G);
    // K-split with at least one whole round: the light tiles go FIRST (they idle their workgroup for half of round 0 -- a handful of
    // them) so that the remainder round holds full tiles only and splits evenly
    s.light_first = (split && s.dp_rounds >= 1 && t_light) ? 1 : 0;
    s.rem0 = (int)((long)s.dp_rounds * s.G);
    s.sk_tiles = (int)(t_all - s.rem0);
    s.split = (split && s.sk_tiles) ? 1 : 0;
    if (s.sk_tiles && !s.split) {
        s.sk_q = s.sk_tiles / s.G;
        s.sk_r = s.sk_tiles % s.G;
    } else if (s.sk_tiles) {
        // remainder tiles in work order: full ones (cost 2), then -- unless they went first -- the light ones (cost 1).  Parts per tile in
        // proportion to cost, at most min(nkp, 8); leftover workgroups give the first full tiles one more part: three classes.
        const int n_light = s.light_first ? 0 : (int)lmin(t_light, s.sk_tiles);
        const int n_full = s.sk_tiles - n_light;
        const long cost2 = 2L * n_full + n_light;
        const int cap = s.nkp < 8 ? s.nkp : 8;
        const int pf = (int)lmax(1, lmin(cap, (long)s.G * 2 / cost2));
        const int pl = (int)lmax(1, lmin(cap, (long)s.G * 1 / cost2));
        long used = (long)n_full * pf + (long)n_light * pl;
        int extra = 0;
        if (pf < cap && used < s.G) extra = (int)lmin(n_full, s.G - used);
        used += extra;
        if (used > s.G) {
            out = s;
            return used;
        }
        s.cls_n[0] = extra; s.cls_p[0] = pf + 1;
        s.cls_n[1] = n_full - extra; s.cls_p[1] = pf;
        s.cls_n[2] = n_light; s.cls_p[2] = pl;
    }
    out = s;
    return 0;
}

// Half-row schedule of the remainder round (16-bit SwiGLU epilogue only; asked FIRST by the launcher, everything it refuses runs
// ph8_schedule_ints above).  With t full 256 x 256 tiles on G compute units, G < t <= 1.5 G, two balanced rounds cost every workgroup two
// tile slots for 1.5-1.6 tiles' worth of work.  Here every compute unit gets a workgroup with ONE full tile and at most ONE half tile (128
// rows x 256 columns: the wave rows move together to a 64-row stride and each wave skips its second quadrant, the kernel's q_valid1 path --
// half the MFMAs, the same MFMA shape and K order per output element, so bit-identical results).  S = t - G row tiles are cut in two,
// the last ones of their columns.  An M tail of <= 16 rows rides on the last half tile of its column as one more 16-row block of wave row 1
// ("extended": 8 more MFMAs per K-tile) instead of a light tile, so with a tail every column needs a cut tile: S = max(t - G, tiles_n).
// Refused: any other epilogue or operand format, a tail of 17..255 rows, t <= G (one round), t > 1.5 G or 2 S > G (a workgroup would need
// two half tiles).  FF-in at one prompt (2050 x 12288 x 1536, 256 CUs): 256 full + 256 half tiles, 48 of them extended, no light tile.
// Measured (profiles/ffin_half_rows_timing.txt): a half tile costs 0.59-0.64 of a full one, the extended block nothing that shows; the
// launch alone 82.4 -> 74.5 us (fp16) / 79.7 -> 71.5 (bf16), in the model 76.5 -> 73.1 us, a generation at one prompt -0.7 .. -1.1 %.
inline bool ph8_half_rows_ints(int M, int N, int K, bool swiglu16, int cus, bool off, Ph8Sched& out) {
    if (off || !swiglu16 || cus < 1 || M < 256 || N < 256 || N % 256 || K < 128 || K % 128) return false;
    const int tail = M % 256;
    if (tail > 16) return false;
    const int tmf = M / 256, tiles_n = N / 256;
    const long t = (long)tmf * tiles_n, G = cus;
    if (!(t > G && 2 * t <= 3 * G)) return false;
    const long S = (tail && t - G < tiles_n) ? tiles_n : t - G;
    if (2 * S > G) return false;
    Ph8Sched s{};
    s.G = (int)G;
    s.tiles_n = tiles_n;
    s.tiles_m_full = tmf;
    s.nkp = K / 128;
    s.hr = 1;
    s.hr_full = (int)(t - S);
    s.hr_half = (int)(2 * S);
    s.hr_q = (int)(S / tiles_n);
    s.hr_r = (int)(S % tiles_n);
    s.hr_ext = tail ? 1 : 0;
    out = s;
    return true;
}

}  // namespace
