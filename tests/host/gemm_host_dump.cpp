// Host driver of tests/test_gemm_host.py: runs the GEMM tile choice (csrc/gemm_tiles.h) and the persistent schedule of the 8-phase
// kernel (csrc/ph8_sched.h) on the CPU.  Plain C++17, no HIP.
//   gemm_host_dump routes [splits]   one case per stdin line -> the kernel template that would be launched, or the error
//   gemm_host_dump sched          every schedule of a grid of shapes is walked workgroup by workgroup and checked to be an exact cover
//   gemm_host_dump ring           the geometry (csrc/gemm_ring_geom.h: RingGeom) of every ring tile x epilogue x operand flavour that gemm_bf16.hip builds
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gemm_ring_geom.h"
#include "gemm_tiles.h"

// error codes of include/sat_hip.h (that header is C ABI + HIP-free, but the route function only names message ids)
static int route_error_code(int msg) { return msg == SAT_ROUTE_XATTN_OPERANDS || msg == SAT_ROUTE_PH8_NOT_BUILT ? -2 : -1; }          // SAT_E_UNSUPPORTED : SAT_E_INVALID

static int routes(bool with_split) {
    int epi, M, N, K, fp8, h8, ln, gate, slab, heads, xattn, variant, f16b, cus;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &epi, &M, &N, &K, &fp8, &h8, &ln, &gate, &slab, &heads, &xattn, &variant, &f16b, &cus) == 14) {
        GemmShape s{};
        s.M = M; s.N = N; s.K = K; s.variant = variant; s.fp8 = fp8;
        s.h8 = h8; s.ln_part = ln; s.gate = gate; s.heads = heads; s.xattn = xattn; s.slab_ok = slab;
        s.e4m3_built = !f16b;
        const GemmRoute r = sat_gemm_route(epi, s, cus);
        const int tepi = epi == EPI_RESID ? EPI_F32 : epi;          // the template argument: EPI_RESID runs the EPI_F32 build
        if (r.msg != SAT_ROUTE_OK) {
            printf("err %d\n", route_error_code(r.msg));
        } else if (r.family == SAT_GEMM_PH8) {
            const SatPh8Params p = sat_ph8_params(r.ph8);
            // (the fixture's lines record `dbg ph2 ph2v wn mfq fp8 gated`; the four in the middle were template parameters of retired variants
            // of the kernel -- four-phase loop, W-hi issue order, 128 x 128 geometry -- and are now the constants 1 1 4 4)
            printf("ph8 %d %d 1 1 4 4 %d %d", tepi, p.dbg, p.fp8, (int)p.gated);
            if (with_split) {          // what the score assumed, and what the schedule of that launch does (launch_ph8: slab_ok = have_slab)
                Ph8Sched sc;
                // (K / 2 for e4m3 operands mirrors launch_ph8, gemm_ph8.hip: `a.K = a0.K / 2` -- the kernel and its schedule count 16-bit columns)
                ph8_schedule_ints(M, N, p.fp8 ? K / 2 : K, sat_variant_split(variant), tepi == EPI_F32, 256, 256, 1, cus, slab != 0, 0, sc);
                printf(" splits=%d schedule.split=%d", (int)r.splits, sc.split);
            }
            printf("\n");
        } else {
            const SatTile t = sat_tile_geom(r.tile);
            if (t.family == SAT_GEMM_PIPE)
                printf("pipe %d %d %d %d %d %d %d %d %d %d\n", t.bm, t.bn, t.bk, t.wm, t.wn, t.ns, tepi, r.e4m3, t.kg, (int)(t.dil && r.e4m3 == 0));
            else
                printf("cfg %d %d %d %d %d %d\n", t.bm, t.bn, t.wm, t.wn, tepi, (int)(t.family == SAT_GEMM_DMA2));
        }
    }
    return 0;
}

// ---- the schedule ---------------------------------------------------------------------------------------------------------------
struct Piece {          // one K-range of one tile, as a workgroup walks it
    int tm, tn, ub, ue, wg;
    bool whole;
};

// The walk of workgroup wgi: the `next_seg` lambda of gemm_ph8_kernel (csrc/gemm_ph8.hip) restated -- change both together.
static void walk(const Ph8Sched& sc, int wgi, std::vector<Piece>& out) {
    int dp_s = 0, sk_b = 0, sk_e = 0;
    if (sc.sk_tiles) ph8_wg_units(sc, wgi, sk_b, sk_e);
    int sk_u = sk_b;
    for (;;) {
        Piece p{};
        p.wg = wgi;
        if (dp_s < sc.dp_rounds) {
            ph8_tile_of(sc, dp_s * sc.G + wgi, p.tm, p.tn);
            ++dp_s;
            p.ub = 0; p.ue = sc.nkp; p.whole = true;
        } else {
            if (sk_u >= sk_e) return;
            const int j = sk_u / sc.nkp;
            const int ub = sk_u - j * sc.nkp;
            const int ue = std::min(sc.nkp, ub + (sk_e - sk_u));
            ph8_tile_of(sc, sc.rem0 + j, p.tm, p.tn);
            p.ub = ub; p.ue = ue; p.whole = (ub == 0 && ue == sc.nkp);
            sk_u += ue - ub;
        }
        out.push_back(p);
    }
}

static int sched() {
    const int CUS[] = {256, 304, 64, 8, 1};
    const int MS[] = {1, 2, 16, 64, 65, 255, 256, 257, 320, 321, 1025, 2050, 3075, 3073, 3329, 4100, 8200, 16400, 32800, 6145, 12290, 24580, 49160, 100000};
    const int NS[] = {256, 512, 1536, 4608, 12288};
    const int KS[] = {128, 256, 1536, 4096, 6144};
    long cases = 0, n_split = 0, refused = 0, failures = 0;
    std::vector<Piece> pieces;
    std::vector<int> whole_cnt, seen;
    std::vector<std::vector<Piece>> parts_of;
    auto fail = [&](const char* what, int cus, int M, int N, int K, int f32, int split, int bal, int geom) {
        if (++failures <= 20) printf("FAIL %s: cus=%d M=%d N=%d K=%d f32=%d split=%d balance=%d geom=%d\n", what, cus, M, N, K, f32, split, bal, geom);
    };
    for (int cus : CUS) for (int M : MS) for (int N : NS) for (int K : KS) for (int f32 = 0; f32 < 2; ++f32) for (int split = -1; split <= 1; ++split)
    for (int bal : {PH8_BALANCE_TWO_ROUNDS, PH8_BALANCE_OFF}) for (int geom : {256, 128}) {
        ++cases;
#define FAIL(what) do { fail(what, cus, M, N, K, f32, split, bal, geom); goto next_case; } while (0)
        {
            Ph8Sched sc;
            if (ph8_schedule_ints(M, N, K, split, f32 != 0, geom, geom, geom == 256 ? 1 : 2, cus, /*have_slab=*/true, bal, sc) != 0) {
                ++refused;
                continue;
            }
            n_split += sc.split;
            const int tiles_m = sc.tiles_m_full + sc.light, tiles_n = sc.tiles_n;
            if (tiles_m != (M + geom - 1) / geom || tiles_n != N / geom || sc.nkp != K / 128) FAIL("tile space");
            if (sc.G < 1 || sc.G > cus * (geom == 256 ? 1 : 2)) FAIL("workgroup count");
            if (sc.split && !(geom == 256 && f32)) FAIL("K-split outside the 256 x 256 fp32-output kernel");
            seen.assign(sc.G, 0);
            pieces.clear();
            for (int bid = 0; bid < sc.G; ++bid) {
                const int wgi = xcd_remap(bid, sc.G);
                if (wgi < 0 || wgi >= sc.G || seen[wgi]++) FAIL("xcd_remap is not a bijection");
                const size_t before = pieces.size();
                walk(sc, wgi, pieces);
                int partial = 0;
                for (size_t i = before; i < pieces.size(); ++i) partial += !pieces[i].whole;
                if (!sc.split && partial) FAIL("partial tile in an unsplit schedule");
                if (partial > 1) FAIL("more than one partial tile (= slab) in a workgroup");
            }
            whole_cnt.assign((size_t)tiles_m * tiles_n, 0);
            parts_of.assign(sc.split ? sc.sk_tiles : 0, {});
            for (const Piece& p : pieces) {
                if (p.tm < 0 || p.tm >= tiles_m || p.tn < 0 || p.tn >= tiles_n || p.ub < 0 || p.ub >= p.ue || p.ue > sc.nkp) FAIL("piece outside the tile space");
                if (p.whole) ++whole_cnt[(size_t)p.tm * tiles_n + p.tn];
            }
            if (sc.split) {
                // remainder tile j <-> its pieces: found through the work order, as ph8_reduce_f32_kernel does
                for (int j = 0; j < sc.sk_tiles; ++j) {
                    int tm, tn, first, parts;
                    ph8_tile_of(sc, sc.rem0 + j, tm, tn);
                    ph8_tile_parts(sc, j, first, parts);
                    std::vector<Piece> mine;
                    for (int w = first; w < first + parts; ++w) {
                        if (w < 0 || w >= sc.G) FAIL("ph8_tile_parts names a workgroup that does not exist");
                        int sk_b, sk_e;
                        ph8_wg_units(sc, w, sk_b, sk_e);
                        if (sk_b >= sk_e || sk_b / sc.nkp != j || (sk_e - 1) / sc.nkp != j) FAIL("a workgroup of ph8_tile_parts does not work on that tile alone");
                        mine.push_back(Piece{tm, tn, sk_b - j * sc.nkp, sk_e - j * sc.nkp, w, false});
                    }
                    int at = 0;          // ascending workgroups hold ascending K-ranges that tile [0, nkp)
                    for (const Piece& p : mine) {
                        if (p.ub != at) FAIL("K-ranges of a split tile do not tile its K");
                        at = p.ue;
                    }
                    if (at != sc.nkp) FAIL("K-ranges of a split tile do not reach K");
                    if (parts > 1 && whole_cnt[(size_t)tm * tiles_n + tn] != 0) FAIL("split tile also computed whole");
                    if (parts > 1) whole_cnt[(size_t)tm * tiles_n + tn] = 1;          // covered once, by its parts
                }
                // no workgroup outside first .. first + parts - 1 of some tile holds remainder work
                int first, parts;
                ph8_tile_parts(sc, sc.sk_tiles - 1, first, parts);
                for (int w = 0; w < sc.G; ++w) {
                    int sk_b, sk_e;
                    ph8_wg_units(sc, w, sk_b, sk_e);
                    if ((sk_b < sk_e) != (w < first + parts)) FAIL("workgroups with remainder work are not exactly those of ph8_tile_parts");
                }
                long partial_pieces = 0, expect = 0;
                for (const Piece& p : pieces) partial_pieces += !p.whole;
                for (int j = 0; j < sc.sk_tiles; ++j) {
                    ph8_tile_parts(sc, j, first, parts);
                    expect += parts > 1 ? parts : 0;
                }
                if (partial_pieces != expect) FAIL("partial pieces walked != parts of the split tiles");
            }
            for (int c : whole_cnt)
                if (c != 1) FAIL("a tile is not covered exactly once");
        }
    next_case:;
#undef FAIL
    }
    printf("cases %ld split %ld refused %ld failures %ld\n", cases, n_split, refused, failures);
    return failures ? 1 : 0;
}

// ---- the ring tiles' geometry ---------------------------------------------------------------------------------------------------
// One line per instantiation of gemm_pipe_kernel: the template arguments launch_tile (csrc/gemm_bf16.hip) hands launch_pipe, then every
// member of RingGeom.  Instantiating the struct also runs its static_asserts.
template <int ID, int EPIX, int F8>
static void ring_one() {
    constexpr SatTile t = sat_tile_geom(ID);
    static_assert(t.family == SAT_GEMM_PIPE, "ring tiles only");
    using G = RingGeom<t.bm, t.bn, t.bk, t.wm, t.wn, t.ns, EPIX, F8, t.kg, t.dil && F8 == 0>;
    printf("tile=%d epix=%d f8=%d", ID, EPIX, F8);
#define M(name) printf(" " #name "=%d", (int)G::name);
    M(TILE_M) M(TILE_N) M(STAGES) M(KGROUPS) M(EPI) M(QKN) M(NT) M(TM) M(TN) M(MI) M(NI) M(S16) M(MB) M(CPR) M(NW) M(WL_A) M(WLG) M(WL) M(LPT) M(N_FULL) M(UNIFORM) M(ROWB) M(MXA) M(SCALE_WAVES)
    M(GROUP_BYTES) M(STAGE_BYTES) M(D) M(DIL_ON) M(NDIL) M(DIL_STEPS) M(DIL_PER) M(LN_CONS) M(LN_OFF) M(PRE_RESID) M(ORI) M(XA_OK) M(XA_OFF) M(LDS) M(XA_LDS)
    M(KG_STAGING_OFF)
#undef M
    printf("\n");
}
// launch_epi (csrc/gemm_bf16.hip) restated: the tiles built for (epilogue, operand flavour) -- change both together
template <int EPIX, int F8>
static void ring_epi() {
    ring_one<SAT_TILE_128, EPIX, F8>();
    ring_one<SAT_TILE_128x64, EPIX, F8>();
    ring_one<SAT_TILE_256, EPIX, F8>();
    ring_one<SAT_TILE_256x192, EPIX, F8>();
    if constexpr (F8 == 0) {
        if constexpr (EPIX == EPI_F32) {
            ring_one<SAT_TILE_128_DEEP, EPIX, F8>();
            ring_one<SAT_TILE_128_KGROUP, EPIX, F8>();
        }
        if constexpr (EPIX == EPI_HEADS || EPIX == EPI_HEADS_QKN) ring_one<SAT_TILE_128x64_XATTN, EPIX, F8>();
    }
}
// launch_flavour and sat_launch_gemm restated: e4m3 flavours 1 and 2 of the three caller epilogues, 3 (MXFP8 A) of the fp32 output
static int ring() {
    ring_epi<EPI_F32, 0>(); ring_epi<EPI_F32, 1>(); ring_epi<EPI_F32, 2>(); ring_epi<EPI_F32, 3>();
    ring_epi<EPI_SWIGLU, 0>(); ring_epi<EPI_SWIGLU, 1>(); ring_epi<EPI_SWIGLU, 2>();
    ring_epi<EPI_HEADS, 0>(); ring_epi<EPI_HEADS, 1>(); ring_epi<EPI_HEADS, 2>();
    ring_epi<EPI_HEADS_QKN, 0>();
    ring_epi<EPI_ACT16, 0>();
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "routes")) return routes(argc >= 3 && !strcmp(argv[2], "splits"));
    if (argc >= 2 && !strcmp(argv[1], "sched")) return sched();
    if (argc >= 2 && !strcmp(argv[1], "ring")) return ring();
    fprintf(stderr, "usage: gemm_host_dump routes | sched | ring\n");
    return 2;
}
