// Host check of csrc/attn_window.h at the key tiles of csrc/attention_hdw_window.hip (tests/test_dit_natten_hdw_host.py runs it): the properties
// of attn_window_dump.cpp at KT = 128 (32-channel heads, four 32-key blocks per tile) as well as KT = 64, key shift ob 0..3, query block 256 in
// waves of 32, for every sequence length S <= argv[1], against brute force over all (query, key) pairs:
//   * every visible pair lies in a tile the workgroup walks and in a 32-key block its wave does not skip;
//   * the first and the last walked tile hold the first and the last visible key of the workgroup, and both lie inside a key buffer of
//     sk_pad = roundup(S + 3, KT) keys -- whatever the first walked tile is and whether or not the last walked one is the sequence's last;
//   * no block classed FULL holds a masked pair; in an EDGE block [key_lo(i), key_hi(i)) is exactly the visibility of the pair;
//   * counted: walked tiles that are neither the sequence's first nor its last, and, per KT, the tiles in which a wave meets a visible block
//     BEHIND a skipped one -- what a `break` at the first SKIP block would lose.  At KT = 64 (two blocks) that is a tile whose first block lies
//     below the wave's union; at KT = 128 also blocks 2 and 3 behind skipped blocks 0 and 1.
// Prints one summary line; exit status 1 and the first counter-example otherwise.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "attn_hdw_tiles.h"
#include "attn_window.h"

static_assert(attnw::Tiles<32>::KV_TILE == 128 && attnw::Tiles<96>::KV_TILE == 64 && attnw::Tiles<128>::KV_TILE == 64, "the tiles this program walks");

static long long g_pairs = 0, g_blocks[3] = {0, 0, 0}, g_walked[2] = {0, 0}, g_all[2] = {0, 0}, g_inner[2] = {0, 0}, g_behind_skip[2] = {0, 0},
                 g_third_behind_skip = 0;

static bool fail(const char* what, int S, int K, int ob, int KT, int q, int key) {
    std::printf("FAIL %s: S %d K %d ob %d KT %d query %d physical key %d\n", what, S, K, ob, KT, q, key);
    return false;
}

static int brute_start(int i, int K, int S) {
    int s = i - K / 2;
    if (s < 0) s = 0;
    if (s > S - K) s = S - K;
    return s;
}

static bool check(int S, int K, int ob, int KT) {
    const int QB = 256, WQ = 32, kt = KT == 128;
    const int sk_pad = (S + 3 + KT - 1) / KT * KT, n_tiles = (ob + S + KT - 1) / KT;
    for (int q0 = 0; q0 < S; q0 += QB) {
        const int t0 = attnw::first_tile(q0, ob, K, S, KT), t1 = attnw::last_tile(q0, QB, ob, K, S, KT);
        const int q_last = attnw::last_query(q0, QB, S);
        if (t0 < 0 || t1 < t0 || (t1 + 1) * KT > sk_pad) return fail("the walked tiles leave the key buffer", S, K, ob, KT, q0, t1 * KT);
        g_walked[kt] += t1 - t0 + 1;
        g_all[kt] += n_tiles;
        for (int t = t0; t <= t1; ++t) g_inner[kt] += t != 0 && t != n_tiles - 1;
        const int k_first = ob + brute_start(q0, K, S), k_last = ob + brute_start(q_last, K, S) + K - 1;
        if (k_first / KT != t0) return fail("the first walked tile does not hold the first visible key", S, K, ob, KT, q0, k_first);
        if (k_last / KT != t1) return fail("the last walked tile does not hold the last visible key", S, K, ob, KT, q_last, k_last);
        for (int w0 = q0; w0 < q0 + QB && w0 < S; w0 += WQ) {
            const int w_last = attnw::last_query(w0, WQ, S);
            const attnw::Range wr = attnw::wave_range(w0, WQ, ob, K, S);
            for (int i = w0; i <= w_last; ++i) {
                const int lo = ob + brute_start(i, K, S), hi = lo + K;
                if (lo < t0 * KT || hi > (t1 + 1) * KT) return fail("a visible key outside the walked tiles", S, K, ob, KT, i, lo);
                if (lo < ob || hi > ob + S) return fail("a window reaches into the pads", S, K, ob, KT, i, lo);
            }
            for (int t = t0; t <= t1; ++t) {
                bool skipped = false;
                for (int kb = 0; kb < KT / 32; ++kb) {
                    const int k0 = t * KT + kb * 32, cls = attnw::block_class(k0, wr);
                    ++g_blocks[cls];
                    if (cls == attnw::SKIP) skipped = true;
                    else if (skipped) {
                        ++g_behind_skip[kt];
                        g_third_behind_skip += kb == 2;
                        skipped = false;          // (count the tile once)
                    }
                    for (int i = w0; i <= w_last; ++i) {
                        const int lo = ob + brute_start(i, K, S);
                        for (int key = k0; key < k0 + 32; ++key) {
                            const bool vis = key >= lo && key < lo + K;
                            ++g_pairs;
                            if (cls == attnw::SKIP && vis) return fail("a visible pair in a skipped block", S, K, ob, KT, i, key);
                            if (cls == attnw::FULL && !vis) return fail("a masked pair in a block classed full", S, K, ob, KT, i, key);
                            if (cls == attnw::EDGE && vis != (key >= attnw::key_lo(i, ob, K, S) && key < attnw::key_hi(i, ob, K, S)))
                                return fail("the per-element rule of an edge block disagrees", S, K, ob, KT, i, key);
                        }
                    }
                }
            }
        }
    }
    return true;
}

int main(int argc, char** argv) {
    const int s_max = argc > 1 ? std::atoi(argv[1]) : 700;
    long long combos = 0;
    for (int S = 3; S <= s_max; ++S) {
        const int k_all = (S & 1) ? S : S - 1;
        auto one = [&](int K) {
            for (int KT : {64, 128})
                for (int ob = 0; ob < 4; ++ob) {
                    if (!check(S, K, ob, KT)) return false;
                    ++combos;
                }
            return true;
        };
        if (S <= 140) {          // every odd kernel size
            for (int K = 3; K <= S; K += 2)
                if (!one(K)) return 1;
        } else {                 // the sizes round the block, tile and workgroup widths, and the whole sequence
            for (int K : {3, 7, 31, 33, 63, 65, 127, 129, 255, 257, k_all})
                if (K <= S && !one(K)) return 1;
        }
    }
    std::printf("attn_window.h: S 3..%d x K x ob 0..3 x KT 64, 128 x QB 256 (%lld combinations): %lld pairs, blocks skipped %lld edge %lld full %lld; "
                "KT 64: tiles walked %lld of %lld, inner %lld, visible behind skipped %lld; KT 128: tiles walked %lld of %lld, inner %lld, visible behind "
                "skipped %lld, third block behind skipped %lld\n",
                s_max, combos, g_pairs, g_blocks[attnw::SKIP], g_blocks[attnw::EDGE], g_blocks[attnw::FULL], g_walked[0], g_all[0], g_inner[0],
                g_behind_skip[0], g_walked[1], g_all[1], g_inner[1], g_behind_skip[1], g_third_behind_skip);
    return 0;
}
