// Host check of csrc/attn_window.h (tests/test_dit_natten_host.py runs it): for every sequence length S <= argv[1], every odd kernel size
// 3 <= K <= S (S <= 140) or those of a fixed list plus S or S - 1 (S > 140), key shift ob 0..3, key tile 64 and query block 256 (waves of 32 queries), against brute force
// over all (query, key) pairs:
//   * every visible pair (physical key ob + j with start(i) <= j < start(i) + K) lies in a tile the workgroup walks and in a 32-key block its
//     wave does not skip;
//   * the first and the last walked tile each hold a key some query of the workgroup sees (nothing outside the union is copied or walked),
//     and both lie inside the padded key buffer;
//   * no block classed FULL holds a masked pair (a pad key, or a key outside the window of one of the wave's queries);
//   * in an EDGE block the per-element rule [key_lo(i), key_hi(i)) is exactly the visibility of the pair;
//   * every query sees exactly K keys.
// The fp32 kernel's use (the interval [union_lo, union_hi) of a wave of 64 queries, no shift) is covered by the union properties at QB = 64.
// Prints one summary line; exit status 1 and the first counter-example otherwise.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "attn_window.h"

static long long g_pairs = 0, g_blocks[3] = {0, 0, 0}, g_tiles_walked = 0, g_tiles_all = 0;

static bool fail(const char* what, int S, int K, int ob, int QB, int q, int key) {
    std::printf("FAIL %s: S %d K %d ob %d QB %d query %d physical key %d\n", what, S, K, ob, QB, q, key);
    return false;
}

static int brute_start(int i, int K, int S) {
    int s = i - K / 2;
    if (s < 0) s = 0;
    if (s > S - K) s = S - K;
    return s;
}

static bool check(int S, int K, int ob, int KT, int QB, int wave_q) {
    const int sk_pad = (S + 3 + KT - 1) / KT * KT;
    for (int q0 = 0; q0 < S; q0 += QB) {
        const int t0 = attnw::first_tile(q0, ob, K, S, KT), t1 = attnw::last_tile(q0, QB, ob, K, S, KT);
        const int q_last = attnw::last_query(q0, QB, S);
        if (t0 < 0 || t1 < t0 || (t1 + 1) * KT > sk_pad) return fail("the walked tiles leave the key buffer", S, K, ob, QB, q0, t1 * KT);
        g_tiles_walked += t1 - t0 + 1;
        g_tiles_all += (ob + S + KT - 1) / KT;
        // both end tiles hold a visible key: the first key of the first query's window, the last key of the last query's
        const int k_first = ob + brute_start(q0, K, S), k_last = ob + brute_start(q_last, K, S) + K - 1;
        if (k_first / KT != t0) return fail("the first walked tile does not hold the first visible key", S, K, ob, QB, q0, k_first);
        if (k_last / KT != t1) return fail("the last walked tile does not hold the last visible key", S, K, ob, QB, q_last, k_last);
        for (int w0 = q0; w0 < q0 + QB && w0 < S; w0 += wave_q) {
            const int w_last = attnw::last_query(w0, wave_q, S);
            const attnw::Range wr = attnw::wave_range(w0, wave_q, ob, K, S);
            for (int i = w0; i <= w_last; ++i) {          // nothing visible outside the walked tiles
                const int lo = ob + brute_start(i, K, S), hi = lo + K;
                if (lo < t0 * KT || hi > (t1 + 1) * KT) return fail("a visible key outside the walked tiles", S, K, ob, QB, i, lo);
                if (attnw::key_lo(i, ob, K, S) != lo || attnw::key_hi(i, ob, K, S) != hi) return fail("key_lo / key_hi", S, K, ob, QB, i, lo);
                if (lo < ob || hi > ob + S) return fail("a window reaches into the pads", S, K, ob, QB, i, lo);
            }
            if (KT < 32) continue;
            for (int k0 = t0 * KT; k0 < (t1 + 1) * KT; k0 += 32) {
                const int cls = attnw::block_class(k0, wr);
                if (cls != attnw::block_class(k0, w0, wave_q, ob, K, S)) return fail("the two forms of block_class disagree", S, K, ob, QB, w0, k0);
                ++g_blocks[cls];
                for (int i = w0; i <= w_last; ++i) {
                    const int lo = ob + brute_start(i, K, S);
                    for (int key = k0; key < k0 + 32; ++key) {
                        const bool vis = key >= lo && key < lo + K;
                        ++g_pairs;
                        if (cls == attnw::SKIP && vis) return fail("a visible pair in a skipped block", S, K, ob, QB, i, key);
                        if (cls == attnw::FULL && !vis) return fail("a masked pair in a block classed full", S, K, ob, QB, i, key);
                        if (cls == attnw::EDGE && vis != (key >= attnw::key_lo(i, ob, K, S) && key < attnw::key_hi(i, ob, K, S)))
                            return fail("the per-element rule of an edge block disagrees", S, K, ob, QB, i, key);
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
            for (int ob = 0; ob < 4; ++ob) {
                if (!check(S, K, ob, 64, 256, 32)) return false;
                ++combos;
            }
            return check(S, K, 0, 8, 64, 64);          // the fp32 kernel: one wave of 64 queries, no shift, the union as an interval
        };
        if (S <= 140) {          // every odd kernel size
            for (int K = 3; K <= S; K += 2)
                if (!one(K)) return 1;
        } else {                 // the sizes round the block, tile and workgroup widths, and the whole sequence
            for (int K : {3, 7, 31, 33, 63, 65, 129, 255, 257, k_all})
                if (K <= S && !one(K)) return 1;
        }
    }
    // a query behind the sequence is computed like the last row
    if (attnw::start(1000, 33, 301) != 301 - 33 || attnw::start(0, 7, 69) != 0 || attnw::start(34, 7, 69) != 31 || attnw::start(68, 7, 69) != 62)
        return std::printf("FAIL start\n"), 1;
    std::printf("attn_window.h: S 3..%d x K x ob 0..3 x KT 64 x QB 256 (%lld combinations) and the fp32 walk: %lld pairs, blocks skipped %lld edge %lld full %lld, "
                "tiles walked %lld of %lld\n",
                s_max, combos, g_pairs, g_blocks[attnw::SKIP], g_blocks[attnw::EDGE], g_blocks[attnw::FULL], g_tiles_walked, g_tiles_all);
    return 0;
}
