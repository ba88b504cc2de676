// Host check of csrc/attn_causal.h (tests/test_dit_causal_host.py runs it): for every sequence length S <= argv[1], key shift ob 0..3, key tile
// 64 and 128 and query block 128 and 256 (waves of 32 queries), against brute force over all (query, key) pairs:
//   * every visible pair (key j <= query i, physical key ob + j) lies in a tile the workgroup walks and in a 32-key block its wave does not skip;
//   * no walked tile is wholly invisible to its workgroup (the last one holds the diagonal key of the workgroup's last query);
//   * no block classed FULL holds a masked pair (a pad key, or a key above the diagonal of one of the wave's queries);
//   * in a DIAG block the per-element rule [ob, key_end(i)) is exactly the visibility of the pair.
// The fp32 kernel's use (tiles of 8 keys, no shift, blocks of 64 queries) is covered by the first two properties at KT = 8.
// Prints one summary line; exit status 1 and the first counter-example otherwise.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "attn_causal.h"

static long long g_pairs = 0, g_blocks[3] = {0, 0, 0};

static bool fail(const char* what, int S, int ob, int KT, int QB, int q, int key) {
    std::printf("FAIL %s: S %d ob %d KT %d QB %d query %d physical key %d\n", what, S, ob, KT, QB, q, key);
    return false;
}

static bool check(int S, int ob, int KT, int QB, int wave_q) {
    for (int q0 = 0; q0 < S; q0 += QB) {
        const int n_tiles = attnc::tiles_walked(q0, QB, ob, S, KT);
        const int q_last = attnc::last_query(q0, QB, S);
        if (n_tiles < 1 || (n_tiles - 1) * KT > ob + q_last || n_tiles * KT <= ob + q_last)
            return fail("the last walked tile does not hold the diagonal key of the workgroup's last query", S, ob, KT, QB, q_last, ob + q_last);
        for (int w0 = q0; w0 < q0 + QB && w0 < S; w0 += wave_q) {
            const int w_last = attnc::last_query(w0, wave_q, S);
            for (int k0 = 0; k0 < n_tiles * KT; k0 += 32) {
                const int cls = KT >= 32 ? attnc::block_class(k0, w0, wave_q, ob, S) : attnc::DIAG;
                ++g_blocks[cls];
                for (int i = w0; i <= w_last; ++i)
                    for (int key = k0; key < k0 + 32; ++key) {
                        const bool vis = key >= ob && key - ob <= i;          // (key - ob <= i < S: a real key)
                        ++g_pairs;
                        if (cls == attnc::SKIP && vis) return fail("a visible pair in a skipped block", S, ob, KT, QB, i, key);
                        if (cls == attnc::FULL && !vis) return fail("a masked pair in a block classed full", S, ob, KT, QB, i, key);
                        if (cls == attnc::DIAG && vis != (key >= ob && key < attnc::key_end(i, ob, S)))
                            return fail("the per-element rule of a diagonal block disagrees", S, ob, KT, QB, i, key);
                    }
            }
            // nothing visible beyond the walked tiles
            if (ob + w_last >= n_tiles * KT) return fail("a visible key beyond the walked tiles", S, ob, KT, QB, w_last, ob + w_last);
        }
    }
    return true;
}

int main(int argc, char** argv) {
    const int s_max = argc > 1 ? std::atoi(argv[1]) : 700;
    for (int S = 1; S <= s_max; ++S)
        for (int ob = 0; ob < 4; ++ob) {
            for (int KT : {64, 128})
                for (int QB : {128, 256})
                    if (!check(S, ob, KT, QB, 32)) return 1;
            if (ob == 0 && !check(S, 0, 8, 64, 64)) return 1;          // f32_ref.hip: 8-key chunks, one wave of 64 queries, no shift
        }
    // a query behind the sequence is computed like the last row
    if (attnc::key_end(1000, 3, 301) != 3 + 301 || attnc::key_end(0, 2, 5) != 3) return std::printf("FAIL key_end\n"), 1;
    std::printf("attn_causal.h: S 1..%d x ob 0..3 x KT {64,128} x QB {128,256} and the fp32 walk: %lld pairs, blocks skipped %lld diagonal %lld full %lld\n",
                s_max, g_pairs, g_blocks[attnc::SKIP], g_blocks[attnc::DIAG], g_blocks[attnc::FULL]);
    return 0;
}
