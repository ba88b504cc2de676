// Key ranges of neighbourhood self-attention (attention_window.hip).  Integer logic only, no device code: host programs and tests include it
// as it is (tests/host/attn_window_dump.cpp checks it against brute force; tests/test_dit_natten_host.py runs that).
//
// The rule (models/transformer.py:479-493 of the reference, natten1dqk / natten1dav with kernel size K, dilation 1): query i of a sequence of
// S >= K rows sees exactly K keys, start(i) .. start(i) + K - 1 with start(i) = min(max(i - K / 2, 0), S - K) -- the window is shifted, not
// truncated, at both ends of the sequence.  start is non-decreasing in i, so the keys a run of queries sees between them are one interval
// (the union) and the keys every one of them sees are one, possibly empty, interval (the intersection).  The K rows / V^T columns of
// sequence b start at the physical row ob = (b * S) & 3: physical key ob + j stands for key j, physical keys below ob or from ob + S on are
// pads and lie in nobody's window.  The fp32 kernel has no shift and asks with ob = 0.
#pragma once

namespace attnw {

enum { SKIP = 0, EDGE = 1, FULL = 2 };

// first key of query i's window; queries behind the sequence are computed like its last row and not stored
constexpr int start(int i, int K, int S) {
    const int ic = i < S ? i : S - 1;
    const int lo = ic - K / 2 > 0 ? ic - K / 2 : 0;
    return lo < S - K ? lo : S - K;
}

// the last real query of a block or wave that owns the queries [q_first, q_first + q_count); q_first < S
constexpr int last_query(int q_first, int q_count, int S) { return q_first + q_count - 1 < S - 1 ? q_first + q_count - 1 : S - 1; }

// The physical keys [union_lo, union_hi) some query of [q_first, q_first + q_count) sees, and [inter_lo, inter_hi) (empty when inter_hi <=
// inter_lo) those all of them see
constexpr int union_lo(int q_first, int ob, int K, int S) { return ob + start(q_first, K, S); }
constexpr int union_hi(int q_first, int q_count, int ob, int K, int S) { return ob + start(last_query(q_first, q_count, S), K, S) + K; }
constexpr int inter_lo(int q_first, int q_count, int ob, int K, int S) { return ob + start(last_query(q_first, q_count, S), K, S); }
constexpr int inter_hi(int q_first, int ob, int K, int S) { return ob + start(q_first, K, S) + K; }

// The key tiles of KT physical keys a workgroup with the queries [q_first, q_first + q_count) walks: [first_tile, last_tile], both walked.
// Nothing outside them is copied
constexpr int first_tile(int q_first, int ob, int K, int S, int KT) { return union_lo(q_first, ob, K, S) / KT; }
constexpr int last_tile(int q_first, int q_count, int ob, int K, int S, int KT) { return (union_hi(q_first, q_count, ob, K, S) - 1) / KT; }

// The block of 32 physical keys from k0 on, for a wave with the queries [q_first, q_first + q_count):
//   SKIP  no key of the block lies in the window of any query of the wave
//   FULL  every key of the block lies in the window of every query of the wave: no compare per element
//   EDGE  the rest: query i keeps the physical keys in [key_lo(i), key_hi(i)), the others are masked per element
// A kernel works the four bounds out once per wave (wave_range) and classes every block of its walk against them
struct Range {
    int u_lo, u_hi, i_lo, i_hi;
};
constexpr Range wave_range(int q_first, int q_count, int ob, int K, int S) {
    return Range{union_lo(q_first, ob, K, S), union_hi(q_first, q_count, ob, K, S), inter_lo(q_first, q_count, ob, K, S), inter_hi(q_first, ob, K, S)};
}
constexpr int block_class(int k0, const Range& r) {
    return (k0 + 32 <= r.u_lo || k0 >= r.u_hi) ? SKIP : (k0 >= r.i_lo && k0 + 32 <= r.i_hi) ? FULL : EDGE;
}
constexpr int block_class(int k0, int q_first, int q_count, int ob, int K, int S) { return block_class(k0, wave_range(q_first, q_count, ob, K, S)); }

// EDGE blocks: the physical keys [key_lo, key_hi) of query i
constexpr int key_lo(int i, int ob, int K, int S) { return ob + start(i, K, S); }
constexpr int key_hi(int i, int ob, int K, int S) { return ob + start(i, K, S) + K; }

}  // namespace attnw
