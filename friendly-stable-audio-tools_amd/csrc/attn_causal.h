// Key ranges of causal self-attention (attention.hip, attention_hdw.hip, f32_ref.hip).  Integer logic only, no device code: host programs and
// tests include it as it is (tests/host/attn_causal_dump.cpp checks it against brute force; tests/test_dit_causal_host.py runs that).
//
// The rule (models/transformer.py:296, 359-398 of the reference, SDPA is_causal=True with q_len == k_len): query i of a sequence of S rows
// sees the keys j <= i of the same sequence.  The K rows / V^T columns of sequence b start at the physical row ob = (b * S) & 3, so the
// physical key ob + j is visible to query i iff j <= i; physical keys below ob or from ob + S on are pads and visible to nobody.  The
// fp32 kernel has no shift and asks with ob = 0.
#pragma once

namespace attnc {

enum { SKIP = 0, DIAG = 1, FULL = 2 };

// the last real query of a block or wave that owns the queries [q_first, q_first + q_count); q_first < S
constexpr int last_query(int q_first, int q_count, int S) { return q_first + q_count - 1 < S - 1 ? q_first + q_count - 1 : S - 1; }

// How many key tiles of KT physical keys a workgroup walks: the tiles [0, n) hold every key one of its queries sees, and the last of them
// holds the diagonal key of its last query
constexpr int tiles_walked(int q_first, int q_count, int ob, int S, int KT) { return (ob + last_query(q_first, q_count, S)) / KT + 1; }

// The block of 32 physical keys from k0 on, for a wave with the queries [q_first, q_first + q_count):
//   SKIP  every key lies above the diagonal of the wave's last query: no query of the wave sees any of them
//   FULL  every key is a real key at or below the diagonal of the wave's FIRST query: every query sees all 32, no compare per element
//   DIAG  the rest: query i keeps the physical keys in [ob, ob + min(i, S - 1)], the others are masked per element
constexpr int block_class(int k0, int q_first, int q_count, int ob, int S) {
    return k0 > ob + last_query(q_first, q_count, S) ? SKIP : (k0 >= ob && k0 + 31 <= ob + q_first) ? FULL : DIAG;
}

// DIAG blocks: one past the last physical key that query i sees (queries behind the sequence are computed like its last row and not stored)
constexpr int key_end(int i, int ob, int S) { return ob + (i < S ? i : S - 1) + 1; }

}  // namespace attnc
