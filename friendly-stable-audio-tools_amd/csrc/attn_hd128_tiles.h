// LDS geometry of the 128-channel-head attention kernel (attention_hd128.hip).  Integer logic only, no device code: host programs and
// tests include it as it is (tests/test_dit_head_dim_host.py checks that both maps are bijections onto their tile).
#pragma once

namespace attn128 {

constexpr int HEAD_DIM = 128;
constexpr int KV_TILE = 64;                                   // keys per ring stage
constexpr int K_ROW_BYTES = HEAD_DIM * 2;                     // K tile: 64 key rows of 256 B (sixteen 16-byte chunks)
constexpr int VT_ROW_BYTES = KV_TILE * 2;                     // V^T tile: 128 channel rows of 128 B (eight chunks)
constexpr int K_TILE_BYTES = KV_TILE * K_ROW_BYTES;           // 16 KiB
constexpr int VT_TILE_BYTES = HEAD_DIM * VT_ROW_BYTES;        // 16 KiB
constexpr int STAGE_BYTES = K_TILE_BYTES + VT_TILE_BYTES;     // 32 KiB
constexpr int STAGES = 3;
constexpr int LDS_BYTES = STAGES * STAGE_BYTES;               // 96 KiB

// A 256-byte row is exactly one LDS bank row (64 banks x 4 B), so the 16-byte slot a chunk occupies is its chunk index alone: un-swizzled,
// the 16 lanes of a ds_read_b128 group -- 16 different key rows, the SAME logical chunk -- would all hit one slot (16-way).  XOR with the
// row's low four bits sends those 16 rows (the groups are rows {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of a 32-key block: every
// value of row & 15 once) to 16 different slots.
constexpr int k_tile_off(int row, int chunk) { return row * K_ROW_BYTES + ((chunk ^ (row & 15)) << 4); }
// 128-byte rows: two rows per bank row, the layout of lds_tile_off (sat_common.h)
constexpr int vt_tile_off(int row, int chunk) { return row * VT_ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4); }

}  // namespace attn128
