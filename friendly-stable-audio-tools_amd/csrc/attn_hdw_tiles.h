// LDS geometry of the attention kernel for 32-, 96- and 128-channel heads (attention_hdw.hip).  Integer logic only, no device code: host
// programs and tests include it as it is (tests/dit_head_width_units.py checks that every map is a bijection onto its tile and that the
// fragment reads of the kernel are free of bank conflicts; tests/test_dit_head_width_host.py and tests/test_dit_head_dim_host.py run it).
#pragma once

namespace attnw {

// One map for every row length the three widths need.  A bank row of LDS is 256 B = sixteen 16-byte slots; a tile row of ROW_BYTES covers
// ROW_BYTES / 16 of them, so 256 / ROW_BYTES tile rows share one bank row.  The 16 lanes of a ds_read_b128 group read the SAME logical chunk
// of 16 different rows (rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} of a 32-row block: every value of row & 15 once); the XOR key is the
// part of row & 15 that does NOT already select the position inside the bank row:
//   256-byte rows: the bank row is the row, so un-swizzled the slot would be the chunk index alone and the 16 lanes would all hit one slot
//                  (16-way); key = row & 15 sends them to 16 different slots
//   128-byte rows: bit 0 of the row selects the half, key = (row >> 1) & 7 (lds_tile_off of sat_common.h)
//    64-byte rows: bits 0-1 select the quarter, key = (row >> 2) & 3
constexpr int swz_off(int row_bytes, int row, int chunk) {
    return row * row_bytes + ((chunk ^ (row_bytes == 256 ? (row & 15) : row_bytes == 128 ? ((row >> 1) & 7) : ((row >> 2) & 3))) << 4);
}

template <int W>
struct Tiles {
    static_assert(W == 32 || W == 96 || W == 128, "head widths of attention_hdw.hip");
    static constexpr int HEAD_DIM = W;
    // W = 32: a 64-key stage would be 4 + 4 KiB and the per-tile barrier would come round after 2 x (2 + 2) MFMAs per wave; 128 keys make it
    // 8 + 8 KiB and 16 MFMAs.  W = 96, 128: 64 keys (24 and 32 MFMAs per wave and tile)
    static constexpr int KV_TILE = W == 32 ? 128 : 64;
    static constexpr int K_CHUNKS = W / 8;                                 // 16-byte chunks of a K row that hold data: 4, 12 or 16
    // K tile rows in LDS.  W = 32: the 64 B of the HBM row.  W = 128: the 256 B of the HBM row, exactly one bank row.  W = 96: the 192-byte
    // HBM row PADDED to 256 B -- chunk ^ (row & 15) is not closed over 12 chunks, over the 16 slots of a padded row it is; the 4 slots of
    // every row that no chunk maps to are never read (the LDS-DMA lanes that land there fetch an in-bounds address of the same row)
    static constexpr int K_ROW_BYTES = W == 32 ? 64 : 256;
    static constexpr int VT_ROW_BYTES = KV_TILE * 2;                       // V^T tile: channel rows of 256 B (W = 32) or 128 B (W = 96, 128)
    static constexpr int VT_ROWS = W == 32 ? 32 : 128;                     // W = 96: 96 channel rows + 32 spare, so that every wave copies two 1-KiB pieces
    static constexpr bool K_HOLES = K_CHUNKS * 16 < K_ROW_BYTES;           // W = 96 only: slots of a K row that no chunk maps to
    static constexpr bool VT_SPARE = VT_ROWS > W;                          // W = 96 only: rows of the V^T tile behind the last channel
    static constexpr int K_TILE_BYTES = KV_TILE * K_ROW_BYTES;             // 8 KiB | 16 KiB
    static constexpr int VT_TILE_BYTES = VT_ROWS * VT_ROW_BYTES;           // 8 KiB | 16 KiB
    static constexpr int STAGE_BYTES = K_TILE_BYTES + VT_TILE_BYTES;       // 16 KiB | 32 KiB
    static constexpr int STAGES = 3;
    static constexpr int LDS_BYTES = STAGES * STAGE_BYTES;                 // 48 KiB (two workgroups per CU) | 96 KiB
    static constexpr int K_PIECES = K_TILE_BYTES / 1024 / 8;               // 1-KiB LDS-DMA pieces per wave (8 waves) and tile: 1 | 2
    static constexpr int VT_PIECES = VT_TILE_BYTES / 1024 / 8;             // 1 | 2

    static constexpr int k_tile_off(int row, int chunk) { return swz_off(K_ROW_BYTES, row, chunk); }
    static constexpr int vt_tile_off(int row, int chunk) { return swz_off(VT_ROW_BYTES, row, chunk); }
    // The LDS-DMA writes lane l of piece p at byte p * 1024 + 16 l: which (row, logical chunk) belongs there.  chunk >= K_CHUNKS: a hole;
    // row >= W of the V^T tile: a spare row
    static constexpr int k_dma_row(int piece, int lane) { return (piece * 1024 + lane * 16) / K_ROW_BYTES; }
    static constexpr int k_dma_chunk(int piece, int lane) {
        return (swz_off(K_ROW_BYTES, k_dma_row(piece, lane), (lane * 16 % K_ROW_BYTES) >> 4) - k_dma_row(piece, lane) * K_ROW_BYTES) >> 4;
    }
    static constexpr int vt_dma_row(int piece, int lane) { return (piece * 1024 + lane * 16) / VT_ROW_BYTES; }
    static constexpr int vt_dma_chunk(int piece, int lane) {
        return (swz_off(VT_ROW_BYTES, vt_dma_row(piece, lane), (lane * 16 % VT_ROW_BYTES) >> 4) - vt_dma_row(piece, lane) * VT_ROW_BYTES) >> 4;
    }
};

}  // namespace attnw
