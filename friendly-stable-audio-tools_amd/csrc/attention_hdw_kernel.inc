// The kernel of attention_hdw.hip, which includes this text twice inside its anonymous namespace: as attention_hdw_kernel<W> (ATTN_HDW_CAUSAL
// false: the kernel as it always was, under the name it always had) and as attention_hdw_causal_kernel<W> (ATTN_HDW_CAUSAL true).  Two kernels of
// one text rather than one template with a flag or a shared device function: the non-causal kernel keeps its symbol and its code, instruction
// for instruction.
// CAUSAL: self-attention of a causal model (Sq == Sk, query i sees the keys j <= i of its sequence), with the ranges of attn_causal.h exactly as
// in attention.hip: the workgroup walks the tiles up to the diagonal of its last query, a wave skips the 32-key blocks above its own last query,
// masks per element where the diagonal crosses a block and runs the blocks below it unmasked.  The first block of every sequence holds key 0,
// which every query sees, so it still sets a real reference.
template <int W>
__global__ __launch_bounds__(512) void ATTN_HDW_KERNEL(const op_t* __restrict__ q, const op_t* __restrict__ k, const op_t* __restrict__ vt,
                                                       op_t* __restrict__ out, int H, int KVH, int Sq, int Sk, int Sq_pad, int Sk_pad) {
    constexpr bool CAUSAL = ATTN_HDW_CAUSAL;
    using T = attnw::Tiles<W>;
    constexpr int KT = T::KV_TILE, KSTEPS = W / 16, DB = W / 32, KB = KT / 32;
    constexpr int K_LPR = T::K_ROW_BYTES / 16, V_LPR = T::VT_ROW_BYTES / 16;      // DMA lanes per LDS row
    sat_f16_saturate();
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    // consecutive LOGICAL workgroup ids (x = query block fastest) share an XCD and so one L2 copy of their K / V^T: attention.hip
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int lid = xcd_remap(lin, gridDim.x * gridDim.y * gridDim.z);
    const int bx = lid % gridDim.x;
    const int h = (lid / gridDim.x) % gridDim.y, b = lid / (gridDim.x * gridDim.y);
    const int kvh = h / (H / KVH);
    const int qi = bx * Q_BLOCK + wave * 32 + l31;         // the last workgroup may reach beyond Sq_pad

    // Q fragments (B operand of S^T): Q[qi][16t + 8*half .. +8]
    opx8 qf[KSTEPS];
    {
        const op_t* qp = q + ((size_t)(b * H + h) * Sq_pad + (qi < Sq_pad ? qi : Sq_pad - 1)) * W + half * 8;
#pragma unroll
        for (int t = 0; t < KSTEPS; ++t) qf[t] = *reinterpret_cast<const opx8*>(qp + t * 16);
    }

    // K rows / V^T columns of sequence b start at ob = (b*Sk) & 3 (head_split_hdw.hip, kind bit 2)
    const int ob = (b * Sk) & 3;
    const int k_end = ob + Sk;
    // n_tiles * KT <= Sk_pad: the launcher checks Sk_pad >= Sk + 3, Sk_pad % KT == 0 (CAUSAL: no more tiles than that)
    const int n_tiles = CAUSAL ? attnc::tiles_walked(bx * Q_BLOCK, Q_BLOCK, ob, Sk, KT) : (k_end + KT - 1) / KT;
    [[maybe_unused]] const int cq_first = CAUSAL ? __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32) : 0;      // CAUSAL: the wave's first query ...
    [[maybe_unused]] const int c_end = CAUSAL ? attnc::key_end(qi, ob, Sk) : 0;                                      // ... and one past the lane's last visible key

    // LDS-DMA pieces of this wave: pieces `wave + 8 i` of the K tile and of the V^T tile.  Lane l of a piece lands at byte 16 l of its KiB,
    // i.e. at row (piece KiB + 16 l) / ROW_BYTES, slot l % (ROW_BYTES / 16), and fetches the logical chunk slot ^ key(row) from HBM
    const op_t* kbase = k + (size_t)(b * KVH + kvh) * Sk_pad * W;
    const op_t* vbase = vt + (size_t)(b * KVH + kvh) * W * Sk_pad;
    const op_t* ksrc[T::K_PIECES];
    const op_t* vsrc[T::VT_PIECES];
#pragma unroll
    for (int i = 0; i < T::K_PIECES; ++i) {
        const int krow = T::k_dma_row(wave + 8 * i, lane);                              // < KT
        int chunk = T::k_dma_chunk(wave + 8 * i, lane);
        if constexpr (T::K_HOLES)
            if (chunk >= T::K_CHUNKS) chunk = 0;                                        // W = 96: a hole of the padded row
        ksrc[i] = kbase + (size_t)krow * W + (chunk << 3);                              // + tile * KT rows
    }
#pragma unroll
    for (int i = 0; i < T::VT_PIECES; ++i) {
        int vrow = T::vt_dma_row(wave + 8 * i, lane);
        const int chunk = T::vt_dma_chunk(wave + 8 * i, lane);                          // (of the LDS row it lands in)
        if constexpr (T::VT_SPARE)
            if (vrow >= W) vrow -= 32;                                                  // W = 96: the spare rows 96..127
        vsrc[i] = vbase + (size_t)vrow * Sk_pad + (chunk << 3);                         // + tile * KT keys
    }
    auto stage_in = [&](int tile, int stage) {
        char* sk = smem + stage * T::STAGE_BYTES;
        char* sv = sk + T::K_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < T::K_PIECES; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ksrc[i] + (size_t)tile * KT * W),
                                             (__attribute__((address_space(3))) void*)(sk + (wave + 8 * i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < T::VT_PIECES; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vsrc[i] + (size_t)tile * KT),
                                             (__attribute__((address_space(3))) void*)(sv + (wave + 8 * i) * 1024), 16, 0, 0);
    };
    constexpr int PIECES = T::K_PIECES + T::VT_PIECES;      // per wave and tile

    f32x16 oacc[DB];        // O^T: channels d = db*32 + 8*(r>>2) + 4*half + (r&3) of the lane's query
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -1e30f;   // reference, log2 units (Q is pre-scaled)
    float l_run = 0.f;      // this lane's partial row sum (its 16 of every 32 keys)

    // a wave whose 32 queries are all beyond Sq still copies tiles and joins the barriers, but skips the matrix and softmax work
    const bool wave_active = __builtin_amdgcn_readfirstlane(bx * Q_BLOCK + wave * 32) < Sq;

    auto process = [&](int tile, int stage) {
        const char* sk = smem + stage * T::STAGE_BYTES;
        const char* sv = sk + T::K_TILE_BYTES;
        const bool edge = (tile == 0 && ob != 0) || (tile == n_tiles - 1 && (k_end & (KT - 1)) != 0);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            if (!CAUSAL && KB > 2 && tile * KT + kb * 32 >= k_end) break;      // the rest of the last tile is pad (wave-uniform); block 0 of a tile never is
            [[maybe_unused]] int cls = attnc::FULL;
            if constexpr (CAUSAL) {
                cls = attnc::block_class(tile * KT + kb * 32, cq_first, 32, ob, Sk);
                if (cls == attnc::SKIP) break;      // (wave-uniform; the later blocks lie higher still)
            }
            // ---- S^T = K Q^T for 32 keys
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int t = 0; t < KSTEPS; ++t) {
                const opx8 kf = *reinterpret_cast<const opx8*>(sk + T::k_tile_off(kb * 32 + l31, t * 2 + half));
                sacc = mfma_32x32x16(kf, qf[t], sacc);
            }
            // V^T fragments do not depend on the softmax: request them now, their LDS latency hides behind the VALU work
            opx8 vf[DB][2];
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int u = 0; u < 2; ++u) vf[db][u] = *reinterpret_cast<const opx8*>(sv + T::vt_tile_off(db * 32 + l31, (kb * 2 + u) * 2 + half));
            // ---- mask the keys outside [ob, k_end) (wave-uniform branch: first and last tile only)
            if (CAUSAL ? cls == attnc::DIAG : edge) {
                const int key0 = tile * KT + kb * 32 + 4 * half;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + (r & 3) + 8 * (r >> 2);
                    if (key < ob || key >= (CAUSAL ? c_end : k_end)) sacc[r] = -INFINITY;      // (in the compare itself: a named copy of the bound changes the non-causal code)
                }
            }
            // ---- online softmax step against the standing reference
            opx8 pb[2];
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(sacc[r] - m_run);
                psum += p;
                pb[r >> 3][r & 7] = f32_to_op(p);
            }
            if (!__all(psum <= 4096.0f)) {      // wave-uniform; always in the sequence's first block (reference -1e30), later for a score > 12 octaves above it
                float mloc = sacc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, sacc[r]);
                const float m_new = fmaxf(m_run, half_max(mloc));
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < DB; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
                psum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sacc[r] - m_run);
                    psum += p;
                    pb[r >> 3][r & 7] = f32_to_op(p);
                }
            }
            l_run += psum;
            // ---- O^T += V^T P^T
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int u = 0; u < 2; ++u) oacc[db] = mfma_32x32x16(vf[db][u], pb[u], oacc[db]);
        }
    };

    // tile it + 1 stays in flight across the barrier (counted vmcnt: this wave issued PIECES pieces for it); tile it + 2 goes into the stage
    // tile it - 1 occupied, which every wave left before this barrier
    stage_in(0, 0);
    if (n_tiles > 1) stage_in(1, 1);
    int st = 0;
    for (int it = 0; it < n_tiles; ++it) {
        if (it + 1 < n_tiles) wait_vmcnt<PIECES>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        const int st2 = st >= 1 ? st - 1 : 2;                 // (it + 2) % 3
        if (it + 2 < n_tiles) stage_in(it + 2, st2);
        if (wave_active) process(it, st);
        st = st == 2 ? 0 : st + 1;
    }

    const float inv = 1.0f / half_sum(l_run);
    op_t* op = out + ((size_t)b * Sq + qi) * ((size_t)H * W) + h * W + 8 * half;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
        unsigned pk[8];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            pk[2 * rq] = pack_op2(oacc[db][rq * 4] * inv, oacc[db][rq * 4 + 1] * inv);
            pk[2 * rq + 1] = pack_op2(oacc[db][rq * 4 + 2] * inv, oacc[db][rq * 4 + 3] * inv);
        }
        half_swap(pk[0], pk[2]);            // 8 consecutive channels per lane: one 16-byte store instead of two 8-byte ones
        half_swap(pk[1], pk[3]);
        half_swap(pk[4], pk[6]);
        half_swap(pk[5], pk[7]);
        if (qi < Sq) {
            *reinterpret_cast<u32x4*>(op + db * 32) = u32x4{pk[0], pk[1], pk[2], pk[3]};
            *reinterpret_cast<u32x4*>(op + db * 32 + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
        }
    }
}
