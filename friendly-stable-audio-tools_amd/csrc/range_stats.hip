// fp16 range use of an activation buffer (include/sat_hip.h: sat_range_record): max |x| over the finite elements, the elements at or beyond
// the fp16 clamp (+-65504) and the non-finite ones, accumulated into one 32-byte record on the device.  The kernel behind
// sat_dit_range_report / sat_oobleck_range_report and the sat_range_stats_* unit entry points; it runs only while a report is enabled.
//   * a strided 2-D view [rows, cols] at `pitch` elements; columns cols..pitch-1 are never loaded into the statistics
//   * 16-byte loads over the aligned part of every row (8 fp16 / bf16 or 4 fp32 elements), a scalar tail for the cols % VEC rest; a view
//     whose rows do not start on 16 bytes (pitch % VEC != 0, an unaligned base) is read element by element
//   * per thread -> wave (__shfl_xor) -> workgroup (LDS) -> ONE global atomic per workgroup and field: atomicMax on the bit pattern of the
//     non-negative float (monotone in the value), 64-bit atomicAdd on the counters.  Maximum and integer sums commute: the record is
//     bit-reproducible whatever the order the workgroups finish in
//   * grid = min(ceil(elements / (256 * 16)), 2 * CUs) workgroups of 256 threads, grid-stride over the work items
#include <stddef.h>

#include "sat_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr float FP16_MAX = 65504.f;

struct Acc {
    float mx = 0.f;
    unsigned over = 0, nonf = 0;          // per thread: at most elements / threads, far below 2^32 for any buffer that fits the device
    __device__ __forceinline__ void add(float v) {
        const float a = fabsf(v);
        const bool fin = a < __builtin_inff();          // false for inf and NaN
        mx = fin ? fmaxf(mx, a) : mx;
        nonf += fin ? 0u : 1u;
        over += (!fin || a >= FP16_MAX) ? 1u : 0u;
    }
};

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void range_stats_kernel(const T* __restrict__ x, long long rows, long long cols, long long pitch,
                                                                 int vec_ok, unsigned long long counted, sat_range_record* __restrict__ rec) {
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const long long vpr = vec_ok ? cols / VEC : 0;          // 16-byte pieces per row
    const long long tail = cols - vpr * VEC;                // elements per row behind them
    const long long step = (long long)gridDim.x * RS_THREADS, first = (long long)blockIdx.x * RS_THREADS + threadIdx.x;
    Acc acc;
    for (long long i = first; i < rows * vpr; i += step) {
        const long long r = rows == 1 ? 0 : i / vpr, c = i - r * vpr;
        const vec_t v = *reinterpret_cast<const vec_t*>(x + r * pitch + c * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.add((float)v[e]);
    }
    for (long long i = first; i < rows * tail; i += step) {
        const long long r = rows == 1 ? 0 : i / tail, c = vpr * VEC + (i - r * tail);
        acc.add((float)x[r * pitch + c]);
    }
    // wave, then workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc.mx = fmaxf(acc.mx, __shfl_xor(acc.mx, o));
        acc.over += __shfl_xor(acc.over, o);
        acc.nonf += __shfl_xor(acc.nonf, o);
    }
    __shared__ float s_mx[RS_THREADS / 64];
    __shared__ unsigned s_over[RS_THREADS / 64], s_nonf[RS_THREADS / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mx[wave] = acc.mx; s_over[wave] = acc.over; s_nonf[wave] = acc.nonf; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float mx = 0.f;
    unsigned long long over = 0, nonf = 0;
#pragma unroll
    for (int w = 0; w < RS_THREADS / 64; ++w) { mx = fmaxf(mx, s_mx[w]); over += s_over[w]; nonf += s_nonf[w]; }
    // (a zero contributes nothing: the atomic is skipped, the result is the same)
    if (mx > 0.f) atomicMax(reinterpret_cast<unsigned*>(&rec->max_abs), __float_as_uint(mx));
    if (over) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->over_fp16), over);
    if (nonf) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->nonfinite), nonf);
    if (blockIdx.x == 0) {
        atomicAdd(&rec->launches, 1u);
        atomicAdd(reinterpret_cast<unsigned long long*>(&rec->elements), counted);
    }
}

template <typename T>
int launch(const void* x, long long rows, long long cols, long long pitch, uint64_t counted, sat_range_record* rec, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (pitch == cols || rows == 1) {          // contiguous: one long row
        cols *= rows; rows = 1; pitch = cols;
    }
    const int vec_ok = ((uintptr_t)x & 15) == 0 && (rows == 1 || pitch % VEC == 0);
    const int cus = sat_device_cus();
    SAT_CHECK_ARG(cus > 0, SAT_E_INVALID, "range_stats: no device");
    const long long want = (rows * cols + RS_THREADS * 16 - 1) / (RS_THREADS * 16);
    const int grid = (int)(want < 2 * cus ? want : 2 * cus);
    hipLaunchKernelGGL(range_stats_kernel<T>, dim3(grid), dim3(RS_THREADS), 0, s, (const T*)x, rows, cols, pitch, vec_ok,
                       (unsigned long long)counted, rec);
    SAT_LAUNCH_CHECK();
    return 0;
}

}  // namespace

static_assert(sizeof(sat_range_record) == 32 && offsetof(sat_range_record, over_fp16) == 8 && offsetof(sat_range_record, elements) == 24,
              "sat_range_record layout");

int sat_launch_range_stats(const void* x, int dtype, int64_t rows, int64_t cols, int64_t pitch, uint64_t counted, sat_range_record* rec,
                           hipStream_t s) {
    SAT_CHECK_ARG(x && rec && ((uintptr_t)rec & 7) == 0, SAT_E_INVALID, "range_stats: null buffer, or a record that is not 8-byte aligned");
    if (rows == 1) pitch = cols;          // (one row: the pitch is never used)
    SAT_CHECK_ARG(rows > 0 && cols > 0 && pitch >= cols, SAT_E_INVALID, "range_stats: view of %lld x %lld at pitch %lld", (long long)rows,
                  (long long)cols, (long long)pitch);
    SAT_CHECK_ARG(rows <= (1ll << 40) / pitch, SAT_E_INVALID, "range_stats: view of %lld rows at pitch %lld is too large", (long long)rows,
                  (long long)pitch);
    switch (dtype) {
        case SAT_GEMM_FP16: return launch<_Float16>(x, rows, cols, pitch, counted, rec, s);
        case SAT_GEMM_BF16: return launch<__bf16>(x, rows, cols, pitch, counted, rec, s);
        case SAT_GEMM_FP32X: return launch<float>(x, rows, cols, pitch, counted, rec, s);
    }
    SAT_CHECK_ARG(false, SAT_E_INVALID, "range_stats: element type %d is not SAT_GEMM_BF16, SAT_GEMM_FP16 or SAT_GEMM_FP32X", dtype);
    return 0;
}
