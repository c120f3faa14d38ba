// l2i_range.hip — the range histogram of a stored map (include/l2i.h: l2i_range_stats): how many elements of a tensor sit in every fp32 octave, how
// many are exactly zero, and the largest finite magnitude.  What nets16.RangeMonitor puts behind the `_probe` points of the 16-bit path: the fp16
// gradient scales are judged by where the stored maps lie between fp16's 2^-24 and 2^16, and this is that statement without a host read, a
// float copy or a sort — one streaming read of the map, integer results, addable across calls, steps and hipGraph replays.
//
// One kernel, three element kinds (a template argument; `kind` is a run-time argument of the entry point, one object serves all three):
//   * every element is converted EXACTLY to the bit pattern of |x| as fp32 (fp16 and bf16 are subsets of fp32: integer operations only, no
//     rounding, no dependence on the denormal mode) and counted in the bin of its biased exponent field, 0 .. 255;
//   * 16-byte loads over the aligned body of the tensor (eight 16-bit or four fp32 elements a lane), block 0 takes the <= 7 elements in front of
//     the first 16-byte boundary and the <= 7 behind the last one by one;
//   * grid-stride loop under RANGE_MAX_BLOCKS blocks;
//   * every wave counts into its own 256-bin histogram in LDS, kept in RANGE_REPLICAS copies selected by the lane so that the lanes of one
//     ds_add — which on a gradient map mostly name the same two or three octaves — spread over that many banks instead of queueing on one
//     address; a lane first merges runs of equal octaves among its own eight elements.  A block reads at most 2^31 elements (entry point), so
//     every 32-bit counter holds;
//   * the zero count is a register per lane and one block sum, the maximum a register per lane and one block maximum (l2i_device.h);
//   * then one 64-bit integer atomic add per NON-EMPTY bin and block, one for the zeros, and one 64-bit atomic maximum per block.  Integer adds and
//     maxima commute: the row is bit-reproducible whatever the arrival order of the blocks, of the streams that share a row, or of the replays.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l2i.h"
#include "l2i_internal.h"
#include "l2i_device.h"

namespace {

constexpr int RANGE_THREADS = 256;                 // four waves
constexpr int RANGE_WAVES = RANGE_THREADS / 64;
constexpr int RANGE_REPLICAS = 8;                  // copies of a wave's histogram: 4 waves * 256 bins * 8 copies * 4 bytes = 32 KiB of LDS a block
constexpr int RANGE_DEPTH = 4;                     // 16-byte loads a lane issues before it counts the first
constexpr int RANGE_VEC_PER_BLOCK = 1024;          // 16-byte vectors a block takes before the grid is capped: one pass of its loop, RANGE_DEPTH loads a lane
constexpr int RANGE_MAX_BLOCKS = 1024;             // the block cap: beyond 2^20 vectors (2^23 16-bit or 2^22 fp32 elements) the loop takes more passes
constexpr int64_t RANGE_MAX_N = (int64_t)1 << 40;  // 2^40 elements / 1024 blocks = 2^30 a block: the 32-bit counters of a block cannot wrap

typedef unsigned long long u64;

// |x| as the fp32 bit pattern, exactly
__device__ __forceinline__ unsigned abs_bits_f16(unsigned h) {
    const unsigned e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return 0x7f800000u | (m << 13);                        // inf / NaN keep field 255 (payload kept)
    if (e) return ((e + 112u) << 23) | (m << 13);
    return __float_as_uint((float)m * 0x1p-24f);                         // zero and subnormals m * 2^-24: an integer <= 1023 times a power of two, exact; fields 103 .. 112
}
__device__ __forceinline__ unsigned abs_bits_bf16(unsigned h) { return (h & 0x7fffu) << 16; }
__device__ __forceinline__ unsigned abs_bits_f32(unsigned u) { return u & 0x7fffffffu; }

struct lane_stats {
    unsigned zeros, amax;          // exact zeros; largest |x| bits among the finite elements
    unsigned cur, run;             // the run of equal octaves being merged (run = 0: none)
};

__device__ __forceinline__ void flush_run(lane_stats& s, unsigned* __restrict__ hist) {
    if (s.run) atomicAdd(&hist[s.cur * RANGE_REPLICAS], s.run);
    s.run = 0;
}
__device__ __forceinline__ void count(lane_stats& s, unsigned a, unsigned* __restrict__ hist) {
    const unsigned f = a >> 23;
    s.zeros += a == 0u;
    if (f != 255u) s.amax = a > s.amax ? a : s.amax;
    if (s.run && f != s.cur) flush_run(s, hist);
    s.cur = f;
    s.run += 1;
}

template <int KIND>
__device__ __forceinline__ void count_vec(lane_stats& s, const u32x4& v, unsigned* __restrict__ hist) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (KIND == L2I_RANGE_F32) {
            count(s, abs_bits_f32(w[j]), hist);
        } else if constexpr (KIND == L2I_RANGE_F16) {
            count(s, abs_bits_f16(w[j] & 0xffffu), hist);
            count(s, abs_bits_f16(w[j] >> 16), hist);
        } else {
            count(s, abs_bits_bf16(w[j] & 0xffffu), hist);
            count(s, abs_bits_bf16(w[j] >> 16), hist);
        }
    }
}

template <int KIND>
__device__ __forceinline__ unsigned load_one(const void* __restrict__ x, long i) {
    if constexpr (KIND == L2I_RANGE_F32) return abs_bits_f32(reinterpret_cast<const unsigned*>(x)[i]);
    else if constexpr (KIND == L2I_RANGE_F16) return abs_bits_f16(reinterpret_cast<const unsigned short*>(x)[i]);
    else return abs_bits_bf16(reinterpret_cast<const unsigned short*>(x)[i]);
}

// x: n elements; the first `head` (< one vector) and the last `tail` (< one vector) are read one by one, the nv 16-byte vectors between them start
// on a 16-byte boundary.
template <int KIND>
__global__ __launch_bounds__(RANGE_THREADS) void range_stats_kernel(u64* __restrict__ row, const void* __restrict__ x, long n, int head, long nv, int tail) {
    __shared__ __attribute__((aligned(16))) unsigned hist_all[RANGE_WAVES * 256 * RANGE_REPLICAS];      // (read back as 16-byte vectors)
    __shared__ unsigned red[RANGE_WAVES];
    constexpr int PER = KIND == L2I_RANGE_F32 ? 4 : 8;
    constexpr int ES = KIND == L2I_RANGE_F32 ? 4 : 2;
    const int t = threadIdx.x;
    for (int i = t; i < RANGE_WAVES * 256 * RANGE_REPLICAS; i += RANGE_THREADS) hist_all[i] = 0u;
    __syncthreads();
    unsigned* __restrict__ hist = hist_all + (t >> 6) * (256 * RANGE_REPLICAS) + (t & (RANGE_REPLICAS - 1));      // this wave's histogram, this lane's copy
    lane_stats s = {0u, 0u, 0u, 0u};
    const u32x4* __restrict__ xv = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(x) + (long)head * ES);
    const long stride = (long)gridDim.x * RANGE_THREADS;
    // RANGE_DEPTH loads in flight per lane before the first is counted: one 16-byte load a wave at a time does not cover the HBM latency
    for (long i = (long)blockIdx.x * RANGE_THREADS + t; i < nv; i += RANGE_DEPTH * stride) {
        u32x4 v[RANGE_DEPTH] = {};
#pragma unroll
        for (int q = 0; q < RANGE_DEPTH; ++q)
            if (i + q * stride < nv) v[q] = xv[i + q * stride];
#pragma unroll
        for (int q = 0; q < RANGE_DEPTH; ++q)
            if (i + q * stride < nv) count_vec<KIND>(s, v[q], hist);
    }
    if (blockIdx.x == 0) {
        if (t < head) count(s, load_one<KIND>(x, t), hist);
        if (t < tail) count(s, load_one<KIND>(x, (long)head + nv * PER + t), hist);
    }
    flush_run(s, hist);
    const unsigned zeros = block_sum(s.zeros, red);                       // (its barriers also publish every wave's histogram)
    const unsigned amax = block_max(s.amax, red);
    u64 bin = 0;                                                          // thread t owns bin t: RANGE_REPLICAS consecutive counters of every wave
#pragma unroll
    for (int w = 0; w < RANGE_WAVES; ++w) {
        const u32x4* __restrict__ c = reinterpret_cast<const u32x4*>(hist_all + (w * 256 + t) * RANGE_REPLICAS);
#pragma unroll
        for (int q = 0; q < RANGE_REPLICAS / 4; ++q) {
            const u32x4 v = c[q];
            bin += (u64)v.x + (u64)v.y + (u64)v.z + (u64)v.w;
        }
    }
    if (bin) atomicAdd(row + t, bin);
    if (t == 0) {
        if (zeros) atomicAdd(row + L2I_RANGE_ZEROS, (u64)zeros);
        if (amax) atomicMax(row + L2I_RANGE_MAX, (u64)amax);
        if (blockIdx.x == 0) {
            atomicAdd(row + L2I_RANGE_CALLS, (u64)1);
            atomicAdd(row + L2I_RANGE_N, (u64)n);
        }
    }
}

}  // namespace

extern "C" int l2i_range_stats(uint64_t* row, const void* x, int64_t n, int kind, void* stream) {
    if (!row || !x || n <= 0) return l2i_set_error(L2I_E_ARG, "range_stats: null row / tensor or n <= 0");
    if (kind != L2I_RANGE_F16 && kind != L2I_RANGE_BF16 && kind != L2I_RANGE_F32) return l2i_set_error(L2I_E_ARG, "range_stats: kind is L2I_RANGE_F16 / _BF16 / _F32");
    const int es = kind == L2I_RANGE_F32 ? 4 : 2, per = 16 / es;
    const uintptr_t a = (uintptr_t)x;
    if ((a % es) || ((uintptr_t)row % 8)) return l2i_set_error(L2I_E_ARG, "range_stats: tensor off its element size or row off 8 bytes");
    if (n > RANGE_MAX_N) return l2i_set_error(L2I_E_UNSUPPORTED, "range_stats: more than 2^40 elements");
    const int mis = (int)(a & 15);
    long head = mis ? (16 - mis) / es : 0;
    if (head > n) head = n;
    const long nv = (n - head) / per;
    const int tail = (int)(n - head - nv * per);
    const int grid = l2i_grid_for(nv, RANGE_VEC_PER_BLOCK, RANGE_MAX_BLOCKS);
    u64* r = reinterpret_cast<u64*>(row);
    hipStream_t st = (hipStream_t)stream;
    if (kind == L2I_RANGE_F16) hipLaunchKernelGGL(range_stats_kernel<L2I_RANGE_F16>, dim3(grid), dim3(RANGE_THREADS), 0, st, r, x, (long)n, (int)head, nv, tail);
    else if (kind == L2I_RANGE_BF16) hipLaunchKernelGGL(range_stats_kernel<L2I_RANGE_BF16>, dim3(grid), dim3(RANGE_THREADS), 0, st, r, x, (long)n, (int)head, nv, tail);
    else hipLaunchKernelGGL(range_stats_kernel<L2I_RANGE_F32>, dim3(grid), dim3(RANGE_THREADS), 0, st, r, x, (long)n, (int)head, nv, tail);
    L2I_CHECK_LAUNCH();
    return L2I_OK;
}
