// bitmap_rank.h -- what samples.hip and select.hip share on the way from a row bitmap (k_prefilter: a bit per physical
// row) to ranked rows: the block descriptor, a block's bitmap word, the wave scan, and the per-block popcount.  Kernels are
// not defined here (a __global__ in two translation units is two host stubs of one name): each file wraps smp_count_block
// in a kernel of its own (k_smp_count, k_sel_count).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sybl {

constexpr int kSmpThreads = 256;           // k_smp_count / k_smp_compact / k_sel_rows: four waves, a 32-bit bitmap word per lane

struct SmpBlock {
    int64_t start;  // first physical row (a multiple of 32)
    int64_t n;      // logical rows
    int64_t lbase;  // table-wide logical index of the block's first row
};

// word i of a block of n rows: its bitmap word (every row when there is no bitmap), rows beyond n masked off
__device__ __forceinline__ uint32_t smp_word(const uint32_t *bits, int64_t w0, int64_t i, int64_t n) {
    uint32_t w = bits ? bits[w0 + i] : 0xFFFFFFFFu;
    const int64_t left = n - i * 32;
    if (left < 32) w &= (1u << (uint32_t)left) - 1u;
    return w;
}

// inclusive scan over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// ---- m_b: a workgroup per block, lanes take 32-bit words, one store per block.  bits is indexed from word `word0`.
__device__ __forceinline__ void smp_count_block(const uint32_t *bits, int64_t word0, const SmpBlock *blk, int64_t *cnt) {
    __shared__ int64_t part[kSmpThreads / 64];
    const SmpBlock B = blk[blockIdx.x];
    const int64_t words = (B.n + 31) >> 5, w0 = (B.start >> 5) - word0;
    int64_t c = 0;
    for (int64_t i = threadIdx.x; i < words; i += kSmpThreads) c += __popc(smp_word(bits, w0, i, B.n));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int w = 0; w < kSmpThreads / 64; w++) s += part[w];
        cnt[blockIdx.x] = s;
    }
}

}  // namespace sybl
