// Loads-only microbenchmark of row -> lane mappings for the config-3 column mix (3 x 2-byte, 2 x 1-byte, 2 x 4-byte columns,
// 16 stored bytes per row): what the load pattern alone delivers, without any row body.  R rows per lane and tile:
//   R = 4  : what k_scan_packed does (one dwordx4 per 2- / 4-byte column -- half of it range-checked away for 2 bytes --
//            and one dword per 1-byte column)
//   R = 8  : 4-byte columns two dwordx4 per lane (lane stride 32 B), 2-byte one dwordx4, 1-byte one dwordx2
//   R = 16 : 4-byte four dwordx4 (lane stride 64 B), 2-byte two, 1-byte one
// and, at R = 4, the same mix with the two 4-byte columns stored at 3 bytes per row (14 B/row, k_loads_narrow): a dwordx4 at a
// 12-byte lane stride behind a 768-byte descriptor (the fourth dword of lane 63 is range-checked away), or a dwordx3.  These
// run in turns against the 16 B mix and print min / median / max, so the two ranges can be set side by side.
// Last, the 14 B mix against two 12 B mixes (k_loads_fword), in turns again: the three 2-byte filter columns as one 4-byte
// "filter word" column (five loads per tile), and that with the two 1-byte key columns as one 2-byte column besides (four).
// And the 12 B filter-word mix against an 11 B mix (V = 3): the two keys and the first aggregation as one 4-byte "key word"
// beside the filter word and the second aggregation's 3-byte twin, three loads per tile, all dwordx4.
// build: hipcc --offload-arch=gfx950 -O3 -o loadpat loadpat.hip ; run: ./loadpat [rows]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
struct Cols { const uint8_t *c[7]; int w[7]; };
constexpr int kThreads = 1024;

template <int BYTES>  // bytes this lane reads of one column for one tile, as 16 / 8 / 4-byte buffer loads
__device__ __forceinline__ uint32_t load_lane(const uint8_t *wave_base, uint32_t wave_bytes, uint32_t lane_off) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)wave_base, 0, (int)wave_bytes, 0x00020000);
    uint32_t acc = 0;
    if (BYTES >= 16) {
#pragma unroll
        for (int k = 0; k < BYTES / 16; k++) {
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane_off + 16 * k), 0, 2);
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    } else if (BYTES == 8) {
        u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)lane_off, 0, 2);
        acc ^= v.x ^ v.y;
    } else {
        acc ^= __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)lane_off, 0, 2);
    }
    return acc;
}

// R rows per lane and tile; OVER: 2-byte columns read with a full dwordx4 per 4 rows (the current kernel's range-checked over-read)
template <int R, bool OVER>
__global__ __launch_bounds__(kThreads) void k_loads(Cols C, int64_t rows, uint32_t *out) {
    const int64_t per_wg = (rows / gridDim.x) / (kThreads * R) * (kThreads * R);
    const int64_t start = (int64_t)blockIdx.x * per_wg;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t acc = 0;
    for (int64_t t = 0; t < per_wg; t += kThreads * R) {
        const int64_t wave_row = start + t + (int64_t)wave * 64 * R;
#pragma unroll
        for (int c = 0; c < 7; c++) {
            const int w = c < 3 ? 2 : c < 5 ? 1 : 4;  // compile-time widths of the mix
            const uint8_t *base = C.c[c] + wave_row * w;
            const uint32_t wave_bytes = 64u * R * w, off = lane * R * w;
            if (w == 4) acc ^= load_lane<R * 4>(base, wave_bytes, off);
            else if (w == 2) acc ^= (OVER && R == 4) ? load_lane<16>(base, wave_bytes, off) : load_lane<R * 2>(base, wave_bytes, off);
            else acc ^= load_lane<R>(base, wave_bytes, off);
        }
    }
    if (acc == 0x12345678u) out[0] = acc;
}

// R = 4 with the two aggregation columns AW bytes wide (4: today's mix, 3: the narrow twins); X3: a dwordx3 for the 3-byte columns
template <int AW, bool X3>
__global__ __launch_bounds__(kThreads) void k_loads_narrow(Cols C, int64_t rows, uint32_t *out) {
    const int64_t per_wg = (rows / gridDim.x) / (kThreads * 4) * (kThreads * 4);
    const int64_t start = (int64_t)blockIdx.x * per_wg;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t acc = 0;
    for (int64_t t = 0; t < per_wg; t += kThreads * 4) {
        const int64_t wave_row = start + t + (int64_t)wave * 256;
#pragma unroll
        for (int c = 0; c < 7; c++) {
            const int w = c < 3 ? 2 : c < 5 ? 1 : AW;
            const uint8_t *base = C.c[c] + wave_row * w;
            const uint32_t wave_bytes = 256u * w, off = lane * 4 * w;
            if (w == 1) acc ^= load_lane<4>(base, wave_bytes, off);
            else if (w == 3 && X3) {
                const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, (int)wave_bytes, 0x00020000);
                u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)off, 0, 2);
                acc ^= v.x ^ v.y ^ v.z;
            } else acc ^= load_lane<16>(base, wave_bytes, off);
        }
    }
    if (acc == 0x12345678u) out[0] = acc;
}

// The 14 B mix (V = 0) against 12 B mixes: V = 1 reads one 4-byte column for the three 2-byte ones (a full dwordx4, 5 loads per
// tile); V = 2 also reads one 2-byte column (a dwordx2) for the two 1-byte ones (4 loads per tile); V = 3 reads the filter word,
// one 4-byte key word (X.c[2]) for the two 1-byte keys and the first 3-byte twin, and the second twin: 11 B/row, 3 loads per
// tile.  X holds the filter word, the key pair and the key word.
template <int V>
__global__ __launch_bounds__(kThreads) void k_loads_fword(Cols C, Cols X, int64_t rows, uint32_t *out) {
    const int64_t per_wg = (rows / gridDim.x) / (kThreads * 4) * (kThreads * 4);
    const int64_t start = (int64_t)blockIdx.x * per_wg;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t acc = 0;
    for (int64_t t = 0; t < per_wg; t += kThreads * 4) {
        const int64_t wave_row = start + t + (int64_t)wave * 256;
        if (V == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) acc ^= load_lane<16>(C.c[c] + wave_row * 2, 512u, lane * 8);
        } else acc ^= load_lane<16>(X.c[0] + wave_row * 4, 1024u, lane * 16);
        if (V <= 1) {
#pragma unroll
            for (int c = 3; c < 5; c++) acc ^= load_lane<4>(C.c[c] + wave_row, 256u, lane * 4);
        } else if (V == 2) acc ^= load_lane<8>(X.c[1] + wave_row * 2, 512u, lane * 8);
        else acc ^= load_lane<16>(X.c[2] + wave_row * 4, 1024u, lane * 16);
#pragma unroll
        for (int c = V == 3 ? 6 : 5; c < 7; c++) acc ^= load_lane<16>(C.c[c] + wave_row * 3, 768u, lane * 12);
    }
    if (acc == 0x12345678u) out[0] = acc;
}

int main(int argc, char **argv) {
    const int64_t rows = argc > 1 ? atoll(argv[1]) : 1000000000LL;
    Cols C;
    const int widths[7] = {2, 2, 2, 1, 1, 4, 4};
    for (int c = 0; c < 7; c++) {
        C.w[c] = widths[c];
        void *p;
        if (hipMalloc(&p, (size_t)rows * widths[c] + 4096) != hipSuccess) { printf("alloc failed\n"); return 1; }
        hipMemset(p, c + 1, (size_t)rows * widths[c] + 4096);
        C.c[c] = (const uint8_t *)p;
    }
    Cols X = {};
    const int xwidths[3] = {4, 2, 4};  // the filter word, the key pair and the key word of k_loads_fword
    for (int c = 0; c < 3; c++) {
        X.w[c] = xwidths[c];
        void *p;
        if (hipMalloc(&p, (size_t)rows * xwidths[c] + 4096) != hipSuccess) { printf("alloc failed\n"); return 1; }
        hipMemset(p, c + 8, (size_t)rows * xwidths[c] + 4096);
        X.c[c] = (const uint8_t *)p;
    }
    uint32_t *out;
    hipMalloc((void **)&out, 4);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    auto run = [&](const char *name, auto kern, int wgs) {
        float best = 1e9f;
        for (int it = 0; it < 5; it++) {
            hipEventRecord(e0);
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(kThreads), 0, 0, C, rows, out);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            if (it > 0 && ms < best) best = ms;
        }
        printf("%-34s wgs %4d  %.3f ms  %.0f GB/s of 16 B/row\n", name, wgs, best, rows * 16.0 / (best * 1e-3) / 1e9);
    };
    for (int wgs : {256, 512}) {
        run("R=4 (current: 2-byte over-read)", k_loads<4, true>, wgs);
        run("R=4 exact (dwordx2 for 2-byte)", k_loads<4, false>, wgs);
        run("R=8", k_loads<8, false>, wgs);
        run("R=16", k_loads<16, false>, wgs);
    }
    // the 16 B mix against the 14 B mix, in turns: one launch of each per turn, the first turn dropped
    for (int wgs : {256, 512}) {
        const int kTurns = 11;
        float ms[3][kTurns];
        for (int it = 0; it < kTurns; it++)
            for (int v = 0; v < 3; v++) {
                hipEventRecord(e0);
                if (v == 0) hipLaunchKernelGGL((k_loads_narrow<4, false>), dim3(wgs), dim3(kThreads), 0, 0, C, rows, out);
                if (v == 1) hipLaunchKernelGGL((k_loads_narrow<3, false>), dim3(wgs), dim3(kThreads), 0, 0, C, rows, out);
                if (v == 2) hipLaunchKernelGGL((k_loads_narrow<3, true>), dim3(wgs), dim3(kThreads), 0, 0, C, rows, out);
                hipEventRecord(e1);
                hipEventSynchronize(e1);
                hipEventElapsedTime(&ms[v][it], e0, e1);
            }
        const char *names[3] = {"16 B mix (4-byte agg, dwordx4)", "14 B mix (3-byte agg, dwordx4)", "14 B mix (3-byte agg, dwordx3)"};
        for (int v = 0; v < 3; v++) {
            float *m = ms[v] + 1;
            for (int i = 0; i < kTurns - 1; i++)
                for (int j = i + 1; j < kTurns - 1; j++)
                    if (m[j] < m[i]) { float t = m[i]; m[i] = m[j]; m[j] = t; }
            const double b = v == 0 ? 16.0 : 14.0;
            printf("%-34s wgs %4d  min %.3f  med %.3f  max %.3f ms  %.0f GB/s of %.0f B/row at the median\n", names[v], wgs, m[0],
                   m[(kTurns - 1) / 2], m[kTurns - 2], rows * b / (m[(kTurns - 1) / 2] * 1e-3) / 1e9, b);
        }
    }
    // the 14 B mix against the 12 B mixes, in turns as above
    for (int wgs : {256, 512}) {
        const int kTurns = 11;
        float ms[3][kTurns];
        for (int it = 0; it < kTurns; it++)
            for (int v = 0; v < 3; v++) {
                hipEventRecord(e0);
                if (v == 0) hipLaunchKernelGGL((k_loads_fword<0>), dim3(wgs), dim3(kThreads), 0, 0, C, X, rows, out);
                if (v == 1) hipLaunchKernelGGL((k_loads_fword<1>), dim3(wgs), dim3(kThreads), 0, 0, C, X, rows, out);
                if (v == 2) hipLaunchKernelGGL((k_loads_fword<2>), dim3(wgs), dim3(kThreads), 0, 0, C, X, rows, out);
                hipEventRecord(e1);
                hipEventSynchronize(e1);
                hipEventElapsedTime(&ms[v][it], e0, e1);
            }
        const char *names[3] = {"14 B mix (3 x 2-byte filters)", "12 B mix (filter word)", "12 B mix (filter word, key pair)"};
        for (int v = 0; v < 3; v++) {
            float *m = ms[v] + 1;
            for (int i = 0; i < kTurns - 1; i++)
                for (int j = i + 1; j < kTurns - 1; j++)
                    if (m[j] < m[i]) { float t = m[i]; m[i] = m[j]; m[j] = t; }
            const double b = v == 0 ? 14.0 : 12.0;
            printf("%-34s wgs %4d  min %.3f  med %.3f  max %.3f ms  %.0f GB/s of %.0f B/row at the median\n", names[v], wgs, m[0],
                   m[(kTurns - 1) / 2], m[kTurns - 2], rows * b / (m[(kTurns - 1) / 2] * 1e-3) / 1e9, b);
        }
    }
    // the 12 B filter-word mix against the 11 B mix with a key word, in turns as above
    for (int wgs : {256, 512}) {
        const int kTurns = 11;
        float ms[2][kTurns];
        for (int it = 0; it < kTurns; it++)
            for (int v = 0; v < 2; v++) {
                hipEventRecord(e0);
                if (v == 0) hipLaunchKernelGGL((k_loads_fword<1>), dim3(wgs), dim3(kThreads), 0, 0, C, X, rows, out);
                if (v == 1) hipLaunchKernelGGL((k_loads_fword<3>), dim3(wgs), dim3(kThreads), 0, 0, C, X, rows, out);
                hipEventRecord(e1);
                hipEventSynchronize(e1);
                hipEventElapsedTime(&ms[v][it], e0, e1);
            }
        const char *names[2] = {"12 B mix (filter word)", "11 B mix (filter word, key word)"};
        for (int v = 0; v < 2; v++) {
            float *m = ms[v] + 1;
            for (int i = 0; i < kTurns - 1; i++)
                for (int j = i + 1; j < kTurns - 1; j++)
                    if (m[j] < m[i]) { float t = m[i]; m[i] = m[j]; m[j] = t; }
            const double b = v == 0 ? 12.0 : 11.0;
            printf("%-34s wgs %4d  min %.3f  med %.3f  max %.3f ms  %.0f GB/s of %.0f B/row at the median\n", names[v], wgs, m[0],
                   m[(kTurns - 1) / 2], m[kTurns - 2], rows * b / (m[(kTurns - 1) / 2] * 1e-3) / 1e9, b);
        }
    }
    return 0;
}
