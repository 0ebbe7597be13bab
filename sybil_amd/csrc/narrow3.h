// narrow3.h -- the 3-byte layout of a narrow twin (Column::narrow, table.cpp: column_build_narrow), host and device.
//
// A twin holds the stored offsets of a 4-byte column whose largest offset is below 2^24 at three bytes a row: row i is the
// little-endian 24-bit number at byte 3 * i.  Four consecutive rows are therefore exactly three little-endian dwords, which is
// what a lane of k_scan_packed loads (scan_packed.h: packed_decode) and what a thread of k_narrow3 writes (kernels.hip).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#ifndef SYBL_HD
#ifdef __HIPCC__
#define SYBL_HD __host__ __device__ __forceinline__
#else
#define SYBL_HD inline
#endif
#endif

namespace sybl {

constexpr int kNarrowWidth = 3;                      // bytes per row of a twin
constexpr uint32_t kNarrowLimit = 1u << 24;          // offsets a twin holds: 0 .. kNarrowLimit - 1

// u[0..3]: four consecutive rows' offsets (bits above the 24th are dropped) -> d[0..2]
SYBL_HD void pack3(const uint32_t (&u)[4], uint32_t (&d)[3]) {
    const uint32_t a = u[0] & 0xFFFFFFu, b = u[1] & 0xFFFFFFu, c = u[2] & 0xFFFFFFu, e = u[3] & 0xFFFFFFu;
    d[0] = a | (b << 24);
    d[1] = (b >> 8) | (c << 16);
    d[2] = (c >> 16) | (e << 8);
}

SYBL_HD void unpack3(const uint32_t (&d)[3], uint32_t (&u)[4]) {
    u[0] = d[0] & 0xFFFFFFu;
    u[1] = (d[0] >> 24) | ((d[1] & 0xFFFFu) << 8);
    u[2] = (d[1] >> 16) | ((d[2] & 0xFFu) << 16);
    u[3] = d[2] >> 8;
}

}  // namespace sybl
