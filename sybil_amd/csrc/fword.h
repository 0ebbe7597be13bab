// fword.h -- the layout of a filter word (Table::fwords, table.cpp: table_build_fword), host and device.
//
// A filter word holds the stored offsets of a query's filter columns as bit fields of ONE 4-byte word per row: field i is
// bits[i] wide -- the bit length of column i's largest exact stored offset, at least 1 -- and starts at shift[i], the sum of the
// earlier fields' bits, the columns in ascending column index.  Four consecutive rows are four dwords, which is what a lane of
// k_scan_packed loads (scan_packed.h: packed_scan_dyn) and what a thread of k_pack_fword writes (kernels.hip).  A word has at
// least two fields and at most 32 bits in all, so no field is 32 bits wide.
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

constexpr int kFwordMaxFields = 4;  // (= kFastMaxF, scan_fast.h: one field per filter column of a FastPlan)
constexpr int kFwordMinFields = 2;
constexpr int kFwordBits = 32;

// bit length of a field whose largest offset is max_off: 0 and 1 -> 1, 999 -> 10, 2^32 - 1 -> 32
SYBL_HD int fword_bits(uint32_t max_off) {
    int b = 1;
    while (b < 32 && (max_off >> b) != 0) b++;
    return b;
}

// bits[i] and shift[i] of n fields from their largest offsets; returns the bits the word needs (a word exists iff <= kFwordBits)
SYBL_HD int fword_layout(const uint32_t *max_off, int n, int32_t *bits, int32_t *shift) {
    int total = 0;
    for (int i = 0; i < n; i++) {
        bits[i] = fword_bits(max_off[i]);
        shift[i] = total;
        total += bits[i];
    }
    return total;
}

// (bits < 32: a 32-bit field would be a word of one column)
SYBL_HD uint32_t fword_mask(int bits) { return (1u << bits) - 1u; }

// offsets[i] < 2^bits[i] for every field: the fields do not overlap, so the word is their sum
SYBL_HD uint32_t fword_pack(const uint32_t *offsets, int n, const int32_t *shifts) {
    uint32_t w = 0;
    for (int i = 0; i < n; i++) w |= offsets[i] << shifts[i];
    return w;
}

SYBL_HD uint32_t fword_field(uint32_t word, int shift, int bits) { return (word >> shift) & fword_mask(bits); }

// The bytes a row of one column costs a scan that reads no word: the stored width, a 4-byte AGGREGATION column that has or can
// get a narrow twin (narrow3.h: offsets below 2^24) counted at the twin's 3.  A word must save bytes over the sum of these, so
// a set must cost at least 5: two 1-byte keys and a 20-bit aggregation do (5 -> 4), one 1-byte key and a 2-byte aggregation do not.
SYBL_HD int word_bytes_today(int elem, uint32_t max_off, bool is_agg) { return is_agg && elem == 4 && max_off < (1u << 24) ? 3 : elem; }

// what k_pack_fword reads (kernels.hip: launch_pack_fword): the n source columns in field order, each at its stored width
struct FwordPack {
    const void *col[kFwordMaxFields];
    int32_t wid[kFwordMaxFields];  // 1 / 2 / 4 bytes a row
    int32_t shift[kFwordMaxFields], bits[kFwordMaxFields];
    int32_t n;
};

}  // namespace sybl
