// pieces.h -- the work list of k_scan_packed's dynamic dealing (scan_packed.h: packed_scan_dyn): host and device, no HIP.
//
// The planner's runs of physical rows are cut into PIECES of at most piece_tiles tiles, in table order.  The workgroups of a scan
// take them from a device counter, one ticket at a time, so the rows being read at any moment are neighbours in the table
// whichever workgroup reads them, and a slow compute unit simply takes fewer pieces.
#pragma once
#include <stdint.h>

#include <vector>

namespace sybl {

constexpr int kPieceTileRows = 4096;                      // == kPackedTileRows (scan_packed.h asserts it)
constexpr int64_t kPieceChunkRows = (int64_t)1 << 28;     // == kPackedChunkRows
constexpr int kPieceTilesDefault = 32, kPieceTilesMax = (int)(kPieceChunkRows / kPieceTileRows);
constexpr int kPieceCapPct = 125;                         // a workgroup takes at most 5/4 of an equal share (+ 2)

struct Piece {
    int64_t start;  // physical row
    uint32_t n;     // rows: 1 .. piece_tiles * kPieceTileRows
};

// runs -> pieces, in table order.  No piece crosses its run's end or a multiple of kPieceChunkRows rows counted from the run's
// start (rows inside a piece are addressed with 32 bits); every piece of a run starts a whole number of tiles after the run's
// start, so only a run's last piece can end on a partial tile.  Run: anything with .start and .n (Segment, plan.h).
template <class Run>
inline void deal_pieces(const std::vector<Run> &runs, int piece_tiles, std::vector<Piece> &out) {
    out.clear();
    if (piece_tiles < 1) piece_tiles = 1;
    if (piece_tiles > kPieceTilesMax) piece_tiles = kPieceTilesMax;
    const int64_t piece_rows = (int64_t)piece_tiles * kPieceTileRows;
    for (const Run &r : runs) {
        for (int64_t off = 0; off < (int64_t)r.n;) {
            const int64_t chunk_end = (off / kPieceChunkRows + 1) * kPieceChunkRows;
            int64_t take = (int64_t)r.n - off;
            if (take > chunk_end - off) take = chunk_end - off;
            if (take > piece_rows) take = piece_rows;
            Piece p;
            p.start = (int64_t)r.start + off;
            p.n = (uint32_t)take;
            out.push_back(p);
            off += take;
        }
    }
}

// The most tickets one workgroup draws: pct / 100 of an equal share, rounded up, and two more (pct == 100, a test's setting:
// the share itself).  Tickets are unique, and a workgroup scans every piece whose ticket it drew.  It stops drawing when a
// ticket is past the table -- every piece has then been drawn by somebody -- or at the cap.  So a piece can only be left over
// if EVERY workgroup stopped at the cap, which takes n_wg * cap >= n_pieces tickets: none is left, and none is scanned twice.
constexpr int64_t piece_cap(int64_t n_pieces, int64_t n_wg, int64_t pct = kPieceCapPct) {
    if (n_wg < 1) n_wg = 1;
    if (pct < 100) pct = 100;
    return (n_pieces * pct + n_wg * 100 - 1) / (n_wg * 100) + (pct > 100 ? 2 : 0);
}
static_assert(piece_cap(0, 256) == 2 && piece_cap(256, 256, 100) == 1 && piece_cap(257, 256, 100) == 2, "piece_cap");
// the headline: 1e9 rows in pieces of 32 tiles on 256 workgroups
static_assert(piece_cap(7630, 256) == 40, "piece_cap");

}  // namespace sybl
