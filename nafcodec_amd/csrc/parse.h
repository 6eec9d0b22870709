// parse.h -- FASTA / FASTQ text in HBM -> records in the layout nafgpu_encode_source takes: what the text parser's host
// front end (parse.cpp) and its kernels (parse.hip) share.
//
// The text is cut into tiles of kParseTile bytes, counted from the 16-byte boundary at or in front of its first byte
// (`shift` = the pointer's low four bits), so that every 16-byte load is aligned whatever the pointer.  Three passes:
//   k_parse_summary  per tile: how it changes the parse state        -> k_parse_scan_*: the state entering every tile
//   k_parse_count    per tile: records opened, bytes per field, longest line, the checks
//                                                                     -> launch_scan_excl_u64 per field: where every tile writes
//   k_parse_write    per tile: the four fields compacted through an LDS image, record ends
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace nafgpu {
namespace parse {

constexpr uint32_t kParseTile = 4096;            // text bytes per workgroup (16 per lane)

// One per tile.  k_parse_summary writes the tile's own; the scan replaces it by that of all tiles in front.
struct ParseTile {
    uint64_t line_start;     // text offset of the last line start (0: none, which is also the first line's)
    uint32_t summary;        // parse.hip: kSum*
    uint32_t pad;
};

enum ParseField : uint32_t { kOpen = 0, kSeq, kQual, kId, kCom, kParseFields };   // counts[f * n_tiles + tile]

struct ParseTotals {         // device memory, zeroed before k_parse_count
    ScanTotals field[kParseFields];   // .sum: the field's total (launch_scan_excl_u64)
    uint64_t line_length;             // longest sequence line
    uint64_t pad;
};

// status words (8 x u32, zeroed first).  [0]: bits; [2..3], [4..5], [6..7]: u64 complements (atomicMax keeps the lowest) of
// the first offending line's offset, the first NUL's offset, the first record whose quality has another length.
constexpr uint32_t kParseStLine = 1, kParseStNul = 2, kParseStQual = 4;

struct ParseOut {            // k_parse_write's destinations and their sizes (the totals of the count pass)
    uint8_t *seq;  uint64_t n_seq;
    uint8_t *qual; uint64_t n_qual;
    uint8_t *ids;  uint64_t n_ids;       // with one NUL per record
    uint8_t *com;  uint64_t n_com;
    uint64_t *rec_end;  uint64_t n_rec;  // inclusive
    uint64_t *qual_end;                  // FASTQ: the same for the quality bytes (scratch: the length check)
};

uint64_t parse_tiles(const uint8_t *text, uint64_t n);
void launch_parse_summary(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, ParseTile *tiles);
uint64_t parse_scan_aggs(uint64_t n_tiles);       // entries of `aggs`: one per 2048 tiles
void launch_parse_scan_tiles(hipStream_t stream, ParseTile *tiles, uint64_t n_tiles, ParseTile *aggs);
void launch_parse_count(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, const ParseTile *tiles, uint64_t *counts,
                        ParseTotals *totals, uint32_t *status);
// counts: scanned in place, field by field
void launch_parse_write(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, const ParseTile *tiles, const uint64_t *counts,
                        const ParseOut &out);
void launch_parse_qual_check(hipStream_t stream, const uint64_t *rec_end, const uint64_t *qual_end, uint64_t n_rec, uint32_t *status);

}  // namespace parse
}  // namespace nafgpu
