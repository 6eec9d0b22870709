// search.h -- records in HBM (the layout of nafgpu_encode_source) -> where a set of short patterns occurs, as regions that
// nafgpu_select takes: what the host side (search.cpp) and the kernels (search.hip) share.  The rules: include/nafgpu.h at
// nafgpu_search.
//
//   k_sum_check      (summary.hip) per record: its end is not below the one in front of it and not beyond the section.  The
//                    kernels below do nothing once the table is flagged.
//   k_search_tiles   per run of kSearchRun tiles of kSearchTile window STARTS, twice:
//                      count   how many hits start in every tile, and how many every row has
//                                                    -> launch_scan_excl_u64 over the tiles: where every tile writes
//                      write   the same match again; every hit goes to its final index (a tile without hits is skipped)
//   k_search_begin   per record: the index of its first hit, a lower bound in the hits' record column
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace srch {

constexpr uint32_t kSearchTile = 4096;           // window starts per workgroup and round (16 per lane)
constexpr uint32_t kSearchHalo = 64;             // letters behind a tile that its windows reach into: NAFGPU_SEARCH_MAX_LENGTH - 1, in whole lanes
constexpr uint32_t kSearchRun = 8;               // consecutive tiles a workgroup takes with one copy of the tables in LDS
constexpr uint32_t kSearchMaxRows = 2 * NAFGPU_SEARCH_MAX_PATTERNS;   // a pattern and its reverse complement
static_assert(kSearchHalo >= NAFGPU_SEARCH_MAX_LENGTH - 1 && kSearchHalo % 16 == 0, "a window that starts in a tile ends in its halo");
static_assert(static_cast<uint64_t>(kSearchTile) * kSearchMaxRows < (1ull << 32), "a tile's hits fit 32 bits");

// What the kernels match by, made on the host: row r is pattern r >> strand_shift, the odd rows (strand_shift 1) its
// reverse complement.  accept[r * n_codes + c]: bit j is set when position j of the row accepts a letter with code c;
// code[b]: the code of byte value b (nucleotide: the 4-bit set, 0 for a byte that is no letter; bytes: b itself).
struct SearchRows {
    uint32_t n_rows, n_codes;                    // n_codes: 16 (nucleotide) or 256 (bytes)
    uint32_t strand_shift, reserved;
    uint8_t length[kSearchMaxRows];
    uint8_t code[256];
    uint64_t accept[NAFGPU_SEARCH_MAX_PATTERNS * 256];    // nucleotide: 32 rows x 16, bytes: 16 rows x 256
};

// status: the eight words of summary.h (k_sum_check fills them).  base: n_tiles + 1 words, count: the tiles' counts come
// here, [n_tiles] = 0; write: the exclusive sums of those.  row_hits: kSearchMaxRows words, zeroed (count pass only).
void launch_search_tiles(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                         const SearchRows *d_rows, bool nucleotide, uint32_t max_mismatches, const uint32_t *status, uint64_t *base,
                         unsigned long long *row_hits, nafgpu_region *regions, nafgpu_hit_info *info);
// begin: n_rec + 1 words
void launch_search_begin(hipStream_t stream, const nafgpu_region *regions, uint64_t n_hits, uint64_t n_rec, uint64_t *begin);

// host: the rules' refusals and the tables.  patterns: n_patterns NUL-terminated strings in n_bytes
Failure build_rows(const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns, const nafgpu_search_opts &opts, SearchRows *out);

}  // namespace srch
}  // namespace nafgpu
