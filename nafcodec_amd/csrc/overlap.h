// overlap.h -- paired records in HBM (the layout of nafgpu_encode_source) -> where read 1 and the reverse complement of read 2
// overlap, the adapter cut as regions that nafgpu_select takes, and the pairs joined into the records of a selection: what the
// host side (overlap.cpp, and select.cpp for nafgpu_merge_pairs) and the kernels (overlap.hip) share.  The rules:
// include/nafgpu.h at nafgpu_overlap.
//
//   k_sum_check        (summary.hip) per record: its end is not below the one in front of it and not beyond the section.  The
//                      kernels below do nothing once the table is flagged.
//   k_ovl_pairs        one wave per pair: the letters of both mates as three bit planes each in LDS, then lane = shift
//   k_ovl_finish       per pair: the regions of its two records, their flags for the compaction, the totals
//                                                   -> launch_scan_excl_u64 over the flags: where every unmerged region goes
//   k_ovl_compact      per record: the whole-record region of a record whose pair is not found to its place
// and for nafgpu_merge_pairs
//   k_ovl_found        per pair: 1 when it is found           -> launch_scan_excl_u64: which output record a found pair becomes
//   k_ovl_merge_sizes  per pair: the checks against the decoder's records, the output record's length, the sizes of its id and
//                      comment, the region {R1, 0, n1} that k_sel_strings copies them by
//                                                   -> launch_scan_excl_u64 per table, as nafgpu_select
//   k_ovl_merge        per tile of kOvlTile OUTPUT positions: letters and qualities, each lane one aligned 16-byte store per section
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace ovl {

constexpr uint32_t kOvlMaxLength = NAFGPU_OVERLAP_MAX_LENGTH;
constexpr uint32_t kOvlWords = kOvlMaxLength / 64;           // 64-bit words of a bit plane
#ifdef NAFGPU_EMU
constexpr uint32_t kOvlWaves = 1;                // (the harness runs one-wave workgroups: its ballot spans the workgroup)
#else
constexpr uint32_t kOvlWaves = 4;                // pairs a workgroup has in flight, a wave each
#endif
constexpr uint32_t kOvlTile = 4096;              // output positions per workgroup of the merge (16 per lane)
static_assert(kOvlMaxLength % 64 == 0 && 2 * kOvlMaxLength - 1 <= 64 * 32, "at most 32 rounds of 64 shifts");

// totals, zeroed: [0] pairs found, [1] too long, [2] records cut, [3] matches, [4] mismatches, [5] the inserts, [6] the regions' letters
constexpr uint32_t kOvlTotals = 7;

// status words as in select.h: [0] bits; [2..3], [4..5]: u64 complements of the lowest offender
constexpr uint32_t kOvlStRefused = 1, kOvlStBeyond = 2;

void launch_ovl_pairs(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_overlap_opts &opts,
                      const uint32_t *status, nafgpu_pair_overlap *pairs);
// flags: n records + 1 words ([n] = 0 here); totals: kOvlTotals words, zeroed
void launch_ovl_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, const uint32_t *status, const nafgpu_pair_overlap *pairs, nafgpu_region *regions,
                       uint64_t *flags, unsigned long long *totals);
// where: the exclusive sums of the flags
void launch_ovl_compact(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, const nafgpu_pair_overlap *pairs, const uint64_t *where, uint64_t n_unmerged,
                        nafgpu_region *unmerged);

// ---- nafgpu_merge_pairs (select.cpp)
// what select.cpp reads of a nafgpu_overlaps
struct OvlView {
    const nafgpu_pair_overlap *pairs;
    uint64_t n_records, n_pairs, n_found;
    int device;
    uint8_t quality_base;
};
OvlView view_of(const nafgpu_overlaps *o);

// flags: n_pairs + 1 words
void launch_ovl_found(hipStream_t stream, const nafgpu_pair_overlap *pairs, uint64_t n_pairs, uint64_t *flags);
// The decoder's buffers as the merge reads them.
struct OvlSource {
    const uint8_t *seq, *qual;                   // qual null: no qualities
    uint64_t n_seq, n_qual;
    const uint64_t *rec_end;  uint64_t n_rec;
    const uint8_t *ids;  const uint64_t *id_end;  uint64_t n_ids;
    const uint8_t *com;  const uint64_t *com_end;  uint64_t n_com;
};
// where: the exclusive sums of the found flags; n_out: the found pairs.  len / id_size / com_size: n_out + 1 words each (the last
// 0; the latter two may be null), pair_of: n_out words, regions: n_out
void launch_ovl_merge_sizes(hipStream_t stream, const nafgpu_pair_overlap *pairs, uint64_t n_pairs, const uint64_t *where, uint64_t n_out, const OvlSource &s,
                            uint64_t *len, uint64_t *id_size, uint64_t *com_size, uint64_t *pair_of, nafgpu_region *regions, uint32_t *status);
// excl: the scanned lengths (n_out + 1 words); table: the 256-byte complement table in device memory; dst_seq / dst_qual:
// 16-byte aligned, n_bytes rounded up to 16 (the bytes behind n_bytes are written as zeros); dst_qual null without qualities
void launch_ovl_merge(hipStream_t stream, const nafgpu_pair_overlap *pairs, const uint64_t *pair_of, const uint64_t *excl, uint64_t n_out, uint64_t n_bytes,
                      const OvlSource &s, const uint8_t *table, uint8_t quality_base, uint8_t *dst_seq, uint8_t *dst_qual);

}  // namespace ovl
}  // namespace nafgpu
