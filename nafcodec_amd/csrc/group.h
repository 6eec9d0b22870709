// group.h -- records in HBM (the layout of nafgpu_encode_source) -> the groups of records whose sequences are equal: what the
// host side (group.cpp) and the kernels (group.hip) share.  The rules: include/nafgpu.h at nafgpu_group.
//
//   k_sum_check    (summary.hip) per record: its end is not below the one in front of it and not beyond the section.  The
//                  kernels below that read letters do nothing once the table is flagged.
//   k_grp_hash     per run of kGrpRun tiles of kGrpTile bytes: a 64-bit hash per record over its canonicalised letters, in
//                  8-letter words counted from the record's start; with both strands a second one over the reverse complement
//   k_grp_table    per record that is not settled: its index into an open-addressing table keyed by (length, hashes); a slot
//   k_grp_probe    keeps the lowest index of its key.  Then per record: cand[k], the lowest index with k's key
//   k_grp_verify   per run of tiles: the letters of every record with cand[k] != k against the same offsets of cand[k],
//                  forwards and (both strands) backwards and complemented; a difference sets a bit of flags[k]
//   k_grp_settle   per record: its representative, or it stays for another round (hashes that collided)
//   k_grp_flag / launch_scan_excl_u64 / k_grp_fill / k_grp_largest   the groups: numbered by ascending representative
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace grp {

constexpr uint32_t kGrpTile = 4096;              // input bytes per workgroup and round (16 per lane)
constexpr uint32_t kGrpRun = 16;                 // consecutive tiles a workgroup takes: it adds to a record's hashes when the record changes or the run ends
constexpr uint32_t kGrpHalo = 16;                // letters behind a tile that its last word reaches into (7 at the most), in whole lanes
constexpr uint32_t kGrpFewPieces = 4;            // a tile with fewer record boundaries than this goes the long route
constexpr uint32_t kGrpSub = 8;                  // the short route: lanes that share a record, each every eighth word

// What the kernels canonicalise by, made on the host.  canon[b]: what byte b is compared as (nucleotide: an IUPAC letter
// becomes its upper case and U becomes T, so that equal 4-bit codes are equal bytes; every other byte and the bytes alphabet:
// b itself).  comp[c]: the complement of the canonical byte c (the code with its bits reversed; any other byte is itself).
struct GroupTables {
    uint8_t canon[256];
    uint8_t comp[256];
};
void group_tables(bool nucleotide, GroupTables *out);     // host

// flags[k] (k_grp_probe sets, k_grp_verify adds to): record k differs from cand[k] read forwards / read backwards and complemented
constexpr uint32_t kGrpDiffForward = 1, kGrpDiffReverse = 2;

// status: the eight words of summary.h (k_sum_check fills them).  hf, hr: n_rec words each, zeroed (hr null: one strand)
void launch_grp_hash(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                     const GroupTables *d_tables, unsigned long long *hf, unsigned long long *hr, const uint32_t *status);
// the hashes cut to their low bits (NAFGPU_GRP_HASH_BITS): tests reach the rounds
void launch_grp_cut(hipStream_t stream, unsigned long long *hf, unsigned long long *hr, uint64_t n_rec, uint64_t mask);
// table: `slots` words (a power of two, >= 2 x n_rec), zeroed.  active: n_rec bytes, 1 = not settled yet.
void launch_grp_table(hipStream_t stream, const uint64_t *ends, const unsigned long long *hf, const unsigned long long *hr, const uint8_t *active,
                      uint64_t n_rec, unsigned long long *table, uint64_t slots, uint64_t *cand, uint32_t *flags);
void launch_grp_verify(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                       const GroupTables *d_tables, const uint64_t *cand, const uint8_t *active, uint32_t *flags, const uint32_t *status);
// representative, strand (null: one strand): written for the records that settle; left: one word, zeroed, the records that stay
void launch_grp_settle(hipStream_t stream, const uint64_t *cand, const uint32_t *flags, uint8_t *active, uint64_t n_rec, uint64_t *representative,
                       uint8_t *strand, unsigned long long *left);
// is_first: n_rec + 1 words, [k] = representative[k] == k, [n_rec] = 0 (the caller scans them in place: group_of of the first ones)
void launch_grp_flag(hipStream_t stream, const uint64_t *representative, uint64_t n_rec, uint64_t *is_first);
// group_of: the scanned words; group_first, group_size (zeroed): n_groups words; largest: one word, zeroed
void launch_grp_fill(hipStream_t stream, const uint64_t *representative, uint64_t n_rec, uint64_t *group_of, uint64_t *group_first,
                     unsigned long long *group_size);
void launch_grp_largest(hipStream_t stream, const unsigned long long *group_size, uint64_t n_groups, unsigned long long *largest);

}  // namespace grp
}  // namespace nafgpu
