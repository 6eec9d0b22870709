// screen.h -- the k-mers of a reference as a set in HBM, and records in HBM screened against it: what the host side
// (screen.cpp) and the kernels (screen.hip) share.  The rules: include/nafgpu.h at nafgpu_kmers_build and nafgpu_screen.
//
//   k_sum_check      (summary.hip) per record: its end is not below the one in front of it and not beyond the section.  The
//                    kernels below do nothing once the table is flagged.
//   k_kmer_count     per run of kScreenRun tiles of kScreenTile window STARTS: the windows of the source, which size the table
//   k_kmer_insert    the same walk: every window's key goes into the table (linear probing, atomicCAS against the zeroed
//                    slot); the winning CAS are the distinct keys
//   k_screen_tiles   the same walk over the query: a window adds to its record's count, a window whose key is in the table
//                    to its hits, and keeps the lowest start and the highest end by 64-bit atomics
//   k_screen_finish  per record (per pair of mates): match, keep, the region, the totals
//                                                    -> launch_scan_excl_u64 over the keep flags: where every kept region goes
//   k_screen_compact per record: a kept record's whole-record region to its place
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace scr {

constexpr uint32_t kScreenTile = 4096;           // window starts per workgroup and round (16 per lane)
constexpr uint32_t kScreenHalo = 32;             // letters behind a tile that its windows reach into: k - 1 <= 30, in whole lanes
constexpr uint32_t kScreenRun = 8;               // consecutive tiles a workgroup takes
constexpr uint32_t kScreenMaxK = 31;             // 2 k bits and the value of an empty slot fit a 64-bit word
static_assert(kScreenHalo >= kScreenMaxK - 1 && kScreenHalo % 16 == 0, "a window that starts in a tile ends in its halo");
static_assert(NAFGPU_KMER_MAX_K == kScreenMaxK, "include/nafgpu.h states the same limit");

// The set as the kernels see it.  A slot holds key + 1 (a key is below 4^31, so the word is never 0), 0: empty.
//   slots      a power of two
//   hash_mask  ~0, or the low bits a hash is cut to (NAFGPU_KMER_HASH_BITS): tests reach long probe chains
struct KmerTable {
    unsigned long long *slot;
    uint64_t slots, hash_mask;
    uint32_t k;
    bool canonical;
};

// status words: the eight of summary.h (k_sum_check fills [0] and [2..5]); bit kScrStFull of [0]: an insert found no free
// slot (only NAFGPU_KMER_SLOTS can make the table that small)
constexpr uint32_t kScrStFull = 0x100;

// what k_screen_tiles leaves per record, zeroed first
//   windows, hits   counts (they are outputs as they are)
//   first           the complement of the lowest start of a matching window, relative to the record (atomicMax keeps the lowest); 0: none
//   last            the highest end of a matching window (at least k, so 0: none)
struct ScreenWork {
    unsigned long long *windows, *hits, *first, *last;
};

// totals, zeroed: [0] matched records, [1] windows, [2] hits, [3] letters of the kept records
constexpr uint32_t kScreenTotals = 4;

// n_rec = 0: the whole section is record 0.  count: one word, zeroed.
void launch_kmer_count(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                       const uint32_t *status, unsigned long long *count);
// table.slot: zeroed; distinct: one word, zeroed; status: written (kScrStFull)
void launch_kmer_insert(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                        uint32_t *status, unsigned long long *distinct);
void launch_screen_tiles(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                         const uint32_t *status, const ScreenWork &work);
// flags: n records + 1 words ([n] = 0 here); totals: kScreenTotals words, zeroed
void launch_screen_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_screen_opts &opts, const uint32_t *status,
                          const ScreenWork &work, nafgpu_region *regions, uint8_t *match, uint8_t *keep, uint64_t *flags, unsigned long long *totals);
// where: the exclusive sums of the flags
void launch_screen_compact(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const uint8_t *keep, const uint64_t *where,
                           uint64_t n_kept, nafgpu_region *kept);

}  // namespace scr
}  // namespace nafgpu
