// trim.h -- records in HBM (the layout of nafgpu_encode_source) -> the window of every record that quality trimming keeps, as
// regions that nafgpu_select takes: what the host side (trim.cpp) and the kernels (trim.hip) share.  The rules:
// include/nafgpu.h at nafgpu_trim.
//
//   k_sum_check     (summary.hip) per record: its end is not below the one in front of it and not beyond the section.  The
//                   kernels below do nothing once the table is flagged.
//   k_trim_init     per record: its window [0, L); a record of more than kTrimShort letters goes onto the lists of the long route
//   k_trim_sum      step 1, per record END: the running sum walks inward in chunks with a carried sum, kTrimShortLanes lanes
//                   of 16 bytes per chunk for a short record (four record ends per wave), a workgroup per chunk for a long one
//   k_trim_window   step 2, per run of kTrimRun tiles of kTrimTile window STARTS: the lowest failing window of every record,
//                   kept by a 64-bit atomic
//   k_trim_n        step 3, per record: the N at either end of what steps 1 and 2 left, in chunks as k_trim_sum
//   k_trim_finish   step 4, per record (per pair of mates): canonical form, keep flag, region, the totals
//                                                   -> launch_scan_excl_u64 over the keep flags: where every kept region goes
//   k_trim_compact  per record: a kept record's region to its place
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace trm {

constexpr uint32_t kTrimTile = 4096;             // window starts per workgroup and round (16 per lane)
constexpr uint32_t kTrimHalo = 64;               // quality bytes behind a tile that its windows reach into: 64 - 1, in whole lanes
constexpr uint32_t kTrimRun = 8;                 // consecutive tiles a workgroup takes
constexpr uint32_t kTrimMaxWindow = 64;
constexpr uint32_t kTrimShort = 1024;            // a record of up to this many letters is walked by kTrimShortLanes lanes
constexpr uint32_t kTrimShortLanes = 16;         // lanes per chunk on the short route: a chunk of 256 bytes
constexpr uint32_t kTrimLongLanes = 256;         // and on the long one: a chunk of 4 096 bytes
static_assert(kTrimHalo >= kTrimMaxWindow - 1 && kTrimHalo % 16 == 0, "a window that starts in a tile ends in its halo");
static_assert(kTrimMaxWindow * 510u < (1u << 16), "a window's sum and its threshold fit 32 bits with room");

// What the kernels work on between the steps, in device memory.
//   win       2 words per record: the window [a, b) relative to the record's first letter (a > b: crossed cuts, empty)
//   cut       a word per record, zeroed: the complement of the lowest failing window start (atomicMax keeps the lowest); 0: none
//   list_sum  [0]: how many items follow (zeroed); an item is record * 2 + end (0 front, 1 tail): the long route of step 1
//   list_n    the same for step 3; an item is a record
//   list_cap  items either list holds; more long records than the section has room for cannot be
struct TrimWork {
    uint64_t *win;
    unsigned long long *cut;
    unsigned long long *list_sum, *list_n;
    uint64_t list_cap;
};
inline uint64_t trim_list_cap(uint64_t n_section) { return 2 * (n_section / kTrimShort) + 2; }

// totals, zeroed: [0] records whose window is not [0, L), [1] the sum of b - a over all records, [2] over the kept ones
constexpr uint32_t kTrimTotals = 3;

// n_rec = 0: the whole section is record 0.  status: the eight words of summary.h (k_sum_check fills them).
void launch_trim_init(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_trim_opts &opts, const uint32_t *status,
                      const TrimWork &work);
void launch_trim_sum(hipStream_t stream, const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_trim_opts &opts,
                     const uint32_t *status, const TrimWork &work);
void launch_trim_window(hipStream_t stream, const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_trim_opts &opts,
                        const uint32_t *status, const TrimWork &work);
void launch_trim_n(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const uint32_t *status,
                   const TrimWork &work);
// flags: n records + 1 words ([n] = 0 here); totals: kTrimTotals words, zeroed
void launch_trim_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_trim_opts &opts, const uint32_t *status,
                        const TrimWork &work, nafgpu_region *regions, uint8_t *keep, uint64_t *flags, unsigned long long *totals);
// where: the exclusive sums of the flags
void launch_trim_compact(hipStream_t stream, const nafgpu_region *regions, const uint8_t *keep, const uint64_t *where, uint64_t n_out, uint64_t n_kept,
                         nafgpu_region *kept);

}  // namespace trm
}  // namespace nafgpu
