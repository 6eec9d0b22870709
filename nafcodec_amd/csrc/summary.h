// summary.h -- records in HBM (the layout of nafgpu_encode_source) -> a small table per record: what the host side
// (summary.cpp) and the kernels (summary.hip) share.  The rules: include/nafgpu.h at nafgpu_summarize.
//
//   k_sum_check    per record: its end is not below the one in front of it and not beyond the section; the lowest offender
//                  of either kind is kept.  The kernels below do nothing once one is flagged.
//   k_sum_hist     per chunk of kSumHistChunk bytes: how often each byte value occurs (one launch per section)
//   k_sum_tiles    per run of kSumRun tiles of kSumTile bytes: the eight class counts (a second instantiation: the sum of
//                  the quality bytes) of every record that has letters in the run, by one of two routes per tile
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace sum {

constexpr uint32_t kSumTile = 4096;              // input bytes per workgroup and round (16 per lane)
constexpr uint32_t kSumRun = 16;                 // consecutive tiles a workgroup takes: it adds to a record's row when the record changes or the run ends
constexpr uint64_t kSumHistChunk = 1ull << 20;   // bytes a workgroup counts into its 32-bit LDS bins before it adds them to the 64-bit ones
constexpr uint32_t kSumFewPieces = 4;            // a tile with fewer record boundaries than this goes the long route
static_assert(kSumHistChunk < (1ull << 32) && kSumHistChunk % kSumTile == 0, "a 32-bit bin holds a whole chunk");

// NAFGPU_SUM_ROUTE (after nafgpu_test_hooks(1)): "long" / "short" force one route on every tile, whatever it holds
enum Route : uint32_t { kRouteAuto = 0, kRouteLong = 1, kRouteShort = 2 };

// status words (8 x u32, zeroed first).  [0]: bits; [2..3], [4..5]: u64 complements (atomicMax keeps the lowest) of the first
// record whose end is below the one in front of it and of the first whose end lies beyond the section; [6..7]: the last end.
constexpr uint32_t kSumStDecreasing = 1, kSumStBeyond = 2;

void launch_sum_check(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, uint32_t *status);
// hist: 256 words, zeroed
void launch_sum_hist(hipStream_t stream, const uint8_t *section, uint64_t n_section, unsigned long long *hist);
// classes: 256 bytes in device memory, rows: n_rec x 8 words, zeroed, 16-byte aligned -- or classes null: the bytes' own values
// are summed, rows: n_rec words, zeroed.  status: as k_sum_check left it.
void launch_sum_tiles(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                      const uint8_t *classes, Route route, unsigned long long *rows, const uint32_t *status);

void default_classes(uint8_t out[256]);          // host: the table of include/nafgpu.h

}  // namespace sum
}  // namespace nafgpu
