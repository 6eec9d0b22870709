// select.h -- records and regions of a decoded archive -> a new set of records in HBM, in the layout nafgpu_encode_source
// takes: what the host side (select.cpp) and the kernels (select.hip) share.  The rules: include/nafgpu.h at nafgpu_select.
//
// Region k becomes output record k.  Three passes:
//   k_sel_sizes    per region: the checks, its length, where its letters lie, the sizes of its id and comment
//                                                    -> launch_scan_excl_u64 per table: the three end tables
//   k_sel_gather   per tile of kSelTile OUTPUT bytes: the letters (and, a second launch, the qualities) of every region that
//                  has bytes in the tile, each lane one aligned 16-byte store
//   k_sel_strings  per region: id (with ":START-END" and "/rc" when the regions are named) and comment, NUL-terminated
// and for nafgpu_find_records k_sel_id_table / k_sel_id_probe: an open-addressing table of record indices keyed by a hash
// of the id bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nafgpu.h"
#include "container.h"
#include "kernels.h"

namespace nafgpu {
namespace sel {

constexpr uint32_t kSelTile = 4096;              // output bytes per workgroup (16 per lane)

// What a decoder holds after decode_all_device (api.cpp fills it; device pointers, null: the field was not decoded).
struct SelSource {
    const uint8_t *seq = nullptr;   uint64_t n_seq = 0;     // letters that were decoded (what format_device checks records against)
    const uint8_t *qual = nullptr;  uint64_t n_qual = 0;
    const uint64_t *rec_end = nullptr;  uint64_t n_rec = 0; // the records the decoder yields
    const uint8_t *ids = nullptr;   const uint64_t *id_end = nullptr;   uint64_t n_ids = 0;
    const uint8_t *com = nullptr;   const uint64_t *com_end = nullptr;  uint64_t n_com = 0;
    uint8_t sequence_type = 0, name_separator = ' ';
    int device = 0;
};
// api.cpp: decodes if nothing is decoded yet, makes the checks nafgpu_format_device makes (shard, tiled output, a section that
// failed) and describes the buffers.  need_lengths: the Length section must be there (nafgpu_select).
Failure decoder_source(nafgpu_decoder *dec, bool need_lengths, SelSource *out);
int decoder_fail(nafgpu_decoder *dec, const Failure &f, nafgpu_error *err);   // *err filled and kept for nafgpu_last_error

// status words (8 x u32, zeroed first).  [0]: bits; [2..3], [4..5]: u64 complements (atomicMax keeps the lowest) of the first
// region the rules refuse and of the first region whose record lies beyond what was decoded.
constexpr uint32_t kSelStRefused = 1, kSelStBeyond = 2;

// An end table of n entries is scanned in place from sizes: `excl` has n + 1 entries (excl[0] = 0, excl[k + 1] = the
// inclusive end k), so table = excl + 1.  Buffers of n + 2 words keep both excl + 1 and the buffer 16-byte aligned.
struct SelSizes {
    uint64_t *len;        // excl of the record ends: n + 1 words, [n] = 0 before the scan
    uint64_t *src;        // n words: offset of the region's first letter in the section; bit 63: reverse strand
    uint64_t *id_size;    // n + 1 words (null: no ids): bytes of the output id with its NUL
    uint64_t *com_size;   // n + 1 words (null: no comments)
};
constexpr uint64_t kSelReverse = 1ull << 63;

void launch_sel_sizes(hipStream_t stream, const nafgpu_region *regions, uint64_t n, const SelSource &s, bool named, const SelSizes &o,
                      uint32_t *status);
// One section (letters: table = the 256-byte complement table in device memory; qualities: null) of all regions.
// dst: 16-byte aligned, at least n_out rounded up to 16 bytes (the bytes behind n_out are written as zeros).
// excl / src as in SelSizes after the scan; any_reverse: some region has bit 63 set.
void launch_sel_gather(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *excl, const uint64_t *src,
                       uint64_t n_regions, uint64_t n_out, const uint8_t *table, bool any_reverse, uint8_t *dst);
void launch_sel_strings(hipStream_t stream, const nafgpu_region *regions, uint64_t n, const SelSource &s, bool named, const uint64_t *len_excl,
                        const uint64_t *id_excl, uint8_t *ids, const uint64_t *com_excl, uint8_t *com);

// nafgpu_find_records.  table: `slots` words (a power of two, >= 2 x n_ids), zeroed; hash_bits < 64: the hash is cut to so
// many bits before the slot is taken (NAFGPU_SEL_HASH_BITS).
void launch_sel_id_table(hipStream_t stream, const uint8_t *ids, const uint64_t *id_end, uint64_t n_ids, unsigned long long *table,
                         uint64_t slots, uint32_t hash_bits);
// names: NUL-terminated, concatenated; name_end[j]: offset just past the NUL of name j
void launch_sel_id_probe(hipStream_t stream, const uint8_t *ids, const uint64_t *id_end, const unsigned long long *table, uint64_t slots,
                         uint32_t hash_bits, const uint8_t *names, const uint64_t *name_end, uint64_t n_names, uint64_t *record_out);

void complement_table(uint8_t sequence_type, uint8_t out[256]);   // host: what a reverse-complemented letter becomes

}  // namespace sel
}  // namespace nafgpu
