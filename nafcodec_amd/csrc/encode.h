// encode.h -- what the host encoder (synth.cpp), the device encoder's front end (encode.cpp) and its kernels
// (encode.hip) share: the block plan of a literal-only section, the literals plan of a block with sequences, and the launchers.
//
// A literal-only block is decided by symbol counts alone (plan_block); only writing its four bit streams needs the
// bytes.  The host path is  count -> plan_block -> emit_block;  the device path is  k_enc_hist -> plan_block on the host
// -> k_enc_streams / k_enc_scatter.  Both give the same frame, byte for byte.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/nafgpu.h"
#include "container.h"

namespace nafgpu {
namespace enc {

constexpr size_t kChunkBlocks = 64;     // blocks encoded as one unit (first block carries a fresh table)

struct HufCode {
    uint8_t len[256];       // 0 = symbol absent
    uint16_t code[256];
    uint8_t weight[256];
    int max_bits = 0;
    int max_sym = -1;
    bool valid = false;
};

enum BlockMode : uint8_t { kRaw = 0, kRle = 1, kHufNew = 2, kHufTreeless = 3 };

struct BlockPlan {
    BlockMode mode = kRaw;
    HufCode code{};              // kHufNew / kHufTreeless: the table the four streams are written with
    std::vector<uint8_t> head;   // everything in front of the streams: block header, then -- raw: nothing more (the bytes follow);
                                 // RLE: the byte; Huffman: literals header, tree description (new tree), 6-byte jump table
    uint32_t stream_size[4] = {0, 0, 0, 0};
    size_t n = 0;                // bytes the block holds
    size_t total = 0;            // bytes the block takes in the frame
};

// per-stream symbol counts of one block: q = (n + 3) / 4, streams [0,q) [q,2q) [2q,3q) [3q,n)
void count_block(const uint8_t *data, size_t n, uint32_t counts[4][256]);
// Every decision about one block.  `counts` is not read when n < 64 (raw).  *prev: the table of the block before in the
// same chunk; replaced only when this block is emitted compressed with a new tree.
void plan_block(const uint32_t counts[4][256], size_t n, bool last, HufCode *prev, BlockPlan *plan);
void emit_block(const BlockPlan &plan, const uint8_t *data, std::vector<uint8_t> &out);
// The Literals_Section of a block with sequences (synth.cpp); `counts` as count_block gives them for the literal bytes.
// plan->head: literals header (+ RLE byte, or tree and jump table); plan->total: the section's bytes.  *prev is only read.
void plan_literals(const uint32_t counts[4][256], size_t n, const HufCode *prev, BlockPlan *plan);
constexpr uint32_t kLzMinMatch = 6;     // shortest match either encoder takes

// one section -> one magicless frame (host code; lz: blocks with LZ sequences, compression levels 0 and >= 3)
void compress_section(const std::vector<uint8_t> &data, unsigned n_threads, bool lz, std::vector<uint8_t> &out);
int nucleotide_code(uint8_t c, uint8_t sequence_type);
void put_varint(std::vector<uint8_t> &out, uint64_t v);
// header, flags, line length, record count: what stands in front of the sections (encoder/mod.rs:327-347)
// opt.mask needs a nucleotide sequence (sequence set, DNA or RNA)
bool mask_opts_ok(const nafgpu_encoder_opts &opt);
constexpr uint64_t kDefaultLineLength = 60;      // Header::default().line_length (data.rs:246)
void put_archive_head(std::vector<uint8_t> &out, const nafgpu_encoder_opts &opt, uint64_t n_records, uint64_t line_length = kDefaultLineLength);

// ---- the device path (encode.cpp) --------------------------------------------------------------
struct EncTimes {            // milliseconds, summed over the slabs and sections of one call
    double hist = 0;         // HIP events around k_enc_hist (device_lz: and k_enc_lz_match, k_enc_lz_parse, k_enc_lz_hist)
    double streams = 0;      // HIP events around k_enc_streams + k_enc_scatter (device_lz: and k_enc_lz_seqbits)
    double plan = 0;         // host: plan_block over the histograms and building the upload
    double total = 0;        // wall time of the call
};
// `src` (host memory, or device memory when src_on_device) -> the frame compress_section(data, ., false) gives, appended to `out`;
// lz: a frame of blocks with sequences found by the device matcher instead
Failure compress_section_device(const uint8_t *src, size_t n, bool src_on_device, int device, unsigned n_threads, bool lz,
                                std::vector<uint8_t> &out, EncTimes *times);
// nafgpu_encode_device with the header's line length given (nafgpu_encode_text: the text's own)
Failure encode_device_archive(const nafgpu_encode_source *src, const nafgpu_encoder_opts *opts, int device, uint64_t line_length,
                              std::vector<uint8_t> &archive);

// ---- kernels (encode.hip); all pointers are device pointers, every launch is asynchronous ---------
struct EncStream {           // one Huffman stream of one block
    uint64_t src;            // offset of its first symbol in the slab
    uint64_t dst;            // offset of its first byte in the slab's output
    uint32_t n_sym;          // <= 32768
    uint32_t size;           // bytes, as planned
    uint32_t table;          // index into the tables
    uint32_t pad;
};
struct EncTable {
    uint16_t code[256];
    uint8_t len[256];
};
struct EncCopy {             // k_enc_scatter: `len` bytes to out + dst, from the header blob or from the slab's input
    uint64_t src;
    uint64_t dst;
    uint32_t len;
    uint32_t from_input;     // kCopyBlob, kCopyInput; device_lz: kCopyLiterals, kCopySeqBits
};
constexpr uint32_t kCopyBlob = 0, kCopyInput = 1, kCopyLiterals = 2, kCopySeqBits = 3;
constexpr uint32_t kEncStBadLetter = 1, kEncStStreamSize = 2;    // status[0] bits; status[2..3]: u64, the complement of the first bad letter's index

// mask: a lower-case letter is packed as its upper-case form
void launch_enc_pack(hipStream_t stream, const uint8_t *ascii, uint64_t n, uint8_t sequence_type, bool mask, uint8_t *packed,
                     uint32_t *status);
// The Mask section of n letters (encode.hip: k_enc_mask_*).  Edges: positions where the case changes (in front of letter 0:
// upper case); n_edges + 1 units when n != 0.
constexpr uint32_t kEncMaskTile = 4096;      // letters per workgroup of the two edge kernels (16 per lane)
uint64_t enc_mask_tiles(uint64_t n);
void launch_enc_mask_count(hipStream_t stream, const uint8_t *ascii, uint64_t n, uint64_t *tile_edges);       // enc_mask_tiles(n) counts
// tile_first: the exclusive prefix sums of tile_edges; unit_end: n_edges + 1 entries, the last one n
void launch_enc_mask_edges(hipStream_t stream, const uint8_t *ascii, uint64_t n, const uint64_t *tile_first, uint64_t n_edges,
                           uint64_t *unit_end);
void launch_enc_mask_sizes(hipStream_t stream, const uint64_t *unit_end, uint64_t n_units, uint64_t *sizes);  // bytes per unit
// offsets: the exclusive prefix sums of sizes, n_bytes their total; `section` holds n_bytes bytes 0xFF already
void launch_enc_mask_bytes(hipStream_t stream, const uint64_t *unit_end, uint64_t n_units, const uint64_t *offsets, uint64_t n_bytes,
                           uint8_t *section);
void launch_enc_length_counts(hipStream_t stream, const uint64_t *rec_end, uint64_t n_rec, uint64_t *counts);
void launch_enc_length_words(hipStream_t stream, const uint64_t *rec_end, uint64_t n_rec, const uint64_t *offsets, uint32_t *words);
void launch_enc_hist(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, uint32_t *hist);
void launch_enc_streams(hipStream_t stream, const uint8_t *src, const EncStream *streams, uint32_t n_streams, const EncTable *tables,
                        uint32_t max_stream_size, uint8_t *out, uint32_t *status);
void launch_enc_scatter(hipStream_t stream, const uint8_t *src, const uint8_t *blob, const EncCopy *copies, uint32_t n_copies,
                        uint8_t *out);

// ---- blocks with LZ sequences (encode.hip: k_enc_lz_*) ------------------------------------------
// Every per-block buffer lies at block index * its stride; block b of the slab holds input bytes [b * kBlockMax, ...).
constexpr uint32_t kLzMatchCap = 256;            // k_enc_lz_match extends a candidate this far; k_enc_lz_parse lengthens a selected match that reached it
constexpr uint32_t kLzMaxSeq = 131072 / kLzMinMatch + 1;     // sequences a block can hold (21 846)
struct LzSeq {               // one sequence: literal run, match length, distance
    uint32_t ll, ml, dist;
};
struct LzBlockInfo {
    uint32_t n_seq, n_lit;
    uint32_t seq_bytes;      // the sequence bitstream; kLzSeqOverflow: it did not fit its scratch, the block goes without sequences
    uint32_t pad;
};
constexpr uint32_t kLzSeqOverflow = 0xFFFFFFFFu;
struct LzSeqTables {         // the predefined FSE tables, encoder side: st_x[symbol][next state] = the state of `symbol` whose
                             // range holds `next state` (last column: any state of the symbol); nb / base per state
    uint8_t st_ll[36][65], st_of[29][33], st_ml[53][65];
    uint8_t nb_ll[64], nb_of[32], nb_ml[64];
    uint16_t base_ll[64], base_of[32], base_ml[64];
    uint32_t ll_base[36], ml_base[53];
    uint8_t ll_bits[36], ml_bits[53];
};
void lz_seq_tables(LzSeqTables *t);              // synth.cpp: from seq_table_build / seq_state_for
// match[p] = length << 17 | distance of the match found at input byte p (0: none), one word per byte of the slab
void launch_enc_lz_match(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, uint32_t *match);
// The greedy parse of every block: info, seqs (kLzMaxSeq per block) and lits (kBlockMax per block).  `exits`: one word per byte, scratch.
void launch_enc_lz_parse(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, const uint32_t *match, uint32_t *exits,
                         LzBlockInfo *info, LzSeq *seqs, uint8_t *lits);
// k_enc_hist over the literal buffers: the four streams of info[b].n_lit bytes
void launch_enc_lz_hist(hipStream_t stream, const uint8_t *lits, const LzBlockInfo *info, uint32_t n_blocks, uint32_t *hist);
// the sequence bitstream of every block into bits + b * kBlockMax; info[b].seq_bytes
void launch_enc_lz_seqbits(hipStream_t stream, const LzSeq *seqs, const LzSeqTables *tables, uint32_t n_blocks, LzBlockInfo *info, uint8_t *bits);
// k_enc_scatter with the two further sources
void launch_enc_scatter_lz(hipStream_t stream, const uint8_t *src, const uint8_t *blob, const uint8_t *lits, const uint8_t *bits,
                           const EncCopy *copies, uint32_t n_copies, uint8_t *out);

}  // namespace enc
}  // namespace nafgpu
