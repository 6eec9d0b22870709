// encode.hip -- gfx950 (CDNA4, wave64) kernels of the encode path: literal-only Zstandard sections.
//
//   k_enc_pack      ASCII nucleotides -> 4-bit codes, two per byte (SequenceWriter, writer.rs:31-93)
//   k_enc_mask_*    the letters' case -> the Mask section's bytes (the inverse of MaskReader, reader.rs:198-231)
//   k_enc_length_*  record ends -> the Length section's 32-bit words (write_length, encoder/mod.rs:37-44)
//   k_enc_hist      per 128 KiB block: symbol counts of its four Huffman streams
//   k_enc_streams   one workgroup per stream: the backward bit stream, built in LDS, stored to its place in the frame
//   k_enc_scatter   block / literals headers, tree descriptions, jump tables; raw blocks' bytes
// Blocks with LZ sequences (opts.device_lz), in front of the host's decisions:
//   k_enc_lz_match    per 128 KiB block: the best of three earlier positions (two hash tables, one look-back) at every position
//   k_enc_lz_parse    the greedy parse over those matches: sequences and literals per block
//   k_enc_lz_hist     k_enc_hist over the literals
//   k_enc_lz_seqbits  the sequences' backward bitstream with the predefined FSE tables
// Between k_enc_hist and the last two the host decides every block from the counts (synth.cpp: plan_block), so each stream
// and each header has its destination before its kernel starts: no kernel waits for another workgroup.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "encode.h"
#include "kernels.h"
#include "plan.h"

namespace nafgpu {
namespace enc {

namespace {

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }
__device__ inline uint32_t byte_of(const uint32_t *w, uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// ======================================================================================
// k_enc_pack
// ======================================================================================
// SequenceWriter::encode (writer.rs:31-56): upper-case IUPAC, '-' = 0; T for DNA, U for RNA; 0xFF: refused
__device__ inline uint32_t enc_nuc(uint32_t c, uint32_t sequence_type) {
    switch (c) {
    case 'A': return 0x08;
    case 'C': return 0x04;
    case 'G': return 0x02;
    case 'T': return sequence_type == 0 ? 0x01 : 0xFF;
    case 'U': return sequence_type == 1 ? 0x01 : 0xFF;
    case 'R': return 0x0A;
    case 'Y': return 0x05;
    case 'S': return 0x06;
    case 'W': return 0x09;
    case 'K': return 0x03;
    case 'M': return 0x0C;
    case 'B': return 0x07;
    case 'D': return 0x0B;
    case 'H': return 0x0D;
    case 'V': return 0x0E;
    case 'N': return 0x0F;
    case '-': return 0x00;
    default: return 0xFF;
    }
}

constexpr uint32_t kPackThreads = 256;

// 16 letters -> 8 bytes per lane and step, the first letter of a pair in the low nibble.  The packing runs over the whole
// section (record boundaries do not show); an odd total leaves a last byte with its high nibble zero.
// MASK: a lower-case letter has the code of its upper-case form (the table's entries 'a'..'z' are those of 'A'..'Z');
// its case goes to the Mask section (k_enc_mask_*).  Nothing but the table differs between the two forms.
template <bool MASK>
__global__ __launch_bounds__(kPackThreads) void k_enc_pack(const uint8_t *ascii, uint64_t n, uint32_t sequence_type, uint8_t *packed,
                                                            uint32_t *status) {
    __shared__ uint32_t s_lut[256];
    const uint32_t tid = threadIdx.x;
    s_lut[tid] = enc_nuc(MASK && tid >= 'a' && tid <= 'z' ? tid - 32u : tid, sequence_type);
    __syncthreads();
    const uint64_t n_groups = (n + 15) / 16;
    const bool aligned = low4(ascii) == 0;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kPackThreads + tid; g < n_groups; g += static_cast<uint64_t>(gridDim.x) * kPackThreads) {
        const uint64_t o = 16 * g;
        const uint32_t cnt = n - o < 16 ? static_cast<uint32_t>(n - o) : 16u;
        uint32_t w[4] = {0, 0, 0, 0};
        if (cnt == 16 && aligned) {
            const uint4 v = *reinterpret_cast<const uint4 *>(ascii + o);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (k < cnt) w[k >> 2] |= static_cast<uint32_t>(ascii[o + k]) << (8u * (k & 3u));
        }
        uint32_t lo = 0, hi = 0, bad = 16;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            if (k >= cnt) continue;
            uint32_t c = s_lut[byte_of(w, k)];
            if (c == 0xFF) {
                if (bad == 16) bad = k;
                c = 0;
            }
            if (k < 8) lo |= c << (4u * k);
            else hi |= c << (4u * (k - 8));
        }
        if (bad < 16) {
            atomicOr(&status[0], kEncStBadLetter);
            atomicMax(reinterpret_cast<unsigned long long *>(status + 2), ~static_cast<unsigned long long>(o + bad));   // the lowest index: the largest complement
        }
        uint8_t *d = packed + 8 * g;
        if (cnt == 16) {
            *reinterpret_cast<uint2 *>(d) = make_uint2(lo, hi);
        } else {
            const uint32_t nb = (cnt + 1) / 2;
            for (uint32_t k = 0; k < nb; k++) d[k] = static_cast<uint8_t>((k < 4 ? lo >> (8u * k) : hi >> (8u * (k - 4))) & 0xFFu);
        }
    }
}

// ======================================================================================
// k_enc_mask_count / k_enc_mask_edges / k_enc_mask_sizes / k_enc_mask_bytes
// ======================================================================================
// The Mask section from the case of the letters.  masked(c) = 'a' <= c <= 'z'.  Letter i is an EDGE when masked(letter i)
// != masked(letter i - 1), with masked(letter -1) = false; the units of the section are what lies between edges: unit k
// spans [edge k-1, edge k), with edge -1 = 0 and the last unit ending at n, so that the first unit is an unmasked one (of
// length 0 when letter 0 is lower case).  A lane takes 16 letters as one 16-bit case word w; its edges are
// w ^ (w << 1 | case of the letter in front), which it reads from memory (the lane, the tile or the 16-byte load in front
// may hold it).  Positions are 64-bit.
//   count : edges per tile of kEncMaskTile letters                 (the caller scans them: launch_scan_excl_u64)
//   edges : unit_end[k] = position of edge k, rank within the tile by a workgroup scan; unit_end[n_edges] = n
//   sizes : bytes of unit k = length / 255 + 1                       (the caller scans them in place)
//   bytes : the section is filled with 0xFF beforehand; unit k's last byte = length % 255
// No lane loops over a unit's length: one unit of a genome without lower case is megabytes of 0xFF.
constexpr uint32_t kMaskThreads = 256;
static_assert(kEncMaskTile == kMaskThreads * 16, "a lane takes 16 letters");

__device__ inline uint32_t masked_letter(uint32_t c) { return c - 'a' < 26u; }

// the edges among letters [16 g, 16 g + 16) of the n letters, bit k = letter 16 g + k; letters from n on have none
__device__ inline uint32_t mask_edges16(const uint8_t *ascii, uint64_t n, uint64_t g, bool aligned) {
    const uint64_t o = 16 * g;
    if (o >= n) return 0;
    const uint32_t cnt = n - o < 16 ? static_cast<uint32_t>(n - o) : 16u;
    uint32_t w[4] = {0, 0, 0, 0};
    if (cnt == 16 && aligned) {
        const uint4 v = *reinterpret_cast<const uint4 *>(ascii + o);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (k < cnt) w[k >> 2] |= static_cast<uint32_t>(ascii[o + k]) << (8u * (k & 3u));
    }
    uint32_t cw = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) cw |= masked_letter(byte_of(w, k)) << k;
    const uint32_t before = o ? masked_letter(ascii[o - 1]) : 0u;
    return (cw ^ ((cw << 1) | before)) & (0xFFFFu >> (16u - cnt));
}

// exclusive scan of one count per lane over the workgroup; *total: the sum
__device__ inline uint32_t mask_scan(uint32_t v, uint32_t *s, uint32_t *total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kMaskThreads; d <<= 1) {
        const uint32_t a = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    *total = s[kMaskThreads - 1];
    const uint32_t incl = s[t];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kMaskThreads) void k_enc_mask_count(const uint8_t *ascii, uint64_t n, uint64_t *tile_edges) {
    __shared__ uint32_t s_cnt[kMaskThreads];
    const uint32_t e = mask_edges16(ascii, n, static_cast<uint64_t>(blockIdx.x) * kMaskThreads + threadIdx.x, low4(ascii) == 0);
    uint32_t total;
    (void)mask_scan(static_cast<uint32_t>(__builtin_popcount(e)), s_cnt, &total);
    if (threadIdx.x == 0) tile_edges[blockIdx.x] = total;
}

// tile_first[t]: edges in front of tile t.  Nothing is stored at or behind unit_end[n_edges] but the closing n: letters
// that changed between the two passes cannot make a store leave the array.
__global__ __launch_bounds__(kMaskThreads) void k_enc_mask_edges(const uint8_t *ascii, uint64_t n, const uint64_t *tile_first, uint64_t n_edges,
                                                                  uint64_t *unit_end) {
    __shared__ uint32_t s_cnt[kMaskThreads];
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kMaskThreads + threadIdx.x;
    uint32_t e = mask_edges16(ascii, n, g, low4(ascii) == 0);
    uint32_t total;
    uint64_t at = tile_first[blockIdx.x] + mask_scan(static_cast<uint32_t>(__builtin_popcount(e)), s_cnt, &total);
    while (e) {                                              // at most 16 rounds
        const uint32_t k = static_cast<uint32_t>(__builtin_ctz(e));
        e &= e - 1;
        if (at < n_edges) unit_end[at] = 16 * g + k;
        at++;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) unit_end[n_edges] = n;
}

__global__ __launch_bounds__(256) void k_enc_mask_sizes(const uint64_t *unit_end, uint64_t n_units, uint64_t *sizes) {
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; k < n_units; k += static_cast<uint64_t>(gridDim.x) * 256)
        sizes[k] = (unit_end[k] - (k ? unit_end[k - 1] : 0)) / 255 + 1;
}

__global__ __launch_bounds__(256) void k_enc_mask_bytes(const uint64_t *unit_end, uint64_t n_units, const uint64_t *offsets, uint64_t n_bytes,
                                                         uint8_t *section) {
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; k < n_units; k += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t behind = k + 1 < n_units ? offsets[k + 1] : n_bytes;
        if (behind - 1 < n_bytes) section[behind - 1] = static_cast<uint8_t>((unit_end[k] - (k ? unit_end[k - 1] : 0)) % 255);
    }
}

// ======================================================================================
// k_enc_length_counts / k_enc_length_words
// ======================================================================================
// write_length: 0xFFFFFFFF as long as that much is left, then the rest (which may be 0).  Words per record first (the
// caller scans them), then the words.
__global__ __launch_bounds__(256) void k_enc_length_counts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *counts) {
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rec; r += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t l = rec_end[r] - (r ? rec_end[r - 1] : 0);
        counts[r] = l / 0xFFFFFFFFull + 1;
    }
}

__global__ __launch_bounds__(256) void k_enc_length_words(const uint64_t *rec_end, uint64_t n_rec, const uint64_t *offsets, uint32_t *words) {
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rec; r += static_cast<uint64_t>(gridDim.x) * 256) {
        uint64_t l = rec_end[r] - (r ? rec_end[r - 1] : 0);
        uint64_t at = offsets[r];
        while (l >= 0xFFFFFFFFull) {
            words[at++] = 0xFFFFFFFFu;
            l -= 0xFFFFFFFFull;
        }
        words[at] = static_cast<uint32_t>(l);
    }
}

// ======================================================================================
// k_enc_hist
// ======================================================================================
// One workgroup per block, counts in LDS.  Packed DNA puts nearly all of a block's bytes on 16 byte values, and atomics
// of a wave on one LDS address are done one after the other; kHistCopies copies of the 4 x 256 counters (one per
// 256 / kHistCopies neighbouring lanes, added up at the end) were tried against that: 1, 4 (one per wave) and 16 copies
// take the same time on an MI355X, on packed DNA and on quality text (profiles/encode_probe.log) -- the lanes of ONE
// wave meet on an address whatever the waves beside them do -- so the product keeps one.  The switch stays for the probe.
#ifndef NAFGPU_ENC_HIST_COPIES
#define NAFGPU_ENC_HIST_COPIES 1
#endif
constexpr uint32_t kHistThreads = 256, kHistCopies = NAFGPU_ENC_HIST_COPIES;

__device__ inline void hist_word(uint32_t *h, uint32_t w) {
    atomicAdd(&h[w & 0xFFu], 1u);
    atomicAdd(&h[(w >> 8) & 0xFFu], 1u);
    atomicAdd(&h[(w >> 16) & 0xFFu], 1u);
    atomicAdd(&h[w >> 24], 1u);
}

__device__ inline uint32_t stream_of(uint32_t i, uint32_t q) { return (i >= q) + (i >= 2 * q) + (i >= 3 * q); }

// the counts of p[0, bn) as four streams -> out[1024]
__device__ inline void hist_block(const uint8_t *p, uint32_t bn, uint32_t *out) {
    __shared__ uint32_t s_h[kHistCopies * 1024];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kHistCopies * 1024; i += kHistThreads) s_h[i] = 0;
    __syncthreads();
    const uint32_t q = bn ? (bn + 3) / 4 : 1;
    uint32_t *mine = s_h + (tid / (kHistThreads / kHistCopies)) * 1024;
    // bytes in front of the first 16-byte boundary and behind the last one by one, what lies between 16 at a time
    uint32_t lead = (16u - low4(p)) & 15u;
    if (lead > bn) lead = bn;
    const uint32_t groups = (bn - lead) / 16, tail = lead + 16 * groups;
    if (tid < lead) atomicAdd(&mine[stream_of(tid, q) * 256 + p[tid]], 1u);
    if (tid < 16 && tail + tid < bn) atomicAdd(&mine[stream_of(tail + tid, q) * 256 + p[tail + tid]], 1u);
    for (uint32_t g = tid; g < groups; g += kHistThreads) {
        const uint32_t o = lead + 16 * g;
        const uint4 v = *reinterpret_cast<const uint4 *>(p + o);
        const uint32_t s0 = stream_of(o, q);
        if (s0 == stream_of(o + 15, q)) {
            uint32_t *h = mine + s0 * 256;
            hist_word(h, v.x);
            hist_word(h, v.y);
            hist_word(h, v.z);
            hist_word(h, v.w);
        } else {                                             // a stream ends inside (the section's last block; literals)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) atomicAdd(&mine[stream_of(o + k, q) * 256 + byte_of(w, k)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 1024; i += kHistThreads) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t c = 0; c < kHistCopies; c++) sum += s_h[c * 1024 + i];
        out[i] = sum;
    }
}

__global__ __launch_bounds__(kHistThreads) void k_enc_hist(const uint8_t *src, uint64_t n, uint32_t *hist) {
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * kBlockMax;
    hist_block(src + p0, n - p0 < kBlockMax ? static_cast<uint32_t>(n - p0) : kBlockMax, hist + static_cast<uint64_t>(blockIdx.x) * 1024);
}

// the literals of block b: info[b].n_lit bytes at lits + b * kBlockMax
__global__ __launch_bounds__(kHistThreads) void k_enc_lz_hist(const uint8_t *lits, const LzBlockInfo *info, uint32_t *hist) {
    uint32_t n_lit = info[blockIdx.x].n_lit;
    if (n_lit > kBlockMax) n_lit = kBlockMax;
    hist_block(lits + static_cast<uint64_t>(blockIdx.x) * kBlockMax, n_lit, hist + static_cast<uint64_t>(blockIdx.x) * 1024);
}

// ======================================================================================
// k_enc_streams
// ======================================================================================
// One workgroup per stream, lane t holds symbols [32 t, 32 t + 32) in registers (a stream has at most 32 768).  The
// stream is written from its LAST symbol (encode_stream: the decoder reads backwards), so a lane's bits start where the
// bits of all lanes behind it end: a suffix sum over the lanes' bit counts.  Each lane then shifts its codes into a
// 64-bit accumulator and puts whole words into an LDS image of the stream -- the first and the last word of its span
// with atomicOr (the neighbours share them), what lies between with plain stores.  Lane 0 adds the end mark.  The image
// goes to the frame with 16-byte stores between the destination's 16-byte boundaries, byte stores in front and behind.
constexpr uint32_t kStreamThreads = 1024, kRun = 32;

__global__ __launch_bounds__(kStreamThreads) void k_enc_streams(const uint8_t *src, const EncStream *streams, const EncTable *tables,
                                                                 uint32_t img_words, uint8_t *out, uint32_t *status) {
    HIP_DYNAMIC_SHARED(uint32_t, s_img)                   // img_words words: >= size / 4 + 2 of the largest stream
    __shared__ uint32_t s_tbl[256];                       // code | length << 16
    __shared__ uint32_t s_scan[kStreamThreads];
    const EncStream st = streams[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    if (tid < 256) {
        const EncTable &t = tables[st.table];
        s_tbl[tid] = t.code[tid] | (static_cast<uint32_t>(t.len[tid]) << 16);
    }
    for (uint32_t i = tid; i < img_words; i += kStreamThreads) s_img[i] = 0;
    const uint32_t a = tid * kRun;
    const uint32_t cnt = a < st.n_sym ? (st.n_sym - a < kRun ? st.n_sym - a : kRun) : 0;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t *p = src + st.src + a;
    if (cnt == kRun && low4(p) == 0) {
        const uint4 v0 = reinterpret_cast<const uint4 *>(p)[0], v1 = reinterpret_cast<const uint4 *>(p)[1];
        w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
        w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kRun; k++)
            if (k < cnt) w[k >> 2] |= static_cast<uint32_t>(p[k]) << (8u * (k & 3u));
    }
    __syncthreads();
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRun; k++)
        if (k < cnt) bits += s_tbl[byte_of(w, k)] >> 16;
    s_scan[tid] = bits;
    __syncthreads();
    for (uint32_t d = 1; d < kStreamThreads; d <<= 1) {     // suffix sums: s_scan[t] = bits of lanes t ..
        const uint32_t v = s_scan[tid] + (tid + d < kStreamThreads ? s_scan[tid + d] : 0u);
        __syncthreads();
        s_scan[tid] = v;
        __syncthreads();
    }
    const uint32_t total = s_scan[0], start = s_scan[tid] - bits;
    if (total / 8 + 1 != st.size) {                         // the plan and the bytes disagree: nothing is written, the call fails
        if (tid == 0) atomicOr(&status[0], kEncStStreamSize);
        return;
    }
    if (cnt || tid == 0) {
        uint32_t wi = start >> 5, nb = start & 31u;
        uint64_t acc = 0;
        bool first = true;
#pragma unroll
        for (uint32_t j = 0; j < kRun; j++) {
            const uint32_t k = kRun - 1 - j;                // last symbol first
            if (k >= cnt) continue;
            const uint32_t e = s_tbl[byte_of(w, k)];
            acc |= static_cast<uint64_t>(e & 0xFFFFu) << nb;
            nb += e >> 16;
            if (nb >= 32) {
                if (first) atomicOr(&s_img[wi], static_cast<uint32_t>(acc));
                else s_img[wi] = static_cast<uint32_t>(acc);
                first = false;
                wi++;
                acc >>= 32;
                nb -= 32;
            }
        }
        if (tid == 0) acc |= 1ull << nb;                    // end mark, above the first symbol's code
        if (acc) atomicOr(&s_img[wi], static_cast<uint32_t>(acc));
    }
    __syncthreads();
    uint8_t *d = out + st.dst;
    const uint8_t *img8 = reinterpret_cast<const uint8_t *>(s_img);
    uint32_t lead = (16u - low4(d)) & 15u;
    if (lead > st.size) lead = st.size;
    const uint32_t groups = (st.size - lead) / 16, tail = lead + 16 * groups;
    if (tid < lead) d[tid] = img8[tid];
    if (tid < 16 && tail + tid < st.size) d[tail + tid] = img8[tail + tid];
    const uint32_t sh = (lead & 3u) * 8u, w0 = lead >> 2;
    for (uint32_t g = tid; g < groups; g += kStreamThreads) {
        const uint32_t *s = s_img + w0 + 4 * g;
        const uint32_t a0 = s[0], a1 = s[1], a2 = s[2], a3 = s[3], a4 = s[4];
        *reinterpret_cast<uint4 *>(d + lead + 16 * g) =
            make_uint4(__builtin_amdgcn_alignbit(a1, a0, sh), __builtin_amdgcn_alignbit(a2, a1, sh), __builtin_amdgcn_alignbit(a3, a2, sh),
                       __builtin_amdgcn_alignbit(a4, a3, sh));
    }
}

// ======================================================================================
// k_enc_scatter
// ======================================================================================
// One workgroup per piece: the bytes in front of a block's streams (from the blob the host made), a raw block's bytes
// (from the input), the "0 sequences" byte behind a compressed block, the frame header; of a block with sequences its raw
// literals (from the literal buffers) and its sequence bitstream (from k_enc_lz_seqbits' scratch).
constexpr uint32_t kScatterThreads = 256;

__global__ __launch_bounds__(kScatterThreads) void k_enc_scatter(const uint8_t *src, const uint8_t *blob, const uint8_t *lits, const uint8_t *bits,
                                                                  const EncCopy *copies, uint8_t *out) {
    const EncCopy c = copies[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint8_t *s = (c.from_input == kCopyInput ? src : c.from_input == kCopyLiterals ? lits : c.from_input == kCopySeqBits ? bits : blob) + c.src;
    uint8_t *d = out + c.dst;
    uint32_t lead = (16u - low4(d)) & 15u;
    if (lead > c.len) lead = c.len;
    const uint32_t groups = (c.len - lead) / 16, tail = lead + 16 * groups;
    if (tid < lead) d[tid] = s[tid];
    if (tid < 16 && tail + tid < c.len) d[tail + tid] = s[tail + tid];
    const bool words = (low4(s + lead) & 3u) == 0;
    for (uint32_t g = tid; g < groups; g += kScatterThreads) {
        const uint8_t *sp = s + lead + 16 * g;
        uint32_t w[4] = {0, 0, 0, 0};
        if (words) {
            const uint32_t *sw = reinterpret_cast<const uint32_t *>(sp);
            w[0] = sw[0]; w[1] = sw[1]; w[2] = sw[2]; w[3] = sw[3];
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) w[k >> 2] |= static_cast<uint32_t>(sp[k]) << (8u * (k & 3u));
        }
        *reinterpret_cast<uint4 *>(d + lead + 16 * g) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ======================================================================================
// k_enc_lz_match
// ======================================================================================
// One workgroup per block, the block walked in tiles of kLzTile positions, one lane per position.  A lane hashes the four
// bytes at its position (the host matcher's multiplier) and tries three earlier positions:
//   A  s_head[h]: the LATEST position in front of the tile,
//   B  s_sub[h'][j]: the latest position in sub-tile j of the tile itself (kLzSubs sub-tiles; h': the hash's top kLzTileBits
//      bits); a lane of sub-tile j takes the nearest non-empty sub-tile in front of its own,
//   C  the nearest position of its own sub-tile with the same four bytes: the lanes' words lie in LDS, a lane looks back
//      through those in front of it (at most kLzSub - 1 of them).
// Near sources matter: their offsets take fewer bits, and in texts that count up (ids) the nearest record shares the most.
// Both tables are filled with atomicMax of position + 1 and read only behind a barrier, so what a lane sees does not depend
// on the order in which lanes or waves run: the frame is the same on every run and on the CPU harness.  A lane
// extends its candidates eight bytes at a time, never past kLzMatchCap bytes (a run of one byte value would otherwise
// make every lane walk the rest of the block) and never past the block's end; it keeps the longer match and, of two
// equally long ones, the nearer.  No candidate lies in front of the block: blocks, chunks and slabs stay independent.
// A lane takes kLzTile / kLzThreads positions of a tile, one in the product; the CPU harness, whose cost is the number of
// fibres it switches at a barrier, runs the same code with 64 lanes of 16 positions.  Nothing a lane sees depends on that.
#if defined(NAFGPU_EMU) && defined(NAFGPU_EMU_LZ_THREADS)
constexpr uint32_t kLzThreads = NAFGPU_EMU_LZ_THREADS;      // `make emu-lz1024`: the product's shape on the harness, for a few inputs
#elif defined(NAFGPU_EMU)
constexpr uint32_t kLzThreads = 64;
#else
constexpr uint32_t kLzThreads = 1024;
#endif
constexpr uint32_t kLzTile = 1024, kLzPerLane = kLzTile / kLzThreads, kLzHeadBits = 14, kLzTileBits = 10, kLzSubs = 16, kLzSub = kLzTile / kLzSubs, kLzLenShift = 17;
constexpr uint32_t kLzDistMask = (1u << kLzLenShift) - 1;
static_assert(kBlockMax == (1u << kLzLenShift), "a distance inside the block takes kLzLenShift bits");
static_assert(kLzMatchCap < (1u << (32 - kLzLenShift)) && kLzMatchCap % 8 == 0, "length << kLzLenShift | distance is one word");
static_assert(kLzMaxSeq == kBlockMax / kLzMinMatch + 1, "sequences a block can hold");

__device__ inline uint32_t load4(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ inline uint64_t load8(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// the number of k < max with b[from + j] == b[p + j] for all j <= k, given that it is at least len
__device__ inline uint32_t lz_extend(const uint8_t *b, uint32_t from, uint32_t p, uint32_t len, uint32_t max) {
    while (len + 8 <= max) {
        const uint64_t x = load8(b + from + len) ^ load8(b + p + len);
        if (x) return len + (static_cast<uint32_t>(__builtin_ctzll(x)) >> 3);
        len += 8;
    }
    while (len < max && b[from + len] == b[p + len]) len++;
    return len;
}

__global__ __launch_bounds__(kLzThreads) void k_enc_lz_match(const uint8_t *src, uint64_t n, uint32_t *match) {
    __shared__ uint32_t s_head[1u << kLzHeadBits];        // position + 1; 0: none
    __shared__ uint32_t s_sub[kLzSubs << kLzTileBits];    // position + 1; 0: none
    __shared__ uint32_t s_val[kLzTile];                   // the four bytes at the tile's positions
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (1u << kLzHeadBits); i += kLzThreads) s_head[i] = 0;
    for (uint32_t i = tid; i < (kLzSubs << kLzTileBits); i += kLzThreads) s_sub[i] = 0;
    __syncthreads();
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * kBlockMax;
    const uint32_t bn = n - p0 < kBlockMax ? static_cast<uint32_t>(n - p0) : kBlockMax;
    const uint8_t *b = src + p0;
    uint32_t *m = match + p0;
    for (uint32_t tile0 = 0; tile0 < bn; tile0 += kLzTile) {
        uint32_t h[kLzPerLane], h2[kLzPerLane], val[kLzPerLane], cand_a[kLzPerLane], cand_b[kLzPerLane], cand_c[kLzPerLane];
#pragma unroll
        for (uint32_t k = 0; k < kLzPerLane; k++) {
            const uint32_t i = tid + k * kLzThreads, p = tile0 + i;
            h[k] = h2[k] = val[k] = cand_a[k] = cand_b[k] = cand_c[k] = 0;
            if (p + kLzMinMatch <= bn) {                    // a match can start here
                val[k] = load4(b + p);
                s_val[i] = val[k];
                const uint32_t prod = val[k] * 2654435761u;
                h[k] = prod >> (32 - kLzHeadBits);
                h2[k] = (prod >> (32 - kLzTileBits)) * kLzSubs;
                cand_a[k] = s_head[h[k]];
                atomicMax(&s_sub[h2[k] + i / kLzSub], p + 1);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kLzPerLane; k++) {
            const uint32_t i = tid + k * kLzThreads, sub = i / kLzSub;
            if (tile0 + i + kLzMinMatch > bn) continue;
            for (uint32_t j = sub; j-- > 0 && !cand_b[k];) cand_b[k] = s_sub[h2[k] + j];
            for (uint32_t q = i; q-- > sub * kLzSub && !cand_c[k];)
                if (s_val[q] == val[k]) cand_c[k] = tile0 + q + 1;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kLzPerLane; k++) {
            const uint32_t i = tid + k * kLzThreads, p = tile0 + i;
            uint32_t best = 0, from = 0;
            if (p + kLzMinMatch <= bn) {
                s_sub[h2[k] + i / kLzSub] = 0;              // the writers clear it for the next tile
                atomicMax(&s_head[h[k]], p + 1);
                const uint32_t max = bn - p < kLzMatchCap ? bn - p : kLzMatchCap;
                if (cand_a[k]) {
                    const uint32_t len = lz_extend(b, cand_a[k] - 1, p, 0, max);
                    if (len >= kLzMinMatch) best = len, from = cand_a[k] - 1;
                }
                if (cand_b[k]) {                            // nearer than A: it wins a tie
                    const uint32_t len = lz_extend(b, cand_b[k] - 1, p, 0, max);
                    if (len >= kLzMinMatch && len >= best) best = len, from = cand_b[k] - 1;
                }
                if (cand_c[k]) {                            // the nearest of the three
                    const uint32_t len = lz_extend(b, cand_c[k] - 1, p, 4, max);
                    if (len >= kLzMinMatch && len >= best) best = len, from = cand_c[k] - 1;
                }
            }
            if (p < bn) m[p] = best ? (best << kLzLenShift) | (p - from) : 0u;
        }
        __syncthreads();
    }
}

// ======================================================================================
// k_enc_lz_parse
// ======================================================================================
// The greedy parse is the chain  next(p) = p + length(p) if a match was found at p, else p + 1,  from the block's first
// byte; only positions on the chain emit.  next(p) > p, so the block is cut into kLzSegs segments, one per lane (16 per
// lane on the CPU harness):
//   A  every lane goes through its segment from the back: exit(p) = next(p) if that leaves the segment, else
//      exit(next(p)) -- where the chain leaves the segment when it enters it at p, for every p, without knowing the entry.
//      Beside it: the first position on the way whose match reached kLzMatchCap.
//   B  lane 0 goes from segment to segment (at most kLzSegs steps), noting each segment's entry.  A capped match on
//      the chain is lengthened here, to the block's end at the most: only selected matches are, so all of them together
//      compare less than the block's bytes.  The final length replaces that position's exit word.
//   C  every lane walks its segment from its entry and counts sequences and literals; lane 0 turns the counts into offsets,
//      and into the literals pending in front of each segment;
//   E  the same walk writes the sequences and copies the literals.
constexpr uint32_t kLzSegs = 1024, kLzSeg = kBlockMax / kLzSegs;      // of 128 positions
constexpr uint32_t kLzExitMask = (1u << 18) - 1, kLzHasCap = 1u << 18, kLzCapShift = 19, kLzNone = 0xFFFFFFFFu;

// the length of the match the chain takes at p (0: a literal)
__device__ inline uint32_t lz_taken(const uint32_t *m, const uint32_t *ex, uint32_t p, uint32_t bn) {
    const uint32_t len = m[p] >> kLzLenShift;
    return len == kLzMatchCap && p + len < bn ? ex[p] : len;
}

__global__ __launch_bounds__(kLzThreads) void k_enc_lz_parse(const uint8_t *src, uint64_t n, const uint32_t *match, uint32_t *exits,
                                                              LzBlockInfo *info, LzSeq *seqs, uint8_t *lits) {
    __shared__ uint32_t s_entry[kLzSegs], s_seq[kLzSegs], s_lit[kLzSegs], s_run[kLzSegs];
    const uint32_t tid = threadIdx.x;
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * kBlockMax;
    const uint32_t bn = n - p0 < kBlockMax ? static_cast<uint32_t>(n - p0) : kBlockMax;
    const uint8_t *b = src + p0;
    const uint32_t *m = match + p0;
    uint32_t *ex = exits + p0;
    auto seg_end_of = [bn](uint32_t seg0) { return seg0 >= bn ? seg0 : (bn - seg0 < kLzSeg ? bn : seg0 + kLzSeg); };
    for (uint32_t sg = tid; sg < kLzSegs; sg += kLzThreads) {   // A
        const uint32_t seg0 = sg * kLzSeg, seg_end = seg_end_of(seg0);
        s_entry[sg] = kLzNone;
        for (uint32_t p = seg_end; p-- > seg0;) {
            const uint32_t len = m[p] >> kLzLenShift, nx = p + (len ? len : 1u);
            uint32_t v = nx >= seg_end ? nx : ex[nx];
            if (len == kLzMatchCap && nx < bn) v = kLzHasCap | ((p - seg0) << kLzCapShift);
            ex[p] = v;
        }
    }
    __syncthreads();
    if (tid == 0) {                                         // B
        uint32_t p = 0;
        while (p < bn) {
            const uint32_t seg = p / kLzSeg, v = ex[p];
            if (s_entry[seg] == kLzNone) s_entry[seg] = p;
            if (v & kLzHasCap) {
                const uint32_t c = seg * kLzSeg + (v >> kLzCapShift);
                const uint32_t len = lz_extend(b, c - (m[c] & kLzDistMask), c, kLzMatchCap, bn - c);
                ex[c] = len;
                p = c + len;
            } else {
                p = v & kLzExitMask;
            }
        }
    }
    __syncthreads();
    for (uint32_t sg = tid; sg < kLzSegs; sg += kLzThreads) {   // C; trail: literals behind the segment's last match
        const uint32_t entry = s_entry[sg], seg_end = seg_end_of(sg * kLzSeg);
        uint32_t n_seq = 0, n_lit = 0, trail = 0;
        if (entry != kLzNone)
            for (uint32_t p = entry; p < seg_end;) {
                const uint32_t len = lz_taken(m, ex, p, bn);
                if (len) n_seq++, trail = 0, p += len;
                else n_lit++, trail++, p++;
            }
        s_seq[sg] = n_seq;
        s_lit[sg] = n_lit;
        s_run[sg] = trail;
    }
    __syncthreads();
    if (tid == 0) {                                         // exclusive sums; s_run: the literals pending in front of the segment
        uint32_t seq_at = 0, lit_at = 0, run = 0;
        for (uint32_t k = 0; k < kLzSegs; k++) {
            const uint32_t ns = s_seq[k], nl = s_lit[k], tr = s_run[k];
            s_seq[k] = seq_at;
            s_lit[k] = lit_at;
            s_run[k] = run;
            seq_at += ns;
            lit_at += nl;
            run = ns ? tr : run + nl;
        }
        info[blockIdx.x] = LzBlockInfo{seq_at, lit_at, 0, 0};
    }
    __syncthreads();
    for (uint32_t sg = tid; sg < kLzSegs; sg += kLzThreads) {   // E
        const uint32_t entry = s_entry[sg], seg_end = seg_end_of(sg * kLzSeg);
        if (entry == kLzNone) continue;
        LzSeq *sq = seqs + static_cast<uint64_t>(blockIdx.x) * kLzMaxSeq + s_seq[sg];
        uint8_t *lt = lits + p0 + s_lit[sg];
        uint32_t run = s_run[sg];
        for (uint32_t p = entry; p < seg_end;) {
            const uint32_t len = lz_taken(m, ex, p, bn);
            if (len) {
                *sq++ = LzSeq{run, len, m[p] & kLzDistMask};
                run = 0;
                p += len;
            } else {
                *lt++ = b[p++];
                run++;
            }
        }
    }
}

// ======================================================================================
// k_enc_lz_seqbits
// ======================================================================================
// One workgroup of one wave per block, so that the blocks spread over the CUs; its lane 0 walks a dependent chain over the
// block's sequences, k_seq_states the other way round (the other lanes only help to fill the tables).  What the decoder
// reads first is written last (sequences_section, synth.cpp): from the last sequence to the first, the state updates that
// lead to the sequence behind (OF, ML, LL), then the extra bits LL, ML, OF; at the end the first sequence's states ML,
// OF, LL and the end mark.  Every offset is a new offset: Offset_Value = distance + 3.
constexpr uint32_t kSeqBitsThreads = 64, kSeqBitsMargin = 32;
static_assert(sizeof(LzSeqTables) % 4 == 0, "copied to LDS as words");

struct BitOut {
    uint32_t *w;
    uint32_t at = 0, nb = 0;
    uint64_t acc = 0;
    __device__ inline void put(uint32_t v, uint32_t bits) {          // bits <= 17
        acc |= static_cast<uint64_t>(v) << nb;
        nb += bits;
        if (nb >= 32) {
            w[at++] = static_cast<uint32_t>(acc);
            acc >>= 32;
            nb -= 32;
        }
    }
};

__global__ __launch_bounds__(kSeqBitsThreads) void k_enc_lz_seqbits(const LzSeq *seqs, const LzSeqTables *tables, uint32_t n_blocks,
                                                                     LzBlockInfo *info, uint8_t *bits) {
    __shared__ LzSeqTables s_t;
    for (uint32_t i = threadIdx.x; i < sizeof(LzSeqTables) / 4; i += kSeqBitsThreads)
        reinterpret_cast<uint32_t *>(&s_t)[i] = reinterpret_cast<const uint32_t *>(tables)[i];
    __syncthreads();
    const uint32_t blk = blockIdx.x;
    if (threadIdx.x || blk >= n_blocks) return;
    const uint32_t n_seq = info[blk].n_seq;
    if (!n_seq) return;
    const LzSeq *sq = seqs + static_cast<uint64_t>(blk) * kLzMaxSeq;
    BitOut o;
    o.w = reinterpret_cast<uint32_t *>(bits + static_cast<uint64_t>(blk) * kBlockMax);
    uint32_t s_ll = 64, s_of = 32, s_ml = 64;               // the states of the sequence behind; at first: any
    for (uint32_t i = n_seq; i-- > 0;) {
        if (o.at * 4 + kSeqBitsMargin > kBlockMax) {        // larger than the block itself: it could not have won
            info[blk].seq_bytes = kLzSeqOverflow;
            return;
        }
        const LzSeq q = sq[i];
        const uint32_t ofv = q.dist + 3, co = 31u - static_cast<uint32_t>(__builtin_clz(ofv));
        uint32_t cl = q.ll, cm = q.ml - 3;
        if (cl >= 16)
            for (cl = 35; q.ll < s_t.ll_base[cl]; cl--) {}
        if (cm >= 32)
            for (cm = 52; q.ml < s_t.ml_base[cm]; cm--) {}
        const uint32_t t_ll = s_t.st_ll[cl][s_ll], t_of = s_t.st_of[co][s_of], t_ml = s_t.st_ml[cm][s_ml];
        if (i + 1 < n_seq) {
            o.put(s_of - s_t.base_of[t_of], s_t.nb_of[t_of]);
            o.put(s_ml - s_t.base_ml[t_ml], s_t.nb_ml[t_ml]);
            o.put(s_ll - s_t.base_ll[t_ll], s_t.nb_ll[t_ll]);
        }
        o.put(q.ll - s_t.ll_base[cl], s_t.ll_bits[cl]);
        o.put(q.ml - s_t.ml_base[cm], s_t.ml_bits[cm]);
        o.put(ofv - (1u << co), co);
        s_ll = t_ll;
        s_of = t_of;
        s_ml = t_ml;
    }
    o.put(s_ml, 6);
    o.put(s_of, 5);
    o.put(s_ll, 6);
    o.put(1, 1);                                            // end mark
    if (o.nb) o.w[o.at] = static_cast<uint32_t>(o.acc);
    info[blk].seq_bytes = o.at * 4 + (o.nb + 7) / 8;
}

uint32_t grid_for(uint64_t items, uint32_t per_block) {
    uint64_t blocks = (items + per_block - 1) / per_block;
    if (blocks > 256u * 32u) blocks = 256u * 32u;
    return blocks ? static_cast<uint32_t>(blocks) : 1u;
}

}  // namespace

void launch_enc_pack(hipStream_t stream, const uint8_t *ascii, uint64_t n, uint8_t sequence_type, bool mask, uint8_t *packed,
                     uint32_t *status) {
    if (!n) return;
    if (mask)
        hipLaunchKernelGGL(k_enc_pack<true>, dim3(grid_for((n + 15) / 16, kPackThreads)), dim3(kPackThreads), 0, stream, ascii, n,
                           static_cast<uint32_t>(sequence_type), packed, status);
    else
        hipLaunchKernelGGL(k_enc_pack<false>, dim3(grid_for((n + 15) / 16, kPackThreads)), dim3(kPackThreads), 0, stream, ascii, n,
                           static_cast<uint32_t>(sequence_type), packed, status);
}

uint64_t enc_mask_tiles(uint64_t n) { return (n + kEncMaskTile - 1) / kEncMaskTile; }

void launch_enc_mask_count(hipStream_t stream, const uint8_t *ascii, uint64_t n, uint64_t *tile_edges) {
    if (!n) return;
    hipLaunchKernelGGL(k_enc_mask_count, dim3(static_cast<uint32_t>(enc_mask_tiles(n))), dim3(kMaskThreads), 0, stream, ascii, n, tile_edges);
}

void launch_enc_mask_edges(hipStream_t stream, const uint8_t *ascii, uint64_t n, const uint64_t *tile_first, uint64_t n_edges,
                           uint64_t *unit_end) {
    if (!n) return;
    hipLaunchKernelGGL(k_enc_mask_edges, dim3(static_cast<uint32_t>(enc_mask_tiles(n))), dim3(kMaskThreads), 0, stream, ascii, n, tile_first,
                       n_edges, unit_end);
}

void launch_enc_mask_sizes(hipStream_t stream, const uint64_t *unit_end, uint64_t n_units, uint64_t *sizes) {
    if (!n_units) return;
    hipLaunchKernelGGL(k_enc_mask_sizes, dim3(grid_for(n_units, 256)), dim3(256), 0, stream, unit_end, n_units, sizes);
}

void launch_enc_mask_bytes(hipStream_t stream, const uint64_t *unit_end, uint64_t n_units, const uint64_t *offsets, uint64_t n_bytes,
                           uint8_t *section) {
    if (!n_units) return;
    hipLaunchKernelGGL(k_enc_mask_bytes, dim3(grid_for(n_units, 256)), dim3(256), 0, stream, unit_end, n_units, offsets, n_bytes, section);
}

void launch_enc_length_counts(hipStream_t stream, const uint64_t *rec_end, uint64_t n_rec, uint64_t *counts) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_enc_length_counts, dim3(grid_for(n_rec, 256)), dim3(256), 0, stream, rec_end, n_rec, counts);
}

void launch_enc_length_words(hipStream_t stream, const uint64_t *rec_end, uint64_t n_rec, const uint64_t *offsets, uint32_t *words) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_enc_length_words, dim3(grid_for(n_rec, 256)), dim3(256), 0, stream, rec_end, n_rec, offsets, words);
}

void launch_enc_hist(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, uint32_t *hist) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_enc_hist, dim3(n_blocks), dim3(kHistThreads), 0, stream, src, n, hist);
}

void launch_enc_streams(hipStream_t stream, const uint8_t *src, const EncStream *streams, uint32_t n_streams, const EncTable *tables,
                        uint32_t max_stream_size, uint8_t *out, uint32_t *status) {
    if (!n_streams) return;
    const uint32_t img_words = max_stream_size / 4 + 2;
    hipLaunchKernelGGL(k_enc_streams, dim3(n_streams), dim3(kStreamThreads), img_words * sizeof(uint32_t), stream, src, streams, tables,
                       img_words, out, status);
}

void launch_enc_scatter(hipStream_t stream, const uint8_t *src, const uint8_t *blob, const EncCopy *copies, uint32_t n_copies,
                        uint8_t *out) {
    if (!n_copies) return;
    launch_enc_scatter_lz(stream, src, blob, nullptr, nullptr, copies, n_copies, out);
}

void launch_enc_scatter_lz(hipStream_t stream, const uint8_t *src, const uint8_t *blob, const uint8_t *lits, const uint8_t *bits,
                           const EncCopy *copies, uint32_t n_copies, uint8_t *out) {
    if (!n_copies) return;
    hipLaunchKernelGGL(k_enc_scatter, dim3(n_copies), dim3(kScatterThreads), 0, stream, src, blob, lits, bits, copies, out);
}

void launch_enc_lz_match(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, uint32_t *match) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_enc_lz_match, dim3(n_blocks), dim3(kLzThreads), 0, stream, src, n, match);
}

void launch_enc_lz_parse(hipStream_t stream, const uint8_t *src, uint64_t n, uint32_t n_blocks, const uint32_t *match, uint32_t *exits,
                         LzBlockInfo *info, LzSeq *seqs, uint8_t *lits) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_enc_lz_parse, dim3(n_blocks), dim3(kLzThreads), 0, stream, src, n, match, exits, info, seqs, lits);
}

void launch_enc_lz_hist(hipStream_t stream, const uint8_t *lits, const LzBlockInfo *info, uint32_t n_blocks, uint32_t *hist) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_enc_lz_hist, dim3(n_blocks), dim3(kHistThreads), 0, stream, lits, info, hist);
}

void launch_enc_lz_seqbits(hipStream_t stream, const LzSeq *seqs, const LzSeqTables *tables, uint32_t n_blocks, LzBlockInfo *info, uint8_t *bits) {
    if (!n_blocks) return;
    hipLaunchKernelGGL(k_enc_lz_seqbits, dim3(n_blocks), dim3(kSeqBitsThreads), 0, stream, seqs, tables, n_blocks, info, bits);
}

}  // namespace enc
}  // namespace nafgpu
