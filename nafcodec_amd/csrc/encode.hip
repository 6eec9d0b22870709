// encode.hip -- gfx950 (CDNA4, wave64) kernels of the encode path: literal-only Zstandard sections.
//
//   k_enc_pack      ASCII nucleotides -> 4-bit codes, two per byte (SequenceWriter, writer.rs:31-93)
//   k_enc_mask_*    the letters' case -> the Mask section's bytes (the inverse of MaskReader, reader.rs:198-231)
//   k_enc_length_*  record ends -> the Length section's 32-bit words (write_length, encoder/mod.rs:37-44)
//   k_enc_hist      per 128 KiB block: symbol counts of its four Huffman streams
//   k_enc_streams   one workgroup per stream: the backward bit stream, built in LDS, stored to its place in the frame
//   k_enc_scatter   block / literals headers, tree descriptions, jump tables; raw blocks' bytes
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

__global__ __launch_bounds__(kHistThreads) void k_enc_hist(const uint8_t *src, uint64_t n, uint32_t *hist) {
    __shared__ uint32_t s_h[kHistCopies * 1024];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kHistCopies * 1024; i += kHistThreads) s_h[i] = 0;
    __syncthreads();
    const uint64_t p0 = static_cast<uint64_t>(blockIdx.x) * kBlockMax;
    const uint32_t bn = n - p0 < kBlockMax ? static_cast<uint32_t>(n - p0) : kBlockMax;
    const uint32_t q = bn ? (bn + 3) / 4 : 1;
    const uint8_t *p = src + p0;
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
        } else {                                             // a stream ends inside (the section's last block only)
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
        hist[static_cast<uint64_t>(blockIdx.x) * 1024 + i] = sum;
    }
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
// (from the input), the "0 sequences" byte behind a compressed block, the frame header.
constexpr uint32_t kScatterThreads = 256;

__global__ __launch_bounds__(kScatterThreads) void k_enc_scatter(const uint8_t *src, const uint8_t *blob, const EncCopy *copies, uint8_t *out) {
    const EncCopy c = copies[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint8_t *s = (c.from_input ? src : blob) + c.src;
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
    hipLaunchKernelGGL(k_enc_scatter, dim3(n_copies), dim3(kScatterThreads), 0, stream, src, blob, copies, out);
}

}  // namespace enc
}  // namespace nafgpu
