// parse.hip -- gfx950 (CDNA4, wave64) kernels of the text parser: FASTA / FASTQ text -> letters, qualities, ids, comments
// and record ends, the inverse of k_fmt_sizes / k_fmt_write (kernels.hip).  The rules: include/nafgpu.h at nafgpu_parse_text.
//
// A lane takes 16 text bytes, a workgroup a tile of 4096.  What a byte is depends on the line it stands in, and a line may
// begin millions of tiles in front of it, so the state travels as a SUMMARY that composes associatively:
//   line feeds seen (count mod 4, and whether any); behind the last one: does a '>' follow (FASTA), was a separator seen,
//   where does the line start.  No line feed: the state in front passes through, only "separator seen" may be added.
// The state entering a lane is the composition of everything in front of it: tiles (k_parse_scan_*), then lanes (a
// workgroup scan).  FASTA: header or sequence line; FASTQ: line index mod 4; both: separator seen since the header began.
// The byte in front of a lane's first one (line start?) and the byte behind its last one (CR before LF, '>' after LF) are
// read from memory, as k_enc_mask_count reads the letter in front.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "parse.h"

namespace nafgpu {
namespace parse {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kParseTile == kThreads * 16, "a lane takes 16 text bytes");

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }
__device__ inline uint32_t byte_of(const uint32_t *w, uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// ---- summaries ------------------------------------------------------------------------------
constexpr uint32_t kSumCnt = 3u;         // line feeds mod 4
constexpr uint32_t kSumAny = 4u;         // a line feed was seen; the fields below describe what follows the last one
constexpr uint32_t kSumSeq = 8u;         // FASTA: no '>' follows it (a sequence line, or nothing)
constexpr uint32_t kSumSep = 16u;        // a separator was seen since (no line feed: anywhere)
constexpr uint32_t kSumLineShift = 8;    // bits 8..20: offset in the tile of the byte behind it, 1..4096 (lanes of one tile only)

// a in front of b
__device__ inline uint32_t sum_combine(uint32_t a, uint32_t b) {
    if (b & kSumAny) return (b & ~kSumCnt) | ((a + b) & kSumCnt);
    return a | (b & kSumSep);
}

// state = kind | separator seen << 2; kind: 0 header line, 1 sequence line, 2 the '+' line, 3 quality line.
// `s`: everything from the text's first byte on, which begins a header line.
__device__ inline uint32_t state_after(uint32_t s, bool fastq) {
    const uint32_t kind = fastq ? (s & kSumCnt) : ((s & kSumAny) && (s & kSumSeq) ? 1u : 0u);
    return kind | ((s & kSumSep) ? 4u : 0u);
}

// ---- a lane's 16 bytes ------------------------------------------------------------------------
// Groups are counted from the 16-byte boundary at or in front of the text: group g holds text bytes [p0, p0 + 16), p0 =
// 16 g - shift.  Whole groups are loaded with one aligned 16-byte load, the first and the last one byte by byte.
struct Lane16 {
    uint32_t w[4];           // bytes outside [first, last) are 0
    int64_t p0;
    uint32_t first, last;    // bytes [first, last) of the group belong to the text
    uint32_t behind, ahead;  // text[p0 - 1], text[p0 + 16] (0: there is none)
};

__device__ inline void load16(const uint8_t *text, uint64_t n, uint64_t g, Lane16 *L) {
    const uint32_t shift = low4(text);
    const uint64_t v0 = 16 * g, nv = n + shift;
    L->w[0] = L->w[1] = L->w[2] = L->w[3] = 0;
    L->p0 = static_cast<int64_t>(v0) - static_cast<int64_t>(shift);
    L->first = L->last = 0;
    L->behind = L->ahead = 0;
    if (v0 >= nv) return;
    L->first = v0 < shift ? shift - static_cast<uint32_t>(v0) : 0u;
    L->last = nv - v0 < 16 ? static_cast<uint32_t>(nv - v0) : 16u;
    if (L->first == 0 && L->last == 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + L->p0);
        L->w[0] = v.x; L->w[1] = v.y; L->w[2] = v.z; L->w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (k >= L->first && k < L->last) L->w[k >> 2] |= static_cast<uint32_t>(text[L->p0 + k]) << (8u * (k & 3u));
    }
    if (L->p0 > 0) L->behind = text[L->p0 - 1];
    if (L->last == 16 && static_cast<uint64_t>(L->p0 + 16) < n) L->ahead = text[L->p0 + 16];
}

__device__ inline uint32_t lane_summary(const Lane16 &L) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        if (k < L.first || k >= L.last) continue;
        const uint32_t c = byte_of(L.w, k);
        if (c == '\n') {
            const uint32_t nxt = k < 15 ? byte_of(L.w, k + 1) : L.ahead;
            s = ((s + 1) & kSumCnt) | kSumAny | (nxt == '>' ? 0u : kSumSeq) | ((threadIdx.x * 16 + k + 1) << kSumLineShift);
        } else if (c == ' ') {
            s |= kSumSep;
        }
    }
    return s;
}

// the composition of the lanes in front of this one (0: none); *total: of all lanes
__device__ inline uint32_t scan_summaries(uint32_t own, uint32_t *s, uint32_t *total) {
    const uint32_t t = threadIdx.x;
    s[t] = own;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        const uint32_t a = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] = sum_combine(a, s[t]);
        __syncthreads();
    }
    *total = s[kThreads - 1];
    const uint32_t ex = t ? s[t - 1] : 0u;
    __syncthreads();
    return ex;
}

// exclusive scan of one packed count word per lane; *total: the sum
__device__ inline uint64_t scan_counts(uint64_t v, uint64_t *s, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        const uint64_t a = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    *total = s[kThreads - 1];
    const uint64_t incl = s[t];
    __syncthreads();
    return incl - v;
}

// the state and the line start entering this lane
__device__ inline uint32_t lane_entering(const Lane16 &L, const uint8_t *text, const ParseTile &in, bool fastq, uint32_t *s_scan,
                                         uint64_t *line_start) {
    uint32_t total;
    const uint32_t ex = scan_summaries(lane_summary(L), s_scan, &total);
    *line_start = (ex & kSumAny) ? static_cast<uint64_t>(blockIdx.x) * kParseTile + ((ex >> kSumLineShift) & 0x1FFFu) - low4(text)
                                 : in.line_start;
    return state_after(sum_combine(in.summary, ex), fastq);
}

// ---- classification -----------------------------------------------------------------------------
// what a byte becomes, 4 bits per byte; an OPEN is a header line's first byte ('>' / '@'): a record begins, and unless it
// is the text's first byte the record in front ends: its NUL in ids and in comments, its record end.
enum : uint32_t { kClNone = 0, kClSeq = 1, kClQual = 2, kClId = 3, kClCom = 4, kClOpen = 5 };
// counts of one lane / one tile in one word: 13 bits each for seq, qual, id, com (<= 4096), 12 for opens (<= 2049)
constexpr uint32_t kCntBits = 13, kCntMask = 0x1FFFu, kCntOpenShift = 4 * kCntBits;

__device__ inline void flag_first(uint32_t *status, uint32_t bit, uint32_t slot, uint64_t at) {
    atomicOr(&status[0], bit);
    atomicMax(reinterpret_cast<unsigned long long *>(status + slot), ~static_cast<unsigned long long>(at));   // the lowest: the largest complement
}

template <bool CHECK>
__device__ inline uint64_t classify16(const Lane16 &L, uint64_t n, bool fastq, uint32_t state, uint64_t line_start, uint32_t *status,
                                      uint64_t *cls_out, uint64_t *longest_out) {
    uint32_t kind = state & 3u;
    bool sep = (state & 4u) != 0;
    uint64_t cls = 0, counts = 0, longest = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        if (k < L.first || k >= L.last) continue;
        const uint64_t p = static_cast<uint64_t>(L.p0 + k);
        const uint32_t c = byte_of(L.w, k);
        const uint32_t prev = k ? byte_of(L.w, k - 1) : L.behind;
        const uint32_t nxt = k < 15 ? byte_of(L.w, k + 1) : L.ahead;
        const bool at_start = p == 0 || prev == '\n';
        uint32_t cl = kClNone;
        bool mark = false;
        if (at_start) {
            sep = false;
            line_start = p;
            if (!fastq) kind = c == '>' ? 0u : 1u;
            if (kind == 0) {
                if (CHECK && fastq && c != '@') flag_first(status, kParseStLine, 2, p);
                if (c != '\n') {
                    cl = kClOpen;
                    mark = true;
                }
            } else if (fastq && kind == 2) {
                if (CHECK && c != '+') flag_first(status, kParseStLine, 2, p);
                mark = c != '\n';
            }
        }
        if (!mark) {
            if (c == '\n') {
                if (kind == 1) {
                    const uint64_t len = at_start ? 0 : p - line_start - (prev == '\r' ? 1u : 0u);
                    if (len > longest) longest = len;
                }
                if (fastq) kind = (kind + 1) & 3u;
            } else if (c == '\r' && (p + 1 == n || nxt == '\n')) {
                // dropped with the line feed (or the text's end) behind it
            } else if (kind == 0) {
                if (!sep && c == ' ') {
                    sep = true;
                } else {
                    cl = sep ? kClCom : kClId;
                    if (CHECK && c == 0) flag_first(status, kParseStNul, 4, p);
                }
            } else if (kind == 1) {
                cl = kClSeq;
            } else if (kind == 3) {
                cl = kClQual;
            }
        }
        if (p + 1 == n) {                                    // the last line may lack its line feed
            if (c != '\n' && kind == 1) {
                const uint64_t len = n - line_start - (c == '\r' ? 1u : 0u);
                if (len > longest) longest = len;
            }
            if (CHECK && fastq && ((kind + (c != '\n' ? 1u : 0u)) & 3u)) flag_first(status, kParseStLine, 2, n);   // lines: not 4 k
        }
        cls |= static_cast<uint64_t>(cl) << (4u * k);
        if (cl == kClOpen) counts += (1ull << kCntOpenShift) + (p ? (1ull << (2 * kCntBits)) + (1ull << (3 * kCntBits)) : 0ull);
        else if (cl) counts += 1ull << (kCntBits * (cl - 1));
    }
    *cls_out = cls;
    *longest_out = longest;
    return counts;
}

// ======================================================================================
// k_parse_summary / k_parse_scan_reduce / k_parse_scan_aggs / k_parse_scan_emit
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_parse_summary(const uint8_t *text, uint64_t n, ParseTile *tiles) {
    __shared__ uint32_t s_scan[kThreads];
    Lane16 L;
    load16(text, n, static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, &L);
    uint32_t total;
    (void)scan_summaries(lane_summary(L), s_scan, &total);
    if (threadIdx.x == 0) {
        ParseTile t;
        t.line_start = (total & kSumAny) ? static_cast<uint64_t>(blockIdx.x) * kParseTile + ((total >> kSumLineShift) & 0x1FFFu) - low4(text) : 0;
        t.summary = total;
        t.pad = 0;
        tiles[blockIdx.x] = t;
    }
}

// The scan over the tiles' summaries, in the three steps of k_scan_reduce / k_scan_tiles / k_scan_emit with the summaries'
// composition in the place of the sum: a workgroup composes kScanSpan tiles (8 per lane) into one aggregate; ONE
// workgroup scans the aggregates (every lane a contiguous share of them, a workgroup scan joins the shares); a workgroup
// rewrites its tiles with what stands in front of each.  A lane rewrites only what it has read itself.
constexpr uint32_t kScanItems = 8, kScanSpan = kThreads * kScanItems;

// exclusive scan of one (summary, line start) pair per lane; the pair of all lanes in *tot / *tot_line
__device__ inline void scan_pairs(uint32_t *acc, uint64_t *line, uint32_t *s_sum, uint64_t *s_line, uint32_t *tot, uint64_t *tot_line) {
    const uint32_t t = threadIdx.x;
    s_sum[t] = *acc;
    s_line[t] = *line;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        const uint32_t a = t >= d ? s_sum[t - d] : 0u;
        const uint64_t al = t >= d ? s_line[t - d] : 0u;
        __syncthreads();
        if (!(s_sum[t] & kSumAny)) s_line[t] = al;
        s_sum[t] = sum_combine(a, s_sum[t]);
        __syncthreads();
    }
    *tot = s_sum[kThreads - 1];
    *tot_line = s_line[kThreads - 1];
    *acc = t ? s_sum[t - 1] : 0u;
    *line = t ? s_line[t - 1] : 0u;
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_parse_scan_reduce(const ParseTile *tiles, uint64_t n_tiles, ParseTile *aggs) {
    __shared__ uint32_t s_sum[kThreads];
    __shared__ uint64_t s_line[kThreads];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kScanSpan + threadIdx.x * kScanItems;
    uint32_t acc = 0, tot;
    uint64_t line = 0, tot_line;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; k++) {
        if (base + k >= n_tiles) break;
        const ParseTile a = tiles[base + k];
        if (a.summary & kSumAny) line = a.line_start;
        acc = sum_combine(acc, a.summary);
    }
    scan_pairs(&acc, &line, s_sum, s_line, &tot, &tot_line);
    if (threadIdx.x == 0) {
        ParseTile o;
        o.line_start = tot_line;
        o.summary = tot;
        o.pad = 0;
        aggs[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(kThreads) void k_parse_scan_aggs(ParseTile *aggs, uint64_t n_aggs) {
    __shared__ uint32_t s_sum[kThreads];
    __shared__ uint64_t s_line[kThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n_aggs + kThreads - 1) / kThreads;
    const uint64_t lo = t * per < n_aggs ? t * per : n_aggs;
    const uint64_t hi = lo + per < n_aggs ? lo + per : n_aggs;
    uint32_t acc = 0, tot;
    uint64_t line = 0, tot_line;
    for (uint64_t i = lo; i < hi; i++) {
        const ParseTile a = aggs[i];
        if (a.summary & kSumAny) line = a.line_start;
        acc = sum_combine(acc, a.summary);
    }
    scan_pairs(&acc, &line, s_sum, s_line, &tot, &tot_line);
    for (uint64_t i = lo; i < hi; i++) {
        const ParseTile a = aggs[i];
        ParseTile o;
        o.line_start = line;
        o.summary = acc;
        o.pad = 0;
        aggs[i] = o;
        if (a.summary & kSumAny) line = a.line_start;
        acc = sum_combine(acc, a.summary);
    }
}

__global__ __launch_bounds__(kThreads) void k_parse_scan_emit(ParseTile *tiles, uint64_t n_tiles, const ParseTile *aggs) {
    __shared__ uint32_t s_sum[kThreads];
    __shared__ uint64_t s_line[kThreads];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kScanSpan + threadIdx.x * kScanItems;
    ParseTile mine[kScanItems];
    uint32_t acc = 0, tot;
    uint64_t line = 0, tot_line;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; k++) {
        mine[k].summary = 0;
        mine[k].line_start = 0;
        if (base + k < n_tiles) mine[k] = tiles[base + k];
        if (mine[k].summary & kSumAny) line = mine[k].line_start;
        acc = sum_combine(acc, mine[k].summary);
    }
    scan_pairs(&acc, &line, s_sum, s_line, &tot, &tot_line);
    const ParseTile front = aggs[blockIdx.x];
    if (!(acc & kSumAny)) line = front.line_start;
    acc = sum_combine(front.summary, acc);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; k++) {
        if (base + k >= n_tiles) break;
        ParseTile o;
        o.line_start = line;
        o.summary = acc;
        o.pad = 0;
        tiles[base + k] = o;
        if (mine[k].summary & kSumAny) line = mine[k].line_start;
        acc = sum_combine(acc, mine[k].summary);
    }
}

// ======================================================================================
// k_parse_count
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_parse_count(const uint8_t *text, uint64_t n, uint32_t fastq, const ParseTile *tiles, uint64_t *counts,
                                                           uint64_t n_tiles, ParseTotals *totals, uint32_t *status) {
    __shared__ uint32_t s_scan[kThreads];
    __shared__ uint64_t s_cnt[kThreads];
    __shared__ unsigned long long s_longest;
    if (threadIdx.x == 0) s_longest = 0;
    Lane16 L;
    load16(text, n, static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, &L);
    uint64_t line_start, cls, longest, total;
    const uint32_t state = lane_entering(L, text, tiles[blockIdx.x], fastq != 0, s_scan, &line_start);
    const uint64_t mine = classify16<true>(L, n, fastq != 0, state, line_start, status, &cls, &longest);
    (void)scan_counts(mine, s_cnt, &total);
    if (longest) atomicMax(&s_longest, static_cast<unsigned long long>(longest));
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[kSeq * n_tiles + blockIdx.x] = total & kCntMask;
        counts[kQual * n_tiles + blockIdx.x] = (total >> kCntBits) & kCntMask;
        counts[kId * n_tiles + blockIdx.x] = (total >> (2 * kCntBits)) & kCntMask;
        counts[kCom * n_tiles + blockIdx.x] = (total >> (3 * kCntBits)) & kCntMask;
        counts[kOpen * n_tiles + blockIdx.x] = total >> kCntOpenShift;
        if (s_longest) atomicMax(reinterpret_cast<unsigned long long *>(&totals->line_length), s_longest);
    }
}

// ======================================================================================
// k_parse_write
// ======================================================================================
// The tile's bytes go to one LDS image, field behind field (letters, qualities, ids, comments: at most 4096 + one NUL
// per record opened, twice), each at its rank from the workgroup scan; every field's piece then goes to its place with
// 16-byte stores between the destination's 16-byte boundaries and byte stores in front and behind (k_enc_streams).
// Nothing is stored outside the sizes the count pass gave: a text that changed between the passes cannot make a store
// leave an array.
constexpr uint32_t kImgBytes = 2 * kParseTile, kImgWords = kImgBytes / 4 + 8;

__device__ inline void img_store(const uint32_t *s_img, uint32_t from, uint32_t len, uint8_t *dst, uint64_t at, uint64_t n_dst) {
    if (!len || at >= n_dst) return;
    if (len > n_dst - at) len = static_cast<uint32_t>(n_dst - at);
    const uint32_t tid = threadIdx.x;
    uint8_t *d = dst + at;
    const uint8_t *img8 = reinterpret_cast<const uint8_t *>(s_img) + from;
    uint32_t lead = (16u - low4(d)) & 15u;
    if (lead > len) lead = len;
    const uint32_t groups = (len - lead) / 16, tail = lead + 16 * groups;
    if (tid < lead) d[tid] = img8[tid];
    if (tid < 16 && tail + tid < len) d[tail + tid] = img8[tail + tid];
    const uint32_t sh = ((from + lead) & 3u) * 8u, w0 = (from + lead) >> 2;
    for (uint32_t g = tid; g < groups; g += kThreads) {
        const uint32_t *s = s_img + w0 + 4 * g;
        const uint32_t a0 = s[0], a1 = s[1], a2 = s[2], a3 = s[3], a4 = s[4];
        *reinterpret_cast<uint4 *>(d + lead + 16 * g) =
            make_uint4(__builtin_amdgcn_alignbit(a1, a0, sh), __builtin_amdgcn_alignbit(a2, a1, sh), __builtin_amdgcn_alignbit(a3, a2, sh),
                       __builtin_amdgcn_alignbit(a4, a3, sh));
    }
}

__global__ __launch_bounds__(kThreads) void k_parse_write(const uint8_t *text, uint64_t n, uint32_t fastq, const ParseTile *tiles,
                                                           const uint64_t *counts, uint64_t n_tiles, ParseOut out) {
    __shared__ uint32_t s_scan[kThreads];
    __shared__ uint64_t s_cnt[kThreads];
    __shared__ uint32_t s_img[kImgWords];
    Lane16 L;
    load16(text, n, static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x, &L);
    uint64_t line_start, cls, longest, total;
    const uint32_t state = lane_entering(L, text, tiles[blockIdx.x], fastq != 0, s_scan, &line_start);
    const uint64_t mine = classify16<false>(L, n, fastq != 0, state, line_start, nullptr, &cls, &longest);
    const uint64_t ex = scan_counts(mine, s_cnt, &total);
    const uint32_t t_seq = total & kCntMask, t_qual = (total >> kCntBits) & kCntMask, t_id = (total >> (2 * kCntBits)) & kCntMask,
                   t_com = (total >> (3 * kCntBits)) & kCntMask;
    const uint32_t o_qual = t_seq, o_id = o_qual + t_qual, o_com = o_id + t_id;
    const uint64_t b_seq = counts[kSeq * n_tiles + blockIdx.x], b_qual = counts[kQual * n_tiles + blockIdx.x],
                   b_id = counts[kId * n_tiles + blockIdx.x], b_com = counts[kCom * n_tiles + blockIdx.x],
                   b_open = counts[kOpen * n_tiles + blockIdx.x];
    uint32_t r_seq = ex & kCntMask, r_qual = (ex >> kCntBits) & kCntMask, r_id = (ex >> (2 * kCntBits)) & kCntMask,
             r_com = (ex >> (3 * kCntBits)) & kCntMask, r_open = static_cast<uint32_t>(ex >> kCntOpenShift);
    uint8_t *img = reinterpret_cast<uint8_t *>(s_img);
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t cl = static_cast<uint32_t>(cls >> (4u * k)) & 15u;
        const uint8_t c = static_cast<uint8_t>(byte_of(L.w, k));
        uint32_t at = kImgBytes;
        if (cl == kClSeq) at = r_seq++;
        else if (cl == kClQual) at = o_qual + r_qual++;
        else if (cl == kClId) at = o_id + r_id++;
        else if (cl == kClCom) at = o_com + r_com++;
        else if (cl == kClOpen) {
            if (L.p0 + static_cast<int64_t>(k) > 0) {      // the record in front ends here
                const uint32_t a = o_id + r_id++, b = o_com + r_com++;
                if (a < kImgBytes) img[a] = 0;
                if (b < kImgBytes) img[b] = 0;
                const uint64_t before = b_open + r_open - 1;
                if (before < out.n_rec) {
                    out.rec_end[before] = b_seq + r_seq;
                    if (out.qual_end) out.qual_end[before] = b_qual + r_qual;
                }
            }
            r_open++;
        }
        if (at < kImgBytes) img[at] = c;
    }
    __syncthreads();
    img_store(s_img, 0, t_seq, out.seq, b_seq, out.n_seq);
    img_store(s_img, o_qual, t_qual, out.qual, b_qual, out.n_qual);
    img_store(s_img, o_id, t_id, out.ids, b_id, out.n_ids);
    img_store(s_img, o_com, t_com, out.com, b_com, out.n_com);
    if (blockIdx.x == 0 && threadIdx.x == 0 && out.n_rec) {     // the last record ends where the text does
        out.rec_end[out.n_rec - 1] = out.n_seq;
        if (out.qual_end) out.qual_end[out.n_rec - 1] = out.n_qual;
        if (out.n_ids) out.ids[out.n_ids - 1] = 0;
        if (out.n_com) out.com[out.n_com - 1] = 0;
    }
}

// FASTQ: a record's quality has the length of its sequence
__global__ __launch_bounds__(256) void k_parse_qual_check(const uint64_t *rec_end, const uint64_t *qual_end, uint64_t n_rec, uint32_t *status) {
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; r < n_rec; r += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t ls = rec_end[r] - (r ? rec_end[r - 1] : 0), lq = qual_end[r] - (r ? qual_end[r - 1] : 0);
        if (ls != lq) flag_first(status, kParseStQual, 6, r);
    }
}

}  // namespace

uint64_t parse_tiles(const uint8_t *text, uint64_t n) {
    return n ? (n + (static_cast<uint32_t>(reinterpret_cast<uintptr_t>(text)) & 15u) + kParseTile - 1) / kParseTile : 0;
}

void launch_parse_summary(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, ParseTile *tiles) {
    if (!n) return;
    hipLaunchKernelGGL(k_parse_summary, dim3(static_cast<uint32_t>(parse_tiles(text, n))), dim3(kThreads), 0, stream, text, n, tiles);
}

uint64_t parse_scan_aggs(uint64_t n_tiles) { return (n_tiles + kScanSpan - 1) / kScanSpan; }

void launch_parse_scan_tiles(hipStream_t stream, ParseTile *tiles, uint64_t n_tiles, ParseTile *aggs) {
    if (!n_tiles) return;
    const uint64_t n_aggs = parse_scan_aggs(n_tiles);
    hipLaunchKernelGGL(k_parse_scan_reduce, dim3(static_cast<uint32_t>(n_aggs)), dim3(kThreads), 0, stream, tiles, n_tiles, aggs);
    hipLaunchKernelGGL(k_parse_scan_aggs, dim3(1), dim3(kThreads), 0, stream, aggs, n_aggs);
    hipLaunchKernelGGL(k_parse_scan_emit, dim3(static_cast<uint32_t>(n_aggs)), dim3(kThreads), 0, stream, tiles, n_tiles, aggs);
}

void launch_parse_count(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, const ParseTile *tiles, uint64_t *counts,
                        ParseTotals *totals, uint32_t *status) {
    if (!n) return;
    const uint64_t n_tiles = parse_tiles(text, n);
    hipLaunchKernelGGL(k_parse_count, dim3(static_cast<uint32_t>(n_tiles)), dim3(kThreads), 0, stream, text, n, fastq ? 1u : 0u, tiles, counts,
                       n_tiles, totals, status);
}

void launch_parse_write(hipStream_t stream, const uint8_t *text, uint64_t n, bool fastq, const ParseTile *tiles, const uint64_t *counts,
                        const ParseOut &out) {
    if (!n) return;
    const uint64_t n_tiles = parse_tiles(text, n);
    hipLaunchKernelGGL(k_parse_write, dim3(static_cast<uint32_t>(n_tiles)), dim3(kThreads), 0, stream, text, n, fastq ? 1u : 0u, tiles, counts,
                       n_tiles, out);
}

void launch_parse_qual_check(hipStream_t stream, const uint64_t *rec_end, const uint64_t *qual_end, uint64_t n_rec, uint32_t *status) {
    if (!n_rec) return;
    uint64_t blocks = (n_rec + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_parse_qual_check, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, stream, rec_end, qual_end, n_rec, status);
}

}  // namespace parse
}  // namespace nafgpu
