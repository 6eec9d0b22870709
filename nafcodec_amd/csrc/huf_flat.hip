// huf_flat.hip -- k_huf_flat: Huffman literal streams whose tree is FLAT (plan.h: kTblFlat), decoded as a gather.
//
// A zstd Huffman tree is complete, so a tree of 2^L symbols gives every one of them a code of exactly L bits, and
// symbol j of a (backward) stream of n symbols then sits at bits [(n - 1 - j) L, (n - j) L) of the stream -- known
// without decoding symbols 0 .. j - 1.  Nothing of k_huf_decode's serial walk is needed: every 16 bytes of output are
// produced on their own from the dwords that cover their codes, and stored as one aligned 16-byte piece.
//   * work unit: one workgroup per stream (<= 32 Ki symbols), kFlatThreads lanes; lane t owns pieces t, t + 256, ...
//     of the destination, so a wave's store instruction writes 1 KB in a row and its loads are dwords in a row
//     (falling addresses: the stream is read backwards).  A lane has 8 (ASCII) or 4 (bytes) pieces in flight: a full
//     stream of a DNA archive is two rounds of the workgroup.
//   * table: the workgroup stages its tree once from the pool (2^L entries of len << 8 | sym) as a table indexed by
//     one code (L > 4) or two codes (L <= 4) whose entries hold the bytes to emit (ASCII: byte_chars of each symbol).
//   * edges: the first and the last piece of a stream may hold bytes of a neighbour, or none: they go out byte-wise.
//   * bounds: dword loads start at most 3 bytes in front of the stream and end at most 7 bytes behind it (inside
//     kSrcFrontPad / kSrcBackPad); nothing is written outside [dst, dst + n_syms * kOutB).
//   * errors: what k_huf_decode's end test amounts to for a flat tree -- the last byte holds the end mark and the bits
//     below it are n_syms * L -- with the same code and detail.
// DESIGN.md section 4 has the argument and the measurements.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kernels.h"
#include "plan.h"

namespace nafgpu {

namespace {

// flat_stream must become part of the kernel: called as a function its pointers lose their address space (flat
// instead of global memory instructions, which count against the LDS counter too)
#ifdef NAFGPU_EMU
#define NAFGPU_FLAT_INLINE inline
#else
#define NAFGPU_FLAT_INLINE __forceinline__
#endif

// The geometry: lanes per stream, and pieces a lane has in flight per round -- by output mode, because a piece in flight
// costs the byte-mode kernel more registers (72 VGPRs at 4, 137 at 8) than the ASCII one (58 at 4, 100 at 8).  Measured on
// the headline archive (profiles/r06_flat_geometry_probe.log): 256 x 8 is 9 % faster than 256 x 4 at
// half its waves per SIMD; 64 and 128 lanes, 512 lanes, and 2, 6, 12 or 16 pieces are no faster than 256 x 4.  The level-3
// leg, where the byte mode runs, does not tell 4 from 8.  Experiment builds override the three values (tools/flat_geometry.sh).
#ifndef NAFGPU_FLAT_THREADS
#define NAFGPU_FLAT_THREADS 256
#endif
#ifndef NAFGPU_FLAT_UNROLL_ASCII
#define NAFGPU_FLAT_UNROLL_ASCII 8
#endif
#ifndef NAFGPU_FLAT_UNROLL_BYTES
#define NAFGPU_FLAT_UNROLL_BYTES 4
#endif
constexpr uint32_t kFlatThreads = NAFGPU_FLAT_THREADS;
constexpr uint32_t kFlatUnrollAscii = NAFGPU_FLAT_UNROLL_ASCII, kFlatUnrollBytes = NAFGPU_FLAT_UNROLL_BYTES;

__device__ inline void flat_flag_error(uint32_t *status, uint32_t code, uint32_t detail) {
    if (atomicCAS(&status[0], 0u, code) == 0u) status[1] = detail;
}

// 4-bit code -> IUPAC character and both characters of a packed byte, as in kernels.hip (reader.rs:121-172)
__device__ inline uint32_t flat_nib_char(uint32_t nib, uint32_t t_char) {
    const uint64_t lo = 0x425359434B47002Dull | (static_cast<uint64_t>(t_char) << 8);   // - T G K C Y S B
    const uint64_t hi = 0x4E56484D44525741ull;                                          // A W R D M H V N
    return static_cast<uint32_t>(((nib & 8u) ? hi : lo) >> (8u * (nib & 7u))) & 0xFFu;
}
__device__ inline uint32_t flat_byte_chars(uint32_t b, uint32_t t_char) {
    return flat_nib_char(b & 15u, t_char) | (flat_nib_char(b >> 4, t_char) << 8);
}

// One stream by the whole workgroup.  sp: the stream's first byte; n: its symbols; dp: where symbol 0 goes;
// x1: the tree's 2^L pool entries.  The caller has checked that the stream holds exactly n * L bits.
template <bool ASCII, uint32_t L>
__device__ NAFGPU_FLAT_INLINE void flat_stream(const uint8_t *sp, uint32_t n, uint8_t *dp, const uint16_t *__restrict__ x1, uint32_t t_char,
                                   uint32_t *s_tbl) {
    constexpr uint32_t kOutB = ASCII ? 2 : 1;              // output bytes per symbol
    constexpr uint32_t kSyms = 16 / kOutB;                 // symbols per piece
    constexpr uint32_t kFlatUnroll = ASCII ? kFlatUnrollAscii : kFlatUnrollBytes;   // pieces per lane in flight
    constexpr uint32_t kPer = L <= 4 ? 2 : 1;              // symbols per look-up
    constexpr uint32_t kIdxBits = kPer * L;
    constexpr uint32_t kLookB = kPer * kOutB;              // bytes per look-up: 1, 2 or 4
    constexpr uint32_t kWords = (kSyms * L + 31) / 32;     // dwords that hold a piece's codes once they start at bit 0
    constexpr uint32_t kCodeMask = (1u << L) - 1u;
    const uint32_t tid = threadIdx.x;

    for (uint32_t i = tid; i < (1u << kIdxBits); i += kFlatThreads) {
        const uint32_t s1 = x1[kPer == 2 ? i >> L : i] & 0xFFu, s2 = x1[i & kCodeMask] & 0xFFu;
        const uint32_t o1 = ASCII ? flat_byte_chars(s1, t_char) : s1, o2 = ASCII ? flat_byte_chars(s2, t_char) : s2;
        s_tbl[i] = kPer == 2 ? o1 | (o2 << (8 * kOutB)) : o1;
    }
    __syncthreads();

    const uint32_t h = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dp) & 15u);    // bytes of piece 0 in front of the stream's
    uint8_t *const d16 = dp - h;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(sp);
    const uint32_t *const sw = reinterpret_cast<const uint32_t *>(sp - (sa & 3u));      // (pointer arithmetic: the address space stays known)
    const uint32_t sbit = static_cast<uint32_t>(sa & 3u) * 8u;                          // bit of *sw at which the stream begins
    // Pieces [pf0, pf1) lie inside the stream; piece 0 (h > 0) and piece pf1 (the stream ends inside it) are its edges.
    const uint32_t end = h + n * kOutB;
    const uint32_t pf0 = h ? 1u : 0u, pf1 = end >> 4;
    // Whole pieces, kFlatUnroll per lane and round (pieces p, p + 256, ...: a round of the workgroup covers
    // kFlatThreads * kFlatUnroll pieces in a row), the dwords of the next round requested before the pieces of this one
    // are stored: memory operations retire in order, so a wait for loads issued BEHIND
    // stores waits for the stores too -- a round trip per kilobyte and wave, 4.3 TB/s (profiles/).  Requested in front of
    // them the loads are waited for with the stores still in flight.
    // Piece p holds symbols j0 .. j0 + kSyms - 1, j0 = (16 p - h) / kOutB (ASCII: h is even, a symbol never straddles
    // two pieces); its codes begin at bit (n - j0 - kSyms) L of the stream: a step of 256 pieces is a whole number of
    // dwords, so the shift `r` is the lane's own.
    constexpr uint32_t kStepWords = kFlatThreads * kSyms * L / 32u;
    uint32_t first = pf0 + tid;
    uint32_t r = 0;
    const uint32_t *w0 = sw;                               // dwords of piece `first`
    if (first < pf1) {
        const uint32_t lo = (n - (first * 16u - h) / kOutB - kSyms) * L + sbit;
        r = lo & 31u;
        w0 = sw + (lo >> 5);
    }
    // the pieces of a round past the last whole one are loaded as that one (the loads stay inside the stream) and not stored
    auto load_round = [&](uint32_t p0, const uint32_t *w, uint32_t (&raw)[kFlatUnroll][kWords + 1]) {
#pragma unroll
        for (uint32_t u = 0; u < kFlatUnroll; u++) {
            const uint32_t *wu = p0 + u * kFlatThreads < pf1 ? w - u * kStepWords : w;
#pragma unroll
            for (uint32_t k = 0; k <= kWords; k++) raw[u][k] = wu[k];
        }
    };
    uint32_t cur[kFlatUnroll][kWords + 1];
    if (first < pf1) load_round(first, w0, cur);
    while (first < pf1) {
        const uint32_t next = first + kFlatUnroll * kFlatThreads;
        const uint32_t *w1 = w0 - kFlatUnroll * kStepWords;
        uint32_t nxt[kFlatUnroll][kWords + 1];
        if (next < pf1) load_round(next, w1, nxt);
#pragma unroll
        for (uint32_t u = 0; u < kFlatUnroll; u++) {
            const uint32_t p = first + u * kFlatThreads;
            uint32_t nw[kWords];
#pragma unroll
            for (uint32_t k = 0; k < kWords; k++) nw[k] = __builtin_amdgcn_alignbit(cur[u][k + 1], cur[u][k], r);
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t t = 0; t < kSyms / kPer; t++) {
                const uint32_t off = (kSyms - kPer * (t + 1u)) * L, q = off >> 5, s = off & 31u;
                uint32_t v = nw[q] >> s;
                if (s + kIdxBits > 32u) v |= nw[q + 1] << (32u - s);
                const uint32_t e = s_tbl[v & ((1u << kIdxBits) - 1u)];
                o[(t * kLookB) >> 2] |= e << (8u * ((t * kLookB) & 3u));
            }
            if (p < pf1) *reinterpret_cast<uint4 *>(d16 + static_cast<size_t>(p) * 16u) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (next < pf1) {
#pragma unroll
            for (uint32_t u = 0; u < kFlatUnroll; u++)
#pragma unroll
                for (uint32_t k = 0; k <= kWords; k++) cur[u][k] = nxt[u][k];
        }
        first = next;
        w0 = w1;
    }
    // the edges, byte-wise: lane 0 the first piece, lane 1 the last (one and the same when the stream lies inside one piece)
    const bool tail = (end & 15u) != 0 && (pf1 != 0 || !h);
    if ((tid == 0 && h) || (tid == 1 && tail)) {
        const uint32_t p = tid == 0 ? 0u : pf1;
        const int32_t j0 = (static_cast<int32_t>(p * 16u) - static_cast<int32_t>(h)) / static_cast<int32_t>(kOutB);
        for (uint32_t i = 0; i < kSyms; i++) {
            const int32_t j = j0 + static_cast<int32_t>(i);
            if (j < 0 || static_cast<uint32_t>(j) >= n) continue;
            const uint32_t b = (n - 1u - static_cast<uint32_t>(j)) * L;
            uint32_t v = sp[b >> 3];
            if ((b & 7u) + L > 8u) v |= static_cast<uint32_t>(sp[(b >> 3) + 1u]) << 8;
            const uint32_t code = (v >> (b & 7u)) & kCodeMask;
            const uint32_t e = s_tbl[kPer == 2 ? code << L : code];
            uint8_t *d = dp + static_cast<size_t>(j) * kOutB;
            d[0] = static_cast<uint8_t>(e);
            if (ASCII) d[1] = static_cast<uint8_t>(e >> 8);
        }
    }
}

// grid: 64 workgroups per task, workgroup k of a task takes its k-th stream
template <bool ASCII>
__global__ __launch_bounds__(kFlatThreads) void k_huf_flat(const uint8_t *__restrict__ src, const HufTask *__restrict__ tasks,
                                                  const HufTblCopy *__restrict__ copies, const HufStream *__restrict__ streams,
                                                  const uint16_t *__restrict__ pool, const uint64_t *__restrict__ blk_base,
                                                  uint8_t *dst_base, uint32_t t_char, uint32_t *status) {
    constexpr uint32_t kOutB = ASCII ? 2 : 1;
    __shared__ uint32_t s_tbl[256];
    if (status[0] != 0) return;
    const HufTask task = tasks[blockIdx.x / static_cast<uint32_t>(kHufWave)];
    const uint32_t k = blockIdx.x % static_cast<uint32_t>(kHufWave);
    if (k >= task.n_streams) return;
    const uint32_t me = task.first_stream + k;
    const HufStream st = streams[me];
    const uint32_t L = st.max_bits;                        // (pack_tasks: the tree's code length; tbl_lds: which of the task's trees)
    const uint32_t lastb = src[st.src_end - 1];
    const uint32_t hb = 31u - static_cast<uint32_t>(__clz(static_cast<int>(lastb | 1u)));
    const uint64_t bits = static_cast<uint64_t>(st.src_len - 1u) * 8u + hb;
    if (lastb == 0 || bits != static_cast<uint64_t>(st.n_syms) * L) {     // no end mark, or not exactly n_syms codes below it
        if (threadIdx.x == 0) flat_flag_error(status, kStHufBadEnd, me);
        return;
    }
    const uint8_t *sp = src + (st.src_end - st.src_len);
    uint8_t *dp = dst_base + ((st.flags & 1u) ? st.dst : (blk_base[st.blk] + static_cast<uint32_t>(st.dst)) * kOutB);
    const uint16_t *x1 = pool + copies[task.first_copy + st.tbl_lds].pool_off;
    switch (L) {
    case 1: flat_stream<ASCII, 1>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 2: flat_stream<ASCII, 2>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 3: flat_stream<ASCII, 3>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 4: flat_stream<ASCII, 4>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 5: flat_stream<ASCII, 5>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 6: flat_stream<ASCII, 6>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 7: flat_stream<ASCII, 7>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    case 8: flat_stream<ASCII, 8>(sp, st.n_syms, dp, x1, t_char, s_tbl); break;
    default:                                               // (a host bug: pack_tasks takes trees of 2 .. 256 symbols only)
        if (threadIdx.x == 0) flat_flag_error(status, kStInternal, me);
        break;
    }
}

}  // namespace

void launch_huf_flat(hipStream_t stream, const uint8_t *src, const HufTask *tasks, const HufClass &cls, const HufTblCopy *copies,
                     const HufStream *streams, const uint16_t *pool, const uint64_t *blk_base, uint8_t *out, uint8_t *lit,
                     bool ascii, uint32_t t_char, uint32_t *status) {
    if (!cls.n_tasks) return;
    const HufTask *t0 = tasks + cls.first_task;
    const dim3 grid(cls.n_tasks * static_cast<uint32_t>(kHufWave));
    if (ascii && !cls.to_lit)                              // the literal buffer always holds packed bytes
        hipLaunchKernelGGL(k_huf_flat<true>, grid, dim3(kFlatThreads), 0, stream, src, t0, copies, streams, pool, blk_base, out, t_char, status);
    else
        hipLaunchKernelGGL(k_huf_flat<false>, grid, dim3(kFlatThreads), 0, stream, src, t0, copies, streams, pool, blk_base,
                           cls.to_lit ? lit : out, t_char, status);
}

}  // namespace nafgpu
