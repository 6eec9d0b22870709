// summary.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_summarize: records in HBM -> eight class counts and a quality
// sum per record, and a histogram of each section.  The rules: include/nafgpu.h at nafgpu_summarize; the passes: summary.h.
//
// The per-record pass is driven by the INPUT: a workgroup takes a run of kSumRun consecutive tiles of kSumTile bytes, a
// lane 16 of them with one aligned 16-byte load, so every letter is read from HBM once.  Which records a tile touches comes
// from the record ends (a search per run, then short searches forward).  Two routes, chosen per tile:
//   long    the tile is cut into pieces at the record ends (a tile inside one record is one piece).  A lane counts those of
//           its 16 bytes that lie in the piece into registers: the class bytes packed in two 64-bit words, a column by two
//           population counts.  The registers are reduced through LDS and added to the record's row (eight atomics) only
//           when the record changes or the run ends: a 250-Mbase record costs one such round per 64 KiB, not per tile.
//   short   the tile's class bytes go to LDS; a lane owns a record (record first + lane, + 256, ...: any number of empty
//           records at one position) and counts its letters there.  A record that lies inside the tile is written with
//           plain stores; the two that reach over the tile's edges are added with atomics.
// The quality sums are the same kernel with the byte's value in the place of the table.  Integer work only: the result does
// not depend on the schedule.  No kernel reads a record end it has not checked: once k_sum_check has flagged the table the
// per-record kernel returns, and every letter address comes from a tile position below the section's size.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "summary.h"

namespace nafgpu {
namespace sum {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
static_assert(kSumTile == kThreads * 16, "a lane takes 16 input bytes");

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

__device__ inline void flag_first(uint32_t *status, uint32_t bit, uint32_t slot, uint64_t at) {
    atomicOr(&status[0], bit);
    atomicMax(reinterpret_cast<unsigned long long *>(status + slot), ~static_cast<unsigned long long>(at));   // the lowest: the largest complement
}

// the low n bytes of a 64-bit word
__device__ inline uint64_t low_bytes(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8u * n)) - 1ull; }

// section[p .. p + 16) as four words; bytes at or behind `bound` read as 0 and are never touched (p < bound)
__device__ inline void load16(const uint8_t *section, uint64_t bound, bool aligned, uint64_t p, uint32_t *w) {
    if (aligned && p + 16 <= bound) {
        const uint4 v = *reinterpret_cast<const uint4 *>(section + p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
    const uint32_t n = bound - p < 16 ? static_cast<uint32_t>(bound - p) : 16u;
    for (uint32_t k = 0; k < n; k++) w[k >> 2] |= static_cast<uint32_t>(section[p + k]) << (8u * (k & 3u));
}

// ======================================================================================
// k_sum_check: one lane per record
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_sum_check(const uint64_t *ends, uint64_t n_rec, uint64_t n_section, uint32_t *status) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n_rec; k += stride) {
        const uint64_t e = ends[k], before = k ? ends[k - 1] : 0;
        if (e < before) flag_first(status, kSumStDecreasing, 2, k);
        if (e > n_section) flag_first(status, kSumStBeyond, 4, k);
        if (k == n_rec - 1) *reinterpret_cast<unsigned long long *>(status + 6) = e;
    }
}

// ======================================================================================
// k_sum_hist: 256 32-bit bins per wave in LDS, added to the 64-bit bins in HBM once per chunk
// ======================================================================================
// A wave of DNA has four or five byte values: one LDS atomic per letter is sixty-four lanes on a handful of addresses,
// and they are served one after the other (measured: 1.18 ms per Gbase, twice the per-record pass).  So a lane first
// gathers equal bytes among its 16 -- it takes its first byte that is not counted yet, finds the others by a zero-byte
// test over the two 64-bit words and adds their number with ONE atomic: as many atomics as the 16 bytes have distinct
// values -- and the wave's bins exist in kHistCopies copies, lane l adding to copy l mod kHistCopies, bin v of copy c at word
// v * kHistCopies + c: lanes that meet on a value are spread over kHistCopies banks.
constexpr uint32_t kHistCopies = 8;

// 0x80 in every byte of `valid` (0x80 per byte that counts) where x holds the value v
__device__ inline uint64_t equal_bytes(uint64_t x, uint32_t v, uint64_t valid) {
    const uint64_t y = x ^ (0x0101010101010101ull * v), low = 0x7F7F7F7F7F7F7F7Full;
    return ~(((y & low) + low) | y | low) & valid;           // exact: no carry leaves a byte
}

__global__ __launch_bounds__(kThreads) void k_sum_hist(const uint8_t *section, uint64_t n_section, unsigned long long *hist) {
    __shared__ uint32_t s_bins[kWaves * 256 * kHistCopies];
    const uint32_t t = threadIdx.x;
    uint32_t *bins = s_bins + 256 * kHistCopies * (t >> 6) + (t & (kHistCopies - 1));
    for (uint32_t i = t; i < kWaves * 256 * kHistCopies; i += kThreads) s_bins[i] = 0;
    __syncthreads();
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * kSumHistChunk;
    const uint64_t c1 = c0 + kSumHistChunk < n_section ? c0 + kSumHistChunk : n_section;
    const bool aligned = low4(section) == 0;
    for (uint64_t p = c0 + 16ull * t; p < c1; p += kSumTile) {
        uint32_t w[4];
        load16(section, c1, aligned, p, w);
        const uint32_t n = c1 - p < 16 ? static_cast<uint32_t>(c1 - p) : 16u;
        const uint64_t x0 = (static_cast<uint64_t>(w[1]) << 32) | w[0], x1 = (static_cast<uint64_t>(w[3]) << 32) | w[2];
        uint64_t m0 = 0x8080808080808080ull & low_bytes(n), m1 = 0x8080808080808080ull & low_bytes(n > 8 ? n - 8 : 0u);   // the bytes not counted yet
        while (m0 | m1) {
            const uint32_t v = m0 ? static_cast<uint32_t>(x0 >> (__builtin_ctzll(m0) - 7)) & 0xFFu : static_cast<uint32_t>(x1 >> (__builtin_ctzll(m1) - 7)) & 0xFFu;
            const uint64_t e0 = equal_bytes(x0, v, m0), e1 = equal_bytes(x1, v, m1);
            atomicAdd(&bins[v * kHistCopies], static_cast<uint32_t>(__popcll(e0) + __popcll(e1)));
            m0 &= ~e0;
            m1 &= ~e1;
        }
    }
    __syncthreads();
    uint32_t v = 0;                                          // (kThreads == 256: lane t owns bin t)
    for (uint32_t i = 0; i < kWaves; i++)
#pragma unroll
        for (uint32_t c = 0; c < kHistCopies; c++) v += s_bins[256 * kHistCopies * i + t * kHistCopies + c];
    if (v) atomicAdd(&hist[t], static_cast<unsigned long long>(v));
}
static_assert(kThreads == 256, "k_sum_hist: one lane per bin");

// ======================================================================================
// k_sum_tiles
// ======================================================================================
// the first k in [lo, last] with ends[k] > at (there is one: ends[last] > at), by doubling steps from lo and then halving:
// the cost grows with the distance, which between two tiles is the number of records in a tile
__device__ inline uint64_t record_from(const uint64_t *ends, uint64_t lo, uint64_t last, uint64_t at) {
    uint64_t hi = lo, step = 1;
    while (hi < last && ends[hi] <= at) {
        lo = hi + 1;
        hi = last - hi > step ? hi + step : last;
        step <<= 1;
    }
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ends[mid] > at) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ inline uint32_t map4(const uint8_t *tab, uint32_t w) {
    return static_cast<uint32_t>(tab[w & 0xFFu]) | (static_cast<uint32_t>(tab[(w >> 8) & 0xFFu]) << 8) |
           (static_cast<uint32_t>(tab[(w >> 16) & 0xFFu]) << 16) | (static_cast<uint32_t>(tab[w >> 24]) << 24);
}

// of the word that holds bytes [base, base + 8) of a lane's 16: those in [lo, hi), lo <= hi
__device__ inline uint64_t byte_range(uint32_t lo, uint32_t hi, uint32_t base) {
    return low_bytes(hi > base ? hi - base : 0u) & ~low_bytes(lo > base ? lo - base : 0u);
}

__device__ inline uint32_t byte_sum(uint64_t x) {
    const uint64_t y = (x & 0x00FF00FF00FF00FFull) + ((x >> 8) & 0x00FF00FF00FF00FFull);    // four sums of two bytes
    return static_cast<uint32_t>((y * 0x0001000100010001ull) >> 48);
}

// eight bytes -> the columns: class bytes by population counts (QUAL: the bytes' sum in column 0)
template <bool QUAL>
__device__ inline void count8(uint64_t x, uint32_t *acc) {
    if constexpr (QUAL) {
        acc[0] += byte_sum(x);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) acc[c] += static_cast<uint32_t>(__popcll(x & (0x0101010101010101ull << c)));
    }
}

// QUAL: `section` holds qualities, a row is one word (the sum of the bytes); else letters, a row is eight words
template <bool QUAL>
__global__ __launch_bounds__(kThreads) void k_sum_tiles(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                                                         const uint8_t *classes, uint32_t route, unsigned long long *rows, const uint32_t *status) {
    constexpr uint32_t C = QUAL ? 1 : 8;
    __shared__ uint8_t s_tab[QUAL ? 16 : 256];
    __shared__ uint4 s_tile[kThreads];                       // the short route: the tile's class bytes
    __shared__ uint32_t s_red[C * kThreads];
    __shared__ uint32_t s_part[C * 8];
    const uint32_t t = threadIdx.x;
    if (status[0] & (kSumStDecreasing | kSumStBeyond)) return;               // the table is refused: none of it is used
    const uint64_t last = n_rec - 1;
    const uint64_t limit = ends[last] < n_section ? ends[last] : n_section;   // letters behind the last record belong to none
    const uint64_t run0 = static_cast<uint64_t>(blockIdx.x) * kSumRun * kSumTile;
    if (run0 >= limit) return;
    const uint64_t run1 = run0 + static_cast<uint64_t>(kSumRun) * kSumTile < limit ? run0 + static_cast<uint64_t>(kSumRun) * kSumTile : limit;
    if constexpr (!QUAL) {
        s_tab[t] = classes[t];
        __syncthreads();
    }
    const bool aligned = low4(section) == 0;
    const uint32_t *tile_words = reinterpret_cast<const uint32_t *>(s_tile);

    uint32_t acc[C];                                         // the long route: this lane's share of record `cur`, not yet added to its row
#pragma unroll
    for (uint32_t c = 0; c < C; c++) acc[c] = 0;
    bool pending = false;
    uint64_t cur = 0;
    // everything below but `acc` and the lane's letters is the same in every lane of the workgroup
    auto flush = [&]() {
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            s_red[c * kThreads + t] = acc[c];
            acc[c] = 0;
        }
        __syncthreads();
        if (t < C * 8) {                                     // eight partial sums per column
            const uint32_t c = t >> 3, part = t & 7u;
            uint32_t v = 0;
            for (uint32_t i = 0; i < kThreads / 8; i++) v += s_red[c * kThreads + part + 8 * i];
            s_part[t] = v;
        }
        __syncthreads();
        if (t < C) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) v += s_part[t * 8 + i];
            if (v) atomicAdd(&rows[cur * C + t], static_cast<unsigned long long>(v));
        }
        pending = false;
    };

    uint64_t k = record_from(ends, 0, last, run0);           // the record of the tile's first byte
    for (uint64_t t0 = run0; t0 < run1; t0 += kSumTile) {
        const uint64_t t1 = t0 + kSumTile < run1 ? t0 + kSumTile : run1;
        const uint64_t p0 = t0 + 16ull * t;
        uint32_t w[4] = {0, 0, 0, 0};
        if (p0 < t1) load16(section, t1, aligned, p0, w);
        if constexpr (!QUAL) {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) w[i] = map4(s_tab, w[i]);   // (bytes behind t1 become the class of 0: no piece holds them)
        }
        const uint64_t kl = ends[k] >= t1 ? k : record_from(ends, k + 1, last, t1 - 1);   // the record of the tile's last byte
        if (route == kRouteLong || (route == kRouteAuto && kl - k < kSumFewPieces)) {
            const uint64_t x0 = (static_cast<uint64_t>(w[1]) << 32) | w[0], x1 = (static_cast<uint64_t>(w[3]) << 32) | w[2];
            for (uint64_t pos = t0; pos < t1;) {             // k: the record of `pos`
                const uint64_t pe = ends[k] < t1 ? ends[k] : t1;
                if (pending && k != cur) flush();
                cur = k;
                pending = true;
                const uint32_t lo = pos > p0 ? (pos - p0 < 16 ? static_cast<uint32_t>(pos - p0) : 16u) : 0u;
                const uint32_t hi = pe > p0 ? (pe - p0 < 16 ? static_cast<uint32_t>(pe - p0) : 16u) : 0u;
                if (lo < hi) {
                    count8<QUAL>(x0 & byte_range(lo, hi, 0), acc);
                    count8<QUAL>(x1 & byte_range(lo, hi, 8), acc);
                }
                pos = pe;
                if (pos < t1) k = record_from(ends, k + 1, last, pos);
            }
        } else {
            s_tile[t] = make_uint4(w[0], w[1], w[2], w[3]);
            __syncthreads();
            for (uint64_t j = k + t; j <= kl; j += kThreads) {
                const uint64_t r0 = j ? ends[j - 1] : 0, r1 = ends[j];
                const uint64_t a = r0 > t0 ? r0 : t0, b = r1 < t1 ? r1 : t1;
                if (a >= b) continue;                        // an empty record: its row stays zero
                const uint32_t ra = static_cast<uint32_t>(a - t0), rb = static_cast<uint32_t>(b - t0);
                uint32_t cnt[C];
#pragma unroll
                for (uint32_t c = 0; c < C; c++) cnt[c] = 0;
                for (uint32_t wi = ra >> 2; wi < (rb + 3) >> 2; wi++) {
                    uint32_t x = tile_words[wi];
                    if (4 * wi < ra) x &= ~0u << (8u * (ra - 4 * wi));
                    if (4 * wi + 4 > rb) x &= ~0u >> (8u * (4 * wi + 4 - rb));
                    count8<QUAL>(x, cnt);
                }
                unsigned long long *row = rows + j * C;
                if (r0 >= t0 && r1 <= t1) {                  // the whole record lies in this tile: nobody else writes its row
                    if constexpr (QUAL) {
                        row[0] = cnt[0];
                    } else {
#pragma unroll
                        for (uint32_t c = 0; c < 8; c += 2) *reinterpret_cast<uint4 *>(row + c) = make_uint4(cnt[c], 0, cnt[c + 1], 0);
                    }
                } else {                                     // it reaches over an edge of the tile (two records per tile at the most)
#pragma unroll
                    for (uint32_t c = 0; c < C; c++)
                        if (cnt[c]) atomicAdd(&row[c], static_cast<unsigned long long>(cnt[c]));
                }
            }
            __syncthreads();                                 // the tile is read before the next one is written
            k = kl;
        }
        if (t1 < run1 && ends[k] <= t1) k = record_from(ends, k + 1, last, t1);
    }
    if (pending) flush();
}

uint32_t blocks_for(uint64_t n) {
    uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    return static_cast<uint32_t>(blocks ? blocks : 1);
}

}  // namespace

void launch_sum_check(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, uint32_t *status) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_sum_check, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, ends, n_rec, n_section, status);
}

void launch_sum_hist(hipStream_t stream, const uint8_t *section, uint64_t n_section, unsigned long long *hist) {
    if (!n_section) return;
    const dim3 grid(static_cast<uint32_t>((n_section + kSumHistChunk - 1) / kSumHistChunk));
    hipLaunchKernelGGL(k_sum_hist, grid, dim3(kThreads), 0, stream, section, n_section, hist);
}

void launch_sum_tiles(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                      const uint8_t *classes, Route route, unsigned long long *rows, const uint32_t *status) {
    if (!n_section || !n_rec) return;
    constexpr uint64_t run = static_cast<uint64_t>(kSumRun) * kSumTile;
    const dim3 grid(static_cast<uint32_t>((n_section + run - 1) / run)), block(kThreads);
    if (classes)
        hipLaunchKernelGGL((k_sum_tiles<false>), grid, block, 0, stream, section, n_section, ends, n_rec, classes, static_cast<uint32_t>(route), rows, status);
    else
        hipLaunchKernelGGL((k_sum_tiles<true>), grid, block, 0, stream, section, n_section, ends, n_rec, classes, static_cast<uint32_t>(route), rows, status);
}

}  // namespace sum
}  // namespace nafgpu
