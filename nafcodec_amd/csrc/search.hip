// search.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_search: records in HBM -> every window of a record that matches
// one of up to 16 patterns within a few substitutions, as nafgpu_region.  The rules: include/nafgpu.h at nafgpu_search; the
// passes: search.h.
//
// The match is bit-parallel Shift-And with one 64-bit state word per allowed mismatch.  A tile is kSearchTile window STARTS;
// its letters and the kSearchHalo behind them go to LDS once (a lane one aligned 16-byte load, as codes: the 4-bit set of a
// nucleotide, the byte itself otherwise), so every letter is read from HBM once per pass.  A lane owns 16 starts.  Per row
// (a pattern or its reverse complement, m letters) it walks the m - 1 + 16 letters from its first start on with an empty
// state -- exact, because a window that starts in the lane's range cannot have begun earlier -- and looks at bit m - 1 after
// each of the last 16.  The row tables (per code the pattern positions that accept it) lie in LDS.  Only a candidate is held
// against the record ends, in a loop of its own behind the 16 positions: its record comes from a search in the end table
// whose result a lane keeps between candidates.
// Sizes and order: the count pass leaves one count per tile, the scan trio turns them into where every tile writes, the write
// pass matches again and places a lane's hits by a prefix sum of the lanes' counts through LDS, positions ascending and rows
// ascending inside a position.  Integer work only, no atomic cursor: the output does not depend on the schedule.
// No kernel reads a record end it has not checked (k_sum_check has run; a flagged table ends every kernel at once), and
// every letter address comes from a position below the section's size.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "search.h"
#include "summary.h"

namespace nafgpu {
namespace srch {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kSearchTile == kThreads * 16, "a lane takes 16 window starts");
constexpr uint32_t kHaloLanes = kSearchHalo / 16;

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

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

__device__ inline uint32_t map4(const uint8_t *tab, uint32_t w) {
    return static_cast<uint32_t>(tab[w & 0xFFu]) | (static_cast<uint32_t>(tab[(w >> 8) & 0xFFu]) << 8) |
           (static_cast<uint32_t>(tab[(w >> 16) & 0xFFu]) << 16) | (static_cast<uint32_t>(tab[w >> 24]) << 24);
}

// the first k in [lo, last] with ends[k] > at (there is one: ends[last] > at), by doubling steps from lo and then halving
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

// one letter: state d keeps the pattern prefixes that end here with at most d substitutions
template <uint32_t K>
__device__ inline void step(uint64_t *R, uint64_t accept) {
#pragma unroll
    for (uint32_t d = K; d > 0; d--) R[d] = (((R[d] << 1) | 1ull) & accept) | ((R[d - 1] << 1) | 1ull);
    R[0] = ((R[0] << 1) | 1ull) & accept;
}

// ======================================================================================
// k_search_tiles
// ======================================================================================
// NUC: the letters go through the 256-byte code table and a row has 16 masks; else a row has 256.  K: the allowed
// substitutions.  WRITE: the second pass.
template <bool NUC, uint32_t K, bool WRITE>
__global__ __launch_bounds__(kThreads) void k_search_tiles(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                                                            const SearchRows *rows, const uint32_t *status, uint64_t *base,
                                                            unsigned long long *row_hits, nafgpu_region *regions, nafgpu_hit_info *info) {
    constexpr uint32_t NC = NUC ? 16 : 256;
    constexpr uint32_t ROWS = NUC ? kSearchMaxRows : NAFGPU_SEARCH_MAX_PATTERNS;
    __shared__ uint64_t s_accept[ROWS * NC];
    __shared__ uint8_t s_code[NUC ? 256 : 16];
    __shared__ uint32_t s_len[kSearchMaxRows];
    __shared__ uint32_t s_row[kSearchMaxRows];               // the count pass: the hits of every row in this run
    __shared__ uint4 s_tile[kThreads + kHaloLanes];          // the tile's codes and its halo's
    __shared__ uint32_t s_scan[2 * kThreads];                // the write pass: the lanes' counts, summed
    __shared__ uint32_t s_total;
    const uint32_t t = threadIdx.x;
    if (n_rec && (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond))) return;   // the table is refused: none of it is used
    const uint64_t last = n_rec ? n_rec - 1 : 0;
    const uint64_t limit = n_rec && ends[last] < n_section ? ends[last] : n_section;  // letters behind the last record belong to none
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kSearchRun;
    if (tile0 * kSearchTile >= limit) return;
    const uint32_t n_rows = rows->n_rows < ROWS ? rows->n_rows : ROWS;
    const uint32_t strand_shift = rows->strand_shift & 1u;
    for (uint32_t i = t; i < n_rows * NC; i += kThreads) s_accept[i] = rows->accept[i];
    if constexpr (NUC) s_code[t] = rows->code[t];
    if (t < kSearchMaxRows) {
        const uint32_t m = t < n_rows ? rows->length[t] : 1u;
        s_len[t] = m < 1 ? 1u : (m > NAFGPU_SEARCH_MAX_LENGTH ? static_cast<uint32_t>(NAFGPU_SEARCH_MAX_LENGTH) : m);
        s_row[t] = 0;
    }
    if (t == 0) s_total = 0;
    __syncthreads();
    const bool aligned = low4(section) == 0;
    const uint8_t *letters = reinterpret_cast<const uint8_t *>(s_tile) + 16u * t;

    // the record of the last candidate: [cur_begin, cur_end) is record cur_rec; a later position is searched from next_lo on
    uint64_t cur_begin = 0, cur_end = 0, cur_rec = 0, next_lo = 0;
    auto locate = [&](uint64_t s) -> bool {
        if (s >= cur_begin && s < cur_end) return true;
        if (s >= limit) return false;
        uint64_t rec = 0, begin = 0, end = n_section;        // without a table the section is record 0
        if (n_rec) {
            rec = record_from(ends, s >= cur_end ? next_lo : 0, last, s);
            end = ends[rec];
            begin = rec ? ends[rec - 1] : 0;
        }
        cur_rec = rec;
        cur_begin = begin;
        cur_end = end;
        next_lo = rec + 1;                                   // (<= last whenever it is used: a position at or behind cur_end and below limit)
        return true;
    };

    for (uint32_t r = 0; r < kSearchRun; r++) {
        const uint64_t tile = tile0 + r, t0 = tile * kSearchTile;
        if (t0 >= limit) break;                              // (the same in every lane, as is all of the loop's control)
        uint64_t at = 0, bound = 0;
        if constexpr (WRITE) {
            at = base[tile];
            bound = base[tile + 1];
            if (bound == at) continue;                       // nothing starts in this tile
        }
        // ---- the tile's letters and its halo's, as codes
        const uint64_t p0 = t0 + 16ull * t;
        {
            uint32_t w[4] = {0, 0, 0, 0};
            if (p0 < n_section) load16(section, n_section, aligned, p0, w);
            if constexpr (NUC) {
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) w[i] = map4(s_code, w[i]);   // (bytes behind the section become the code of 0: no record holds them)
            }
            s_tile[t] = make_uint4(w[0], w[1], w[2], w[3]);
            if (t < kHaloLanes) {
                const uint64_t ph = t0 + kSearchTile + 16ull * t;
                uint32_t h[4] = {0, 0, 0, 0};
                if (ph < n_section) load16(section, n_section, aligned, ph, h);
                if constexpr (NUC) {
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++) h[i] = map4(s_code, h[i]);
                }
                s_tile[kThreads + t] = make_uint4(h[0], h[1], h[2], h[3]);
            }
        }
        __syncthreads();

        // ---- the match: hit[i] holds the rows that start at p0 + i, mism[i] two bits per row
        uint32_t hit[16];
        uint64_t mism[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            hit[i] = 0;
            mism[i] = 0;
        }
        uint32_t lane_count = 0;
        if (p0 < limit) {
            for (uint32_t row = 0; row < n_rows; row++) {
                const uint32_t m = s_len[row];
                const uint64_t *accept = s_accept + row * NC;
                uint64_t R[K + 1];
#pragma unroll
                for (uint32_t d = 0; d <= K; d++) R[d] = 0;
                for (uint32_t j = 0; j + 1 < m; j++) step<K>(R, accept[letters[j]]);
                uint32_t candidates = 0, subs = 0;           // bit i: a window at p0 + i is within K; two bits per i: its substitutions
#pragma unroll
                for (uint32_t i = 0; i < 16; i++) {
                    step<K>(R, accept[letters[m - 1 + i]]);
                    candidates |= (static_cast<uint32_t>(R[K] >> (m - 1)) & 1u) << i;
                    if constexpr (WRITE && K > 0) {
                        uint32_t within = 0;                 // the states that hold it: K + 1 - its substitutions
#pragma unroll
                        for (uint32_t d = 0; d < K; d++) within += static_cast<uint32_t>(R[d] >> (m - 1)) & 1u;
                        subs |= (K - within) << (2u * i);
                    }
                }
                // only a candidate is held against its record's end
                uint32_t accepted = 0;
                for (uint32_t c = candidates; c; c &= c - 1) {
                    const uint32_t i = static_cast<uint32_t>(__builtin_ctz(c));
                    const uint64_t s = p0 + i;
                    if (locate(s) && s + m <= cur_end) accepted |= 1u << i;
                }
                if (!accepted) continue;
                const uint32_t row_count = static_cast<uint32_t>(__popcll(accepted));
                lane_count += row_count;
                if constexpr (WRITE) {
#pragma unroll
                    for (uint32_t i = 0; i < 16; i++)
                        if (accepted >> i & 1u) {
                            hit[i] |= 1u << row;
                            mism[i] |= static_cast<uint64_t>((subs >> (2u * i)) & 3u) << (2u * row);
                        }
                } else {
                    atomicAdd(&s_row[row], row_count);
                }
            }
        }

        if constexpr (!WRITE) {
            if (lane_count) atomicAdd(&s_total, lane_count);
            __syncthreads();                                 // (and the tile is read before the next one is written)
            if (t == 0) {
                base[tile] = s_total;
                s_total = 0;
            }
            __syncthreads();
        } else {
            // ---- where the lane writes: the sum of the counts of the lanes in front of it
            uint32_t from = 0;
            s_scan[t] = lane_count;
            __syncthreads();
            for (uint32_t off = 1; off < kThreads; off <<= 1) {
                uint32_t v = s_scan[from + t];
                if (t >= off) v += s_scan[from + t - off];
                from ^= kThreads;
                s_scan[from + t] = v;
                __syncthreads();
            }
            at += s_scan[from + t] - lane_count;
            uint32_t positions = 0;
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) positions |= (hit[i] ? 1u : 0u) << i;
            for (; positions; positions &= positions - 1) {
                const uint32_t i = static_cast<uint32_t>(__builtin_ctz(positions));
                uint32_t h = 0;
                uint64_t sub = 0;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++)            // (a choice among registers, not an indexed array)
                    if (j == i) {
                        h = hit[j];
                        sub = mism[j];
                    }
                const uint64_t s = p0 + i;
                (void)locate(s);                             // (a hit: it has a record)
                const uint64_t start = s - cur_begin;
                while (h && at < bound) {                    // (the bound holds unless the letters changed between the passes)
                    const uint32_t row = static_cast<uint32_t>(__builtin_ctz(h));
                    h &= h - 1;
                    const uint64_t end = start + s_len[row];
                    uint4 *out = reinterpret_cast<uint4 *>(regions + at);
                    out[0] = make_uint4(static_cast<uint32_t>(cur_rec), static_cast<uint32_t>(cur_rec >> 32), static_cast<uint32_t>(start),
                                        static_cast<uint32_t>(start >> 32));
                    out[1] = make_uint4(static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32), row & strand_shift, 0);
                    *reinterpret_cast<uint2 *>(info + at) = make_uint2(row >> strand_shift, static_cast<uint32_t>(sub >> (2u * row)) & 3u);
                    at++;
                }
            }
            __syncthreads();                                 // the sums are read before the next tile's are written
        }
    }
    if constexpr (!WRITE) {
        if (t < n_rows && s_row[t]) atomicAdd(&row_hits[t], static_cast<unsigned long long>(s_row[t]));
    }
}
static_assert(sizeof(nafgpu_region) == 32 && sizeof(nafgpu_hit_info) == 8, "a region is two 16-byte stores, a hit's info one of 8");

// ======================================================================================
// k_search_begin: one lane per record (and one behind the last): the first hit whose record is not below it
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_search_begin(const nafgpu_region *regions, uint64_t n_hits, uint64_t n_rec, uint64_t *begin) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k <= n_rec; k += stride) {
        uint64_t lo = 0, hi = n_hits;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (regions[mid].record >= k) hi = mid;
            else lo = mid + 1;
        }
        begin[k] = lo;
    }
}

template <bool NUC, uint32_t K>
void launch_tiles(hipStream_t stream, dim3 grid, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                  const SearchRows *d_rows, const uint32_t *status, uint64_t *base, unsigned long long *row_hits, nafgpu_region *regions,
                  nafgpu_hit_info *info) {
    if (regions)
        hipLaunchKernelGGL((k_search_tiles<NUC, K, true>), grid, dim3(kThreads), 0, stream, section, n_section, ends, n_rec, d_rows, status, base, row_hits,
                           regions, info);
    else
        hipLaunchKernelGGL((k_search_tiles<NUC, K, false>), grid, dim3(kThreads), 0, stream, section, n_section, ends, n_rec, d_rows, status, base, row_hits,
                           regions, info);
}

template <bool NUC>
void launch_tiles_k(hipStream_t stream, dim3 grid, uint32_t k, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                    const SearchRows *d_rows, const uint32_t *status, uint64_t *base, unsigned long long *row_hits, nafgpu_region *regions,
                    nafgpu_hit_info *info) {
    switch (k) {
    case 0: launch_tiles<NUC, 0>(stream, grid, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info); break;
    case 1: launch_tiles<NUC, 1>(stream, grid, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info); break;
    case 2: launch_tiles<NUC, 2>(stream, grid, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info); break;
    default: launch_tiles<NUC, 3>(stream, grid, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info); break;
    }
}

}  // namespace

void launch_search_tiles(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                         const SearchRows *d_rows, bool nucleotide, uint32_t max_mismatches, const uint32_t *status, uint64_t *base,
                         unsigned long long *row_hits, nafgpu_region *regions, nafgpu_hit_info *info) {
    if (!n_section) return;
    constexpr uint64_t run = static_cast<uint64_t>(kSearchRun) * kSearchTile;
    const dim3 grid(static_cast<uint32_t>((n_section + run - 1) / run));
    if (nucleotide) launch_tiles_k<true>(stream, grid, max_mismatches, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info);
    else launch_tiles_k<false>(stream, grid, max_mismatches, section, n_section, ends, n_rec, d_rows, status, base, row_hits, regions, info);
}

void launch_search_begin(hipStream_t stream, const nafgpu_region *regions, uint64_t n_hits, uint64_t n_rec, uint64_t *begin) {
    uint64_t blocks = (n_rec + 1 + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_search_begin, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, stream, regions, n_hits, n_rec, begin);
}

}  // namespace srch
}  // namespace nafgpu
