// screen.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_kmers_build and nafgpu_screen: the distinct k-mers of a source as an
// open-addressing table in HBM, and per record of a query how many of its windows are in that table.  The rules:
// include/nafgpu.h at nafgpu_kmers_build; the passes: screen.h.
//
// A tile is kScreenTile window STARTS; its letters and the kScreenHalo behind them go to LDS once as codes (A C G T/U in either
// case: 0 1 2 3, every other byte: 4, no letter), a lane one aligned 16-byte load, so every letter is read from HBM once per
// pass.  A lane owns 16 starts.  It builds the forward and the reverse-complement word of its first window from the k - 1
// letters in front of its last one and then rolls: per letter two shifts and a mask, and a count of the letters since the last
// non-letter.  A start whose k letters are letters is held against the record ends: its record comes from a search in the end
// table whose result the lane keeps, so a lane of reads searches once or twice and a lane inside a contig never again.  One
// body (tiles<>) serves the count, the insert and the probe.
// The table holds the key itself (plus one: 0 is the empty slot), so membership is exact; the hash only says where the
// probing starts.  Inserts are atomicCAS against the zeroed slot: whichever lane wins, the set of words in the table's chains
// answers the same probes, and the number of winners is the number of distinct keys.
// Lane 0 finds the record of a tile's first start; the other lanes search from it on, and not at all when every start of the
// tile lies in it.  The screen adds a lane's counts to its record when the record changes or its starts end: into LDS, where
// the tile keeps the sums of the kSlots records from its first one on, and from there one atomic per output word and record
// goes to HBM.  A long contig costs four atomics a tile, a read inside a tile four in all (one, without a hit).
// Integer work only: sums, and a lowest start kept by atomicMax of its complement; every output is a function of the input
// alone.  No kernel reads a record end it has not checked (k_sum_check has run; a flagged table ends every kernel at once),
// every letter address comes from a position below the section's size, and every probe stays below `slots`.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "hash64.h"
#include "screen.h"
#include "summary.h"

namespace nafgpu {
namespace scr {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kScreenTile == kThreads * 16, "a lane takes 16 window starts");
constexpr uint32_t kHaloLanes = kScreenHalo / 16;
constexpr uint32_t kNoLetter = 4;

enum Mode : uint32_t { kCount = 0, kInsert = 1, kProbe = 2 };

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

__device__ inline bool flagged(uint64_t n_rec, const uint32_t *status) {
    return n_rec && (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond));
}

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

// the project's 4-bit rule cut to the four letters: case and T/U play no part, every other byte (N, the other IUPAC codes,
// '-', a byte at or above 128, the 0 behind the section) is no letter
__device__ inline uint32_t code_of(uint32_t byte) {
    const uint32_t c = byte & 0xDFu;
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : (c == 'T' || c == 'U') ? 3u : kNoLetter;
}

__device__ inline uint32_t codes4(uint32_t w) {
    return code_of(w & 0xFFu) | (code_of((w >> 8) & 0xFFu) << 8) | (code_of((w >> 16) & 0xFFu) << 16) | (code_of(w >> 24) << 24);
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

// the record of the last start that was looked up: [begin, end) is record rec; a later position is searched from next_lo on
struct Cursor {
    uint64_t begin = 0, end = 0, rec = 0, next_lo = 0;
};

// limit: the end of the last record, or the section's without a table.  -> whether position s lies in a record, then cur's
__device__ inline bool locate(Cursor &cur, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, uint64_t limit, uint64_t s) {
    if (s >= cur.begin && s < cur.end) return true;
    if (s >= limit) return false;
    uint64_t rec = 0, begin = 0, end = n_section;            // without a table the section is record 0
    if (n_rec) {
        rec = record_from(ends, s >= cur.end ? cur.next_lo : 0, n_rec - 1, s);
        end = ends[rec];
        begin = rec ? ends[rec - 1] : 0;
    }
    cur.rec = rec;
    cur.begin = begin;
    cur.end = end;
    cur.next_lo = rec + 1;                                   // (<= last whenever it is used: a position at or behind cur.end and below limit)
    return true;
}

__device__ inline uint64_t first_slot(const KmerTable &table, uint64_t key) { return (hash_mix64(key) & table.hash_mask) & (table.slots - 1); }

// -> 1: this lane's CAS put the key there, 0: it was there, 2: no free slot
__device__ inline uint32_t insert(const KmerTable &table, uint64_t key) {
    const unsigned long long want = key + 1;
    uint64_t at = first_slot(table, key);
    for (uint64_t n = 0; n < table.slots; n++) {
        unsigned long long seen = table.slot[at];
        if (!seen) seen = atomicCAS(&table.slot[at], 0ull, want);
        if (!seen) return 1;
        if (seen == want) return 0;
        at = (at + 1) & (table.slots - 1);
    }
    return 2;
}

__device__ inline bool holds(const KmerTable &table, uint64_t key) {
    const unsigned long long want = key + 1;
    uint64_t at = first_slot(table, key);
    for (uint64_t n = 0; n < table.slots; n++) {
        const unsigned long long seen = table.slot[at];
        if (seen == want) return true;
        if (!seen) return false;
        at = (at + 1) & (table.slots - 1);
    }
    return false;                                            // (a full table without the key)
}

// what a workgroup's lanes share
constexpr uint32_t kSlots = kThreads;                        // records from the tile's first one on that have their sums in LDS
struct Shared {
    uint4 tile[kThreads + kHaloLanes];                       // the tile's codes and its halo's
    unsigned long long sum;                                  // count, insert: the workgroup's
    uint32_t windows[kSlots], hits[kSlots];                  // probe: the tile's sums of record rec + i, zero between the tiles
    unsigned long long first[kSlots], last[kSlots];
    uint64_t rec, begin, end;                                // the record of the tile's first start (lane 0 finds it)
};

// a lane's sums for the record it is in (probe)
struct Sums {
    uint64_t rec = 0;
    unsigned long long windows = 0, hits = 0, first = 0, last = 0;
};

__device__ inline void add_to(const ScreenWork &work, uint64_t rec, unsigned long long windows, unsigned long long hits, unsigned long long first,
                              unsigned long long last) {
    atomicAdd(&work.windows[rec], windows);
    if (hits) {
        atomicAdd(&work.hits[rec], hits);
        atomicMax(&work.first[rec], first);
        atomicMax(&work.last[rec], last);
    }
}

// a lane's sums go to the tile's in LDS, or to the record's in HBM when the record lies kSlots or more behind the tile's first
// (empty records in between)
__device__ inline void flush(Sums &s, Shared &sh, uint64_t tile_rec, const ScreenWork &work) {
    if (s.windows) {
        const uint64_t i = s.rec - tile_rec;                 // (a start of the tile lies in no record in front of the tile's first)
        if (i < kSlots) {
            atomicAdd(&sh.windows[i], static_cast<uint32_t>(s.windows));
            if (s.hits) {
                atomicAdd(&sh.hits[i], static_cast<uint32_t>(s.hits));
                atomicMax(&sh.first[i], s.first);
                atomicMax(&sh.last[i], s.last);
            }
        } else {
            add_to(work, s.rec, s.windows, s.hits, s.first, s.last);
        }
    }
    s.windows = s.hits = s.first = s.last = 0;
}

// ======================================================================================
// the walk over the tiles: k_kmer_count, k_kmer_insert and k_screen_tiles
// ======================================================================================
template <uint32_t MODE>
__device__ inline void tiles(Shared &sh, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                             const uint32_t *status, uint32_t *status_out, unsigned long long *word, const ScreenWork &work) {
    const uint32_t t = threadIdx.x;
    if (flagged(n_rec, status)) return;                      // the table is refused: none of it is used
    const uint64_t limit = n_rec && ends[n_rec - 1] < n_section ? ends[n_rec - 1] : n_section;   // letters behind the last record belong to none
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kScreenRun;
    if (tile0 * kScreenTile >= limit) return;
    const uint32_t k = table.k < 1 ? 1u : (table.k > kScreenMaxK ? kScreenMaxK : table.k);
    const uint64_t mask = (1ull << (2u * k)) - 1;
    const uint32_t top = 2u * (k - 1);
    const bool aligned = low4(section) == 0;
    const uint8_t *codes = reinterpret_cast<const uint8_t *>(sh.tile) + 16u * t;
    if (t < kSlots) {
        sh.windows[t] = sh.hits[t] = 0;
        sh.first[t] = sh.last[t] = 0;
    }
    if (t == 0) sh.sum = 0;
    // (the first tile's barrier stands between these stores and their use)

    Cursor cur, tile_cur;                                    // tile_cur: lane 0's, for the tiles' first starts
    unsigned long long lane_sum = 0;                         // count: windows; insert: CAS won
    bool full = false;
    Sums sums;

    for (uint32_t r = 0; r < kScreenRun; r++) {
        const uint64_t t0 = (tile0 + r) * kScreenTile;
        if (t0 >= limit) break;                              // (the same in every lane, as is all of the loop's control)
        const uint64_t p0 = t0 + 16ull * t;
        {
            uint32_t w[4] = {0, 0, 0, 0};
            if (p0 < n_section) load16(section, n_section, aligned, p0, w);
            sh.tile[t] = make_uint4(codes4(w[0]), codes4(w[1]), codes4(w[2]), codes4(w[3]));   // (bytes behind the section: no letters)
            if (t < kHaloLanes) {
                const uint64_t ph = t0 + kScreenTile + 16ull * t;
                uint32_t h[4] = {0, 0, 0, 0};
                if (ph < n_section) load16(section, n_section, aligned, ph, h);
                sh.tile[kThreads + t] = make_uint4(codes4(h[0]), codes4(h[1]), codes4(h[2]), codes4(h[3]));
            }
            if (t == 0) {
                // the record of the tile's first start (t0 < limit: there is one): the lanes search from it on, not from the
                // table's begin, and a lane whose starts lie in it does not search at all
                (void)locate(tile_cur, ends, n_rec, n_section, limit, t0);
                sh.rec = tile_cur.rec;
                sh.begin = tile_cur.begin;
                sh.end = tile_cur.end;
            }
        }
        __syncthreads();
        const uint64_t tile_rec = sh.rec;
        if (cur.end <= t0) {                                 // (the lane's record ends in front of the tile: the tile's first is nearer)
            cur.rec = tile_rec;
            cur.begin = sh.begin;
            cur.end = sh.end;
            cur.next_lo = tile_rec + 1;
        }
        if (p0 < limit) {
            uint64_t fwd = 0, rev = 0;
            uint32_t run = 0;                                // letters since the last non-letter
            for (uint32_t j = 0; j + 1 < k; j++) {
                const uint32_t c = codes[j];
                fwd = ((fwd << 2) | (c & 3u)) & mask;
                rev = (rev >> 2) | (static_cast<uint64_t>(3u - (c & 3u)) << top);
                run = c < kNoLetter ? run + 1 : 0;
            }
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const uint32_t c = codes[k - 1 + i];
                fwd = ((fwd << 2) | (c & 3u)) & mask;
                rev = (rev >> 2) | (static_cast<uint64_t>(3u - (c & 3u)) << top);
                run = c < kNoLetter ? run + 1 : 0;
                if (run < k) continue;                       // (a non-letter k - 1 or fewer letters back: its bits are still in the words)
                const uint64_t s = p0 + i;
                if (!locate(cur, ends, n_rec, n_section, limit, s) || s + k > cur.end) continue;
                const uint64_t key = table.canonical && rev < fwd ? rev : fwd;
                if (MODE == kCount) {
                    lane_sum++;
                } else if (MODE == kInsert) {
                    const uint32_t won = insert(table, key);
                    lane_sum += won & 1u;
                    full = full || won == 2;
                } else {
                    if (sums.rec != cur.rec) {
                        flush(sums, sh, tile_rec, work);
                        sums.rec = cur.rec;
                    }
                    sums.windows++;
                    if (holds(table, key)) {
                        const uint64_t rel = s - cur.begin;
                        if (!sums.hits) sums.first = ~static_cast<unsigned long long>(rel);   // (starts ascend: the first is the lowest)
                        sums.hits++;
                        sums.last = rel + k;
                    }
                }
            }
            if (MODE == kProbe) flush(sums, sh, tile_rec, work);
        }
        __syncthreads();                                     // the tile is read before the next one is written
        if (MODE == kProbe && t < kSlots) {
            // the tile's sums: one atomic per output word of a record (a record inside the tile gets no other)
            const uint32_t w = sh.windows[t];
            if (w) {
                add_to(work, tile_rec + t, w, sh.hits[t], sh.first[t], sh.last[t]);
                sh.windows[t] = sh.hits[t] = 0;
                sh.first[t] = sh.last[t] = 0;
            }
            // (the next tile's barrier stands between these stores and the lanes' sums)
        }
    }
    if (MODE != kProbe) {
        if (lane_sum) atomicAdd(&sh.sum, lane_sum);
        if (MODE == kInsert && full) atomicOr(status_out, kScrStFull);
        __syncthreads();
        if (t == 0 && sh.sum) atomicAdd(word, sh.sum);
    }
}

__global__ __launch_bounds__(kThreads) void k_kmer_count(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, KmerTable table,
                                                          const uint32_t *status, unsigned long long *count) {
    __shared__ Shared sh;
    tiles<kCount>(sh, section, n_section, ends, n_rec, table, status, nullptr, count, ScreenWork{nullptr, nullptr, nullptr, nullptr});
}

__global__ __launch_bounds__(kThreads) void k_kmer_insert(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, KmerTable table,
                                                           uint32_t *status, unsigned long long *distinct) {
    __shared__ Shared sh;
    tiles<kInsert>(sh, section, n_section, ends, n_rec, table, status, status, distinct, ScreenWork{nullptr, nullptr, nullptr, nullptr});
}

__global__ __launch_bounds__(kThreads) void k_screen_tiles(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, KmerTable table,
                                                            const uint32_t *status, ScreenWork work) {
    __shared__ Shared sh;
    tiles<kProbe>(sh, section, n_section, ends, n_rec, table, status, nullptr, nullptr, work);
}

// record k: positions [lo, hi) of the section; without a table the section is record 0
__device__ inline void bounds(const uint64_t *ends, uint64_t n_rec, uint64_t n_section, uint64_t k, uint64_t &lo, uint64_t &hi) {
    lo = 0;
    hi = n_section;
    if (n_rec) {
        hi = ends[k];
        if (k) lo = ends[k - 1];
    }
}

__device__ inline void store_region(nafgpu_region *at, uint64_t k, uint64_t a, uint64_t b) {
    uint4 *out = reinterpret_cast<uint4 *>(at);
    out[0] = make_uint4(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32), static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32));
    out[1] = make_uint4(static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32), 0, 0);
}
static_assert(sizeof(nafgpu_region) == 32, "a region is two 16-byte stores");

// ======================================================================================
// k_screen_finish: one lane per record, or per pair of mates
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_screen_finish(const uint64_t *ends, uint64_t n_rec, uint64_t n_out, uint64_t n_section, uint64_t min_hits,
                                                             uint32_t min_percent, bool interleaved, bool keep_matched, const uint32_t *status, ScreenWork work,
                                                             nafgpu_region *regions, uint8_t *match, uint8_t *keep, uint64_t *flags,
                                                             unsigned long long *totals) {
    __shared__ unsigned long long s_totals[kScreenTotals];
    if (flagged(n_rec, status)) return;
    const uint32_t t = threadIdx.x;
    if (t < kScreenTotals) s_totals[t] = 0;
    if (blockIdx.x == 0 && t == 0) flags[n_out] = 0;
    __syncthreads();
    const uint32_t per = interleaved ? 2 : 1;
    const uint64_t n_units = n_out / per, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    unsigned long long matched = 0, windows = 0, hits = 0, kept = 0;
    for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kThreads + t; u < n_units; u += stride) {
        bool any = false, mine[2] = {false, false};
#pragma unroll
        for (uint32_t m = 0; m < 2; m++)
            if (m < per) {
                const uint64_t k = u * per + m;
                const unsigned long long w = work.windows[k], h = work.hits[k];
                windows += w;
                hits += h;
                mine[m] = h >= (min_hits > 1 ? min_hits : 1) && h * 100ull >= static_cast<unsigned long long>(min_percent) * w;
                any = any || mine[m];
                uint64_t a = 0, b = 0;
                if (h) {
                    a = ~work.first[k];
                    b = work.last[k];
                }
                store_region(regions + k, k, a, b);
            }
        const bool pass = any == keep_matched;
#pragma unroll
        for (uint32_t m = 0; m < 2; m++)
            if (m < per) {
                const uint64_t k = u * per + m;
                uint64_t lo, hi;
                bounds(ends, n_rec, n_section, k, lo, hi);
                match[k] = any ? 1 : 0;
                keep[k] = pass ? 1 : 0;
                flags[k] = pass ? 1 : 0;
                matched += any ? 1 : 0;
                if (pass) kept += hi - lo;
            }
    }
    if (matched) atomicAdd(&s_totals[0], matched);
    if (windows) atomicAdd(&s_totals[1], windows);
    if (hits) atomicAdd(&s_totals[2], hits);
    if (kept) atomicAdd(&s_totals[3], kept);
    __syncthreads();
    if (t < kScreenTotals && s_totals[t]) atomicAdd(&totals[t], s_totals[t]);
}

// ======================================================================================
// k_screen_compact: one lane per record
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_screen_compact(const uint64_t *ends, uint64_t n_rec, uint64_t n_out, uint64_t n_section, const uint8_t *keep,
                                                              const uint64_t *where, uint64_t n_kept, nafgpu_region *kept) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n_out; k += stride) {
        if (!keep[k] || where[k] >= n_kept) continue;
        uint64_t lo, hi;
        bounds(ends, n_rec, n_section, k, lo, hi);
        store_region(kept + where[k], k, 0, hi - lo);
    }
}

uint32_t blocks_for(uint64_t items, uint64_t per_block, uint32_t most) {
    const uint64_t blocks = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(blocks < 1 ? 1 : (blocks > most ? most : blocks));
}

dim3 tile_grid(uint64_t n_section) {
    constexpr uint64_t run = static_cast<uint64_t>(kScreenRun) * kScreenTile;
    return dim3(static_cast<uint32_t>((n_section + run - 1) / run));
}

}  // namespace

void launch_kmer_count(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                       const uint32_t *status, unsigned long long *count) {
    if (!n_section) return;
    hipLaunchKernelGGL(k_kmer_count, tile_grid(n_section), dim3(kThreads), 0, stream, letters, n_section, ends, n_rec, table, status, count);
}

void launch_kmer_insert(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                        uint32_t *status, unsigned long long *distinct) {
    if (!n_section) return;
    hipLaunchKernelGGL(k_kmer_insert, tile_grid(n_section), dim3(kThreads), 0, stream, letters, n_section, ends, n_rec, table, status, distinct);
}

void launch_screen_tiles(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const KmerTable &table,
                         const uint32_t *status, const ScreenWork &work) {
    if (!n_section) return;
    hipLaunchKernelGGL(k_screen_tiles, tile_grid(n_section), dim3(kThreads), 0, stream, letters, n_section, ends, n_rec, table, status, work);
}

void launch_screen_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_screen_opts &opts, const uint32_t *status,
                          const ScreenWork &work, nafgpu_region *regions, uint8_t *match, uint8_t *keep, uint64_t *flags, unsigned long long *totals) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL(k_screen_finish, dim3(blocks_for(n_out, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec, n_out, n_section, opts.min_hits,
                       static_cast<uint32_t>(opts.min_percent), opts.interleaved != 0, opts.keep_matched != 0, status, work, regions, match, keep, flags, totals);
}

void launch_screen_compact(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const uint8_t *keep, const uint64_t *where,
                           uint64_t n_kept, nafgpu_region *kept) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL(k_screen_compact, dim3(blocks_for(n_out, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec, n_out, n_section, keep, where, n_kept,
                       kept);
}

}  // namespace scr
}  // namespace nafgpu
