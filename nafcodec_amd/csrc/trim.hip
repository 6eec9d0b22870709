// trim.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_trim: records in HBM -> the window of every record that quality trimming
// keeps, as nafgpu_region.  The rules: include/nafgpu.h at nafgpu_trim; the passes: trim.h.
//
// Steps 1 and 3 walk inward from a record's end in chunks of 16 bytes per lane, and stop where the rule stops: on a good read
// that is the first chunk.  A chunk is G lanes: 16 for a record of up to kTrimShort letters, so that a wave holds four record
// ends, and a whole workgroup of 256 for a longer one, so that a record of all-low qualities is still walked 4 096 letters at
// a time.  The chunks lie on the 16-byte grid of the section's address, so a lane's bytes are one aligned 16-byte load
// wherever all 16 lie inside the section, and bounded byte loads of the positions it may use elsewhere.  The running sum of a
// chunk is a prefix sum of the lanes' totals through LDS under the carried sum; every lane then walks its 16 values under its
// own prefix, and the stop, the running maximum and its first position come out of one ordered tree reduction: of two
// neighbouring pieces the later one counts only when the earlier did not stop, and wins only with a strictly larger sum.
// Step 2 is the shape of k_search_tiles: a tile of window STARTS and its halo go to LDS once, a lane slides the window over
// its 16 starts, and only a start whose window fails is held against the record ends and [a, b); the lowest per record is
// kept by a 64-bit atomicMax of its complement, whose result does not depend on the order.
// Integer work only; every kernel's output is a function of its input alone.  No kernel reads a record end it has not
// checked (k_sum_check has run; a flagged table ends every kernel at once), and every byte address comes from a position
// inside a record, so below the section's size.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "summary.h"
#include "trim.h"

namespace nafgpu {
namespace trm {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kTrimTile == kThreads * 16, "a lane takes 16 window starts");
static_assert(kTrimLongLanes == kThreads, "the long route's chunk is a workgroup");
constexpr uint32_t kShortThreads = 64;           // the short route: one wave, four chunks
constexpr uint32_t kHaloLanes = kTrimHalo / 16;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

__device__ inline bool flagged(uint64_t n_rec, const uint32_t *status) {
    return n_rec && (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond));
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

// the window of record k as steps 1 and 2 left it
__device__ inline void window_of(const TrimWork &work, uint64_t k, uint64_t &a, uint64_t &b) {
    a = work.win[2 * k];
    b = work.win[2 * k + 1];
    const unsigned long long c = work.cut[k];
    if (c && ~c < b) b = ~c;
}

// ======================================================================================
// a chunk of G lanes at `cur`, walked up (positions [cur, ..)) or down (tail: positions [.., cur))
// ======================================================================================
// Walking index idx = 16 * lane + slot.  Up: the chunk begins at `edge` on the 16-byte grid at or below cur, idx is position
// edge + idx.  Down: it ends at `edge` on the grid at or above cur, idx is position edge - 1 - idx.
__device__ inline int64_t chunk_edge(uint32_t residue, bool tail, uint64_t cur) {
    const uint32_t m = (static_cast<uint32_t>(cur) + residue) & 15u;
    return tail ? static_cast<int64_t>(cur + ((16u - m) & 15u)) : static_cast<int64_t>(cur) - static_cast<int64_t>(m);
}

struct LaneBytes {
    uint32_t w[4];               // the lane's 16 bytes in walking order
    uint32_t lo, hi;             // the slots [lo, hi) of them that are positions of [vlo, vhi)
};

__device__ inline uint32_t slot(const LaneBytes &lb, uint32_t j) { return (lb.w[j >> 2] >> (8u * (j & 3u))) & 0xFFu; }

// 0 <= vlo <= vhi <= n_section: only positions of [vlo, vhi) are used, and only they are read where the lane's 16 bytes do
// not all lie inside the section
__device__ inline void lane_load(const uint8_t *section, uint64_t n_section, bool tail, int64_t edge, uint32_t lane, uint64_t vlo, uint64_t vhi,
                                 LaneBytes &out) {
    const int64_t pos0 = tail ? edge - 16 * static_cast<int64_t>(lane + 1) : edge + 16 * static_cast<int64_t>(lane);
    int64_t klo = static_cast<int64_t>(vlo) - pos0, khi = static_cast<int64_t>(vhi) - pos0;
    klo = klo < 0 ? 0 : (klo > 16 ? 16 : klo);
    khi = khi < 0 ? 0 : (khi > 16 ? 16 : khi);
    out.w[0] = out.w[1] = out.w[2] = out.w[3] = 0;
    out.lo = out.hi = 0;
    if (khi <= klo) return;
    if (pos0 >= 0 && static_cast<uint64_t>(pos0) + 16 <= n_section) {
        const uint4 v = *reinterpret_cast<const uint4 *>(section + pos0);   // (aligned: the grid is the address's)
        out.w[0] = v.x; out.w[1] = v.y; out.w[2] = v.z; out.w[3] = v.w;
    } else {
#pragma unroll
        for (int64_t k = 0; k < 16; k++)
            if (k >= klo && k < khi) out.w[k >> 2] |= static_cast<uint32_t>(section[pos0 + k]) << (8u * (k & 3u));
    }
    out.lo = static_cast<uint32_t>(klo);
    out.hi = static_cast<uint32_t>(khi);
    if (tail) {
        const uint32_t a = __builtin_bswap32(out.w[3]), b = __builtin_bswap32(out.w[2]), c = __builtin_bswap32(out.w[1]), d = __builtin_bswap32(out.w[0]);
        out.w[0] = a; out.w[1] = b; out.w[2] = c; out.w[3] = d;
        out.lo = 16u - static_cast<uint32_t>(khi);
        out.hi = 16u - static_cast<uint32_t>(klo);
    }
}

// the walk's next chunk, or its end: -> whether it goes on
template <uint32_t G>
__device__ inline bool advance(bool tail, int64_t edge, uint64_t vlo, uint64_t vhi, uint64_t &cur) {
    if (tail) {
        const int64_t next = edge - 16 * static_cast<int64_t>(G);
        if (next <= static_cast<int64_t>(vlo)) return false;
        cur = static_cast<uint64_t>(next);
        return true;
    }
    cur = static_cast<uint64_t>(edge + 16 * static_cast<int64_t>(G));
    return cur < vhi;
}

// ======================================================================================
// step 1: the running sum from one end of record [lo, hi)
// ======================================================================================
// add: the cutoff plus the quality base, so that a byte q adds (add - q).  -> a (front) or b (tail), relative to lo.  Every
// lane of the workgroup calls it; `on` is the same in the G lanes of a chunk.
template <uint32_t G, uint32_t B>
__device__ inline uint64_t walk_sum(const uint8_t *quality, uint64_t n_section, uint32_t residue, bool on, bool tail, uint64_t lo, uint64_t hi, int32_t add,
                                    int32_t *s_scan, long long *s_max, uint32_t *s_arg, uint32_t *s_stop) {
    const uint32_t t = threadIdx.x, lane = t % G, g0 = t - lane;
    uint64_t cur = tail ? hi : lo, res = tail ? hi - lo : 0;
    long long sum = 0, best = 0;
    bool go = on && hi > lo;
    while (__syncthreads_or(go)) {
        LaneBytes lb;
        lb.w[0] = lb.w[1] = lb.w[2] = lb.w[3] = 0;
        lb.lo = lb.hi = 0;
        int64_t edge = 0;
        if (go) {
            edge = chunk_edge(residue, tail, cur);
            lane_load(quality, n_section, tail, edge, lane, tail ? lo : cur, tail ? cur : hi, lb);
        }
        int32_t total = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (j >= lb.lo && j < lb.hi) total += add - static_cast<int32_t>(slot(lb, j));
        // ---- the lanes' totals, summed over the chunk
        uint32_t from = 0;
        s_scan[t] = total;
        __syncthreads();
        for (uint32_t off = 1; off < G; off <<= 1) {
            int32_t v = s_scan[from + t];
            if (lane >= off) v += s_scan[from + t - off];
            from ^= B;
            s_scan[from + t] = v;
            __syncthreads();
        }
        const int32_t chunk_total = s_scan[from + g0 + G - 1];
        // ---- the lane's 16 values under its prefix: where it stops, its maximum above the carried one and where that is first
        long long s = sum + (s_scan[from + t] - total), mine = best;
        uint32_t arg = kNone;
        bool stopped = false;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (!stopped && j >= lb.lo && j < lb.hi) {
                s += add - static_cast<int32_t>(slot(lb, j));
                if (s < 0) {
                    stopped = true;
                } else if (s > mine) {
                    mine = s;
                    arg = 16u * lane + j;
                }
            }
        s_stop[t] = stopped ? 1u : 0u;
        s_max[t] = mine;
        s_arg[t] = arg;
        // ---- in walking order: a later piece counts while the earlier ones have not stopped, and wins only when it is larger
        for (uint32_t off = 1; off < G; off <<= 1) {
            __syncthreads();
            if ((lane & (2u * off - 1u)) == 0 && !s_stop[t]) {
                if (s_max[t + off] > s_max[t]) {
                    s_max[t] = s_max[t + off];
                    s_arg[t] = s_arg[t + off];
                }
                s_stop[t] = s_stop[t + off];
            }
        }
        __syncthreads();
        if (go) {
            if (s_max[g0] > best) {
                best = s_max[g0];
                const int64_t p = tail ? edge - 1 - static_cast<int64_t>(s_arg[g0]) : edge + static_cast<int64_t>(s_arg[g0]);
                res = static_cast<uint64_t>(p) - lo + (tail ? 0 : 1);
            }
            sum += chunk_total;
            go = advance<G>(tail, edge, lo, hi, cur) && !s_stop[g0];
        }
    }
    return res;
}

// ======================================================================================
// step 3: the N at one end of the positions [vlo, vhi)
// ======================================================================================
// -> front: the first position that holds no N, or vhi; tail: one past the last that holds none, or vlo
template <uint32_t G>
__device__ inline uint64_t walk_n(const uint8_t *letters, uint64_t n_section, uint32_t residue, bool on, bool tail, uint64_t vlo, uint64_t vhi, uint32_t *s_arg) {
    const uint32_t t = threadIdx.x, lane = t % G, g0 = t - lane;
    uint64_t cur = tail ? vhi : vlo, res = tail ? vlo : vhi;
    bool go = on && vhi > vlo;
    while (__syncthreads_or(go)) {
        LaneBytes lb;
        lb.w[0] = lb.w[1] = lb.w[2] = lb.w[3] = 0;
        lb.lo = lb.hi = 0;
        int64_t edge = 0;
        if (go) {
            edge = chunk_edge(residue, tail, cur);
            lane_load(letters, n_section, tail, edge, lane, tail ? vlo : cur, tail ? cur : vhi, lb);
        }
        uint32_t first = kNone;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t j = 15u - i;                      // (downward: the lowest slot is the one that stays)
            if (j >= lb.lo && j < lb.hi && (slot(lb, j) & 0xDFu) != 'N') first = 16u * lane + j;
        }
        s_arg[t] = first;
        for (uint32_t off = 1; off < G; off <<= 1) {
            __syncthreads();
            if ((lane & (2u * off - 1u)) == 0 && s_arg[t + off] < s_arg[t]) s_arg[t] = s_arg[t + off];
        }
        __syncthreads();
        if (go) {
            const uint32_t arg = s_arg[g0];
            if (arg != kNone) {
                const int64_t p = tail ? edge - 1 - static_cast<int64_t>(arg) : edge + static_cast<int64_t>(arg);
                res = static_cast<uint64_t>(p) + (tail ? 1 : 0);
                go = false;
            } else {
                go = advance<G>(tail, edge, vlo, vhi, cur);
            }
        }
    }
    return res;
}

// ======================================================================================
// k_trim_init: one lane per record
// ======================================================================================
__device__ inline void push(unsigned long long *list, uint64_t cap, unsigned long long item) {
    const unsigned long long at = atomicAdd(&list[0], 1ull);
    if (at < cap) list[1 + at] = item;                       // (the order of the items plays no part in what they give)
}

__global__ __launch_bounds__(kThreads) void k_trim_init(const uint64_t *ends, uint64_t n_rec, uint64_t n_out, uint64_t n_section, bool cut_front, bool cut_tail,
                                                         bool trim_n, const uint32_t *status, TrimWork work) {
    if (flagged(n_rec, status)) return;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n_out; k += stride) {
        uint64_t lo, hi;
        bounds(ends, n_rec, n_section, k, lo, hi);
        work.win[2 * k] = 0;
        work.win[2 * k + 1] = hi - lo;
        if (hi - lo <= kTrimShort) continue;
        if (cut_front) push(work.list_sum, work.list_cap, 2 * k);
        if (cut_tail) push(work.list_sum, work.list_cap, 2 * k + 1);
        if (trim_n) push(work.list_n, work.list_cap, k);
    }
}

// ======================================================================================
// k_trim_sum: G lanes per record end; the short route takes every end of a record of up to kTrimShort letters, the long
// route the ends on the list
// ======================================================================================
template <uint32_t G, uint32_t B>
__global__ __launch_bounds__(B) void k_trim_sum(const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, uint64_t n_out,
                                                 uint32_t cut_front, uint32_t cut_tail, uint32_t base, const uint32_t *status, TrimWork work) {
    constexpr bool kLong = G > kTrimShortLanes;
    constexpr uint32_t kPer = B / G;
    __shared__ int32_t s_scan[2 * B];
    __shared__ long long s_max[B];
    __shared__ uint32_t s_arg[B];
    __shared__ uint32_t s_stop[B];
    if (flagged(n_rec, status)) return;
    const uint32_t residue = low4(quality), t = threadIdx.x;
    uint64_t n_items = 2 * n_out;
    if constexpr (kLong) n_items = work.list_sum[0] < work.list_cap ? work.list_sum[0] : work.list_cap;
    for (uint64_t first = static_cast<uint64_t>(blockIdx.x) * kPer; first < n_items; first += static_cast<uint64_t>(gridDim.x) * kPer) {
        const uint64_t at = first + t / G;
        bool on = at < n_items;
        uint64_t item = 0, lo = 0, hi = 0;
        if (on) item = kLong ? work.list_sum[1 + at] : at;
        const uint64_t k = item >> 1;
        const bool tail = item & 1;
        const uint32_t cutoff = tail ? cut_tail : cut_front;
        on = on && k < n_out && cutoff;
        if (on) bounds(ends, n_rec, n_section, k, lo, hi);
        if (!kLong && hi - lo > kTrimShort) on = false;      // (it is on the list)
        const uint64_t res = walk_sum<G, B>(quality, n_section, residue, on, tail, lo, hi, static_cast<int32_t>(cutoff + base), s_scan, s_max, s_arg, s_stop);
        if (on && t % G == 0) work.win[2 * k + (tail ? 1 : 0)] = res;
    }
}

// ======================================================================================
// k_trim_window: the lowest window start of every record whose W values sum to less than W * Q
// ======================================================================================
// section[p .. p + 16) as four words; bytes at or behind `bound` read as 0 and are never touched (p < bound)
__device__ inline void load16(const uint8_t *section, uint64_t bound, bool aligned, uint64_t p, uint32_t *w) {
    if (aligned && p + 16 <= bound) {
        const uint4 v = *reinterpret_cast<const uint4 *>(section + p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (p + k < bound) w[k >> 2] |= static_cast<uint32_t>(section[p + k]) << (8u * (k & 3u));
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

// threshold: W * (Q + the quality base): a window fails when its BYTES sum to less
__global__ __launch_bounds__(kThreads) void k_trim_window(const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, uint32_t W,
                                                           uint32_t threshold, const uint32_t *status, TrimWork work) {
    __shared__ uint4 s_tile[kThreads + kHaloLanes];          // the tile's bytes and its halo's
    const uint32_t t = threadIdx.x;
    if (flagged(n_rec, status)) return;
    const uint64_t last = n_rec ? n_rec - 1 : 0;
    const uint64_t limit = n_rec && ends[last] < n_section ? ends[last] : n_section;   // bytes behind the last record belong to none
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kTrimRun;
    if (tile0 * kTrimTile >= limit) return;
    const bool aligned = low4(quality) == 0;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(s_tile) + 16u * t;

    // the record of the last candidate: [cur_begin, cur_end) is record cur_rec with the window [cur_a, cur_b); a later position
    // is searched from next_lo on
    uint64_t cur_begin = 0, cur_end = 0, cur_rec = 0, next_lo = 0, cur_a = 0, cur_b = 0;
    bool cur_done = false;                                   // this lane has given cur_rec a start: its later ones are higher
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
        cur_a = work.win[2 * rec];
        cur_b = work.win[2 * rec + 1];
        cur_done = false;
        return true;
    };

    for (uint32_t r = 0; r < kTrimRun; r++) {
        const uint64_t t0 = (tile0 + r) * kTrimTile;
        if (t0 >= limit) break;                              // (the same in every lane, as is all of the loop's control)
        const uint64_t p0 = t0 + 16ull * t;
        {
            uint32_t w[4] = {0, 0, 0, 0};
            if (p0 < n_section) load16(quality, n_section, aligned, p0, w);
            s_tile[t] = make_uint4(w[0], w[1], w[2], w[3]);
            if (t < kHaloLanes) {
                const uint64_t ph = t0 + kTrimTile + 16ull * t;
                uint32_t h[4] = {0, 0, 0, 0};
                if (ph < n_section) load16(quality, n_section, aligned, ph, h);
                s_tile[kThreads + t] = make_uint4(h[0], h[1], h[2], h[3]);
            }
        }
        __syncthreads();
        if (p0 < limit) {
            uint32_t s = 0, candidates = 0;                  // bit i: the window at p0 + i fails, whatever record holds it
            for (uint32_t j = 0; j + 1 < W; j++) s += bytes[j];
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                s += bytes[W - 1 + i];
                candidates |= (s < threshold ? 1u : 0u) << i;
                s -= bytes[i];
            }
            // only a candidate is held against its record's end and window
            for (uint32_t c = candidates; c; c &= c - 1) {
                const uint64_t at = p0 + static_cast<uint32_t>(__builtin_ctz(c));
                if (!locate(at)) break;
                if (cur_done) continue;
                const uint64_t rel = at - cur_begin;
                if (rel < cur_a || rel + W > cur_b) continue;
                const unsigned long long mine = ~static_cast<unsigned long long>(rel);
                if (work.cut[cur_rec] < mine) atomicMax(&work.cut[cur_rec], mine);   // (a stale read costs an atomic, never a start)
                cur_done = true;
            }
        }
        __syncthreads();                                     // the tile is read before the next one is written
    }
}

// ======================================================================================
// k_trim_n: G lanes per record, its front and then its tail
// ======================================================================================
template <uint32_t G, uint32_t B>
__global__ __launch_bounds__(B) void k_trim_n(const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, uint64_t n_out,
                                               const uint32_t *status, TrimWork work) {
    constexpr bool kLong = G > kTrimShortLanes;
    constexpr uint32_t kPer = B / G;
    __shared__ uint32_t s_arg[B];
    if (flagged(n_rec, status)) return;
    const uint32_t residue = low4(letters), t = threadIdx.x;
    uint64_t n_items = n_out;
    if constexpr (kLong) n_items = work.list_n[0] < work.list_cap ? work.list_n[0] : work.list_cap;
    for (uint64_t first = static_cast<uint64_t>(blockIdx.x) * kPer; first < n_items; first += static_cast<uint64_t>(gridDim.x) * kPer) {
        const uint64_t at = first + t / G;
        bool on = at < n_items;
        uint64_t k = 0, lo = 0, hi = 0, a = 0, b = 0;
        if (on) k = kLong ? work.list_n[1 + at] : at;
        on = on && k < n_out;
        if (on) bounds(ends, n_rec, n_section, k, lo, hi);
        if (!kLong && hi - lo > kTrimShort) on = false;      // (it is on the list)
        if (on) window_of(work, k, a, b);
        on = on && a < b && b <= hi - lo;
        const uint64_t from = walk_n<G>(letters, n_section, residue, on, false, lo + a, lo + b, s_arg);
        const uint64_t to = walk_n<G>(letters, n_section, residue, on && from < lo + b, true, from, lo + b, s_arg);
        if (on && t % G == 0) {
            work.win[2 * k] = from - lo;
            work.win[2 * k + 1] = to - lo;
        }
    }
}

// ======================================================================================
// k_trim_finish: one lane per record, or per pair of mates
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_trim_finish(const uint64_t *ends, uint64_t n_rec, uint64_t n_out, uint64_t n_section, uint64_t min_length,
                                                           bool interleaved, const uint32_t *status, TrimWork work, nafgpu_region *regions, uint8_t *keep,
                                                           uint64_t *flags, unsigned long long *totals) {
    __shared__ unsigned long long s_totals[kTrimTotals];
    if (flagged(n_rec, status)) return;
    const uint32_t t = threadIdx.x;
    if (t < kTrimTotals) s_totals[t] = 0;
    if (blockIdx.x == 0 && t == 0) flags[n_out] = 0;
    __syncthreads();
    const uint32_t per = interleaved ? 2 : 1;
    const uint64_t n_units = n_out / per, stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    unsigned long long changed = 0, in_windows = 0, kept = 0;
    for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kThreads + t; u < n_units; u += stride) {
        uint64_t a[2] = {0, 0}, b[2] = {0, 0};
        bool pass = true;
#pragma unroll
        for (uint32_t m = 0; m < 2; m++)
            if (m < per) {
                const uint64_t k = u * per + m;
                uint64_t lo, hi;
                bounds(ends, n_rec, n_section, k, lo, hi);
                window_of(work, k, a[m], b[m]);
                if (a[m] >= b[m]) a[m] = b[m] = 0;           // an empty window has one form
                if (a[m] != 0 || b[m] != hi - lo) changed++;
                in_windows += b[m] - a[m];
                pass = pass && b[m] - a[m] >= min_length;
            }
#pragma unroll
        for (uint32_t m = 0; m < 2; m++)
            if (m < per) {
                const uint64_t k = u * per + m;
                uint4 *out = reinterpret_cast<uint4 *>(regions + k);
                out[0] = make_uint4(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32), static_cast<uint32_t>(a[m]), static_cast<uint32_t>(a[m] >> 32));
                out[1] = make_uint4(static_cast<uint32_t>(b[m]), static_cast<uint32_t>(b[m] >> 32), 0, 0);
                keep[k] = pass ? 1 : 0;
                flags[k] = pass ? 1 : 0;
                if (pass) kept += b[m] - a[m];
            }
    }
    if (changed) atomicAdd(&s_totals[0], changed);
    if (in_windows) atomicAdd(&s_totals[1], in_windows);
    if (kept) atomicAdd(&s_totals[2], kept);
    __syncthreads();
    if (t < kTrimTotals && s_totals[t]) atomicAdd(&totals[t], s_totals[t]);
}
static_assert(sizeof(nafgpu_region) == 32, "a region is two 16-byte stores");

// ======================================================================================
// k_trim_compact: one lane per record
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_trim_compact(const nafgpu_region *regions, const uint8_t *keep, const uint64_t *where, uint64_t n_out,
                                                            uint64_t n_kept, nafgpu_region *kept) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n_out; k += stride) {
        if (!keep[k] || where[k] >= n_kept) continue;
        const uint4 *in = reinterpret_cast<const uint4 *>(regions + k);
        uint4 *out = reinterpret_cast<uint4 *>(kept + where[k]);
        out[0] = in[0];
        out[1] = in[1];
    }
}

uint32_t blocks_for(uint64_t items, uint64_t per_block, uint32_t most) {
    const uint64_t blocks = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(blocks < 1 ? 1 : (blocks > most ? most : blocks));
}

}  // namespace

void launch_trim_init(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_trim_opts &opts, const uint32_t *status,
                      const TrimWork &work) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL(k_trim_init, dim3(blocks_for(n_out, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec, n_out, n_section, opts.cut_front != 0,
                       opts.cut_tail != 0, opts.trim_n != 0, status, work);
}

void launch_trim_sum(hipStream_t stream, const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_trim_opts &opts,
                     const uint32_t *status, const TrimWork &work) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL((k_trim_sum<kTrimShortLanes, kShortThreads>), dim3(blocks_for(2 * n_out, kShortThreads / kTrimShortLanes, 65536)), dim3(kShortThreads), 0,
                       stream, quality, n_section, ends, n_rec, n_out, static_cast<uint32_t>(opts.cut_front), static_cast<uint32_t>(opts.cut_tail),
                       static_cast<uint32_t>(opts.quality_base), status, work);
    hipLaunchKernelGGL((k_trim_sum<kTrimLongLanes, kThreads>), dim3(blocks_for(work.list_cap, 1, 2048)), dim3(kThreads), 0, stream, quality, n_section, ends,
                       n_rec, n_out, static_cast<uint32_t>(opts.cut_front), static_cast<uint32_t>(opts.cut_tail), static_cast<uint32_t>(opts.quality_base), status,
                       work);
}

void launch_trim_window(hipStream_t stream, const uint8_t *quality, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_trim_opts &opts,
                        const uint32_t *status, const TrimWork &work) {
    if (!n_section) return;
    constexpr uint64_t run = static_cast<uint64_t>(kTrimRun) * kTrimTile;
    const uint32_t W = opts.window;
    hipLaunchKernelGGL(k_trim_window, dim3(static_cast<uint32_t>((n_section + run - 1) / run)), dim3(kThreads), 0, stream, quality, n_section, ends, n_rec, W,
                       W * (static_cast<uint32_t>(opts.window_quality) + opts.quality_base), status, work);
}

void launch_trim_n(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const uint32_t *status,
                   const TrimWork &work) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL((k_trim_n<kTrimShortLanes, kShortThreads>), dim3(blocks_for(n_out, kShortThreads / kTrimShortLanes, 65536)), dim3(kShortThreads), 0, stream,
                       letters, n_section, ends, n_rec, n_out, status, work);
    hipLaunchKernelGGL((k_trim_n<kTrimLongLanes, kThreads>), dim3(blocks_for(work.list_cap, 1, 2048)), dim3(kThreads), 0, stream, letters, n_section, ends, n_rec,
                       n_out, status, work);
}

void launch_trim_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, uint64_t n_section, const nafgpu_trim_opts &opts, const uint32_t *status,
                        const TrimWork &work, nafgpu_region *regions, uint8_t *keep, uint64_t *flags, unsigned long long *totals) {
    const uint64_t n_out = n_rec ? n_rec : 1;
    hipLaunchKernelGGL(k_trim_finish, dim3(blocks_for(n_out, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec, n_out, n_section, opts.min_length,
                       opts.interleaved != 0, status, work, regions, keep, flags, totals);
}

void launch_trim_compact(hipStream_t stream, const nafgpu_region *regions, const uint8_t *keep, const uint64_t *where, uint64_t n_out, uint64_t n_kept,
                         nafgpu_region *kept) {
    hipLaunchKernelGGL(k_trim_compact, dim3(blocks_for(n_out, kThreads, 8192)), dim3(kThreads), 0, stream, regions, keep, where, n_out, n_kept, kept);
}

}  // namespace trm
}  // namespace nafgpu
