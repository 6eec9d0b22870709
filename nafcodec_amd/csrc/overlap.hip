// overlap.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_overlap and nafgpu_merge_pairs: for every pair of mates the shift at
// which read 1 and the reverse complement of read 2 agree best, the adapter cut as regions, and the pairs joined into records.
// The rules: include/nafgpu.h at nafgpu_overlap; the passes: overlap.h.
//
// k_ovl_pairs gives a pair to a wave.  The letters of both mates come in once, a lane one letter per 64 (read 2 through the
// reversed index, complemented), and a wave64 ballot turns 64 letters into one word of each of three bit planes: bit 0 and
// bit 1 of the code and is-a-letter.  That is at most kOvlWords words a plane and read, kept in LDS.  Then a lane is a SHIFT:
// it reads y's planes moved by d (two words and a funnel shift per plane and word), forms valid = vx & vy and
// diff = (x0 ^ y0) | (x1 ^ y1) and counts valid & ~diff and valid & diff over the words the two reads share, 64 shifts a
// round and at most 32 rounds.  A lane keeps the best key of its shifts (fewest mismatches, most matches, lowest d: one 64-bit
// word, so the best is a maximum of complements); the wave's best is one LDS atomic per lane that has an accepted shift.
// The waves of a workgroup share nothing and never wait for each other.  Positions outside a read are no letters in its valid
// plane, so no count needs a mask of its own; y's planes have a zero word on either side, which is all a funnel shift can
// reach (see the bounds at the loop).
// Integer work only; every loop is bounded by the cap (kOvlMaxLength); no kernel reads a record end it has not checked
// (k_sum_check has run; a flagged table ends every kernel at once), and every letter address lies inside a checked record.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu), one wave per workgroup there.
#include <hip/hip_runtime.h>

#include "overlap.h"
#include "summary.h"

namespace nafgpu {
namespace ovl {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPairThreads = 64 * kOvlWaves;
constexpr uint32_t kNoLetter = 4;
static_assert(kOvlTile == kThreads * 16, "a lane takes 16 output positions");

__device__ inline bool flagged(const uint32_t *status) { return (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) != 0; }

__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the project's 4-bit rule cut to the four letters, as in screen.hip: case and T/U play no part, every other byte is no letter
__device__ inline uint32_t code_of(uint32_t byte) {
    const uint32_t c = byte & 0xDFu;
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : (c == 'T' || c == 'U') ? 3u : kNoLetter;
}

__device__ inline void flag_first(uint32_t *status, uint32_t bit, uint32_t slot, uint64_t at) {
    atomicOr(&status[0], bit);
    atomicMax(reinterpret_cast<unsigned long long *>(status + slot), ~static_cast<unsigned long long>(at));   // the lowest: the largest complement
}

__device__ inline void store_region(nafgpu_region *at, uint64_t k, uint64_t a, uint64_t b) {
    uint4 *out = reinterpret_cast<uint4 *>(at);
    out[0] = make_uint4(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32), static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32));
    out[1] = make_uint4(static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32), 0, 0);
}
static_assert(sizeof(nafgpu_region) == 32, "a region is two 16-byte stores");

__device__ inline void store_pair(nafgpu_pair_overlap *at, int64_t shift, uint64_t insert, uint32_t matches, uint32_t mismatches, uint32_t compared,
                                  uint32_t found, uint32_t too_long) {
    uint4 *out = reinterpret_cast<uint4 *>(at);
    const uint64_t s = static_cast<uint64_t>(shift);
    out[0] = make_uint4(static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32), static_cast<uint32_t>(insert), static_cast<uint32_t>(insert >> 32));
    out[1] = make_uint4(matches, mismatches, compared, found | (too_long << 8));
}
static_assert(sizeof(nafgpu_pair_overlap) == 32, "a pair is two 16-byte stores");

// bits [sh, sh + 64) of the 128-bit word {hi, lo}
__device__ inline uint64_t funnel(uint64_t lo, uint64_t hi, uint32_t sh) { return sh ? (lo >> sh) | (hi << (64u - sh)) : lo; }

// what a wave keeps of its pair: plane 0, 1: the code's bits, plane 2: is-a-letter.  y[.][1 + i] is word i of y; y[.][0] and
// the word behind y's last are zero.
struct Planes {
    uint64_t x[3][kOvlWords];
    uint64_t y[3][kOvlWords + 2];
    unsigned long long best;
};

// ======================================================================================
// k_ovl_pairs: one wave per pair
// ======================================================================================
__global__ __launch_bounds__(kPairThreads) void k_ovl_pairs(const uint8_t *letters, const uint64_t *ends, uint64_t n_pairs, uint32_t min_matches,
                                                             uint32_t max_mismatches, uint32_t max_percent, const uint32_t *status,
                                                             nafgpu_pair_overlap *pairs) {
    __shared__ Planes s_planes[kOvlWaves];
    if (flagged(status)) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Planes &p = s_planes[wave];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kOvlWaves;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kOvlWaves + wave; j < n_pairs; j += stride) {
        // (everything that steers the loops below is the same in all lanes of the wave)
        const uint64_t r0 = j ? ends[2 * j - 1] : 0, r1 = ends[2 * j], r2 = ends[2 * j + 1];
        const uint64_t l1 = r1 - r0, l2 = r2 - r1;
        if (l1 > kOvlMaxLength || l2 > kOvlMaxLength || !l1 || !l2) {
            if (lane == 0) store_pair(pairs + j, 0, 0, 0, 0, 0, 0, l1 > kOvlMaxLength || l2 > kOvlMaxLength ? 1u : 0u);
            continue;
        }
        const uint32_t n1 = static_cast<uint32_t>(l1), n2 = static_cast<uint32_t>(l2);
        // ---- the planes
        const uint32_t cx = (n1 + 63u) >> 6, cy = (n2 + 63u) >> 6;          // 1 .. kOvlWords
        for (uint32_t c = 0; c < cx; c++) {
            const uint32_t i = 64u * c + lane;
            const uint32_t code = i < n1 ? code_of(letters[r0 + i]) : kNoLetter;
            const unsigned long long b0 = __ballot(code < kNoLetter && (code & 1u)), b1 = __ballot(code < kNoLetter && (code & 2u)),
                                     v = __ballot(code < kNoLetter);
            if (lane == 0) {
                p.x[0][c] = b0;
                p.x[1][c] = b1;
                p.x[2][c] = v;
            }
        }
        for (uint32_t c = 0; c < cy; c++) {
            const uint32_t i = 64u * c + lane;
            uint32_t code = i < n2 ? code_of(letters[r1 + (n2 - 1u - i)]) : kNoLetter;
            if (code < kNoLetter) code = 3u - code;
            const unsigned long long b0 = __ballot(code < kNoLetter && (code & 1u)), b1 = __ballot(code < kNoLetter && (code & 2u)),
                                     v = __ballot(code < kNoLetter);
            if (lane == 0) {
                p.y[0][1 + c] = b0;
                p.y[1][1 + c] = b1;
                p.y[2][1 + c] = v;
            }
        }
        if (lane < 3) {
            p.y[lane][0] = 0;
            p.y[lane][1 + cy] = 0;
        }
        if (lane == 0) p.best = 0;
        wave_sync();

        // ---- lane = shift: shift index s = d + n2 - 1 in 0 .. n1 + n2 - 2
        const uint32_t n_shifts = n1 + n2 - 1u;
        unsigned long long best = 0;                         // the complement of the best key; 0: no accepted shift
        for (uint32_t s0 = 0; s0 < n_shifts; s0 += 64) {     // at most 32 rounds
            const uint32_t s = s0 + lane;
            if (s >= n_shifts) continue;
            const int32_t d = static_cast<int32_t>(s) - static_cast<int32_t>(n2 - 1u);
            const uint32_t lo = d > 0 ? static_cast<uint32_t>(d) : 0u;
            const uint32_t top = static_cast<uint32_t>(d + static_cast<int32_t>(n2));   // (d + n2 >= 1)
            const uint32_t hi = top < n1 ? top : n1;                                     // lo < hi
            uint32_t m = 0, mm = 0;
            // Word w of x lies over bits [64 w - d, 64 w - d + 64) of y.  At the first word 64 w - d is in -63 .. n2 - 1 and at
            // the last one at most n2 - 1, so with q = 64 w - d + kOvlMaxLength the words read are y[-1 .. cy]: inside p.y.
            for (uint32_t w = lo >> 6; w <= (hi - 1u) >> 6; w++) {           // at most kOvlWords
                const uint32_t q = static_cast<uint32_t>(static_cast<int32_t>(64u * w) - d + static_cast<int32_t>(kOvlMaxLength));
                const uint32_t at = (q >> 6) - (kOvlWords - 1u), sh = q & 63u;       // at = 1 + floor((64 w - d) / 64)
                const uint64_t y0 = funnel(p.y[0][at], p.y[0][at + 1], sh), y1 = funnel(p.y[1][at], p.y[1][at + 1], sh),
                               vy = funnel(p.y[2][at], p.y[2][at + 1], sh);
                const uint64_t valid = p.x[2][w] & vy, diff = (p.x[0][w] ^ y0) | (p.x[1][w] ^ y1);
                m += static_cast<uint32_t>(__popcll(valid & ~diff));
                mm += static_cast<uint32_t>(__popcll(valid & diff));
            }
            if (m >= min_matches && mm <= max_mismatches && mm * 100u <= max_percent * (m + mm)) {
                const unsigned long long key = (static_cast<unsigned long long>(mm) << 32) | (static_cast<unsigned long long>(kOvlMaxLength - m) << 16) | s;
                if (~key > best) best = ~key;
            }
        }
        if (best) atomicMax(&p.best, best);
        wave_sync();
        if (lane == 0) {
            const unsigned long long won = p.best;
            if (!won) {
                store_pair(pairs + j, 0, 0, 0, 0, 0, 0, 0);
            } else {
                const unsigned long long key = ~won;
                const uint32_t s = static_cast<uint32_t>(key & 0xFFFFu), m = kOvlMaxLength - static_cast<uint32_t>((key >> 16) & 0xFFFFu);
                const int32_t d = static_cast<int32_t>(s) - static_cast<int32_t>(n2 - 1u);
                const uint32_t lo = d > 0 ? static_cast<uint32_t>(d) : 0u, top = s + 1u, hi = top < n1 ? top : n1;
                store_pair(pairs + j, d, top, m, static_cast<uint32_t>(key >> 32), hi - lo, 1, 0);
            }
        }
        wave_sync();                                         // the planes and the best are read before the next pair writes them
    }
}

// ======================================================================================
// k_ovl_finish: one lane per pair
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_ovl_finish(const uint64_t *ends, uint64_t n_pairs, const uint32_t *status, const nafgpu_pair_overlap *pairs,
                                                          nafgpu_region *regions, uint64_t *flags, unsigned long long *totals) {
    __shared__ unsigned long long s_totals[kOvlTotals];
    if (flagged(status)) return;
    const uint32_t t = threadIdx.x;
    if (t < kOvlTotals) s_totals[t] = 0;
    if (blockIdx.x == 0 && t == 0) flags[2 * n_pairs] = 0;
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    unsigned long long sums[kOvlTotals] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + t; j < n_pairs; j += stride) {
        const uint64_t r0 = j ? ends[2 * j - 1] : 0, r1 = ends[2 * j], r2 = ends[2 * j + 1];
        const nafgpu_pair_overlap pr = pairs[j];
        const uint64_t len[2] = {r1 - r0, r2 - r1};
#pragma unroll
        for (uint32_t m = 0; m < 2; m++) {
            const uint64_t b = pr.found && pr.insert < len[m] ? pr.insert : len[m];
            store_region(regions + 2 * j + m, 2 * j + m, 0, b);
            flags[2 * j + m] = pr.found ? 0 : 1;
            sums[2] += b < len[m] ? 1 : 0;
            sums[6] += b;
        }
        sums[1] += pr.too_long ? 1 : 0;
        if (pr.found) {
            sums[0]++;
            sums[3] += pr.matches;
            sums[4] += pr.mismatches;
            sums[5] += pr.insert;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kOvlTotals; i++)
        if (sums[i]) atomicAdd(&s_totals[i], sums[i]);
    __syncthreads();
    if (t < kOvlTotals && s_totals[t]) atomicAdd(&totals[t], s_totals[t]);
}

// ======================================================================================
// k_ovl_compact: one lane per record
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_ovl_compact(const uint64_t *ends, uint64_t n_rec, const nafgpu_pair_overlap *pairs, const uint64_t *where,
                                                           uint64_t n_unmerged, nafgpu_region *unmerged) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        if (pairs[r >> 1].found || where[r] >= n_unmerged) continue;
        store_region(unmerged + where[r], r, 0, ends[r] - (r ? ends[r - 1] : 0));
    }
}

// ======================================================================================
// nafgpu_merge_pairs: k_ovl_found, k_ovl_merge_sizes (one lane per pair), k_ovl_merge
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_ovl_found(const nafgpu_pair_overlap *pairs, uint64_t n_pairs, uint64_t *flags) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j <= n_pairs; j += stride) flags[j] = j < n_pairs && pairs[j].found ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_ovl_merge_sizes(const nafgpu_pair_overlap *pairs, uint64_t n_pairs, const uint64_t *where, uint64_t n_out,
                                                               OvlSource s, uint64_t *len, uint64_t *id_size, uint64_t *com_size, uint64_t *pair_of,
                                                               nafgpu_region *regions, uint32_t *status) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j <= n_pairs; j += stride) {
        if (j == n_pairs) {                                  // the scans' last item: its exclusive sum is the last end
            len[n_out] = 0;
            if (id_size) id_size[n_out] = 0;
            if (com_size) com_size[n_out] = 0;
            continue;
        }
        const nafgpu_pair_overlap pr = pairs[j];
        if (!pr.found) continue;
        const uint64_t k = where[j], rec = 2 * j;
        // the pair against THESE records: overlaps of other records with as many of them are refused, never followed
        bool ok = k < n_out && rec + 1 < s.n_rec;
        uint64_t r0 = 0, r1 = 0, r2 = 0;
        if (ok) {
            r0 = rec ? s.rec_end[rec - 1] : 0;
            r1 = s.rec_end[rec];
            r2 = s.rec_end[rec + 1];
            ok = r0 < r1 && r1 < r2 && r1 - r0 <= kOvlMaxLength && r2 - r1 <= kOvlMaxLength;
        }
        if (ok) {
            const int64_t n1 = static_cast<int64_t>(r1 - r0), n2 = static_cast<int64_t>(r2 - r1);
            ok = pr.shift > -n2 && pr.shift < n1 && pr.insert == static_cast<uint64_t>(pr.shift + n2);
        }
        if (!ok) {
            flag_first(status, kOvlStRefused, 2, j);
            if (k >= n_out) continue;
        } else if (r2 > s.n_seq || (s.qual && r2 > s.n_qual)) {
            flag_first(status, kOvlStBeyond, 4, j);
        }
        uint64_t ids = 1, com = 1;
        if (ok && s.ids && rec < s.n_ids) ids += s.id_end[rec] - (rec ? s.id_end[rec - 1] : 0) - 1;
        if (ok && s.com && rec < s.n_com) com += s.com_end[rec] - (rec ? s.com_end[rec - 1] : 0) - 1;
        len[k] = ok ? pr.insert : 0;
        pair_of[k] = j;
        if (id_size) id_size[k] = ids;
        if (com_size) com_size[k] = com;
        store_region(regions + k, rec, 0, r1 - r0);
    }
}

// the first k in [lo, hi] with excl[k + 1] > at (hi: when there is none below it); records of length 0 are never found
__device__ inline uint64_t record_of(const uint64_t *excl, uint64_t lo, uint64_t hi, uint64_t at) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (excl[mid + 1] > at) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// a found pair as the merge reads it (k_ovl_merge_sizes has checked it against the records)
struct Mate {
    uint64_t r0, r1;             // where R1 and R2 begin
    int64_t d, n1, n2;
};
__device__ inline Mate mate_of(const nafgpu_pair_overlap *pairs, const uint64_t *rec_end, uint64_t j) {
    Mate m;
    m.r0 = j ? rec_end[2 * j - 1] : 0;
    m.r1 = rec_end[2 * j];
    m.n1 = static_cast<int64_t>(m.r1 - m.r0);
    m.n2 = static_cast<int64_t>(rec_end[2 * j + 1] - m.r1);
    m.d = pairs[j].shift;
    return m;
}

template <bool QUAL>
__global__ __launch_bounds__(kThreads) void k_ovl_merge(const nafgpu_pair_overlap *pairs, const uint64_t *pair_of, const uint64_t *excl, uint64_t n_out,
                                                         uint64_t n_bytes, OvlSource s, const uint8_t *table, uint32_t quality_base, uint8_t *dst_seq,
                                                         uint8_t *dst_qual) {
    __shared__ uint64_t s_bound[2];
    __shared__ uint8_t s_tab[256];
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kOvlTile;
    if (tile0 >= n_bytes) return;
    s_tab[t] = table[t];
    // the records of the tile's first and last position, searched by two waves side by side
    if (t == 0) s_bound[0] = record_of(excl, 0, n_out - 1, tile0);
    if (t == 64) s_bound[1] = record_of(excl, 0, n_out - 1, (tile0 + kOvlTile <= n_bytes ? tile0 + kOvlTile : n_bytes) - 1);
    __syncthreads();
    const uint64_t o0 = tile0 + 16ull * t;
    if (o0 >= n_bytes) return;
    uint64_t k = record_of(excl, s_bound[0], s_bound[1], o0);
    uint64_t k0 = excl[k], k1 = excl[k + 1];                 // output positions [k0, k1) are record k's
    Mate m = mate_of(pairs, s.rec_end, pair_of[k]);
    uint32_t w[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint64_t o = o0 + i;
        if (o >= n_bytes) break;
        while (o >= k1) {                                    // (o < n_bytes = the last end: there is such a record)
            k++;
            k0 = k1;
            k1 = excl[k + 1];
            if (o < k1) m = mate_of(pairs, s.rec_end, pair_of[k]);
        }
        const int64_t pos = static_cast<int64_t>(o - k0);    // 0 .. insert - 1
        const bool in1 = pos < m.n1, in2 = pos >= m.d;       // (one of them holds: insert = d + n2)
        uint32_t a = 0, b = 0, qa = 0, qb = 0;
        if (in1) {
            a = s.seq[m.r0 + static_cast<uint64_t>(pos)];
            if (QUAL) qa = s.qual[m.r0 + static_cast<uint64_t>(pos)];
        }
        if (in2) {
            const uint64_t at = m.r1 + static_cast<uint64_t>(m.n2 - 1 - (pos - m.d));
            b = s_tab[s.seq[at]];
            if (QUAL) qb = s.qual[at];
        }
        uint32_t c = in1 ? a : b, q = in1 ? qa : qb;
        if (in1 && in2) {
            if (QUAL && qb > qa) c = b;
            const uint32_t ca = code_of(a), cb = code_of(b);
            if (ca < kNoLetter && ca == cb) {
                q = qa > qb ? qa : qb;
            } else {
                const uint32_t gap = qa > qb ? qa - qb : qb - qa;
                q = quality_base + (gap > 2u ? gap : 2u);
                if (q > 255u) q = 255u;
            }
        }
        w[i >> 2] |= c << (8u * (i & 3u));
        if (QUAL) v[i >> 2] |= q << (8u * (i & 3u));
    }
    *reinterpret_cast<uint4 *>(dst_seq + o0) = make_uint4(w[0], w[1], w[2], w[3]);
    if (QUAL) *reinterpret_cast<uint4 *>(dst_qual + o0) = make_uint4(v[0], v[1], v[2], v[3]);
}

uint32_t blocks_for(uint64_t items, uint64_t per_block, uint32_t most) {
    const uint64_t blocks = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(blocks < 1 ? 1 : (blocks > most ? most : blocks));
}

}  // namespace

void launch_ovl_pairs(hipStream_t stream, const uint8_t *letters, uint64_t n_section, const uint64_t *ends, uint64_t n_rec, const nafgpu_overlap_opts &opts,
                      const uint32_t *status, nafgpu_pair_overlap *pairs) {
    const uint64_t n_pairs = n_rec / 2;
    if (!n_pairs) return;
    hipLaunchKernelGGL(k_ovl_pairs, dim3(blocks_for(n_pairs, kOvlWaves, 1u << 16)), dim3(kPairThreads), 0, stream, letters, ends, n_pairs,
                       opts.min_overlap > 1 ? opts.min_overlap : 1u, opts.max_mismatches, static_cast<uint32_t>(opts.max_mismatch_percent), status, pairs);
}

void launch_ovl_finish(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, const uint32_t *status, const nafgpu_pair_overlap *pairs, nafgpu_region *regions,
                       uint64_t *flags, unsigned long long *totals) {
    hipLaunchKernelGGL(k_ovl_finish, dim3(blocks_for(n_rec / 2, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec / 2, status, pairs, regions, flags,
                       totals);
}

void launch_ovl_compact(hipStream_t stream, const uint64_t *ends, uint64_t n_rec, const nafgpu_pair_overlap *pairs, const uint64_t *where, uint64_t n_unmerged,
                        nafgpu_region *unmerged) {
    if (!n_unmerged) return;
    hipLaunchKernelGGL(k_ovl_compact, dim3(blocks_for(n_rec, kThreads, 8192)), dim3(kThreads), 0, stream, ends, n_rec, pairs, where, n_unmerged, unmerged);
}

void launch_ovl_found(hipStream_t stream, const nafgpu_pair_overlap *pairs, uint64_t n_pairs, uint64_t *flags) {
    hipLaunchKernelGGL(k_ovl_found, dim3(blocks_for(n_pairs + 1, kThreads, 8192)), dim3(kThreads), 0, stream, pairs, n_pairs, flags);
}

void launch_ovl_merge_sizes(hipStream_t stream, const nafgpu_pair_overlap *pairs, uint64_t n_pairs, const uint64_t *where, uint64_t n_out, const OvlSource &s,
                            uint64_t *len, uint64_t *id_size, uint64_t *com_size, uint64_t *pair_of, nafgpu_region *regions, uint32_t *status) {
    hipLaunchKernelGGL(k_ovl_merge_sizes, dim3(blocks_for(n_pairs + 1, kThreads, 8192)), dim3(kThreads), 0, stream, pairs, n_pairs, where, n_out, s, len, id_size,
                       com_size, pair_of, regions, status);
}

void launch_ovl_merge(hipStream_t stream, const nafgpu_pair_overlap *pairs, const uint64_t *pair_of, const uint64_t *excl, uint64_t n_out, uint64_t n_bytes,
                      const OvlSource &s, const uint8_t *table, uint8_t quality_base, uint8_t *dst_seq, uint8_t *dst_qual) {
    if (!n_bytes || !n_out) return;
    const dim3 grid(static_cast<uint32_t>((n_bytes + kOvlTile - 1) / kOvlTile)), block(kThreads);
    if (s.qual && dst_qual)
        hipLaunchKernelGGL((k_ovl_merge<true>), grid, block, 0, stream, pairs, pair_of, excl, n_out, n_bytes, s, table, static_cast<uint32_t>(quality_base), dst_seq,
                           dst_qual);
    else
        hipLaunchKernelGGL((k_ovl_merge<false>), grid, block, 0, stream, pairs, pair_of, excl, n_out, n_bytes, s, table, static_cast<uint32_t>(quality_base),
                           dst_seq, dst_qual);
}

}  // namespace ovl
}  // namespace nafgpu
