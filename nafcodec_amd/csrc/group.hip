// group.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_group: records in HBM -> for every record the lowest record with an
// equal sequence, and the groups those form.  The rules: include/nafgpu.h at nafgpu_group; the passes: group.h.
//
// The hash pass is driven by the INPUT like k_sum_tiles: a workgroup takes a run of kGrpRun consecutive tiles of kGrpTile
// bytes, a lane 16 of them with one aligned 16-byte load, so every letter is read from HBM once.  The tile goes to LDS as
// canonical bytes (group.h) with the 16 behind it.  A record's hash is the sum, over its 8-letter words counted from the
// record's START, of hash_word(word, its number) (hash64.h: a bijection keyed by the position, the sum commutative), the
// last word padded with zeros: equal records hash alike at any alignment, and a word belongs to the tile it starts in (it
// reaches at most 7 letters into the next one).  With both strands a second hash is that of the record's reverse
// complement: words counted from the record's END, every word complemented and its bytes reversed.  Two routes per tile:
//   long    the tile is cut into pieces at the record ends; lane l takes words l, l + 256, ... of a piece into registers, which
//           are reduced through LDS and added to the record's hashes (one atomic each) only when the record changes or the
//           run ends: a 250-Mbase record costs one such round per 64 KiB.
//   short   kGrpSub lanes share a record (32 records per round of the workgroup); a record that lies inside the tile is
//           written with plain stores, the two that reach over the tile's edges are added with atomics.
// The table keeps, per key (length, hash or the unordered pair of hashes), the lowest record index as its complement under
// atomicMax; the comparison there is of lengths and hashes only.  The verify pass is driven by the input again: a lane holds
// its 16 letters against the same offsets of the candidate (two aligned loads and a shift), forwards when the forward hashes
// agree and backwards, complemented, when the record's forward hash is the candidate's reverse one; equal hashes alone settle
// nothing.  Integer work only: sums, maxima and or-ed bits, so the result does not depend on the schedule.
// No kernel reads a record end it has not checked (k_sum_check has run; a flagged table ends every kernel that reads letters
// at once), every letter address comes from a position below the section's size, and a table slot holds only record indices
// below n_rec (anything else is passed over).
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "group.h"
#include "hash64.h"
#include "summary.h"

namespace nafgpu {
namespace grp {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kGrpTile == kThreads * 16, "a lane takes 16 input bytes");
static_assert(kGrpHalo % 16 == 0 && kGrpHalo >= 8 && kGrpHalo / 16 <= kThreads, "a word that starts in a tile ends in its halo");
static_assert(kThreads % kGrpSub == 0 && kGrpSub <= 8, "the short route: whole groups of lanes");

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

// the low n bytes of a 64-bit word
__device__ inline uint64_t low_bytes(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8u * n)) - 1ull; }

// of the word that holds bytes [base, base + 8) of a lane's 16: those in [lo, hi), lo <= hi
__device__ inline uint64_t byte_range(uint32_t lo, uint32_t hi, uint32_t base) {
    return low_bytes(hi > base ? hi - base : 0u) & ~low_bytes(lo > base ? lo - base : 0u);
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

__device__ inline uint32_t map4(const uint8_t *tab, uint32_t w) {
    return static_cast<uint32_t>(tab[w & 0xFFu]) | (static_cast<uint32_t>(tab[(w >> 8) & 0xFFu]) << 8) |
           (static_cast<uint32_t>(tab[(w >> 16) & 0xFFu]) << 16) | (static_cast<uint32_t>(tab[w >> 24]) << 24);
}

__device__ inline uint64_t map8(const uint8_t *tab, uint64_t x) {
    return static_cast<uint64_t>(map4(tab, static_cast<uint32_t>(x))) | (static_cast<uint64_t>(map4(tab, static_cast<uint32_t>(x >> 32))) << 32);
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

uint32_t blocks_for(uint64_t n) {
    uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    return static_cast<uint32_t>(blocks ? blocks : 1);
}

// ======================================================================================
// k_grp_hash
// ======================================================================================
template <bool BOTH>
__global__ __launch_bounds__(kThreads) void k_grp_hash(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                                                        const GroupTables *tables, unsigned long long *hf_out, unsigned long long *hr_out,
                                                        const uint32_t *status) {
    __shared__ uint8_t s_canon[256];
    __shared__ uint8_t s_comp[256];
    __shared__ uint32_t s_words[(kGrpTile + kGrpHalo) / 4];  // the tile's canonical bytes and its halo's
    __shared__ unsigned long long s_red[2 * kThreads];
    __shared__ unsigned long long s_part[16];
    const uint32_t t = threadIdx.x;
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) return;      // the table is refused: none of it is used
    const uint64_t last = n_rec - 1;
    const uint64_t limit = ends[last] < n_section ? ends[last] : n_section;   // letters behind the last record belong to none
    const uint64_t run0 = static_cast<uint64_t>(blockIdx.x) * kGrpRun * kGrpTile;
    if (run0 >= limit) return;
    const uint64_t run1 = run0 + static_cast<uint64_t>(kGrpRun) * kGrpTile < limit ? run0 + static_cast<uint64_t>(kGrpRun) * kGrpTile : limit;
    s_canon[t] = tables->canon[t];
    s_comp[t] = tables->comp[t];
    __syncthreads();
    const bool aligned = low4(section) == 0;

    uint64_t t0 = run0;
    // the eight canonical bytes at tile offset o (o < kGrpTile: the word starts in the tile)
    auto read8 = [&](uint32_t o) -> uint64_t {
        const uint32_t i = o >> 2, sh = 8u * (o & 3u);
        const uint64_t lo = static_cast<uint64_t>(s_words[i]) | (static_cast<uint64_t>(s_words[i + 1]) << 32);
        return sh ? (lo >> sh) | (static_cast<uint64_t>(s_words[i + 2]) << (64u - sh)) : lo;
    };
    // record [b, e) has the letters [pos, pe) in this tile (pos = max(b, t0) < pe = min(e, end of the tile)): of the words that
    // START there, this lane takes number li, li + ls, ... into f (and the reverse complement's into r)
    auto piece = [&](uint64_t b, uint64_t e, uint64_t pos, uint64_t pe, uint32_t li, uint32_t ls, uint64_t &f, uint64_t &r) {
        for (uint64_t j = ((pos - b + 7) >> 3) + li; j < ((pe - b + 7) >> 3); j += ls) {
            const uint64_t s = b + 8 * j;
            const uint32_t n = e - s < 8 ? static_cast<uint32_t>(e - s) : 8u;
            f += hash_word(read8(static_cast<uint32_t>(s - t0)) & low_bytes(n), j);
        }
        if constexpr (BOTH) {
            // word j of the reverse complement is the letters [e - 8 j - 8, e - 8 j), those below b missing: it belongs to the
            // tile that holds its lowest letter
            const uint64_t j1 = pos == b ? (e - b + 7) >> 3 : (e - pos) >> 3;
            for (uint64_t j = ((e - pe) >> 3) + li; j < j1; j += ls) {
                const uint64_t top = e - 8 * j;
                const uint32_t n = top - b < 8 ? static_cast<uint32_t>(top - b) : 8u;
                const uint64_t w = (read8(static_cast<uint32_t>(top - n - t0)) & low_bytes(n)) << (8u * (8u - n));
                r += hash_word(__builtin_bswap64(map8(s_comp, w)), j);      // (comp[0] = 0: the padding stays)
            }
        }
    };

    uint64_t hf = 0, hr = 0;                                 // the long route: this lane's share of record `cur`, not yet added
    bool pending = false;
    uint64_t cur = 0;
    // everything below but the hashes and the lane's letters is the same in every lane of the workgroup
    auto flush = [&]() {
        s_red[t] = hf;
        s_red[kThreads + t] = hr;
        hf = hr = 0;
        __syncthreads();
        if (t < 16) {                                        // eight partial sums per hash
            const uint32_t c = t >> 3, part = t & 7u;
            unsigned long long v = 0;
            for (uint32_t i = 0; i < kThreads / 8; i++) v += s_red[c * kThreads + part + 8 * i];
            s_part[t] = v;
        }
        __syncthreads();
        if (t < (BOTH ? 2u : 1u)) {
            unsigned long long v = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) v += s_part[t * 8 + i];
            if (v) atomicAdd(t ? &hr_out[cur] : &hf_out[cur], v);
        }
        pending = false;
    };

    uint64_t k = record_from(ends, 0, last, run0);           // the record of the tile's first byte
    for (; t0 < run1; t0 += kGrpTile) {
        const uint64_t t1 = t0 + kGrpTile < run1 ? t0 + kGrpTile : run1;
        {
            const uint64_t p0 = t0 + 16ull * t;
            uint32_t w[4] = {0, 0, 0, 0};
            if (p0 < limit) load16(section, limit, aligned, p0, w);
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) s_words[4 * t + i] = map4(s_canon, w[i]);   // (bytes behind `limit`: no word keeps them)
            if (t < kGrpHalo / 16) {
                const uint64_t ph = t0 + kGrpTile + 16ull * t;
                uint32_t h[4] = {0, 0, 0, 0};
                if (ph < limit) load16(section, limit, aligned, ph, h);
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) s_words[kGrpTile / 4 + 4 * t + i] = map4(s_canon, h[i]);
            }
        }
        __syncthreads();
        const uint64_t kl = ends[k] >= t1 ? k : record_from(ends, k + 1, last, t1 - 1);   // the record of the tile's last byte
        if (kl - k < kGrpFewPieces) {
            for (uint64_t pos = t0; pos < t1;) {             // k: the record of `pos`
                const uint64_t e = ends[k], pe = e < t1 ? e : t1;
                if (pending && k != cur) flush();
                cur = k;
                pending = true;
                piece(k ? ends[k - 1] : 0, e, pos, pe, t, kThreads, hf, hr);
                pos = pe;
                if (pos < t1) k = record_from(ends, k + 1, last, pos);
            }
            __syncthreads();                                 // the tile is read before the next one is written
        } else {
            for (uint64_t first = k; first <= kl; first += kThreads / kGrpSub) {
                const uint64_t j = first + t / kGrpSub;
                uint64_t f = 0, r = 0, r0 = 0, r1 = 0;
                bool any = false;
                if (j <= kl) {
                    r0 = j ? ends[j - 1] : 0;
                    r1 = ends[j];
                    const uint64_t a = r0 > t0 ? r0 : t0, b = r1 < t1 ? r1 : t1;
                    if (a < b) {                             // (an empty record: its hashes stay zero)
                        any = true;
                        piece(r0, r1, a, b, t % kGrpSub, kGrpSub, f, r);
                    }
                }
                s_red[t] = f;
                s_red[kThreads + t] = r;
                __syncthreads();
                if (any && t % kGrpSub == 0) {
                    f = r = 0;
#pragma unroll
                    for (uint32_t i = 0; i < kGrpSub; i++) {
                        f += s_red[t + i];
                        r += s_red[kThreads + t + i];
                    }
                    if (r0 >= t0 && r1 <= t1) {              // the whole record lies in this tile: nobody else writes its hashes
                        hf_out[j] = f;
                        if constexpr (BOTH) hr_out[j] = r;
                    } else {                                 // it reaches over an edge of the tile (two records per tile at the most)
                        if (f) atomicAdd(&hf_out[j], static_cast<unsigned long long>(f));
                        if constexpr (BOTH)
                            if (r) atomicAdd(&hr_out[j], static_cast<unsigned long long>(r));
                    }
                }
                __syncthreads();                             // the sums and the tile are read before they are written again
            }
            k = kl;
        }
        if (t1 < run1 && ends[k] <= t1) k = record_from(ends, k + 1, last, t1);
    }
    if (pending) flush();
}

__global__ __launch_bounds__(kThreads) void k_grp_cut(unsigned long long *hf, unsigned long long *hr, uint64_t n_rec, uint64_t mask) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        hf[r] &= mask;
        if (hr) hr[r] &= mask;
    }
}

// ======================================================================================
// k_grp_table / k_grp_probe
// ======================================================================================
// A slot holds the COMPLEMENT of a record index (0: empty), so that atomicMax keeps the lowest index among equal keys.
struct Key {
    uint64_t len, a, b;                                      // one strand: b = 0; both: a <= b, the unordered pair
};

__device__ inline Key key_of(const uint64_t *ends, const unsigned long long *hf, const unsigned long long *hr, uint64_t r) {
    Key k;
    k.len = ends[r] - (r ? ends[r - 1] : 0);
    k.a = hf[r];
    k.b = hr ? hr[r] : 0;
    if (k.b < k.a && hr) {
        const uint64_t x = k.a;
        k.a = k.b;
        k.b = x;
    }
    return k;
}

__device__ inline bool same_key(const Key &x, const Key &y) { return x.len == y.len && x.a == y.a && x.b == y.b; }

__device__ inline uint64_t slot_of(const Key &k) { return hash_mix64(k.a ^ hash_mix64(k.b + (k.len + 1) * kHashKey)); }

__global__ __launch_bounds__(kThreads) void k_grp_table(const uint64_t *ends, const unsigned long long *hf, const unsigned long long *hr,
                                                         const uint8_t *active, uint64_t n_rec, unsigned long long *table, uint64_t slots) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        if (!active[r]) continue;
        const Key mine = key_of(ends, hf, hr, r);
        uint64_t slot = slot_of(mine) & (slots - 1);
        const unsigned long long me = ~static_cast<unsigned long long>(r);
        for (uint64_t tries = 0; tries < slots; tries++, slot = (slot + 1) & (slots - 1)) {
            const unsigned long long old = atomicCAS(&table[slot], 0ull, me);
            if (old == 0) break;
            // the slot is taken: by a record of this key (whichever of them holds it now, the key is this one) or of another
            const uint64_t q = ~old;
            if (q < n_rec && same_key(mine, key_of(ends, hf, hr, q))) {
                atomicMax(&table[slot], me);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_grp_probe(const uint64_t *ends, const unsigned long long *hf, const unsigned long long *hr,
                                                         const uint8_t *active, uint64_t n_rec, const unsigned long long *table, uint64_t slots,
                                                         uint64_t *cand, uint32_t *flags) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        if (!active[r]) continue;
        const Key mine = key_of(ends, hf, hr, r);
        uint64_t slot = slot_of(mine) & (slots - 1), found = r;
        for (uint64_t tries = 0; tries < slots; tries++, slot = (slot + 1) & (slots - 1)) {
            const unsigned long long v = table[slot];
            if (v == 0) break;
            const uint64_t q = ~v;
            if (q < n_rec && same_key(mine, key_of(ends, hf, hr, q))) {
                found = q;
                break;
            }
        }
        if (found > r) found = r;                            // (the table keeps the lowest: never above the record itself)
        cand[r] = found;
        // which readings of the candidate can be this record at all: equal letters have equal hashes
        flags[r] = found == r ? 0u : (hf[r] == hf[found] ? 0u : kGrpDiffForward) | (hr && hf[r] == hr[found] ? 0u : kGrpDiffReverse);
    }
}

// ======================================================================================
// k_grp_verify
// ======================================================================================
// section[q .. q + 16) as two words, q of either sign; bytes in front of the section or behind it read as 0
__device__ inline void gather16(const uint8_t *section, uint64_t n_section, bool aligned, int64_t q, uint64_t &x0, uint64_t &x1) {
    x0 = x1 = 0;
    if (q >= static_cast<int64_t>(n_section) || q <= -16) return;
    if (aligned && q >= 0) {
        const uint64_t a = static_cast<uint64_t>(q) & ~15ull;
        const uint32_t sh = static_cast<uint32_t>(q) & 15u;
        uint32_t w[4], h[4] = {0, 0, 0, 0};
        load16(section, n_section, true, a, w);
        if (sh && a + 16 < n_section) load16(section, n_section, true, a + 16, h);
        const uint64_t v0 = (static_cast<uint64_t>(w[1]) << 32) | w[0], v1 = (static_cast<uint64_t>(w[3]) << 32) | w[2];
        const uint64_t v2 = (static_cast<uint64_t>(h[1]) << 32) | h[0], v3 = (static_cast<uint64_t>(h[3]) << 32) | h[2];
        const bool upper = sh >= 8;
        const uint64_t a0 = upper ? v1 : v0, a1 = upper ? v2 : v1, a2 = upper ? v3 : v2;
        const uint32_t bs = 8u * (sh & 7u);
        x0 = bs ? (a0 >> bs) | (a1 << (64u - bs)) : a0;
        x1 = bs ? (a1 >> bs) | (a2 << (64u - bs)) : a1;
        return;
    }
    for (uint32_t i = 0; i < 16; i++) {
        const int64_t p = q + i;
        if (p < 0 || static_cast<uint64_t>(p) >= n_section) continue;
        const uint64_t byte = section[p];
        if (i < 8) x0 |= byte << (8u * i);
        else x1 |= byte << (8u * (i - 8));
    }
}

__global__ __launch_bounds__(kThreads) void k_grp_verify(const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                                                          const GroupTables *tables, const uint64_t *cand, const uint8_t *active, uint32_t *flags,
                                                          const uint32_t *status) {
    __shared__ uint8_t s_canon[256];
    __shared__ uint8_t s_rc[256];                            // a byte as it reads on the other strand: comp[canon[b]]
    const uint32_t t = threadIdx.x;
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) return;      // the table is refused: none of it is used
    const uint64_t last = n_rec - 1;
    const uint64_t limit = ends[last] < n_section ? ends[last] : n_section;
    const uint64_t run0 = static_cast<uint64_t>(blockIdx.x) * kGrpRun * kGrpTile;
    if (run0 >= limit) return;
    const uint64_t run1 = run0 + static_cast<uint64_t>(kGrpRun) * kGrpTile < limit ? run0 + static_cast<uint64_t>(kGrpRun) * kGrpTile : limit;
    s_canon[t] = tables->canon[t];
    s_rc[t] = tables->comp[tables->canon[t]];
    __syncthreads();
    const bool aligned = low4(section) == 0;

    uint64_t k = record_from(ends, 0, last, run0);           // the record of the tile's first byte: the same in every lane
    for (uint64_t t0 = run0; t0 < run1; t0 += kGrpTile) {
        const uint64_t t1 = t0 + kGrpTile < run1 ? t0 + kGrpTile : run1;
        const uint64_t kl = ends[k] >= t1 ? k : record_from(ends, k + 1, last, t1 - 1);   // the record of the tile's last byte
        const uint64_t p0 = t0 + 16ull * t, p1 = p0 + 16 < t1 ? p0 + 16 : t1;
        if (p0 < t1) {
            uint64_t lo = k, hi = kl;                        // the record of the lane's first byte
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (ends[mid] > p0) hi = mid;
                else lo = mid + 1;
            }
            uint64_t r = lo, x0 = 0, x1 = 0;
            bool loaded = false;
            for (uint64_t pos = p0; pos < p1;) {             // r: the record of `pos`
                const uint64_t e = ends[r], b = r ? ends[r - 1] : 0, pe = e < p1 ? e : p1;
                const uint64_t c = cand[r];
                const uint32_t f = active[r] && c < r ? flags[r] : (kGrpDiffForward | kGrpDiffReverse);
                if ((f & (kGrpDiffForward | kGrpDiffReverse)) != (kGrpDiffForward | kGrpDiffReverse)) {
                    if (!loaded) {
                        uint32_t w[4];
                        load16(section, n_section, aligned, p0, w);
                        x0 = map8(s_canon, (static_cast<uint64_t>(w[1]) << 32) | w[0]);
                        x1 = map8(s_canon, (static_cast<uint64_t>(w[3]) << 32) | w[2]);
                        loaded = true;
                    }
                    const uint32_t from = static_cast<uint32_t>(pos - p0), to = static_cast<uint32_t>(pe - p0);
                    const uint64_t m0 = byte_range(from, to, 0), m1 = byte_range(from, to, 8);
                    const uint64_t cb = c ? ends[c - 1] : 0, ce = ends[c];
                    if (ce - cb != e - b || ce > n_section) {                 // (equal keys have equal lengths)
                        atomicOr(&flags[r], kGrpDiffForward | kGrpDiffReverse);
                    } else {
                        // lane byte i is letter p0 + i - b of the record: the candidate's lies at cb + that, or at ce - 1 - that
                        if (!(f & kGrpDiffForward)) {
                            uint64_t y0, y1;
                            gather16(section, n_section, aligned, static_cast<int64_t>(cb) + (static_cast<int64_t>(p0) - static_cast<int64_t>(b)), y0, y1);
                            if (((x0 ^ map8(s_canon, y0)) & m0) | ((x1 ^ map8(s_canon, y1)) & m1)) atomicOr(&flags[r], kGrpDiffForward);
                        }
                        if (!(f & kGrpDiffReverse)) {
                            uint64_t y0, y1;                 // the 16 letters that end at lane byte 0's partner, the last of them byte 0's
                            gather16(section, n_section, aligned, static_cast<int64_t>(ce) - 16 - (static_cast<int64_t>(p0) - static_cast<int64_t>(b)), y0, y1);
                            const uint64_t z0 = __builtin_bswap64(map8(s_rc, y1)), z1 = __builtin_bswap64(map8(s_rc, y0));
                            if (((x0 ^ z0) & m0) | ((x1 ^ z1) & m1)) atomicOr(&flags[r], kGrpDiffReverse);
                        }
                    }
                }
                pos = pe;
                if (pos < p1) r = record_from(ends, r + 1, kl, pos);
            }
        }
        k = kl;
        if (t1 < run1 && ends[k] <= t1) k = record_from(ends, k + 1, last, t1);
    }
}

// ======================================================================================
// k_grp_settle and the groups
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_grp_settle(const uint64_t *cand, const uint32_t *flags, uint8_t *active, uint64_t n_rec,
                                                          uint64_t *representative, uint8_t *strand, unsigned long long *left) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        if (!active[r]) continue;
        const uint64_t c = cand[r];
        const uint32_t f = flags[r] & (kGrpDiffForward | kGrpDiffReverse);
        if (c != r && f == (kGrpDiffForward | kGrpDiffReverse)) {              // another sequence under this key: the next round
            atomicAdd(left, 1ull);
            continue;
        }
        representative[r] = c;                               // (the candidate is the lowest of its key: it settles as itself in this round)
        if (strand) strand[r] = c != r && (f & kGrpDiffForward) ? 1 : 0;
        active[r] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_grp_flag(const uint64_t *representative, uint64_t n_rec, uint64_t *is_first) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r <= n_rec; r += stride)
        is_first[r] = r < n_rec && representative[r] == r ? 1 : 0;
}

// group_of holds the exclusive sums of the flags: right for a representative already, and only those words are read here
__global__ __launch_bounds__(kThreads) void k_grp_fill(const uint64_t *representative, uint64_t n_rec, uint64_t *group_of, uint64_t *group_first,
                                                        unsigned long long *group_size) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_rec; r += stride) {
        const uint64_t first = representative[r];
        const uint64_t g = group_of[first < n_rec ? first : r];
        if (first == r) group_first[g] = r;
        else group_of[r] = g;
        atomicAdd(&group_size[g], 1ull);
    }
}

__global__ __launch_bounds__(kThreads) void k_grp_largest(const unsigned long long *group_size, uint64_t n_groups, unsigned long long *largest) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    unsigned long long most = 0;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < n_groups; g += stride)
        if (group_size[g] > most) most = group_size[g];
    if (most) atomicMax(largest, most);
}

}  // namespace

void launch_grp_hash(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                     const GroupTables *d_tables, unsigned long long *hf, unsigned long long *hr, const uint32_t *status) {
    if (!n_section || !n_rec) return;
    constexpr uint64_t run = static_cast<uint64_t>(kGrpRun) * kGrpTile;
    const dim3 grid(static_cast<uint32_t>((n_section + run - 1) / run)), block(kThreads);
    if (hr) hipLaunchKernelGGL((k_grp_hash<true>), grid, block, 0, stream, section, n_section, ends, n_rec, d_tables, hf, hr, status);
    else hipLaunchKernelGGL((k_grp_hash<false>), grid, block, 0, stream, section, n_section, ends, n_rec, d_tables, hf, hr, status);
}

void launch_grp_cut(hipStream_t stream, unsigned long long *hf, unsigned long long *hr, uint64_t n_rec, uint64_t mask) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_grp_cut, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, hf, hr, n_rec, mask);
}

void launch_grp_table(hipStream_t stream, const uint64_t *ends, const unsigned long long *hf, const unsigned long long *hr, const uint8_t *active,
                      uint64_t n_rec, unsigned long long *table, uint64_t slots, uint64_t *cand, uint32_t *flags) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_grp_table, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, ends, hf, hr, active, n_rec, table, slots);
    hipLaunchKernelGGL(k_grp_probe, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, ends, hf, hr, active, n_rec, table, slots, cand, flags);
}

void launch_grp_verify(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *ends, uint64_t n_rec,
                       const GroupTables *d_tables, const uint64_t *cand, const uint8_t *active, uint32_t *flags, const uint32_t *status) {
    if (!n_section || !n_rec) return;
    constexpr uint64_t run = static_cast<uint64_t>(kGrpRun) * kGrpTile;
    const dim3 grid(static_cast<uint32_t>((n_section + run - 1) / run));
    hipLaunchKernelGGL(k_grp_verify, grid, dim3(kThreads), 0, stream, section, n_section, ends, n_rec, d_tables, cand, active, flags, status);
}

void launch_grp_settle(hipStream_t stream, const uint64_t *cand, const uint32_t *flags, uint8_t *active, uint64_t n_rec, uint64_t *representative,
                       uint8_t *strand, unsigned long long *left) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_grp_settle, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, cand, flags, active, n_rec, representative, strand, left);
}

void launch_grp_flag(hipStream_t stream, const uint64_t *representative, uint64_t n_rec, uint64_t *is_first) {
    hipLaunchKernelGGL(k_grp_flag, dim3(blocks_for(n_rec + 1)), dim3(kThreads), 0, stream, representative, n_rec, is_first);
}

void launch_grp_fill(hipStream_t stream, const uint64_t *representative, uint64_t n_rec, uint64_t *group_of, uint64_t *group_first,
                     unsigned long long *group_size) {
    if (!n_rec) return;
    hipLaunchKernelGGL(k_grp_fill, dim3(blocks_for(n_rec)), dim3(kThreads), 0, stream, representative, n_rec, group_of, group_first, group_size);
}

void launch_grp_largest(hipStream_t stream, const unsigned long long *group_size, uint64_t n_groups, unsigned long long *largest) {
    if (!n_groups) return;
    hipLaunchKernelGGL(k_grp_largest, dim3(blocks_for(n_groups)), dim3(kThreads), 0, stream, group_size, n_groups, largest);
}

}  // namespace grp
}  // namespace nafgpu
