// select.hip -- gfx950 (CDNA4, wave64) kernels of nafgpu_select and nafgpu_find_records: regions of decoded records ->
// letters, qualities, ids, comments and the three end tables of a new set of records.  The rules: include/nafgpu.h at
// nafgpu_select; the passes: select.h.
//
// The gather is driven by the OUTPUT: a workgroup takes a tile of kSelTile output bytes, a lane 16 of them, stored with one
// aligned 16-byte store.  Which region a byte belongs to comes from the scanned ends (two searches per workgroup bound one
// search per lane; a tile inside one region searches nothing).  A lane whose 16 bytes lie in one region reads the two
// aligned 16-byte groups its source span touches and realigns them in registers (the second group is the next lane's
// first: it comes from the cache); a lane that crosses region ends, or the output's end, goes byte by byte.  Loads are
// bounded by the section: a group that reaches in front of it or behind it is read byte by byte, never whole.
// Plain C++ and vector stores only; the same source runs in the CPU fibre harness (tests/emu).
#include <hip/hip_runtime.h>

#include "select.h"

namespace nafgpu {
namespace sel {

namespace {

constexpr uint32_t kThreads = 256;
static_assert(kSelTile == kThreads * 16, "a lane takes 16 output bytes");

__device__ inline uint32_t low4(const void *p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 15u; }

__device__ inline void flag_first(uint32_t *status, uint32_t bit, uint32_t slot, uint64_t at) {
    atomicOr(&status[0], bit);
    atomicMax(reinterpret_cast<unsigned long long *>(status + slot), ~static_cast<unsigned long long>(at));   // the lowest: the largest complement
}

__device__ inline uint32_t decimal_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}

// ":START-END" and "/rc": START = start + 1, END = the resolved end
__device__ inline uint32_t suffix_size(uint64_t start, uint64_t end, bool reverse) {
    return 2 + decimal_digits(start + 1) + decimal_digits(end) + (reverse ? 3u : 0u);
}

__device__ inline uint8_t *put_decimal(uint8_t *p, uint64_t v) {
    const uint32_t d = decimal_digits(v);
    for (uint32_t k = d; k-- > 0;) {
        p[k] = static_cast<uint8_t>('0' + v % 10);
        v /= 10;
    }
    return p + d;
}

struct SelArgs {                 // the decoder's buffers, by value
    const uint64_t *rec_end;  uint64_t n_rec;
    const uint8_t *ids;  const uint64_t *id_end;  uint64_t n_ids;
    const uint8_t *com;  const uint64_t *com_end;  uint64_t n_com;
    uint64_t n_seq, n_qual;      // decoded letters / qualities (n_seq: ~0 when the letters were not selected)
    uint32_t nucleotide, has_qual, named, pad;
};

// ======================================================================================
// k_sel_sizes: one lane per region
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_sel_sizes(const nafgpu_region *regions, uint64_t n, SelArgs a, SelSizes o, uint32_t *status) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k <= n; k += stride) {
        if (k == n) {                                        // the scans' last item: its exclusive sum is the last end
            o.len[k] = 0;
            if (o.id_size) o.id_size[k] = 0;
            if (o.com_size) o.com_size[k] = 0;
            continue;
        }
        const nafgpu_region r = regions[k];
        uint64_t len = 0, src = 0, id_size = 1, com_size = 1;
        bool ok = r.record < a.n_rec && !(r.reverse_complement && !a.nucleotide);
        if (ok) {
            const uint64_t r0 = r.record ? a.rec_end[r.record - 1] : 0, r1 = a.rec_end[r.record];
            const uint64_t rec_len = r1 - r0;
            const uint64_t end = r.end == NAFGPU_REGION_END ? rec_len : r.end;
            if (end > rec_len || r.start > end) {
                ok = false;
            } else {
                if (r1 > a.n_seq || (a.has_qual && r1 > a.n_qual)) flag_first(status, kSelStBeyond, 4, k);
                len = end - r.start;
                src = (r0 + r.start) | (r.reverse_complement ? kSelReverse : 0ull);
                if (a.ids && r.record < a.n_ids) id_size += a.id_end[r.record] - (r.record ? a.id_end[r.record - 1] : 0) - 1;
                if (a.named) id_size += suffix_size(r.start, end, r.reverse_complement != 0);
                if (a.com && r.record < a.n_com) com_size += a.com_end[r.record] - (r.record ? a.com_end[r.record - 1] : 0) - 1;
            }
        }
        if (!ok) flag_first(status, kSelStRefused, 2, k);
        o.len[k] = len;
        o.src[k] = src;
        if (o.id_size) o.id_size[k] = id_size;
        if (o.com_size) o.com_size[k] = com_size;
    }
}

// ======================================================================================
// k_sel_gather
// ======================================================================================
// the first k in [lo, hi] with excl[k + 1] > at (hi: when there is none below it); regions of length 0 are never found
__device__ inline uint64_t region_of(const uint64_t *excl, uint64_t lo, uint64_t hi, uint64_t at) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (excl[mid + 1] > at) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Bytes [16 g - shift, 16 g - shift + 16) of the section, shift = the section pointer's low four bits: one aligned 16-byte
// load when all of them are inside the section, else those that are, byte by byte (the others read as 0).
__device__ inline void load_group(const uint8_t *section, uint64_t n_section, uint32_t shift, uint64_t g, uint32_t *w) {
    const int64_t p0 = static_cast<int64_t>(16 * g) - static_cast<int64_t>(shift);
    if (p0 >= 0 && static_cast<uint64_t>(p0) + 16 <= n_section) {
        const uint4 v = *reinterpret_cast<const uint4 *>(section + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const int64_t p = p0 + static_cast<int64_t>(k);
        if (p >= 0 && static_cast<uint64_t>(p) < n_section) w[k >> 2] |= static_cast<uint32_t>(section[p]) << (8u * (k & 3u));
    }
}

// section[at .. at + 16), all of it inside the section, from the (at most two) aligned groups it touches
__device__ inline void load_span16(const uint8_t *section, uint64_t n_section, uint64_t at, uint32_t *out) {
    const uint32_t shift = low4(section);
    const uint64_t v = at + shift;
    const uint32_t sh = static_cast<uint32_t>(v) & 15u;
    uint32_t w[8];
    load_group(section, n_section, shift, v >> 4, w);
    if (sh == 0) {
        out[0] = w[0]; out[1] = w[1]; out[2] = w[2]; out[3] = w[3];
        return;
    }
    load_group(section, n_section, shift, (v >> 4) + 1, w + 4);
    const uint32_t bits = (sh & 3u) * 8u;
    switch (sh >> 2) {                                       // (a switch: every index below is a constant)
#define NAFGPU_SEL_SPAN(W)                                          \
    out[0] = __builtin_amdgcn_alignbit(w[W + 1], w[W + 0], bits);   \
    out[1] = __builtin_amdgcn_alignbit(w[W + 2], w[W + 1], bits);   \
    out[2] = __builtin_amdgcn_alignbit(w[W + 3], w[W + 2], bits);   \
    out[3] = __builtin_amdgcn_alignbit(w[W + 4], w[W + 3], bits);
    case 0: NAFGPU_SEL_SPAN(0) break;
    case 1: NAFGPU_SEL_SPAN(1) break;
    case 2: NAFGPU_SEL_SPAN(2) break;
    default: NAFGPU_SEL_SPAN(3) break;
#undef NAFGPU_SEL_SPAN
    }
}

__device__ inline uint32_t map4(const uint8_t *tab, uint32_t w) {
    return static_cast<uint32_t>(tab[w & 0xFFu]) | (static_cast<uint32_t>(tab[(w >> 8) & 0xFFu]) << 8) |
           (static_cast<uint32_t>(tab[(w >> 16) & 0xFFu]) << 16) | (static_cast<uint32_t>(tab[w >> 24]) << 24);
}

// REVERSE: some region is on the reverse strand (the forward-only launch has none of that code);
// TABLE: reversed letters go through the complement table (the Sequence section; not the qualities)
template <bool REVERSE, bool TABLE>
__global__ __launch_bounds__(kThreads) void k_sel_gather(const uint8_t *section, uint64_t n_section, const uint64_t *excl, const uint64_t *src,
                                                          uint64_t n_regions, uint64_t n_out, const uint8_t *table, uint8_t *dst) {
    __shared__ uint64_t s_bound[2];
    __shared__ uint8_t s_tab[TABLE ? 256 : 1];               // (only <true, true> has the table in LDS, and reads `table` at all)
    const uint32_t t = threadIdx.x;
    const uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * kSelTile;
    if (tile0 >= n_out) return;
    if constexpr (TABLE) s_tab[t] = table[t];
    // the regions of the tile's first and last byte, searched by two waves side by side
    if (t == 0) s_bound[0] = region_of(excl, 0, n_regions - 1, tile0);
    if (t == 64) s_bound[1] = region_of(excl, 0, n_regions - 1, (tile0 + kSelTile <= n_out ? tile0 + kSelTile : n_out) - 1);
    __syncthreads();
    const uint64_t o0 = tile0 + 16ull * t;
    if (o0 >= n_out) return;
    uint64_t k = region_of(excl, s_bound[0], s_bound[1], o0);
    uint64_t k0 = excl[k], k1 = excl[k + 1];                 // output bytes [k0, k1) are region k's
    uint32_t w[4];
    if (o0 + 16 <= k1) {                                     // all 16 in one region
        const uint64_t s = src[k], from = (s & ~kSelReverse) + (o0 - k0);
        if (REVERSE && (s & kSelReverse)) {
            uint32_t f[4];
            load_span16(section, n_section, (s & ~kSelReverse) + (k1 - o0) - 16, f);
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t x = __builtin_bswap32(f[3 - i]);
                if constexpr (TABLE) w[i] = map4(s_tab, x);
                else w[i] = x;
            }
        } else {
            load_span16(section, n_section, from, w);
        }
    } else {                                                 // region ends, or the output's end, inside the 16: byte by byte
        w[0] = w[1] = w[2] = w[3] = 0;
        uint64_t s = src[k];
        for (uint32_t i = 0; i < 16; i++) {
            const uint64_t o = o0 + i;
            if (o >= n_out) break;
            while (o >= k1) {                                // (o < n_out = the last end: there is such a region)
                k++;
                k0 = k1;
                k1 = excl[k + 1];
                s = src[k];
            }
            uint32_t c;
            if (REVERSE && (s & kSelReverse)) {
                c = section[(s & ~kSelReverse) + (k1 - 1 - o)];
                if constexpr (TABLE) c = s_tab[c];
            } else {
                c = section[s + (o - k0)];
            }
            w[i >> 2] |= c << (8u * (i & 3u));
        }
    }
    *reinterpret_cast<uint4 *>(dst + o0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ======================================================================================
// k_sel_strings: one lane per region
// ======================================================================================
__global__ __launch_bounds__(kThreads) void k_sel_strings(const nafgpu_region *regions, uint64_t n, SelArgs a, const uint64_t *len_excl,
                                                           const uint64_t *id_excl, uint8_t *ids, const uint64_t *com_excl, uint8_t *com) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; k < n; k += stride) {
        const nafgpu_region r = regions[k];
        if (ids) {
            uint8_t *p = ids + id_excl[k];
            if (a.ids && r.record < a.n_ids) {
                const uint64_t i0 = r.record ? a.id_end[r.record - 1] : 0, l = a.id_end[r.record] - i0 - 1;
                for (uint64_t i = 0; i < l; i++) p[i] = a.ids[i0 + i];
                p += l;
            }
            if (a.named) {
                *p++ = ':';
                p = put_decimal(p, r.start + 1);
                *p++ = '-';
                p = put_decimal(p, r.start + (len_excl[k + 1] - len_excl[k]));
                if (r.reverse_complement) {
                    *p++ = '/';
                    *p++ = 'r';
                    *p++ = 'c';
                }
            }
            *p = 0;
        }
        if (com) {
            uint8_t *p = com + com_excl[k];
            if (a.com && r.record < a.n_com) {
                const uint64_t c0 = r.record ? a.com_end[r.record - 1] : 0, l = a.com_end[r.record] - c0 - 1;
                for (uint64_t i = 0; i < l; i++) p[i] = a.com[c0 + i];
                p += l;
            }
            *p = 0;
        }
    }
}

// ======================================================================================
// k_sel_id_table / k_sel_id_probe
// ======================================================================================
// A slot holds the COMPLEMENT of a record index (0: empty), so that atomicMax keeps the lowest index among equal ids.
__device__ inline uint64_t hash_bytes(const uint8_t *p, uint64_t n, uint32_t hash_bits) {
    uint64_t h = 0xCBF29CE484222325ull;                      // FNV-1a, then a finaliser that spreads it over the low bits
    for (uint64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return hash_bits < 64 ? h & ((1ull << hash_bits) - 1) : h;
}

__device__ inline bool same_bytes(const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb) {
    if (na != nb) return false;
    for (uint64_t i = 0; i < na; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__global__ __launch_bounds__(kThreads) void k_sel_id_table(const uint8_t *ids, const uint64_t *id_end, uint64_t n_ids, unsigned long long *table,
                                                            uint64_t slots, uint32_t hash_bits) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; r < n_ids; r += stride) {
        const uint64_t i0 = r ? id_end[r - 1] : 0, l = id_end[r] - i0 - 1;
        uint64_t slot = hash_bytes(ids + i0, l, hash_bits) & (slots - 1);
        const unsigned long long mine = ~static_cast<unsigned long long>(r);
        for (uint64_t tries = 0; tries < slots; tries++, slot = (slot + 1) & (slots - 1)) {
            const unsigned long long old = atomicCAS(&table[slot], 0ull, mine);
            if (old == 0) break;
            // the slot is taken: by an equal id (whichever of them holds it now, the bytes are these) or by another one
            const uint64_t q = ~old, q0 = q ? id_end[q - 1] : 0;
            if (same_bytes(ids + i0, l, ids + q0, id_end[q] - q0 - 1)) {
                atomicMax(&table[slot], mine);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_sel_id_probe(const uint8_t *ids, const uint64_t *id_end, const unsigned long long *table,
                                                            uint64_t slots, uint32_t hash_bits, const uint8_t *names, const uint64_t *name_end,
                                                            uint64_t n_names, uint64_t *record_out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n_names; j += stride) {
        const uint64_t n0 = j ? name_end[j - 1] : 0, l = name_end[j] - n0 - 1;
        uint64_t slot = hash_bytes(names + n0, l, hash_bits) & (slots - 1), found = ~0ull;
        for (uint64_t tries = 0; tries < slots; tries++, slot = (slot + 1) & (slots - 1)) {
            const unsigned long long v = table[slot];
            if (v == 0) break;
            const uint64_t q = ~v, q0 = q ? id_end[q - 1] : 0;
            if (same_bytes(names + n0, l, ids + q0, id_end[q] - q0 - 1)) {
                found = q;
                break;
            }
        }
        record_out[j] = found;
    }
}

uint32_t blocks_for(uint64_t n) {
    uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 8192) blocks = 8192;
    return static_cast<uint32_t>(blocks ? blocks : 1);
}

SelArgs args_of(const SelSource &s, bool named) {
    SelArgs a;
    a.rec_end = s.rec_end;  a.n_rec = s.n_rec;
    a.ids = s.ids;  a.id_end = s.id_end;  a.n_ids = s.n_ids;
    a.com = s.com;  a.com_end = s.com_end;  a.n_com = s.n_com;
    a.n_seq = s.seq ? s.n_seq : ~0ull;
    a.n_qual = s.n_qual;
    a.nucleotide = s.sequence_type <= 1 ? 1u : 0u;
    a.has_qual = s.qual ? 1u : 0u;
    a.named = named ? 1u : 0u;
    a.pad = 0;
    return a;
}

}  // namespace

void launch_sel_sizes(hipStream_t stream, const nafgpu_region *regions, uint64_t n, const SelSource &s, bool named, const SelSizes &o,
                      uint32_t *status) {
    hipLaunchKernelGGL(k_sel_sizes, dim3(blocks_for(n + 1)), dim3(kThreads), 0, stream, regions, n, args_of(s, named), o, status);
}

void launch_sel_gather(hipStream_t stream, const uint8_t *section, uint64_t n_section, const uint64_t *excl, const uint64_t *src,
                       uint64_t n_regions, uint64_t n_out, const uint8_t *table, bool any_reverse, uint8_t *dst) {
    if (!n_out || !n_regions) return;
    const dim3 grid(static_cast<uint32_t>((n_out + kSelTile - 1) / kSelTile)), block(kThreads);
    if (!any_reverse)
        hipLaunchKernelGGL((k_sel_gather<false, false>), grid, block, 0, stream, section, n_section, excl, src, n_regions, n_out, table, dst);
    else if (table)
        hipLaunchKernelGGL((k_sel_gather<true, true>), grid, block, 0, stream, section, n_section, excl, src, n_regions, n_out, table, dst);
    else
        hipLaunchKernelGGL((k_sel_gather<true, false>), grid, block, 0, stream, section, n_section, excl, src, n_regions, n_out, table, dst);
}

void launch_sel_strings(hipStream_t stream, const nafgpu_region *regions, uint64_t n, const SelSource &s, bool named, const uint64_t *len_excl,
                        const uint64_t *id_excl, uint8_t *ids, const uint64_t *com_excl, uint8_t *com) {
    if (!n || (!ids && !com)) return;
    hipLaunchKernelGGL(k_sel_strings, dim3(blocks_for(n)), dim3(kThreads), 0, stream, regions, n, args_of(s, named), len_excl, id_excl, ids,
                       com_excl, com);
}

void launch_sel_id_table(hipStream_t stream, const uint8_t *ids, const uint64_t *id_end, uint64_t n_ids, unsigned long long *table,
                         uint64_t slots, uint32_t hash_bits) {
    if (!n_ids) return;
    hipLaunchKernelGGL(k_sel_id_table, dim3(blocks_for(n_ids)), dim3(kThreads), 0, stream, ids, id_end, n_ids, table, slots, hash_bits);
}

void launch_sel_id_probe(hipStream_t stream, const uint8_t *ids, const uint64_t *id_end, const unsigned long long *table, uint64_t slots,
                         uint32_t hash_bits, const uint8_t *names, const uint64_t *name_end, uint64_t n_names, uint64_t *record_out) {
    if (!n_names) return;
    hipLaunchKernelGGL(k_sel_id_probe, dim3(blocks_for(n_names)), dim3(kThreads), 0, stream, ids, id_end, table, slots, hash_bits, names,
                       name_end, n_names, record_out);
}

}  // namespace sel
}  // namespace nafgpu
