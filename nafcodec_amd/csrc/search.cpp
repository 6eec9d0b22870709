// search.cpp -- host side of nafgpu_search / nafgpu_search_decoder and the owner of the hits' buffers.  The kernels are in
// search.hip; the rules in include/nafgpu.h.
//
// Two round trips: the host reads the status words, the number of hits and the rows' counts behind the count pass, allocates
// the three tables by them, and waits for the write pass.  Beside the outputs: the row tables (4 KiB, 32 KiB for the bytes
// alphabet), eight words per tile of 4 096 letters and the scan's scratch.
#include "search.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device.h"
#include "select.h"
#include "summary.h"

using namespace nafgpu;
using namespace nafgpu::srch;

struct nafgpu_hits {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_regions, d_info, d_begin;
    nafgpu_search_result res{};
    ~nafgpu_hits() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace nafgpu {
namespace srch {

namespace {

// the 4-bit set of a nucleotide letter (A 1, C 2, G 4, T and U 8, the IUPAC codes their unions), 0 for any other byte
uint8_t letter_set(uint8_t b) {
    static const char letters[] = "ACGTURYKMSWBDHVN";
    static const uint8_t sets[] = {1, 2, 4, 8, 8, 5, 10, 12, 3, 6, 9, 14, 13, 11, 7, 15};
    for (int i = 0; letters[i]; i++)
        if ((b & ~0x20u) == static_cast<uint8_t>(letters[i])) return sets[i];   // either case
    return 0;
}

uint8_t reverse4(uint8_t s) { return static_cast<uint8_t>(((s & 1) << 3) | ((s & 2) << 1) | ((s & 4) >> 1) | ((s & 8) >> 3)); }

}  // namespace

Failure build_rows(const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns, const nafgpu_search_opts &opts, SearchRows *out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "search: " + what); };
    if (opts.alphabet > 1) return refuse("alphabet " + std::to_string(opts.alphabet) + " (0 nucleotide, 1 bytes)");
    const bool nuc = opts.alphabet == 0;
    if (!nuc && opts.both_strands) return refuse("both_strands needs the nucleotide alphabet");
    if (n_patterns == 0 || n_patterns > NAFGPU_SEARCH_MAX_PATTERNS)
        return refuse(std::to_string(n_patterns) + " patterns (1 to " + std::to_string(NAFGPU_SEARCH_MAX_PATTERNS) + ")");
    std::vector<uint64_t> ends;
    for (uint64_t i = 0; i < n_bytes; i++)
        if (patterns[i] == 0) ends.push_back(i);
    if (ends.size() != n_patterns || (n_bytes && patterns[n_bytes - 1] != 0))
        return refuse("patterns: " + std::to_string(n_patterns) + " NUL-terminated strings expected, " + std::to_string(ends.size()) + " found in " +
                      std::to_string(n_bytes) + " bytes");
    std::memset(out, 0, sizeof *out);
    const uint32_t shift = opts.both_strands ? 1 : 0;
    out->n_rows = static_cast<uint32_t>(n_patterns) << shift;
    out->n_codes = nuc ? 16 : 256;
    out->strand_shift = shift;
    for (int b = 0; b < 256; b++) out->code[b] = nuc ? letter_set(static_cast<uint8_t>(b)) : static_cast<uint8_t>(b);
    uint64_t shortest = UINT64_MAX, at = 0;
    for (uint64_t p = 0; p < n_patterns; at = ends[p] + 1, p++) {
        const uint8_t *text = patterns + at;
        const uint64_t m = ends[p] - at;
        const std::string head = "pattern " + std::to_string(p) + ": ";
        if (m == 0) return refuse(head + "empty");
        if (m > NAFGPU_SEARCH_MAX_LENGTH) return refuse(head + std::to_string(m) + " letters (at most " + std::to_string(NAFGPU_SEARCH_MAX_LENGTH) + ")");
        shortest = std::min(shortest, m);
        for (uint32_t strand = 0; strand <= shift; strand++) {
            const uint32_t row = (static_cast<uint32_t>(p) << shift) | strand;
            out->length[row] = static_cast<uint8_t>(m);
            uint64_t *accept = out->accept + static_cast<size_t>(row) * out->n_codes;
            for (uint64_t j = 0; j < m; j++) {
                if (!nuc) {
                    accept[text[j]] |= 1ull << j;
                    continue;
                }
                const uint8_t forward = letter_set(text[strand ? m - 1 - j : j]);
                if (!forward)
                    return refuse(head + "letter " + std::to_string(strand ? m - 1 - j : j) + " (byte " + std::to_string(text[strand ? m - 1 - j : j]) +
                                  ") is none of ACGTURYKMSWBDHVN");
                const uint8_t set = strand ? reverse4(forward) : forward;
                for (uint32_t c = 1; c < 16; c++)            // a letter is accepted when its set is not empty and lies inside the pattern's
                    if ((c & ~set) == 0) accept[c] |= 1ull << j;
            }
        }
    }
    if (opts.max_mismatches > NAFGPU_SEARCH_MAX_MISMATCHES)
        return refuse("max_mismatches " + std::to_string(opts.max_mismatches) + " (at most " + std::to_string(NAFGPU_SEARCH_MAX_MISMATCHES) + ")");
    if (opts.max_mismatches >= shortest)
        return refuse("max_mismatches " + std::to_string(opts.max_mismatches) + " with a pattern of " + std::to_string(shortest) + " letters");
    return Failure();
}

}  // namespace srch
}  // namespace nafgpu

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("search: ") + what); }

// a failure behind work that was enqueued: the stream is drained first, so that the buffers the work uses are idle when
// they are released
Failure drained_failure(hipStream_t stream, const char *what) {
    (void)hipStreamSynchronize(stream);
    return device_failure(what);
}

struct Events {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    bool create() {
        for (hipEvent_t &e : ev)
            if (hipEventCreate(&e) != hipSuccess) return false;
        return true;
    }
};

uint64_t complement_at(const uint32_t *status, int slot) { return ~((static_cast<uint64_t>(status[slot + 1]) << 32) | status[slot]); }

// eof_beyond: a record end beyond the section is an archive that ends early (the decoder's entry point), not a bad argument
Failure search(const nafgpu_encode_source &src, const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns, const nafgpu_search_opts &opts, int device,
               bool eof_beyond, std::unique_ptr<nafgpu_hits> &out) {
    if (!src.d_sequence) return Failure::make(NAFGPU_E_INVALID_ARG, "search needs the sequence field");
    std::unique_ptr<SearchRows> rows(new SearchRows);
    Failure f = build_rows(patterns, n_bytes, n_patterns, opts, rows.get());
    if (!f.ok()) return f;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the search runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_hits> hits(new nafgpu_hits);
    hits->device = device;
    hits->stream = pooled_stream_get(device);
    if (!hits->stream) return device_failure("no stream");
    hipStream_t stream = hits->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const bool nuc = opts.alphabet == 0;
    const uint64_t n_section = src.n_bases;
    const uint64_t n_rec = src.d_record_end ? src.n_records : 0;       // 0: the whole section is record 0
    const uint64_t n_out_rec = n_rec ? n_rec : 1;
    const uint64_t n_tiles = (n_section + kSearchTile - 1) / kSearchTile;
    const size_t rows_bytes = offsetof(SearchRows, accept) + static_cast<size_t>(rows->n_rows) * rows->n_codes * sizeof(uint64_t);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ScanTotals tot{0, 0};
    uint64_t row_hits[kSearchMaxRows];
    DevBuf d_rows, d_status, d_base, d_scan_tmp, d_totals, d_row_hits;
    if (!d_rows.alloc(rows_bytes) || !d_status.alloc(sizeof status) || !d_base.alloc_items(n_tiles + 1, 8) || !d_scan_tmp.alloc(scan_tmp_bytes(n_tiles + 1)) ||
        !d_totals.alloc(sizeof tot) || !d_row_hits.alloc(sizeof row_hits) || !hits->d_begin.alloc_items(n_out_rec + 1, 8))
        return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    uint64_t *base = d_base.as<uint64_t>();
    const SearchRows *dr = d_rows.as<SearchRows>();
    // the tiles' counts are zeroed: a tile behind the last record end is not visited
    bool ok = upload_staged(d_rows.bytes(), reinterpret_cast<const uint8_t *>(rows.get()), rows_bytes, stream) &&
              hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(base, 0, (n_tiles + 1) * 8, stream) == hipSuccess &&
              hipMemsetAsync(d_totals.bytes(), 0, sizeof tot, stream) == hipSuccess && hipMemsetAsync(d_row_hits.bytes(), 0, sizeof row_hits, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "host-to-device copy failed");
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_search_tiles(stream, src.d_sequence, n_section, src.d_record_end, n_rec, dr, nuc, opts.max_mismatches, d_st, base,
                        d_row_hits.as<unsigned long long>(), nullptr, nullptr);
    // the existing scan, in place (a lane of k_scan_emit has read its items before it writes them), over n_tiles + 1 items: the
    // last exclusive sum is the number of hits
    launch_scan_excl_u64(stream, base, n_tiles + 1, base, d_scan_tmp.bytes(), d_totals.as<ScanTotals>(), d_st);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(row_hits, d_row_hits.bytes(), sizeof row_hits, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the count pass failed");
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) {
        const uint64_t down = status[0] & sum::kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
        const uint64_t beyond = status[0] & sum::kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
        if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "search: the end of record " + std::to_string(down) + " lies below the end in front of it");
        const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
        return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "search: " + what);
    }
    const uint64_t n_hits = tot.sum;
    if (opts.max_hits && n_hits > opts.max_hits)
        return Failure::make(NAFGPU_E_INVALID_ARG, "search: " + std::to_string(n_hits) + " hits, more than max_hits " + std::to_string(opts.max_hits));

    // ---- the outputs (never empty, so that an empty table still has an address), the write pass, the rows of the records
    if (!hits->d_regions.alloc_items(std::max<uint64_t>(n_hits, 1), sizeof(nafgpu_region)) || !hits->d_info.alloc_items(std::max<uint64_t>(n_hits, 1), sizeof(nafgpu_hit_info)))
        return device_failure("out of device memory");
    nafgpu_region *d_regions = hits->d_regions.as<nafgpu_region>();
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    if (n_hits)
        launch_search_tiles(stream, src.d_sequence, n_section, src.d_record_end, n_rec, dr, nuc, opts.max_mismatches, d_st, base, nullptr, d_regions,
                            hits->d_info.as<nafgpu_hit_info>());
    launch_search_begin(stream, d_regions, n_hits, n_out_rec, hits->d_begin.as<uint64_t>());
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the write pass failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_search_result &r = hits->res;
    std::memset(&r, 0, sizeof r);
    r.d_regions = d_regions;
    r.d_info = hits->d_info.as<nafgpu_hit_info>();
    r.d_record_hit_begin = hits->d_begin.as<uint64_t>();
    r.n_hits = n_hits;
    r.n_records = n_out_rec;
    r.n_bases = n_section;
    for (uint32_t row = 0; row < rows->n_rows; row++) r.pattern_hits[row >> rows->strand_shift] += row_hits[row];
    r.ms = ms;
    out = std::move(hits);
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_search(const nafgpu_encode_source *src, const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns, const nafgpu_search_opts *opts, int device,
                  nafgpu_hits **out, nafgpu_search_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !out || !res || (!patterns && n_bytes) || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    nafgpu_search_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    std::unique_ptr<nafgpu_hits> hits;
    const Failure f = search(*src, patterns, n_bytes, n_patterns, o, device, false, hits);
    if (!f.ok()) return fail_c(err, f);
    *res = hits->res;
    *out = hits.release();
    return fail_c(err, Failure());
}

int nafgpu_search_decoder(nafgpu_decoder *dec, const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns, const nafgpu_search_opts *opts, nafgpu_hits **out,
                          nafgpu_search_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!out || !res || (!patterns && n_bytes)) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, false, &s);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    const bool nucleotide = s.sequence_type <= 1;            // dna and rna; protein and text are searched as bytes
    nafgpu_search_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    else o.alphabet = nucleotide ? 0 : 1;
    if (o.alphabet == 0 && !nucleotide)
        return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "search: the nucleotide alphabet needs a nucleotide archive (dna or rna)"), err);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = s.seq;
    src.n_bases = s.seq ? s.n_seq : 0;
    src.d_record_end = s.rec_end;
    src.n_records = s.rec_end ? s.n_rec : 0;
    std::unique_ptr<nafgpu_hits> hits;
    f = search(src, patterns, n_bytes, n_patterns, o, s.device, true, hits);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = hits->res;
    *out = hits.release();
    return fail_c(err, Failure());
}

int nafgpu_hits_copy_to_host(nafgpu_hits *h, const void *d_ptr, uint64_t n, void *dst) {
    if (!h || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(h->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_hits_free(nafgpu_hits *h) { delete h; }

}  // extern "C"
