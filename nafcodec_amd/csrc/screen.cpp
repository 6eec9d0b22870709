// screen.cpp -- host side of nafgpu_kmers_build / nafgpu_screen and their _decoder forms, and the owner of the set's table
// and the screens' buffers.  The kernels are in screen.hip; the rules in include/nafgpu.h.
//
// The build makes two round trips: the host reads the number of windows behind the count and sizes the table by it, then the
// status words and the number of distinct keys behind the insert.  The screen makes two as trim does: the status words, the
// totals and the number of kept records behind the probes and the scan of the keep flags, then the compaction into a buffer
// of that size.  Beside its outputs a screen holds two words per record (the first and the last matching window), a word per
// record for the scan and the scan's scratch.
#include "screen.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "device.h"
#include "select.h"
#include "summary.h"

using namespace nafgpu;
using namespace nafgpu::scr;

struct nafgpu_kmers {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_table;
    KmerTable table{};
    nafgpu_kmers_result res{};
    ~nafgpu_kmers() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

struct nafgpu_screens {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_windows, d_hits, d_regions, d_match, d_keep, d_kept;
    nafgpu_screen_result res{};
    ~nafgpu_screens() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("screen: ") + what); }

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

// what k_sum_check flagged; eof_beyond: a record end beyond the section is an archive that ends early (the decoder's entry
// points), not a bad argument
Failure table_failure(const uint32_t *status, uint64_t n_section, bool eof_beyond) {
    const uint64_t down = status[0] & sum::kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
    const uint64_t beyond = status[0] & sum::kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
    if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "screen: the end of record " + std::to_string(down) + " lies below the end in front of it");
    const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
    return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "screen: " + what);
}

Failure pick_device(int &device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the screening runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    return Failure();
}

Failure build(const nafgpu_encode_source &src, const nafgpu_kmer_opts &opts, int device, bool eof_beyond, std::unique_ptr<nafgpu_kmers> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "kmers: " + what); };
    if (!src.d_sequence) return refuse("the sequence field is needed");
    if (opts.k < 1 || opts.k > NAFGPU_KMER_MAX_K) return refuse("k " + std::to_string(opts.k) + " (1 .. " + std::to_string(NAFGPU_KMER_MAX_K) + ")");
    Failure f = pick_device(device);
    if (!f.ok()) return f;
    std::unique_ptr<nafgpu_kmers> set(new nafgpu_kmers);
    set->device = device;
    set->stream = pooled_stream_get(device);
    if (!set->stream) return device_failure("no stream");
    hipStream_t stream = set->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const uint64_t n_section = src.n_bases;
    const uint64_t n_rec = src.d_record_end ? src.n_records : 0;           // 0: the whole section is record 0
    KmerTable &table = set->table;
    table.slot = nullptr;
    table.slots = 1;
    table.hash_mask = ~0ull;
    table.k = opts.k;
    table.canonical = opts.canonical != 0;
    if (const char *e = hook_env("NAFGPU_KMER_HASH_BITS")) {  // tests: hashes that collide, so that long chains and the wrap are reached
        const unsigned long bits = std::strtoul(e, nullptr, 10);
        if (bits < 64) table.hash_mask = (1ull << bits) - 1;
    }
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long words[2] = {0, 0};                    // [0]: the windows; [1]: the distinct keys
    DevBuf d_status, d_words;
    if (!d_status.alloc(sizeof status) || !d_words.alloc(sizeof words)) return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    unsigned long long *d_w = d_words.as<unsigned long long>();
    bool ok = hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(d_w, 0, sizeof words, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "clearing the work buffers failed");
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_kmer_count(stream, src.d_sequence, n_section, src.d_record_end, n_rec, table, d_st, d_w);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(words, d_w, sizeof words, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the count kernel failed");
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) return table_failure(status, n_section, eof_beyond);
    const uint64_t n_windows = words[0];
    if (n_windows > n_section) return device_failure("the number of windows is out of range");

    // ---- the table: a power of two at least twice the windows (never empty, so that an empty set still answers probes)
    uint64_t slots = 64;
    while (slots < 2 * n_windows) slots <<= 1;
    if (const char *e = hook_env("NAFGPU_KMER_SLOTS")) {      // tests: a load factor above one half
        const unsigned long long n = std::strtoull(e, nullptr, 10);
        if (n && !(n & (n - 1))) slots = n;
    }
    if (!set->d_table.alloc_items(slots, 8)) return device_failure("out of device memory");
    table.slot = set->d_table.as<unsigned long long>();
    table.slots = slots;
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess && hipMemsetAsync(table.slot, 0, slots * 8, stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "clearing the table failed");
    if (n_windows) launch_kmer_insert(stream, src.d_sequence, n_section, src.d_record_end, n_rec, table, d_st, d_w + 1);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(words, d_w, sizeof words, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the insert kernel failed");
    if (status[0] & kScrStFull) return refuse("a table of " + std::to_string(slots) + " slots is too small for the keys of " + std::to_string(n_windows) + " windows");
    if (words[1] > n_windows) return device_failure("the number of keys is out of range");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_kmers_result &r = set->res;
    std::memset(&r, 0, sizeof r);
    r.n_windows = n_windows;
    r.n_kmers = words[1];
    r.n_bases = n_section;
    r.n_records = n_rec ? n_rec : 1;
    r.slots = slots;
    r.k = opts.k;
    r.canonical = table.canonical ? 1 : 0;
    r.ms = ms;
    out = std::move(set);
    return Failure();
}

Failure screen(const nafgpu_encode_source &src, const nafgpu_kmers &set, const nafgpu_screen_opts &opts, int device, bool eof_beyond,
               std::unique_ptr<nafgpu_screens> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "screen: " + what); };
    if (!src.d_sequence) return refuse("the sequence field is needed");
    if (opts.min_percent > 100) return refuse("min_percent " + std::to_string(opts.min_percent) + " (at most 100)");
    const uint64_t n_rec = src.d_record_end ? src.n_records : 0;           // 0: the whole section is record 0
    const uint64_t n_out = n_rec ? n_rec : 1;
    if (opts.interleaved && (n_out & 1)) return refuse("interleaved with " + std::to_string(n_out) + " records, an odd number");
    Failure f = pick_device(device);
    if (!f.ok()) return f;
    if (device != set.device) return refuse("the set was built on device " + std::to_string(set.device) + ", the records lie on device " + std::to_string(device));
    std::unique_ptr<nafgpu_screens> screens(new nafgpu_screens);
    screens->device = device;
    screens->stream = pooled_stream_get(device);
    if (!screens->stream) return device_failure("no stream");
    hipStream_t stream = screens->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const uint64_t n_section = src.n_bases;
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long totals[kScreenTotals] = {0, 0, 0, 0};
    ScanTotals tot{0, 0};
    DevBuf d_status, d_ends, d_flags, d_scan_tmp, d_totals, d_sums;
    if (!d_status.alloc(sizeof status) || !d_ends.alloc_items(n_out, 16) || !d_flags.alloc_items(n_out + 1, 8) || !d_scan_tmp.alloc(scan_tmp_bytes(n_out + 1)) ||
        !d_totals.alloc(sizeof tot) || !d_sums.alloc(sizeof totals) || !screens->d_windows.alloc_items(n_out, 8) || !screens->d_hits.alloc_items(n_out, 8) ||
        !screens->d_regions.alloc_items(n_out, sizeof(nafgpu_region)) || !screens->d_match.alloc(n_out) || !screens->d_keep.alloc(n_out))
        return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    ScreenWork work;
    work.windows = screens->d_windows.as<unsigned long long>();
    work.hits = screens->d_hits.as<unsigned long long>();
    work.first = d_ends.as<unsigned long long>();
    work.last = work.first + n_out;
    nafgpu_region *d_regions = screens->d_regions.as<nafgpu_region>();
    uint64_t *flags = d_flags.as<uint64_t>();
    // the counts and the two ends are zeroed: atomics work on them
    bool ok = hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(work.windows, 0, n_out * 8, stream) == hipSuccess &&
              hipMemsetAsync(work.hits, 0, n_out * 8, stream) == hipSuccess && hipMemsetAsync(work.first, 0, n_out * 16, stream) == hipSuccess &&
              hipMemsetAsync(d_totals.bytes(), 0, sizeof tot, stream) == hipSuccess && hipMemsetAsync(d_sums.bytes(), 0, sizeof totals, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "clearing the work buffers failed");
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_screen_tiles(stream, src.d_sequence, n_section, src.d_record_end, n_rec, set.table, d_st, work);
    launch_screen_finish(stream, src.d_record_end, n_rec, n_section, opts, d_st, work, d_regions, screens->d_match.bytes(), screens->d_keep.bytes(), flags,
                         d_sums.as<unsigned long long>());
    // the existing scan, in place, over n + 1 items: the last exclusive sum is the number of kept records
    launch_scan_excl_u64(stream, flags, n_out + 1, flags, d_scan_tmp.bytes(), d_totals.as<ScanTotals>(), d_st);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(totals, d_sums.bytes(), sizeof totals, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the screen kernels failed");
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) return table_failure(status, n_section, eof_beyond);
    const uint64_t n_kept = tot.sum;
    if (n_kept > n_out) return device_failure("the number of kept records is out of range");

    // ---- the kept regions (never empty, so that an empty table still has an address)
    if (!screens->d_kept.alloc_items(std::max<uint64_t>(n_kept, 1), sizeof(nafgpu_region))) return device_failure("out of device memory");
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    if (n_kept) launch_screen_compact(stream, src.d_record_end, n_rec, n_section, screens->d_keep.bytes(), flags, n_kept, screens->d_kept.as<nafgpu_region>());
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the compaction failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_screen_result &r = screens->res;
    std::memset(&r, 0, sizeof r);
    r.d_windows = screens->d_windows.as<uint64_t>();
    r.d_hits = screens->d_hits.as<uint64_t>();
    r.d_regions = d_regions;
    r.d_match = screens->d_match.bytes();
    r.d_keep = screens->d_keep.bytes();
    r.d_kept_regions = screens->d_kept.as<nafgpu_region>();
    r.n_records = n_out;
    r.n_matched = totals[0];
    r.n_kept = n_kept;
    r.n_bases = n_section;
    r.n_windows = totals[1];
    r.n_hits = totals[2];
    r.bases_kept = totals[3];
    r.ms = ms;
    out = std::move(screens);
    return Failure();
}

// the letters and the records a decoder holds, as a source; a protein or text archive has no k-mers of nucleotides
Failure decoder_letters(nafgpu_decoder *dec, nafgpu_encode_source *src, int *device) {
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, true, &s);
    if (!f.ok()) return f;
    if (s.sequence_type > 1) return Failure::make(NAFGPU_E_INVALID_ARG, "screen: k-mers need a nucleotide archive (dna or rna)");
    std::memset(src, 0, sizeof *src);
    src->d_sequence = s.seq;
    src->n_bases = s.seq ? s.n_seq : 0;
    src->d_record_end = s.rec_end;
    src->n_records = s.rec_end ? s.n_rec : 0;
    *device = s.device;
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_kmers_build(const nafgpu_encode_source *src, const nafgpu_kmer_opts *opts, int device, nafgpu_kmers **out, nafgpu_kmers_result *res,
                       nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !opts || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_kmers> set;
    const Failure f = build(*src, *opts, device, false, set);
    if (!f.ok()) return fail_c(err, f);
    *res = set->res;
    *out = set.release();
    return fail_c(err, Failure());
}

int nafgpu_kmers_build_decoder(nafgpu_decoder *dec, const nafgpu_kmer_opts *opts, nafgpu_kmers **out, nafgpu_kmers_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!opts || !out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    nafgpu_encode_source src;
    int device = -1;
    Failure f = decoder_letters(dec, &src, &device);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    std::unique_ptr<nafgpu_kmers> set;
    f = build(src, *opts, device, true, set);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = set->res;
    *out = set.release();
    return fail_c(err, Failure());
}

void nafgpu_kmers_free(nafgpu_kmers *set) { delete set; }

int nafgpu_screen(const nafgpu_encode_source *src, const nafgpu_kmers *set, const nafgpu_screen_opts *opts, int device, nafgpu_screens **out,
                  nafgpu_screen_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !set || !opts || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_screens> screens;
    const Failure f = screen(*src, *set, *opts, device, false, screens);
    if (!f.ok()) return fail_c(err, f);
    *res = screens->res;
    *out = screens.release();
    return fail_c(err, Failure());
}

int nafgpu_screen_decoder(nafgpu_decoder *dec, const nafgpu_kmers *set, const nafgpu_screen_opts *opts, nafgpu_screens **out, nafgpu_screen_result *res,
                          nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!set || !opts || !out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    nafgpu_encode_source src;
    int device = -1;
    Failure f = decoder_letters(dec, &src, &device);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    std::unique_ptr<nafgpu_screens> screens;
    f = screen(src, *set, *opts, device, true, screens);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = screens->res;
    *out = screens.release();
    return fail_c(err, Failure());
}

int nafgpu_screens_copy_to_host(nafgpu_screens *s, const void *d_ptr, uint64_t n, void *dst) {
    if (!s || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(s->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_screens_free(nafgpu_screens *s) { delete s; }

}  // extern "C"
