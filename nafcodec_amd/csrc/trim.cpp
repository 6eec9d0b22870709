// trim.cpp -- host side of nafgpu_trim / nafgpu_trim_decoder and the owner of the trims' buffers.  The kernels are in
// trim.hip; the rules in include/nafgpu.h.
//
// Two round trips: the host reads the status words, the totals and the number of kept records behind the steps and the scan of
// the keep flags, allocates the kept regions by it, and waits for the compaction.  Beside the outputs: three words per record
// (the window between the steps, the lowest failing window start), a word per record for the scan, the lists of the long route
// (two words per kTrimShort letters of the section) and the scan's scratch.
#include "trim.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "device.h"
#include "select.h"
#include "summary.h"

using namespace nafgpu;
using namespace nafgpu::trm;

struct nafgpu_trims {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_regions, d_keep, d_kept;
    nafgpu_trim_result res{};
    ~nafgpu_trims() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("trim: ") + what); }

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
Failure trim(const nafgpu_encode_source &src, const nafgpu_trim_opts &opts, int device, bool eof_beyond, std::unique_ptr<nafgpu_trims> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "trim: " + what); };
    if (!src.d_sequence && !src.d_quality) return refuse("the sequence or the quality field is needed");
    if ((opts.cut_front || opts.cut_tail || opts.window) && !src.d_quality) return refuse("cut_front, cut_tail and window need the quality field");
    if (opts.trim_n && !src.d_sequence) return refuse("trim_n needs the sequence field");
    if (opts.window > NAFGPU_TRIM_MAX_WINDOW) return refuse("window " + std::to_string(opts.window) + " (at most " + std::to_string(NAFGPU_TRIM_MAX_WINDOW) + ")");
    const uint64_t n_rec = src.d_record_end ? src.n_records : 0;           // 0: the whole section is record 0
    const uint64_t n_out = n_rec ? n_rec : 1;
    if (opts.interleaved && (n_out & 1)) return refuse("interleaved with " + std::to_string(n_out) + " records, an odd number");
    if (src.d_sequence && src.d_quality && src.n_quality != src.n_bases)
        return Failure::make(NAFGPU_E_INVALID_LENGTH, "trim: " + std::to_string(src.n_quality) + " quality bytes for " + std::to_string(src.n_bases) + " letters");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the trimming runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_trims> trims(new nafgpu_trims);
    trims->device = device;
    trims->stream = pooled_stream_get(device);
    if (!trims->stream) return device_failure("no stream");
    hipStream_t stream = trims->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const uint64_t n_section = src.d_sequence ? src.n_bases : src.n_quality;
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long totals[kTrimTotals] = {0, 0, 0};
    ScanTotals tot{0, 0};
    TrimWork work;
    work.list_cap = trim_list_cap(n_section);
    DevBuf d_status, d_win, d_cut, d_lists, d_flags, d_scan_tmp, d_totals, d_sums;
    if (!d_status.alloc(sizeof status) || !d_win.alloc_items(n_out, 16) || !d_cut.alloc_items(n_out, 8) || !d_lists.alloc_items(2 * (work.list_cap + 1), 8) ||
        !d_flags.alloc_items(n_out + 1, 8) || !d_scan_tmp.alloc(scan_tmp_bytes(n_out + 1)) || !d_totals.alloc(sizeof tot) || !d_sums.alloc(sizeof totals) ||
        !trims->d_regions.alloc_items(n_out, sizeof(nafgpu_region)) || !trims->d_keep.alloc(n_out))
        return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    work.win = d_win.as<uint64_t>();
    work.cut = d_cut.as<unsigned long long>();
    work.list_sum = d_lists.as<unsigned long long>();
    work.list_n = work.list_sum + work.list_cap + 1;
    nafgpu_region *d_regions = trims->d_regions.as<nafgpu_region>();
    uint64_t *flags = d_flags.as<uint64_t>();
    // the lowest failing starts and the lists' counts are zeroed: atomics work on them
    bool ok = hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(work.cut, 0, n_out * 8, stream) == hipSuccess &&
              hipMemsetAsync(work.list_sum, 0, 8, stream) == hipSuccess && hipMemsetAsync(work.list_n, 0, 8, stream) == hipSuccess &&
              hipMemsetAsync(d_totals.bytes(), 0, sizeof tot, stream) == hipSuccess && hipMemsetAsync(d_sums.bytes(), 0, sizeof totals, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "clearing the work buffers failed");
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_trim_init(stream, src.d_record_end, n_rec, n_section, opts, d_st, work);
    if (opts.cut_front || opts.cut_tail) launch_trim_sum(stream, src.d_quality, n_section, src.d_record_end, n_rec, opts, d_st, work);
    if (opts.window) launch_trim_window(stream, src.d_quality, n_section, src.d_record_end, n_rec, opts, d_st, work);
    if (opts.trim_n) launch_trim_n(stream, src.d_sequence, n_section, src.d_record_end, n_rec, d_st, work);
    launch_trim_finish(stream, src.d_record_end, n_rec, n_section, opts, d_st, work, d_regions, trims->d_keep.bytes(), flags, d_sums.as<unsigned long long>());
    // the existing scan, in place, over n + 1 items: the last exclusive sum is the number of kept records
    launch_scan_excl_u64(stream, flags, n_out + 1, flags, d_scan_tmp.bytes(), d_totals.as<ScanTotals>(), d_st);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(totals, d_sums.bytes(), sizeof totals, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the trim kernels failed");
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) {
        const uint64_t down = status[0] & sum::kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
        const uint64_t beyond = status[0] & sum::kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
        if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "trim: the end of record " + std::to_string(down) + " lies below the end in front of it");
        const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
        return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "trim: " + what);
    }
    const uint64_t n_kept = tot.sum;
    if (n_kept > n_out) return device_failure("the number of kept records is out of range");

    // ---- the kept regions (never empty, so that an empty table still has an address)
    if (!trims->d_kept.alloc_items(std::max<uint64_t>(n_kept, 1), sizeof(nafgpu_region))) return device_failure("out of device memory");
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    if (n_kept) launch_trim_compact(stream, d_regions, trims->d_keep.bytes(), flags, n_out, n_kept, trims->d_kept.as<nafgpu_region>());
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the compaction failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_trim_result &r = trims->res;
    std::memset(&r, 0, sizeof r);
    r.d_regions = d_regions;
    r.d_keep = trims->d_keep.bytes();
    r.d_kept_regions = trims->d_kept.as<nafgpu_region>();
    r.n_records = n_out;
    r.n_kept = n_kept;
    r.n_bases = n_section;
    r.n_changed = totals[0];
    r.bases_in_windows = totals[1];
    r.bases_kept = totals[2];
    r.ms = ms;
    out = std::move(trims);
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_trim(const nafgpu_encode_source *src, const nafgpu_trim_opts *opts, int device, nafgpu_trims **out, nafgpu_trim_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !opts || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_trims> trims;
    const Failure f = trim(*src, *opts, device, false, trims);
    if (!f.ok()) return fail_c(err, f);
    *res = trims->res;
    *out = trims.release();
    return fail_c(err, Failure());
}

int nafgpu_trim_decoder(nafgpu_decoder *dec, const nafgpu_trim_opts *opts, nafgpu_trims **out, nafgpu_trim_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!opts || !out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, true, &s);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = s.seq;
    src.n_bases = s.seq ? s.n_seq : 0;
    src.d_quality = s.qual;
    src.n_quality = s.qual ? s.n_qual : 0;
    src.d_record_end = s.rec_end;
    src.n_records = s.rec_end ? s.n_rec : 0;
    std::unique_ptr<nafgpu_trims> trims;
    f = trim(src, *opts, s.device, true, trims);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = trims->res;
    *out = trims.release();
    return fail_c(err, Failure());
}

int nafgpu_trims_copy_to_host(nafgpu_trims *t, const void *d_ptr, uint64_t n, void *dst) {
    if (!t || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(t->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, t->stream) != hipSuccess || hipStreamSynchronize(t->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_trims_free(nafgpu_trims *t) { delete t; }

}  // extern "C"
