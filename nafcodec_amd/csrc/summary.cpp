// summary.cpp -- host side of nafgpu_summarize / nafgpu_summarize_decoder and the owner of a summary's buffers.  The
// kernels are in summary.hip; the rules in include/nafgpu.h.
//
// One round trip: everything is enqueued, then the host reads the status words and the two histograms in one wait and makes
// the totals from them.  Beside the outputs: the 256-byte table and eight status words.
#include "summary.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device.h"
#include "select.h"

using namespace nafgpu;
using namespace nafgpu::sum;

struct nafgpu_summary {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_counts, d_qsum, d_hist, d_status, d_table;
    nafgpu_summary_result res{};
    ~nafgpu_summary() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace nafgpu {
namespace sum {

void default_classes(uint8_t out[256]) {
    for (int b = 0; b < 256; b++) out[b] = 1u << 6;          // whatever is in none of the columns below, '-' included
    const char *column[6] = {"A", "C", "G", "TU", "N", "RYKMSWBDHV"};
    for (int c = 0; c < 6; c++)
        for (const char *p = column[c]; *p; p++) out[static_cast<uint8_t>(*p)] = out[static_cast<uint8_t>(*p) | 0x20] = static_cast<uint8_t>(1u << c);
    for (int b = 'a'; b <= 'z'; b++) out[b] |= 1u << 7;      // lower case, beside the letter's own column
}

}  // namespace sum
}  // namespace nafgpu

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("summarize: ") + what); }

// a failure behind work that was enqueued: the stream is drained first, so that the buffers the work uses are idle when
// they are released
Failure drained_failure(hipStream_t stream, const char *what) {
    (void)hipStreamSynchronize(stream);
    return device_failure(what);
}

struct Events {
    hipEvent_t ev[2] = {nullptr, nullptr};
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

Route forced_route() {
    const char *e = hook_env("NAFGPU_SUM_ROUTE");           // tests: every tile by one route, whatever it holds
    if (e && !std::strcmp(e, "long")) return kRouteLong;
    if (e && !std::strcmp(e, "short")) return kRouteShort;
    return kRouteAuto;
}

// eof_beyond: a record end beyond the section is an archive that ends early (the decoder's entry point), not a bad argument
Failure summarize(const nafgpu_encode_source &src, const nafgpu_summary_opts *opts, int device, bool eof_beyond, std::unique_ptr<nafgpu_summary> &out) {
    if (!src.d_sequence && !src.d_quality) return Failure::make(NAFGPU_E_INVALID_ARG, "summarize needs the sequence or the quality field");
    if (src.d_sequence && src.d_quality && src.n_quality != src.n_bases)
        return Failure::make(NAFGPU_E_INVALID_LENGTH, "summarize: " + std::to_string(src.n_quality) + " quality bytes for " + std::to_string(src.n_bases) + " letters");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the summary runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_summary> sm(new nafgpu_summary);
    sm->device = device;
    sm->stream = pooled_stream_get(device);
    if (!sm->stream) return device_failure("no stream");
    hipStream_t stream = sm->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const uint64_t n_section = src.d_sequence ? src.n_bases : src.n_quality;
    const uint64_t n_rec = src.d_record_end ? src.n_records : 0;
    const bool rows_seq = n_rec && src.d_sequence, rows_qual = n_rec && src.d_quality;
    uint8_t table[256];
    if (opts && opts->use_classes) std::memcpy(table, opts->classes, sizeof table);
    else default_classes(table);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t hist[512];
    if ((rows_seq && !sm->d_counts.alloc_items(n_rec, 64)) || (rows_qual && !sm->d_qsum.alloc_items(n_rec, 8)) || !sm->d_hist.alloc(sizeof hist) ||
        !sm->d_status.alloc(sizeof status) || !sm->d_table.alloc(sizeof table))
        return device_failure("out of device memory");
    unsigned long long *d_hist = sm->d_hist.as<unsigned long long>();
    uint32_t *d_status = sm->d_status.as<uint32_t>();
    // the outputs are zeroed where atomics add into them (and an empty record's row is never written)
    bool ok = hipMemcpyAsync(sm->d_table.bytes(), table, sizeof table, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemsetAsync(d_status, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(d_hist, 0, sizeof hist, stream) == hipSuccess &&
              (!rows_seq || hipMemsetAsync(sm->d_counts.bytes(), 0, n_rec * 64, stream) == hipSuccess) &&
              (!rows_qual || hipMemsetAsync(sm->d_qsum.bytes(), 0, n_rec * 8, stream) == hipSuccess) && hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "host-to-device copy failed");
    const Route route = forced_route();
    launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_status);
    if (src.d_sequence) {
        launch_sum_hist(stream, src.d_sequence, src.n_bases, d_hist);
        if (rows_seq)
            launch_sum_tiles(stream, src.d_sequence, src.n_bases, src.d_record_end, n_rec, sm->d_table.bytes(), route, sm->d_counts.as<unsigned long long>(), d_status);
    }
    if (src.d_quality) {
        launch_sum_hist(stream, src.d_quality, src.n_quality, d_hist + 256);
        if (rows_qual) launch_sum_tiles(stream, src.d_quality, src.n_quality, src.d_record_end, n_rec, nullptr, route, sm->d_qsum.as<unsigned long long>(), d_status);
    }
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(hist, d_hist, sizeof hist, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the summary kernels failed");
    if (status[0] & (kSumStDecreasing | kSumStBeyond)) {
        const uint64_t down = status[0] & kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
        const uint64_t beyond = status[0] & kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
        if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "summarize: the end of record " + std::to_string(down) + " lies below the end in front of it");
        const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
        return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "summarize: " + what);
    }

    nafgpu_summary_result &r = sm->res;
    std::memset(&r, 0, sizeof r);
    r.d_counts = rows_seq ? sm->d_counts.as<uint64_t>() : nullptr;
    r.d_quality_sum = rows_qual ? sm->d_qsum.as<uint64_t>() : nullptr;
    r.d_letter_hist = src.d_sequence ? sm->d_hist.as<uint64_t>() : nullptr;
    r.d_quality_hist = src.d_quality ? sm->d_hist.as<uint64_t>() + 256 : nullptr;
    r.n_records = n_rec;
    r.n_bases = src.d_sequence ? src.n_bases : 0;
    r.n_quality = src.d_quality ? src.n_quality : 0;
    // the totals: the records' column sums.  When the records cover the section (or there is no record table, and the section
    // is all there is to sum) these are the histogram's; letters behind the last record are taken off it by the table itself.
    const uint64_t last_end = n_rec ? (static_cast<uint64_t>(status[7]) << 32) | status[6] : n_section;
    if (last_end == n_section) {
        for (int b = 0; b < 256; b++) {
            for (int c = 0; c < 8; c++)
                if (table[b] >> c & 1) r.totals[c] += hist[b];
            r.quality_total += hist[256 + b] * static_cast<uint64_t>(b);
        }
    } else {
        std::vector<uint64_t> rows;
        if (rows_seq) {
            rows.resize(n_rec * 8);
            if (hipMemcpyAsync(rows.data(), sm->d_counts.bytes(), n_rec * 64, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
                return drained_failure(stream, "device-to-host copy failed");
            for (uint64_t i = 0; i < n_rec * 8; i++) r.totals[i & 7] += rows[i];
        }
        if (rows_qual) {
            rows.resize(n_rec);
            if (hipMemcpyAsync(rows.data(), sm->d_qsum.bytes(), n_rec * 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
                return drained_failure(stream, "device-to-host copy failed");
            for (uint64_t i = 0; i < n_rec; i++) r.quality_total += rows[i];
        }
    }
    (void)hipEventElapsedTime(&r.ms, ev.ev[0], ev.ev[1]);
    out = std::move(sm);
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_summarize(const nafgpu_encode_source *src, const nafgpu_summary_opts *opts, int device, nafgpu_summary **out, nafgpu_summary_result *res,
                     nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_summary> sm;
    const Failure f = summarize(*src, opts, device, false, sm);
    if (!f.ok()) return fail_c(err, f);
    *res = sm->res;
    *out = sm.release();
    return fail_c(err, Failure());
}

int nafgpu_summarize_decoder(nafgpu_decoder *dec, const nafgpu_summary_opts *opts, nafgpu_summary **out, nafgpu_summary_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, false, &s);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = s.seq;
    src.n_bases = s.seq ? s.n_seq : 0;
    src.d_quality = s.qual;
    src.n_quality = s.qual ? s.n_qual : 0;
    src.d_record_end = s.rec_end;
    src.n_records = s.rec_end ? s.n_rec : 0;
    std::unique_ptr<nafgpu_summary> sm;
    f = summarize(src, opts, s.device, true, sm);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = sm->res;
    *out = sm.release();
    return fail_c(err, Failure());
}

int nafgpu_summary_copy_to_host(nafgpu_summary *s, const void *d_ptr, uint64_t n, void *dst) {
    if (!s || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(s->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_summary_free(nafgpu_summary *s) { delete s; }

}  // extern "C"
