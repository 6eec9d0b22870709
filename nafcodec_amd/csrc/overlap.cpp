// overlap.cpp -- host side of nafgpu_overlap / nafgpu_overlap_decoder and the owner of the overlaps' buffers.  The kernels are
// in overlap.hip; the rules in include/nafgpu.h.  nafgpu_merge_pairs, which makes a selection, is in select.cpp.
//
// Two round trips: the host reads the status words, the totals and the number of unmerged records behind the pair kernel, the
// finish and the scan of the flags, allocates the unmerged regions by it, and waits for the compaction.  Beside the outputs: a
// word per record for the scan and the scan's scratch.
#include "overlap.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "device.h"
#include "select.h"
#include "summary.h"

using namespace nafgpu;
using namespace nafgpu::ovl;

struct nafgpu_overlaps {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_pairs, d_regions, d_unmerged;
    nafgpu_overlap_result res{};
    uint8_t quality_base = 33;
    ~nafgpu_overlaps() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace nafgpu {
namespace ovl {

OvlView view_of(const nafgpu_overlaps *o) {
    OvlView v;
    v.pairs = o->res.d_pairs;
    v.n_records = o->res.n_records;
    v.n_pairs = o->res.n_pairs;
    v.n_found = o->res.n_found;
    v.device = o->device;
    v.quality_base = o->quality_base;
    return v;
}

}  // namespace ovl
}  // namespace nafgpu

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("overlap: ") + what); }

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
Failure overlap(const nafgpu_encode_source &src, const nafgpu_overlap_opts &opts, int device, bool eof_beyond, std::unique_ptr<nafgpu_overlaps> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "overlap: " + what); };
    if (!src.d_sequence) return refuse("the sequence field is needed");
    if (!src.d_record_end || !src.n_records) return refuse("a record table is needed: records 2j and 2j+1 are mates");
    if (src.n_records & 1) return refuse(std::to_string(src.n_records) + " records, an odd number");
    if (opts.max_mismatch_percent > 100) return refuse("max_mismatch_percent " + std::to_string(opts.max_mismatch_percent) + " (at most 100)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the overlaps are found on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_overlaps> ovl(new nafgpu_overlaps);
    ovl->device = device;
    ovl->quality_base = opts.quality_base;
    ovl->stream = pooled_stream_get(device);
    if (!ovl->stream) return device_failure("no stream");
    hipStream_t stream = ovl->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const uint64_t n_rec = src.n_records, n_pairs = n_rec / 2, n_section = src.n_bases;
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long totals[kOvlTotals] = {0, 0, 0, 0, 0, 0, 0};
    ScanTotals tot{0, 0};
    DevBuf d_status, d_flags, d_scan_tmp, d_totals, d_sums;
    if (!d_status.alloc(sizeof status) || !d_flags.alloc_items(n_rec + 1, 8) || !d_scan_tmp.alloc(scan_tmp_bytes(n_rec + 1)) || !d_totals.alloc(sizeof tot) ||
        !d_sums.alloc(sizeof totals) || !ovl->d_pairs.alloc_items(n_pairs, sizeof(nafgpu_pair_overlap)) || !ovl->d_regions.alloc_items(n_rec, sizeof(nafgpu_region)))
        return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    nafgpu_pair_overlap *d_pairs = ovl->d_pairs.as<nafgpu_pair_overlap>();
    nafgpu_region *d_regions = ovl->d_regions.as<nafgpu_region>();
    uint64_t *flags = d_flags.as<uint64_t>();
    bool ok = hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(d_totals.bytes(), 0, sizeof tot, stream) == hipSuccess &&
              hipMemsetAsync(d_sums.bytes(), 0, sizeof totals, stream) == hipSuccess && hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "clearing the work buffers failed");
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_ovl_pairs(stream, src.d_sequence, n_section, src.d_record_end, n_rec, opts, d_st, d_pairs);
    launch_ovl_finish(stream, src.d_record_end, n_rec, d_st, d_pairs, d_regions, flags, d_sums.as<unsigned long long>());
    // the existing scan, in place, over n + 1 items: the last exclusive sum is the number of unmerged records
    launch_scan_excl_u64(stream, flags, n_rec + 1, flags, d_scan_tmp.bytes(), d_totals.as<ScanTotals>(), d_st);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(totals, d_sums.bytes(), sizeof totals, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the overlap kernels failed");
    if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) {
        const uint64_t down = status[0] & sum::kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
        const uint64_t beyond = status[0] & sum::kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
        if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "overlap: the end of record " + std::to_string(down) + " lies below the end in front of it");
        const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
        return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "overlap: " + what);
    }
    const uint64_t n_unmerged = tot.sum;
    if (n_unmerged > n_rec || n_unmerged != 2 * (n_pairs - totals[0])) return device_failure("the number of unmerged records is out of range");

    // ---- the unmerged regions (never empty, so that an empty table still has an address)
    if (!ovl->d_unmerged.alloc_items(std::max<uint64_t>(n_unmerged, 1), sizeof(nafgpu_region))) return device_failure("out of device memory");
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    launch_ovl_compact(stream, src.d_record_end, n_rec, d_pairs, flags, n_unmerged, ovl->d_unmerged.as<nafgpu_region>());
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the compaction failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_overlap_result &r = ovl->res;
    std::memset(&r, 0, sizeof r);
    r.d_pairs = d_pairs;
    r.d_regions = d_regions;
    r.d_unmerged_regions = ovl->d_unmerged.as<nafgpu_region>();
    r.n_records = n_rec;
    r.n_pairs = n_pairs;
    r.n_bases = n_section;
    r.n_found = totals[0];
    r.n_too_long = totals[1];
    r.n_unmerged = n_unmerged;
    r.n_cut = totals[2];
    r.matches = totals[3];
    r.mismatches = totals[4];
    r.bases_merged = totals[5];
    r.bases_after_cut = totals[6];
    r.ms = ms;
    out = std::move(ovl);
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_overlap(const nafgpu_encode_source *src, const nafgpu_overlap_opts *opts, int device, nafgpu_overlaps **out, nafgpu_overlap_result *res,
                   nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !opts || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_overlaps> ovl;
    const Failure f = overlap(*src, *opts, device, false, ovl);
    if (!f.ok()) return fail_c(err, f);
    *res = ovl->res;
    *out = ovl.release();
    return fail_c(err, Failure());
}

int nafgpu_overlap_decoder(nafgpu_decoder *dec, const nafgpu_overlap_opts *opts, nafgpu_overlaps **out, nafgpu_overlap_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!opts || !out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, true, &s);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    if (s.sequence_type > 1) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "overlap: mates need a nucleotide archive (dna or rna)"), err);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = s.seq;
    src.n_bases = s.seq ? s.n_seq : 0;
    src.d_record_end = s.rec_end;
    src.n_records = s.rec_end ? s.n_rec : 0;
    std::unique_ptr<nafgpu_overlaps> ovl;
    f = overlap(src, *opts, s.device, true, ovl);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = ovl->res;
    *out = ovl.release();
    return fail_c(err, Failure());
}

int nafgpu_overlaps_copy_to_host(nafgpu_overlaps *o, const void *d_ptr, uint64_t n, void *dst) {
    if (!o || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(o->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, o->stream) != hipSuccess || hipStreamSynchronize(o->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_overlaps_free(nafgpu_overlaps *o) { delete o; }

}  // extern "C"
