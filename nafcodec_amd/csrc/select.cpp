// select.cpp -- host side of nafgpu_select / nafgpu_find_records and the owner of a selection's buffers.  The kernels are
// in select.hip; the rules in include/nafgpu.h.  nafgpu_merge_pairs is here too: it makes a selection (its kernels: overlap.hip).
//
// Two round trips: the host reads the status words and the three totals of the size pass, allocates the outputs by them,
// and waits for the gather.  Beside the outputs: 32 bytes per region (the regions themselves), 8 for where its letters lie,
// and the end tables, which are part of the result.
#include "select.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device.h"
#include "overlap.h"

using namespace nafgpu;
using namespace nafgpu::sel;

struct nafgpu_selection {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_seq, d_qual, d_len, d_ids, d_id_off, d_com, d_com_off, d_hash;
    DevBuf d_fmt_sizes, d_fmt_off, d_scan_tmp, d_totals, d_status, d_text;
    nafgpu_select_result res{};
    uint8_t name_separator = ' ';
    ~nafgpu_selection() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace nafgpu {
namespace sel {

void complement_table(uint8_t sequence_type, uint8_t out[256]) {
    for (int c = 0; c < 256; c++) out[c] = static_cast<uint8_t>(c);
    // the format's 4-bit codes with their bits reversed (- T G K C Y S B A W R D M H V N, code 0 .. 15)
    const char *pairs = sequence_type == 1 ? "AUCGRYKMBVDH" : "ATCGRYKMBVDH";
    for (int i = 0; pairs[i]; i += 2) {
        const uint8_t a = static_cast<uint8_t>(pairs[i]), b = static_cast<uint8_t>(pairs[i + 1]);
        out[a] = b;
        out[b] = a;
        out[a | 0x20] = b | 0x20;
        out[b | 0x20] = a | 0x20;
    }
}

}  // namespace sel
}  // namespace nafgpu

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("select: ") + what); }

// a failure behind work that was enqueued: the stream is drained first (whatever that gives), so that the buffers the work
// uses are idle when the caller's locals release them
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

bool open_selection(const SelSource &s, std::unique_ptr<nafgpu_selection> &out) {
    std::unique_ptr<nafgpu_selection> p(new nafgpu_selection);
    if (hipSetDevice(s.device) != hipSuccess) return false;
    p->device = s.device;
    p->stream = pooled_stream_get(s.device);
    if (!p->stream || !p->d_hash.alloc(8)) return false;
    p->name_separator = s.name_separator;
    out = std::move(p);
    return true;
}

// why the rules refuse region k (the kernel found the lowest such k; the host has the region itself)
std::string refusal(const nafgpu_region &r, uint64_t k, const SelSource &s) {
    const std::string head = "region " + std::to_string(k) + ": ";
    if (r.record >= s.n_rec) return head + "record " + std::to_string(r.record) + " of " + std::to_string(s.n_rec);
    if (r.reverse_complement && s.sequence_type > 1) return head + "reverse_complement needs a nucleotide archive (dna or rna)";
    if (r.end == NAFGPU_REGION_END) return head + "start " + std::to_string(r.start) + " lies behind the record's end";
    if (r.start > r.end) return head + "start " + std::to_string(r.start) + " lies behind end " + std::to_string(r.end);
    return head + "end " + std::to_string(r.end) + " lies behind the record's end";
}

// a table of n + 1 exclusive sums whose entry 1 (the first inclusive end) is 16-byte aligned
bool alloc_ends(DevBuf &b, uint64_t n) { return b.alloc_items(n + 2, 8, 8); }
uint64_t *excl_of(const DevBuf &b) { return b.as<uint64_t>() + 1; }

Failure select(const SelSource &s, const nafgpu_region *regions, uint64_t n, bool named, std::unique_ptr<nafgpu_selection> &out) {
    std::unique_ptr<nafgpu_selection> sel;
    if (!open_selection(s, sel)) return device_failure("no stream");
    hipStream_t stream = sel->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");
    const bool with_ids = s.ids != nullptr, with_com = s.com != nullptr;
    bool any_reverse = false;
    for (uint64_t k = 0; k < n; k++) any_reverse = any_reverse || regions[k].reverse_complement != 0;

    // ---- sizes, the checks, the three end tables
    ScanTotals tot[3];
    std::memset(tot, 0, sizeof tot);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t table[256];
    complement_table(s.sequence_type, table);
    DevBuf d_regions, d_src, d_table;
    if (!d_regions.alloc_items(std::max<uint64_t>(n, 1), sizeof(nafgpu_region)) || !d_src.alloc_items(std::max<uint64_t>(n, 1), 8) ||
        !alloc_ends(sel->d_len, n) || (with_ids && !alloc_ends(sel->d_id_off, n)) || (with_com && !alloc_ends(sel->d_com_off, n)) ||
        !sel->d_scan_tmp.alloc(scan_tmp_bytes(n + 1)) || !sel->d_totals.alloc(sizeof tot) || !sel->d_status.alloc(sizeof status) ||
        !d_table.alloc(sizeof table))
        return device_failure("out of device memory");
    SelSizes sz;
    sz.len = excl_of(sel->d_len);
    sz.src = d_src.as<uint64_t>();
    sz.id_size = with_ids ? excl_of(sel->d_id_off) : nullptr;
    sz.com_size = with_com ? excl_of(sel->d_com_off) : nullptr;
    ScanTotals *d_tot = sel->d_totals.as<ScanTotals>();
    uint32_t *d_status = sel->d_status.as<uint32_t>();
    bool ok = (!n || upload_staged(d_regions.bytes(), reinterpret_cast<const uint8_t *>(regions), n * sizeof(nafgpu_region), stream)) &&
              hipMemcpyAsync(d_tot, tot, sizeof tot, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_status, status, sizeof status, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_table.bytes(), table, sizeof table, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "host-to-device copy failed");
    launch_sel_sizes(stream, d_regions.as<nafgpu_region>(), n, s, named, sz, d_status);
    // The existing scan, once per table and in place (a lane of k_scan_emit has read its items before it writes them), over
    // n + 1 items: the exclusive sums behind the first are the inclusive ends.
    launch_scan_excl_u64(stream, sz.len, n + 1, sz.len, sel->d_scan_tmp.bytes(), &d_tot[0], d_status);
    if (with_ids) launch_scan_excl_u64(stream, sz.id_size, n + 1, sz.id_size, sel->d_scan_tmp.bytes(), &d_tot[1], d_status);
    if (with_com) launch_scan_excl_u64(stream, sz.com_size, n + 1, sz.com_size, sel->d_scan_tmp.bytes(), &d_tot[2], d_status);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the size pass failed");
    if (status[0] & kSelStRefused) {
        const uint64_t k = complement_at(status, 2);
        return Failure::make(NAFGPU_E_INVALID_ARG, k < n ? refusal(regions[k], k, s) : "a region is refused");
    }
    if (status[0] & kSelStBeyond)
        return Failure::io(NAFGPU_IO_UNEXPECTED_EOF, "region " + std::to_string(complement_at(status, 4)) + ": record lengths exceed the decoded sequence");
    const uint64_t n_out = tot[0].sum, n_ids_bytes = with_ids ? tot[1].sum : 0, n_com_bytes = with_com ? tot[2].sum : 0;

    // ---- the outputs (never empty, so that an empty field still has an address; whole 16-byte groups), gather, strings
    const uint64_t n_alloc = std::max<uint64_t>((n_out + 15) / 16 * 16, 16);
    if ((s.seq && !sel->d_seq.alloc(n_alloc)) || (s.qual && !sel->d_qual.alloc(n_alloc)) || (with_ids && !sel->d_ids.alloc(std::max<uint64_t>(n_ids_bytes, 16))) ||
        (with_com && !sel->d_com.alloc(std::max<uint64_t>(n_com_bytes, 16))))
        return device_failure("out of device memory");
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    if (s.seq) launch_sel_gather(stream, s.seq, s.n_seq, sz.len, sz.src, n, n_out, d_table.bytes(), any_reverse, sel->d_seq.bytes());
    if (s.qual) launch_sel_gather(stream, s.qual, s.n_qual, sz.len, sz.src, n, n_out, nullptr, any_reverse, sel->d_qual.bytes());
    launch_sel_strings(stream, d_regions.as<nafgpu_region>(), n, s, named, sz.len, sz.id_size, with_ids ? sel->d_ids.bytes() : nullptr, sz.com_size,
                       with_com ? sel->d_com.bytes() : nullptr);
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the gather failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_select_result &r = sel->res;
    std::memset(&r, 0, sizeof r);
    r.src.d_sequence = s.seq ? sel->d_seq.bytes() : nullptr;
    r.src.n_bases = s.seq ? n_out : 0;
    r.src.d_quality = s.qual ? sel->d_qual.bytes() : nullptr;
    r.src.n_quality = s.qual ? n_out : 0;
    r.src.d_record_end = sz.len + 1;
    r.src.n_records = n;
    r.src.d_ids = with_ids ? sel->d_ids.bytes() : nullptr;
    r.src.n_ids_bytes = n_ids_bytes;
    r.src.d_comments = with_com ? sel->d_com.bytes() : nullptr;
    r.src.n_comments_bytes = n_com_bytes;
    r.d_id_end = with_ids ? sz.id_size + 1 : nullptr;
    r.d_comment_end = with_com ? sz.com_size + 1 : nullptr;
    r.n_regions = n;
    r.ms = ms;
    out = std::move(sel);
    return Failure();
}

// nafgpu_merge_pairs: one record per found pair.  The passes of select() with the kernels of overlap.hip in the place of the
// size pass and the gather; ids and comments are R1's, copied by k_sel_strings.
Failure merge_pairs(const SelSource &s, const ovl::OvlView &v, std::unique_ptr<nafgpu_selection> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "merge_pairs: " + what); };
    if (s.sequence_type > 1) return refuse("mates need a nucleotide archive (dna or rna)");
    if (!s.seq) return refuse("the sequence field is needed");
    if (v.n_records != s.n_rec) return refuse("the overlaps are of " + std::to_string(v.n_records) + " records, the decoder has " + std::to_string(s.n_rec));
    if (v.device != s.device) return refuse("the overlaps were found on another device");
    std::unique_ptr<nafgpu_selection> sel;
    if (!open_selection(s, sel)) return device_failure("no stream");
    hipStream_t stream = sel->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");
    const bool with_ids = s.ids != nullptr, with_com = s.com != nullptr;
    const uint64_t n = v.n_found, n_pairs = v.n_pairs;

    ScanTotals tot[4];
    std::memset(tot, 0, sizeof tot);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t table[256];
    complement_table(s.sequence_type, table);
    DevBuf d_regions, d_pair_of, d_where, d_table;
    if (!d_regions.alloc_items(std::max<uint64_t>(n, 1), sizeof(nafgpu_region)) || !d_pair_of.alloc_items(std::max<uint64_t>(n, 1), 8) ||
        !d_where.alloc_items(n_pairs + 1, 8) || !alloc_ends(sel->d_len, n) || (with_ids && !alloc_ends(sel->d_id_off, n)) ||
        (with_com && !alloc_ends(sel->d_com_off, n)) || !sel->d_scan_tmp.alloc(scan_tmp_bytes(std::max(n, n_pairs) + 1)) || !sel->d_totals.alloc(sizeof tot) ||
        !sel->d_status.alloc(sizeof status) || !d_table.alloc(sizeof table))
        return device_failure("out of device memory");
    uint64_t *len = excl_of(sel->d_len), *id_size = with_ids ? excl_of(sel->d_id_off) : nullptr, *com_size = with_com ? excl_of(sel->d_com_off) : nullptr;
    ScanTotals *d_tot = sel->d_totals.as<ScanTotals>();
    uint32_t *d_status = sel->d_status.as<uint32_t>();
    ovl::OvlSource os;
    os.seq = s.seq;  os.qual = s.qual;  os.n_seq = s.n_seq;  os.n_qual = s.n_qual;
    os.rec_end = s.rec_end;  os.n_rec = s.n_rec;
    os.ids = s.ids;  os.id_end = s.id_end;  os.n_ids = s.n_ids;
    os.com = s.com;  os.com_end = s.com_end;  os.n_com = s.n_com;
    bool ok = hipMemcpyAsync(d_tot, tot, sizeof tot, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_status, status, sizeof status, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemcpyAsync(d_table.bytes(), table, sizeof table, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipEventRecord(ev.ev[0], stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "host-to-device copy failed");
    ovl::launch_ovl_found(stream, v.pairs, n_pairs, d_where.as<uint64_t>());
    launch_scan_excl_u64(stream, d_where.as<uint64_t>(), n_pairs + 1, d_where.as<uint64_t>(), sel->d_scan_tmp.bytes(), &d_tot[3], d_status);
    ovl::launch_ovl_merge_sizes(stream, v.pairs, n_pairs, d_where.as<uint64_t>(), n, os, len, id_size, com_size, d_pair_of.as<uint64_t>(),
                                d_regions.as<nafgpu_region>(), d_status);
    launch_scan_excl_u64(stream, len, n + 1, len, sel->d_scan_tmp.bytes(), &d_tot[0], d_status);
    if (with_ids) launch_scan_excl_u64(stream, id_size, n + 1, id_size, sel->d_scan_tmp.bytes(), &d_tot[1], d_status);
    if (with_com) launch_scan_excl_u64(stream, com_size, n + 1, com_size, sel->d_scan_tmp.bytes(), &d_tot[2], d_status);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
         hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the size pass failed");
    if (tot[3].sum != n) return refuse("the overlaps hold " + std::to_string(tot[3].sum) + " found pairs, their totals say " + std::to_string(n));
    if (status[0] & ovl::kOvlStRefused) return refuse("pair " + std::to_string(complement_at(status, 2)) + " does not fit the decoder's records");
    if (status[0] & ovl::kOvlStBeyond)
        return Failure::io(NAFGPU_IO_UNEXPECTED_EOF, "pair " + std::to_string(complement_at(status, 4)) + ": record lengths exceed the decoded sequence");
    const uint64_t n_out = tot[0].sum, n_ids_bytes = with_ids ? tot[1].sum : 0, n_com_bytes = with_com ? tot[2].sum : 0;

    const uint64_t n_alloc = std::max<uint64_t>((n_out + 15) / 16 * 16, 16);
    if (!sel->d_seq.alloc(n_alloc) || (s.qual && !sel->d_qual.alloc(n_alloc)) || (with_ids && !sel->d_ids.alloc(std::max<uint64_t>(n_ids_bytes, 16))) ||
        (with_com && !sel->d_com.alloc(std::max<uint64_t>(n_com_bytes, 16))))
        return device_failure("out of device memory");
    ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
    ovl::launch_ovl_merge(stream, v.pairs, d_pair_of.as<uint64_t>(), len, n, n_out, os, d_table.bytes(), v.quality_base, sel->d_seq.bytes(),
                          s.qual ? sel->d_qual.bytes() : nullptr);
    launch_sel_strings(stream, d_regions.as<nafgpu_region>(), n, s, false, len, id_size, with_ids ? sel->d_ids.bytes() : nullptr, com_size,
                       with_com ? sel->d_com.bytes() : nullptr);
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the merge failed");
    float a = 0, b = 0, ms = 0;
    if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;

    nafgpu_select_result &r = sel->res;
    std::memset(&r, 0, sizeof r);
    r.src.d_sequence = sel->d_seq.bytes();
    r.src.n_bases = n_out;
    r.src.d_quality = s.qual ? sel->d_qual.bytes() : nullptr;
    r.src.n_quality = s.qual ? n_out : 0;
    r.src.d_record_end = len + 1;
    r.src.n_records = n;
    r.src.d_ids = with_ids ? sel->d_ids.bytes() : nullptr;
    r.src.n_ids_bytes = n_ids_bytes;
    r.src.d_comments = with_com ? sel->d_com.bytes() : nullptr;
    r.src.n_comments_bytes = n_com_bytes;
    r.d_id_end = with_ids ? id_size + 1 : nullptr;
    r.d_comment_end = with_com ? com_size + 1 : nullptr;
    r.n_regions = n;
    r.ms = ms;
    out = std::move(sel);
    return Failure();
}

Failure find_records(const SelSource &s, const uint8_t *names, uint64_t n_bytes, uint64_t n_names, uint64_t *record_out) {
    if (!s.ids) return Failure::make(NAFGPU_E_INVALID_ARG, "find_records needs the ids decoded (opts.id)");
    std::vector<uint64_t> name_end;
    name_end.reserve(static_cast<size_t>(n_names));
    for (uint64_t i = 0; i < n_bytes; i++)
        if (names[i] == 0) name_end.push_back(i + 1);
    if (name_end.size() != n_names || (n_bytes && names[n_bytes - 1] != 0))
        return Failure::make(NAFGPU_E_INVALID_ARG, "names: " + std::to_string(n_names) + " NUL-terminated strings expected, " + std::to_string(name_end.size()) +
                                                       " found in " + std::to_string(n_bytes) + " bytes");
    if (!n_names) return Failure();
    if (!s.n_ids) {
        std::fill(record_out, record_out + n_names, UINT64_MAX);
        return Failure();
    }
    uint32_t hash_bits = 64;
    if (const char *e = hook_env("NAFGPU_SEL_HASH_BITS")) hash_bits = static_cast<uint32_t>(std::min<unsigned long>(std::strtoul(e, nullptr, 10), 64));
    uint64_t slots = 16;
    while (slots < 2 * s.n_ids) slots <<= 1;
    if (hipSetDevice(s.device) != hipSuccess) return device_failure("hipSetDevice failed");
    hipStream_t stream = pooled_stream_get(s.device);
    if (!stream) return device_failure("no stream");
    Failure f;
    {
        DevBuf d_table, d_names, d_name_end, d_out;
        if (!d_table.alloc_items(slots, 8) || !d_names.alloc(n_bytes) || !d_name_end.alloc_items(n_names, 8) || !d_out.alloc_items(n_names, 8)) {
            f = device_failure("out of device memory");
        } else {
            bool ok = hipMemsetAsync(d_table.bytes(), 0, slots * 8, stream) == hipSuccess &&
                      upload_staged(d_names.bytes(), names, n_bytes, stream) &&
                      upload_staged(d_name_end.bytes(), reinterpret_cast<const uint8_t *>(name_end.data()), n_names * 8, stream);
            if (ok) {
                launch_sel_id_table(stream, s.ids, s.id_end, s.n_ids, d_table.as<unsigned long long>(), slots, hash_bits);
                launch_sel_id_probe(stream, s.ids, s.id_end, d_table.as<unsigned long long>(), slots, hash_bits, d_names.bytes(),
                                    d_name_end.as<uint64_t>(), n_names, d_out.as<uint64_t>());
                ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(record_out, d_out.bytes(), n_names * 8, hipMemcpyDeviceToHost, stream) == hipSuccess;
            }
            ok = hipStreamSynchronize(stream) == hipSuccess && ok;
            if (!ok) f = device_failure("the id lookup failed");
        }
    }
    pooled_stream_put(s.device, stream);
    return f;
}

Failure format(nafgpu_selection *sel, uint64_t line_length, nafgpu_text_result *out) {
    const nafgpu_select_result &r = sel->res;
    if (!r.src.d_sequence) return Failure::make(NAFGPU_E_INVALID_ARG, "text output needs the sequence field");
    if (hipSetDevice(sel->device) != hipSuccess) return device_failure("hipSetDevice failed");
    const uint64_t n_rec = r.src.n_records;
    out->fastq = r.src.d_quality ? 1 : 0;
    if (!n_rec) return Failure();
    hipStream_t stream = sel->stream;
    FmtText t{};
    t.seq = r.src.d_sequence;
    t.qual = r.src.d_quality;
    t.rec_end = r.src.d_record_end;
    t.ids = r.src.d_ids;
    t.id_end = r.d_id_end;
    t.n_ids = r.src.d_ids ? n_rec : 0;
    t.com = r.src.d_comments;
    t.com_end = r.d_comment_end;
    t.n_com = r.src.d_comments ? n_rec : 0;
    t.n_rec = n_rec;
    t.line_length = line_length;
    t.sep = sel->name_separator;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");
    if (!sel->d_fmt_sizes.alloc_items(n_rec, 8) || !sel->d_fmt_off.alloc_items(n_rec + 1, 8) || !sel->d_scan_tmp.alloc(scan_tmp_bytes(n_rec + 1)))
        return device_failure("out of device memory");
    ScanTotals *d_tot = sel->d_totals.as<ScanTotals>();
    ScanTotals tot{0, 0};
    bool ok = hipEventRecord(ev.ev[0], stream) == hipSuccess && hipMemsetAsync(d_tot, 0, sizeof tot, stream) == hipSuccess;
    launch_fmt_sizes(stream, t, sel->d_fmt_sizes.as<uint64_t>());
    launch_scan_excl_u64(stream, sel->d_fmt_sizes.as<uint64_t>(), n_rec, sel->d_fmt_off.as<uint64_t>(), sel->d_scan_tmp.bytes(), d_tot,
                         sel->d_status.as<uint32_t>());
    ok = ok && hipMemcpyAsync(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return device_failure("text size read-back failed");
    if (!sel->d_text.alloc(static_cast<size_t>(tot.sum) + 64)) return device_failure("out of device memory for the text");
    launch_fmt_write(stream, t, sel->d_fmt_off.as<uint64_t>(), tot.sum, sel->d_text.bytes());
    if (hipGetLastError() != hipSuccess || hipEventRecord(ev.ev[1], stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
        return device_failure("text formatting failed");
    (void)hipEventElapsedTime(&out->ms, ev.ev[0], ev.ev[1]);
    out->d_text = sel->d_text.bytes();
    out->n_text = tot.sum;
    out->n_records = n_rec;
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_select(nafgpu_decoder *dec, const nafgpu_region *regions, uint64_t n_regions, const nafgpu_select_opts *opts, nafgpu_selection **out,
                  nafgpu_select_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if ((!regions && n_regions) || !out || !res) return decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    SelSource s;
    Failure f = decoder_source(dec, true, &s);
    if (!f.ok()) return decoder_fail(dec, f, err);
    std::unique_ptr<nafgpu_selection> sel;
    f = select(s, regions, n_regions, opts && opts->name_regions, sel);
    if (!f.ok()) return decoder_fail(dec, f, err);
    *res = sel->res;
    *out = sel.release();
    return fail_c(err, Failure());
}

int nafgpu_merge_pairs(nafgpu_decoder *dec, const nafgpu_overlaps *overlaps, nafgpu_selection **out, nafgpu_select_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!overlaps || !out || !res) return decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    SelSource s;
    Failure f = decoder_source(dec, true, &s);
    if (!f.ok()) return decoder_fail(dec, f, err);
    std::unique_ptr<nafgpu_selection> sel;
    f = merge_pairs(s, ovl::view_of(overlaps), sel);
    if (!f.ok()) return decoder_fail(dec, f, err);
    *res = sel->res;
    *out = sel.release();
    return fail_c(err, Failure());
}

int nafgpu_find_records(nafgpu_decoder *dec, const uint8_t *names, uint64_t n_bytes, uint64_t n_names, uint64_t *record_out, nafgpu_error *err) {
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if ((!names && n_bytes) || (!record_out && n_names)) return decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    SelSource s;
    Failure f = decoder_source(dec, false, &s);
    if (f.ok()) f = find_records(s, names, n_bytes, n_names, record_out);
    if (!f.ok()) return decoder_fail(dec, f, err);
    return fail_c(err, Failure());
}

int nafgpu_selection_format(nafgpu_selection *sel, uint64_t line_length, nafgpu_text_result *out) {
    if (!sel || !out) return NAFGPU_E_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    nafgpu_text_result r;
    std::memset(&r, 0, sizeof r);
    Failure f = format(sel, line_length, &r);
    if (!f.ok()) return f.status;
    *out = r;
    return NAFGPU_OK;
}

int nafgpu_selection_copy_to_host(nafgpu_selection *sel, const void *d_ptr, uint64_t n, void *dst) {
    if (!sel || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(sel->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, sel->stream) != hipSuccess || hipStreamSynchronize(sel->stream) != hipSuccess)
        return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

int nafgpu_selection_hash64(nafgpu_selection *sel, const void *d_ptr, uint64_t n, uint64_t first_chunk, uint64_t *out) {
    if (!sel || !out || (n && !d_ptr)) return NAFGPU_E_INVALID_ARG;
    (void)hipSetDevice(sel->device);
    unsigned long long *acc = sel->d_hash.as<unsigned long long>(), v = 0;
    if (hipMemsetAsync(acc, 0, 8, sel->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    launch_hash64(sel->stream, static_cast<const uint8_t *>(d_ptr), n, first_chunk, acc);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&v, acc, 8, hipMemcpyDeviceToHost, sel->stream) != hipSuccess ||
        hipStreamSynchronize(sel->stream) != hipSuccess)
        return NAFGPU_E_DEVICE;
    *out = v;
    return NAFGPU_OK;
}

void nafgpu_selection_free(nafgpu_selection *sel) { delete sel; }

}  // extern "C"
