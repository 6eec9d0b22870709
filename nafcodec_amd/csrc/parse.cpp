// parse.cpp -- host front end of the text parser: FASTA / FASTQ text -> records in HBM (nafgpu_parse_text), and text ->
// archive in one call (nafgpu_encode_text).  The kernels are in parse.hip; the rules in include/nafgpu.h.
//
// Two round trips: the host allocates the outputs by the totals of the count pass, then reads the result of the length
// check.  Beside the text and the outputs: 16 + 5 x 8 bytes per tile of 4096 text bytes (summaries, counts), the scans'
// 16 + 16 bytes per 2048 tiles, and 8 bytes per record (FASTQ: the quality ends).  Nothing has an entry per line.
#include "parse.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "encode.h"
#include "device.h"

using namespace nafgpu;
using namespace nafgpu::parse;

struct nafgpu_parsed {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_text, d_seq, d_qual, d_rec_end, d_ids, d_com, d_hash;
    ~nafgpu_parsed() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("parse: ") + what); }

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

Failure parse_text(const uint8_t *text, uint64_t n, const nafgpu_parse_opts &po, int device, std::unique_ptr<nafgpu_parsed> &out,
                   nafgpu_parse_result *res) {
    if (po.format > 2) return Failure::make(NAFGPU_E_INVALID_ARG, "format: 0 (auto), 1 (FASTA) or 2 (FASTQ)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the text parser runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_parsed> ps(new nafgpu_parsed);
    ps->device = device;
    ps->stream = pooled_stream_get(device);
    if (!ps->stream) return device_failure("no stream");
    hipStream_t stream = ps->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");
    if (!ps->d_hash.alloc(8)) return device_failure("out of device memory");

    // ---- the format, from the first byte
    uint8_t first = 0;
    if (n) {
        if (!po.text_on_device) first = text[0];
        else if (hipMemcpyAsync(&first, text, 1, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
            return device_failure("device-to-host copy failed");
        if (first != '>' && first != '@') return Failure::make(NAFGPU_E_INVALID_ARG, "the text begins with neither '>' nor '@' (byte offset 0)");
        if ((po.format == 1 && first != '>') || (po.format == 2 && first != '@'))
            return Failure::make(NAFGPU_E_INVALID_ARG, po.format == 1 ? "FASTA text does not begin with '>' (byte offset 0)"
                                                                      : "FASTQ text does not begin with '@' (byte offset 0)");
    }
    const bool fastq = n ? first == '@' : po.format == 2;

    const uint8_t *d_text = text;
    if (n && !po.text_on_device) {
        if (!ps->d_text.alloc(n)) return device_failure("out of device memory");
        if (!upload_staged(ps->d_text.bytes(), text, n, stream)) return device_failure("host-to-device copy failed");
        d_text = ps->d_text.bytes();
    }

    // ---- summaries, states, counts, their prefix sums
    const uint64_t n_tiles = parse_tiles(d_text, n);
    ParseTotals tot;
    std::memset(&tot, 0, sizeof tot);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float ms = 0;
    DevBuf d_tiles, d_aggs, d_counts, d_tmp, d_totals, d_status, d_qual_end;
    if (n) {
        if (!d_tiles.alloc_items(n_tiles, sizeof(ParseTile)) || !d_aggs.alloc_items(parse_scan_aggs(n_tiles), sizeof(ParseTile)) || !d_counts.alloc_items(n_tiles, 8 * kParseFields) ||
            !d_tmp.alloc(scan_tmp_bytes(n_tiles)) || !d_totals.alloc(sizeof tot) || !d_status.alloc(sizeof status))
            return device_failure("out of device memory");
        bool ok = hipMemcpyAsync(d_totals.bytes(), &tot, sizeof tot, hipMemcpyHostToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(d_status.bytes(), status, sizeof status, hipMemcpyHostToDevice, stream) == hipSuccess &&
                  hipEventRecord(ev.ev[0], stream) == hipSuccess;
        launch_parse_summary(stream, d_text, n, fastq, d_tiles.as<ParseTile>());
        launch_parse_scan_tiles(stream, d_tiles.as<ParseTile>(), n_tiles, d_aggs.as<ParseTile>());
        launch_parse_count(stream, d_text, n, fastq, d_tiles.as<ParseTile>(), d_counts.as<uint64_t>(), d_totals.as<ParseTotals>(),
                           d_status.as<uint32_t>());
        // The existing scan, once per field and in place (a lane of k_scan_emit has read its items before it writes them):
        // one item per tile, 1 / 4096 of the text, so five passes over it cost less than a sibling kernel would save.
        // (The exclusive mode never touches the status words.)
        for (uint32_t f = 0; f < kParseFields; f++)
            launch_scan_excl_u64(stream, d_counts.as<uint64_t>() + f * n_tiles, n_tiles, d_counts.as<uint64_t>() + f * n_tiles, d_tmp.bytes(),
                                 &d_totals.as<ParseTotals>()->field[f], d_status.as<uint32_t>());
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess &&
             hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
             hipMemcpyAsync(status, d_status.bytes(), sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
             hipStreamSynchronize(stream) == hipSuccess;
        if (!ok) return device_failure("the count pass failed");
        if (status[0] & (kParseStLine | kParseStNul)) {
            const uint64_t line_at = (status[0] & kParseStLine) ? complement_at(status, 2) : ~0ull;
            const uint64_t nul_at = (status[0] & kParseStNul) ? complement_at(status, 4) : ~0ull;
            if (nul_at < line_at)
                return Failure::make(NAFGPU_E_INVALID_ARG, "NUL byte in a header line (byte offset " + std::to_string(nul_at) + ")");
            if (line_at == n)
                return Failure::make(NAFGPU_E_INVALID_ARG,
                                     "FASTQ text: the number of lines is not a multiple of 4 (a line is missing at byte offset " + std::to_string(line_at) + ")");
            return Failure::make(NAFGPU_E_INVALID_ARG, "FASTQ text: a header line without '@' or a third line without '+' (byte offset " +
                                                           std::to_string(line_at) + ")");
        }
    }
    const uint64_t n_rec = tot.field[kOpen].sum, n_seq = tot.field[kSeq].sum, n_qual = tot.field[kQual].sum;
    const uint64_t n_ids = tot.field[kId].sum + (n_rec ? 1 : 0), n_com = tot.field[kCom].sum + (n_rec ? 1 : 0);

    // ---- the outputs (never empty, so that an empty field still has an address), the write pass, the length check
    if (!ps->d_seq.alloc(std::max<uint64_t>(n_seq, 16)) || !ps->d_ids.alloc(std::max<uint64_t>(n_ids, 16)) ||
        !ps->d_com.alloc(std::max<uint64_t>(n_com, 16)) || !ps->d_rec_end.alloc_items(std::max<uint64_t>(n_rec, 2), 8) ||
        (fastq && (!ps->d_qual.alloc(std::max<uint64_t>(n_qual, 16)) || !d_qual_end.alloc_items(std::max<uint64_t>(n_rec, 2), 8))))
        return device_failure("out of device memory");
    if (n) {
        ParseOut o;
        o.seq = ps->d_seq.bytes();  o.n_seq = n_seq;
        o.qual = ps->d_qual.bytes(); o.n_qual = n_qual;
        o.ids = ps->d_ids.bytes();  o.n_ids = n_ids;
        o.com = ps->d_com.bytes();  o.n_com = n_com;
        o.rec_end = ps->d_rec_end.as<uint64_t>(); o.n_rec = n_rec;
        o.qual_end = fastq ? d_qual_end.as<uint64_t>() : nullptr;
        bool ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
        launch_parse_write(stream, d_text, n, fastq, d_tiles.as<ParseTile>(), d_counts.as<uint64_t>(), o);
        if (fastq) launch_parse_qual_check(stream, o.rec_end, o.qual_end, n_rec, d_status.as<uint32_t>());
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[3], stream) == hipSuccess &&
             hipMemcpyAsync(status, d_status.bytes(), sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
             hipStreamSynchronize(stream) == hipSuccess;
        if (!ok) return device_failure("the write pass failed");
        if (status[0] & kParseStQual)
            return Failure::make(NAFGPU_E_INVALID_LENGTH, "inconsistent sequence length: the quality of record " +
                                                              std::to_string(complement_at(status, 6)) + " is not as long as its sequence");
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms = a + b;
    }
    std::memset(res, 0, sizeof *res);
    res->src.d_sequence = ps->d_seq.bytes();
    res->src.n_bases = n_seq;
    res->src.d_quality = fastq ? ps->d_qual.bytes() : nullptr;
    res->src.n_quality = fastq ? n_qual : 0;
    res->src.d_record_end = ps->d_rec_end.as<uint64_t>();
    res->src.n_records = n_rec;
    res->src.d_ids = ps->d_ids.bytes();
    res->src.n_ids_bytes = n_ids;
    res->src.d_comments = ps->d_com.bytes();
    res->src.n_comments_bytes = n_com;
    res->line_length = tot.line_length;
    res->n_text = n;
    res->fastq = fastq ? 1 : 0;
    res->ms = ms;
    out = std::move(ps);
    return Failure();
}

}  // namespace

extern "C" {

void nafgpu_parse_opts_default(nafgpu_parse_opts *opts) {
    if (opts) std::memset(opts, 0, sizeof *opts);
}

int nafgpu_parse_text(const uint8_t *text, uint64_t n, const nafgpu_parse_opts *opts, int device, nafgpu_parsed **out,
                      nafgpu_parse_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if ((!text && n) || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    nafgpu_parse_opts po;
    nafgpu_parse_opts_default(&po);
    if (opts) po = *opts;
    std::unique_ptr<nafgpu_parsed> ps;
    nafgpu_parse_result r;
    Failure f = parse_text(text, n, po, device, ps, &r);
    if (!f.ok()) return fail_c(err, f);
    *res = r;
    *out = ps.release();
    return fail_c(err, Failure());
}

int nafgpu_parse_copy_to_host(nafgpu_parsed *ps, const void *d_ptr, uint64_t n, void *dst) {
    if (!ps || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(ps->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, ps->stream) != hipSuccess || hipStreamSynchronize(ps->stream) != hipSuccess)
        return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

int nafgpu_parse_hash64(nafgpu_parsed *ps, const void *d_ptr, uint64_t n, uint64_t *out) {
    if (!ps || !out || (n && !d_ptr)) return NAFGPU_E_INVALID_ARG;
    (void)hipSetDevice(ps->device);
    unsigned long long *acc = ps->d_hash.as<unsigned long long>(), v = 0;
    if (hipMemsetAsync(acc, 0, 8, ps->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    launch_hash64(ps->stream, static_cast<const uint8_t *>(d_ptr), n, 0, acc);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&v, acc, 8, hipMemcpyDeviceToHost, ps->stream) != hipSuccess ||
        hipStreamSynchronize(ps->stream) != hipSuccess)
        return NAFGPU_E_DEVICE;
    *out = v;
    return NAFGPU_OK;
}

void nafgpu_parse_free(nafgpu_parsed *ps) { delete ps; }

int nafgpu_encode_text(const uint8_t *text, uint64_t n, const nafgpu_parse_opts *popts, const nafgpu_encoder_opts *opts, int keep_line_length,
                       int device, uint8_t **bytes, uint64_t *n_out, nafgpu_error *err) {
    if (bytes) *bytes = nullptr;
    if (n_out) *n_out = 0;
    if ((!text && n) || !opts || !bytes || !n_out || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    // what nafgpu_encode_device refuses whatever the records are: before any work
    if (opts->sequence_type > 3) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "invalid encoder options"));
    if (!enc::mask_opts_ok(*opts))
        return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "mask needs a nucleotide sequence: sequence set, sequence_type dna or rna"));
    if (opts->compression_level != 1 && opts->compression_level != 2 && !opts->device_lz)
        return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "the device encoder writes literal-only blocks: compression_level 1 or 2"));
    nafgpu_parse_opts po;
    nafgpu_parse_opts_default(&po);
    if (popts) po = *popts;
    std::unique_ptr<nafgpu_parsed> ps;
    nafgpu_parse_result r;
    Failure f = parse_text(text, n, po, device, ps, &r);
    if (!f.ok()) return fail_c(err, f);
    if (opts->quality && !r.fastq) return fail_c(err, Failure::make(NAFGPU_E_MISSING_FIELD, "missing record field: \"quality\" (the text is FASTA)"));
    nafgpu_encode_source src = r.src;
    if (!opts->id) src.d_ids = nullptr, src.n_ids_bytes = 0;
    if (!opts->comment) src.d_comments = nullptr, src.n_comments_bytes = 0;
    if (!opts->sequence) src.d_sequence = nullptr, src.n_bases = 0;
    if (!opts->quality) src.d_quality = nullptr, src.n_quality = 0;
    (void)hipStreamSynchronize(ps->stream);
    std::vector<uint8_t> archive;
    f = enc::encode_device_archive(&src, opts, ps->device, keep_line_length ? r.line_length : enc::kDefaultLineLength, archive);
    if (!f.ok()) return fail_c(err, f);
    uint8_t *p = static_cast<uint8_t *>(std::malloc(archive.size() ? archive.size() : 1));
    if (!p) return fail_c(err, Failure::make(NAFGPU_E_IO, "out of memory"));
    std::memcpy(p, archive.data(), archive.size());
    *bytes = p;
    *n_out = archive.size();
    return fail_c(err, Failure());
}

}  // extern "C"
