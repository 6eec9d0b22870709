// encode.cpp -- host front end of the device encoder: literal-only Zstandard sections written by the kernels of
// encode.hip, and the container around them.
//
// One section goes slab by slab (a multiple of 64 blocks, so that slabs end on chunk boundaries and stay independent):
//   input in HBM -> k_enc_hist -> histograms to the host -> plan_block per block (chunks in parallel, the blocks of a
//   chunk in order: a block may reuse the table of the one before) -> offsets, stream records, tables and header bytes to
//   the device -> k_enc_streams + k_enc_scatter -> the slab's piece of the frame back to the host.
// The frame is the one compress_section(data, ., lz = false) writes: plan_block is the same function on both paths.
//
// With LZ (opts.device_lz at compression levels 0 and >= 3) four kernels run in front of the host's decisions:
//   k_enc_lz_match -> k_enc_lz_parse -> k_enc_lz_hist + k_enc_lz_seqbits -> counts of the block and of its literals, the
//   number of sequences and the size of their bitstream to the host -> per block the smaller of plan_block's block and
//   [plan_literals + sequences] -> k_enc_streams over the input and over the literal buffers, k_enc_scatter.
// The container is that of compress_section(data, ., lz = true); the matches are the device matcher's own.
#include "encode.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "device.h"
#include "kernels.h"
#include "plan.h"

namespace nafgpu {
namespace enc {

namespace {

thread_local EncTimes g_last_times;

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("encode: ") + what); }

// What the kernels of one slab need, in host memory.
struct SlabPlan {
    std::vector<EncStream> streams;
    std::vector<EncTable> tables;
    std::vector<EncCopy> copies;
    std::vector<uint8_t> blob;
    uint64_t out_bytes = 0;
    uint32_t max_stream = 0;
    std::vector<EncStream> lit_streams;      // LZ: streams whose symbols lie in the literal buffers
};

struct LzBlockPlan {         // a block with sequences: the literals plan and what stands between the literals and the bitstream
    bool taken = false;
    BlockPlan lits;
    uint32_t n_seq = 0, seq_bytes = 0;
};

// Sections of one call share a stream, the events and the buffers.
class SectionEncoder {
public:
    ~SectionEncoder() {
        for (hipEvent_t e : ev_)
            if (e) (void)hipEventDestroy(e);
        if (stream_) pooled_stream_put(device_, stream_);
    }
    Failure init(int device) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the device encoder runs on the GPU only");
        if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
        if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
        if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
        device_ = device;
        stream_ = pooled_stream_get(device);
        if (!stream_) return device_failure("no stream");
        for (hipEvent_t &e : ev_)
            if (hipEventCreate(&e) != hipSuccess) return device_failure("hipEventCreate failed");
        return Failure();
    }
    hipStream_t stream() const { return stream_; }
    EncTimes times;

    // `src` -> the section's frame, appended to `out`
    // lz: blocks with sequences (a section under 64 bytes is raw blocks either way, as compress_section writes it)
    Failure compress(const uint8_t *src, size_t n, bool src_on_device, unsigned n_threads, bool lz, std::vector<uint8_t> &out) {
        lz = lz && n >= 64;
        size_t slab = size_t(lz ? 128 : 512) << 20;                   // LZ: 14 bytes of scratch per input byte
        if (const char *e = hook_env("NAFGPU_ENC_SLAB_MIB")) {        // tests: several slabs over a small section
            const size_t mib = std::max<size_t>(1, std::strtoull(e, nullptr, 10));
            slab = ((mib + 7) / 8 * 8) << 20;                          // whole chunks of 64 blocks
        }
        if (n_threads == 0) n_threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        size_t off = 0;
        do {
            const size_t sn = std::min(slab, n - off);
            Failure f = compress_slab(src + off, sn, src_on_device, off == 0, off + sn == n, n_threads, lz, out);
            if (!f.ok()) return f;
            off += sn;
        } while (off < n);
        return Failure();
    }

private:
    Failure compress_slab(const uint8_t *src, size_t sn, bool src_on_device, bool first, bool last, unsigned n_threads, bool lz,
                          std::vector<uint8_t> &out) {
        const uint32_t nb = static_cast<uint32_t>(std::max<size_t>(1, (sn + kBlockMax - 1) / kBlockMax));
        const uint8_t *d_in = src;
        if (!src_on_device) {
            if (!d_in_.alloc(sn)) return device_failure("out of device memory");
            if (sn && !upload_staged(d_in_.bytes(), src, sn, stream_)) return device_failure("host-to-device copy failed");
            d_in = d_in_.bytes();
        }
        const uint32_t status0[4] = {0, 0, 0, 0};
        if (!d_status_.alloc(sizeof status0) || !d_hist_.alloc(size_t(nb) * 4096)) return device_failure("out of device memory");
        if (lz) {
            const size_t padded = size_t(nb) * kBlockMax;
            if (!d_match_.alloc_items(padded, 4) || !d_exits_.alloc_items(padded, 4) || !d_lits_.alloc(padded) || !d_bits_.alloc(padded) ||
                !d_seqs_.alloc_items(size_t(nb) * kLzMaxSeq, sizeof(LzSeq)) || !d_info_.alloc_items(nb, sizeof(LzBlockInfo)) ||
                !d_lit_hist_.alloc(size_t(nb) * 4096))
                return device_failure("out of device memory");
            if (!d_seq_tables_.size()) {
                LzSeqTables t;
                lz_seq_tables(&t);
                if (!d_seq_tables_.upload(&t, sizeof t, stream_) || hipStreamSynchronize(stream_) != hipSuccess)
                    return device_failure("out of device memory");
            }
            lit_hist_.resize(size_t(nb) * 1024);
            info_.resize(nb);
        }
        hist_.resize(size_t(nb) * 1024);
        bool ok = hipMemcpyAsync(d_status_.bytes(), status0, sizeof status0, hipMemcpyHostToDevice, stream_) == hipSuccess;
        ok = ok && hipEventRecord(ev_[0], stream_) == hipSuccess;
        if (sn >= 64) launch_enc_hist(stream_, d_in, sn, nb, d_hist_.as<uint32_t>());
        if (lz) {
            launch_enc_lz_match(stream_, d_in, sn, nb, d_match_.as<uint32_t>());
            launch_enc_lz_parse(stream_, d_in, sn, nb, d_match_.as<uint32_t>(), d_exits_.as<uint32_t>(), d_info_.as<LzBlockInfo>(),
                                d_seqs_.as<LzSeq>(), d_lits_.bytes());
            launch_enc_lz_hist(stream_, d_lits_.bytes(), d_info_.as<LzBlockInfo>(), nb, d_lit_hist_.as<uint32_t>());
        }
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev_[1], stream_) == hipSuccess;
        if (lz) {
            ok = ok && hipEventRecord(ev_[4], stream_) == hipSuccess;
            launch_enc_lz_seqbits(stream_, d_seqs_.as<LzSeq>(), d_seq_tables_.as<LzSeqTables>(), nb, d_info_.as<LzBlockInfo>(), d_bits_.bytes());
            ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev_[5], stream_) == hipSuccess;
            ok = ok && hipMemcpyAsync(lit_hist_.data(), d_lit_hist_.bytes(), size_t(nb) * 4096, hipMemcpyDeviceToHost, stream_) == hipSuccess;
            ok = ok && hipMemcpyAsync(info_.data(), d_info_.bytes(), size_t(nb) * sizeof(LzBlockInfo), hipMemcpyDeviceToHost, stream_) == hipSuccess;
        }
        if (sn >= 64) ok = ok && hipMemcpyAsync(hist_.data(), d_hist_.bytes(), size_t(nb) * 4096, hipMemcpyDeviceToHost, stream_) == hipSuccess;
        ok = ok && hipStreamSynchronize(stream_) == hipSuccess;
        if (!ok) return device_failure("the histogram pass failed");

        const double t0 = now_ms();
        SlabPlan sp;
        plan_slab(sn, nb, first, last, n_threads, lz, &sp);
        times.plan += now_ms() - t0;

        if (!d_out_.alloc(sp.out_bytes) || !d_streams_.upload(sp.streams.data(), sp.streams.size() * sizeof(EncStream), stream_) ||
            !d_tables_.upload(sp.tables.data(), sp.tables.size() * sizeof(EncTable), stream_) ||
            !d_copies_.upload(sp.copies.data(), sp.copies.size() * sizeof(EncCopy), stream_) ||
            !d_blob_.upload(sp.blob.data(), sp.blob.size(), stream_) ||
            (lz && !d_lit_streams_.upload(sp.lit_streams.data(), sp.lit_streams.size() * sizeof(EncStream), stream_)))
            return device_failure("out of device memory");
        ok = hipEventRecord(ev_[2], stream_) == hipSuccess;
        launch_enc_streams(stream_, d_in, d_streams_.as<EncStream>(), static_cast<uint32_t>(sp.streams.size()), d_tables_.as<EncTable>(),
                           sp.max_stream, d_out_.bytes(), d_status_.as<uint32_t>());
        if (lz) {
            launch_enc_streams(stream_, d_lits_.bytes(), d_lit_streams_.as<EncStream>(), static_cast<uint32_t>(sp.lit_streams.size()),
                               d_tables_.as<EncTable>(), sp.max_stream, d_out_.bytes(), d_status_.as<uint32_t>());
            launch_enc_scatter_lz(stream_, d_in, d_blob_.bytes(), d_lits_.bytes(), d_bits_.bytes(), d_copies_.as<EncCopy>(),
                                  static_cast<uint32_t>(sp.copies.size()), d_out_.bytes());
        } else {
            launch_enc_scatter(stream_, d_in, d_blob_.bytes(), d_copies_.as<EncCopy>(), static_cast<uint32_t>(sp.copies.size()), d_out_.bytes());
        }
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev_[3], stream_) == hipSuccess;
        uint32_t status[4] = {0, 0, 0, 0};
        const size_t at = out.size();
        out.resize(at + sp.out_bytes);
        ok = ok && hipMemcpyAsync(status, d_status_.bytes(), sizeof status, hipMemcpyDeviceToHost, stream_) == hipSuccess;
        ok = ok && hipMemcpyAsync(out.data() + at, d_out_.bytes(), sp.out_bytes, hipMemcpyDeviceToHost, stream_) == hipSuccess;
        ok = ok && hipStreamSynchronize(stream_) == hipSuccess;
        if (!ok) {
            out.resize(at);
            return device_failure("the stream pass failed");
        }
        if (status[0] & kEncStStreamSize) {
            out.resize(at);
            return device_failure("a stream did not have its planned size");
        }
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, ev_[0], ev_[1]) == hipSuccess && hipEventElapsedTime(&b, ev_[2], ev_[3]) == hipSuccess)
            times.hist += a, times.streams += b;
        if (lz && hipEventElapsedTime(&a, ev_[4], ev_[5]) == hipSuccess) times.streams += a;
        return Failure();
    }

    void plan_slab(size_t sn, uint32_t nb, bool first, bool last, unsigned n_threads, bool lz, SlabPlan *sp) {
        std::vector<BlockPlan> plans(nb);
        std::vector<LzBlockPlan> lz_plans(lz ? nb : 0);
        const uint32_t n_chunks = static_cast<uint32_t>((nb + kChunkBlocks - 1) / kChunkBlocks);
        std::atomic<uint32_t> next{0};
        auto worker = [&]() {
            for (;;) {
                const uint32_t c = next.fetch_add(1);
                if (c >= n_chunks) break;
                HufCode prev{};
                for (uint32_t b = c * kChunkBlocks; b < std::min<uint64_t>(nb, (c + 1) * kChunkBlocks); b++) {
                    const size_t p0 = size_t(b) * kBlockMax, bn = std::min<size_t>(kBlockMax, sn - p0);
                    const auto counts = reinterpret_cast<const uint32_t(*)[256]>(hist_.data() + size_t(b) * 1024);
                    if (!lz || !info_[b].n_seq || info_[b].seq_bytes == kLzSeqOverflow) {
                        plan_block(counts, bn, last && b == nb - 1, &prev, &plans[b]);
                        continue;
                    }
                    // with sequences: literals, sequence count, Symbol_Compression_Modes, bitstream -- if that is the smaller block
                    LzBlockPlan &lp = lz_plans[b];
                    lp.n_seq = info_[b].n_seq;
                    lp.seq_bytes = info_[b].seq_bytes;
                    plan_literals(reinterpret_cast<const uint32_t(*)[256]>(lit_hist_.data() + size_t(b) * 1024), info_[b].n_lit, &prev, &lp.lits);
                    const size_t body = lp.lits.total + (lp.n_seq < 128 ? 1 : 2) + 1 + lp.seq_bytes;
                    HufCode prev_plain = prev;
                    plan_block(counts, bn, last && b == nb - 1, &prev_plain, &plans[b]);
                    if (body < plans[b].total - 3) {
                        lp.taken = true;
                        plans[b].total = 3 + body;
                        if (lp.lits.mode == kHufNew) prev = lp.lits.code;
                    } else {
                        prev = prev_plain;
                    }
                }
            }
        };
        n_threads = std::min(n_threads, n_chunks);
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < n_threads; t++) pool.emplace_back(worker);
        worker();
        for (auto &t : pool) t.join();

        uint64_t pos = 0;
        auto from_blob = [&](const uint8_t *p, size_t len) {
            sp->copies.push_back(EncCopy{sp->blob.size(), pos, static_cast<uint32_t>(len), 0});
            sp->blob.insert(sp->blob.end(), p, p + len);
            pos += len;
        };
        // FHD: no content size, no checksum, no dictionary; window 512 KiB, or 1 MiB as compress_section(., lz = true) says it
        const uint8_t frame_head[2] = {0x00, static_cast<uint8_t>(lz ? 0x50 : 0x48)};
        if (first) from_blob(frame_head, 2);
        sp->blob.push_back(0x00);                               // Number_of_Sequences = 0, behind every compressed block
        const uint64_t zero_at = sp->blob.size() - 1;
        auto add_streams = [&](std::vector<EncStream> &list, const BlockPlan &p, uint64_t p0) {
            if (p.mode == kHufNew) {
                EncTable t;
                std::memcpy(t.code, p.code.code, sizeof t.code);
                std::memcpy(t.len, p.code.len, sizeof t.len);
                sp->tables.push_back(t);
            }
            const size_t q = (p.n + 3) / 4;
            for (int k = 0; k < 4; k++) {
                const uint32_t n_sym = static_cast<uint32_t>(k < 3 ? q : p.n - 3 * q);
                list.push_back(EncStream{p0 + k * q, pos, n_sym, p.stream_size[k], static_cast<uint32_t>(sp->tables.size() - 1), 0});
                sp->max_stream = std::max(sp->max_stream, p.stream_size[k]);
                pos += p.stream_size[k];
            }
        };
        for (uint32_t b = 0; b < nb; b++) {
            const BlockPlan &p = plans[b];
            const uint64_t p0 = uint64_t(b) * kBlockMax, end = pos + p.total;
            if (lz && lz_plans[b].taken) {
                const LzBlockPlan &lp = lz_plans[b];
                const uint32_t bh = static_cast<uint32_t>((p.total - 3) << 3) | (2u << 1) | (last && b == nb - 1 ? 1u : 0u);
                const uint8_t bh3[3] = {static_cast<uint8_t>(bh), static_cast<uint8_t>(bh >> 8), static_cast<uint8_t>(bh >> 16)};
                from_blob(bh3, 3);
                from_blob(lp.lits.head.data(), lp.lits.head.size());
                if (lp.lits.mode == kRaw && lp.lits.n) {
                    sp->copies.push_back(EncCopy{p0, pos, static_cast<uint32_t>(lp.lits.n), kCopyLiterals});
                    pos += lp.lits.n;
                } else if (lp.lits.mode == kHufNew || lp.lits.mode == kHufTreeless) {
                    add_streams(sp->lit_streams, lp.lits, p0);
                }
                // Number_of_Sequences (one byte under 128, else two; a block holds fewer than 0x7F00), then "predefined x 3"
                uint8_t sh[3];
                size_t shn = 0;
                if (lp.n_seq < 128) {
                    sh[shn++] = static_cast<uint8_t>(lp.n_seq);
                } else {
                    sh[shn++] = static_cast<uint8_t>((lp.n_seq >> 8) + 128);
                    sh[shn++] = static_cast<uint8_t>(lp.n_seq & 0xFF);
                }
                sh[shn++] = 0x00;
                from_blob(sh, shn);
                sp->copies.push_back(EncCopy{p0, pos, lp.seq_bytes, kCopySeqBits});
                pos = end;
                continue;
            }
            from_blob(p.head.data(), p.head.size());
            if (p.mode == kRaw && p.n) {
                sp->copies.push_back(EncCopy{p0, pos, static_cast<uint32_t>(p.n), 1});
            } else if (p.mode == kHufNew || p.mode == kHufTreeless) {
                add_streams(sp->streams, p, p0);
                sp->copies.push_back(EncCopy{zero_at, pos, 1, 0});
            }
            pos = end;
        }
        sp->out_bytes = pos;
    }

    int device_ = -1;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<uint32_t> hist_, lit_hist_;
    std::vector<LzBlockInfo> info_;
    DevBuf d_in_, d_hist_, d_out_, d_streams_, d_tables_, d_copies_, d_blob_, d_status_;
    DevBuf d_match_, d_exits_, d_lits_, d_bits_, d_seqs_, d_info_, d_lit_hist_, d_lit_streams_, d_seq_tables_;   // LZ
};

}  // namespace

Failure compress_section_device(const uint8_t *src, size_t n, bool src_on_device, int device, unsigned n_threads, bool lz,
                                std::vector<uint8_t> &out, EncTimes *times) {
    const double t0 = now_ms();
    SectionEncoder se;
    Failure f = se.init(device);
    if (f.ok()) f = se.compress(src, n, src_on_device, n_threads, lz, out);
    se.times.total = now_ms() - t0;
    g_last_times = se.times;
    if (times) *times = se.times;
    return f;
}

namespace {

Failure encode_device(const nafgpu_encode_source *src, const nafgpu_encoder_opts *opts, int device, uint64_t line_length, std::vector<uint8_t> &o) {
    if (opts->sequence_type > 3) return Failure::make(NAFGPU_E_INVALID_ARG, "invalid encoder options");
    if (!mask_opts_ok(*opts))
        return Failure::make(NAFGPU_E_INVALID_ARG, "mask needs a nucleotide sequence: sequence set, sequence_type dna or rna");
    const bool lz = opts->compression_level != 1 && opts->compression_level != 2;
    if (lz && !opts->device_lz)
        return Failure::make(NAFGPU_E_INVALID_ARG, "the device encoder writes literal-only blocks: compression_level 1 or 2");
    if ((opts->id != 0) != (src->d_ids != nullptr) || (opts->comment != 0) != (src->d_comments != nullptr) ||
        (opts->sequence != 0) != (src->d_sequence != nullptr) || (opts->quality != 0) != (src->d_quality != nullptr))
        return Failure::make(NAFGPU_E_INVALID_ARG, "the source's fields and the options disagree");
    if (src->n_records && !src->d_record_end) return Failure::make(NAFGPU_E_INVALID_ARG, "records without record ends");
    if (opts->sequence && opts->quality && src->n_bases != src->n_quality)
        return Failure::make(NAFGPU_E_INVALID_LENGTH, "inconsistent sequence length");
    const double t0 = now_ms();
    SectionEncoder se;
    Failure f = se.init(device);
    if (!f.ok()) return f;
    hipStream_t stream = se.stream();
    const uint64_t n_rec = src->n_records;
    const bool nuc = opts->sequence_type <= 1;

    // ---- every check first, as nafgpu_encoder_push does record by record
    DevBuf d_tmp, d_totals, d_status, d_dummy, d_counts, d_offsets, d_words, d_packed, d_mask;
    const uint32_t status0[4] = {0, 0, 0, 0};
    if (!d_tmp.alloc(scan_tmp_bytes(std::max<uint64_t>({n_rec, src->n_ids_bytes, src->n_comments_bytes, 1}))) ||
        !d_totals.alloc(sizeof(ScanTotals)) || !d_status.alloc(sizeof status0) || !d_dummy.alloc(16))
        return device_failure("out of device memory");
    auto reset_status = [&]() { return hipMemcpyAsync(d_status.bytes(), status0, sizeof status0, hipMemcpyHostToDevice, stream) == hipSuccess; };
    if (n_rec && (opts->sequence || opts->quality)) {            // the last record ends where the letters end
        uint64_t last_end = 0;
        if (hipMemcpyAsync(&last_end, src->d_record_end + (n_rec - 1), 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return device_failure("device-to-host copy failed");
        if (last_end != (opts->sequence ? src->n_bases : src->n_quality)) return Failure::make(NAFGPU_E_INVALID_LENGTH, "inconsistent sequence length");
    } else if (!n_rec && ((opts->sequence && src->n_bases) || (opts->quality && src->n_quality))) {
        return Failure::make(NAFGPU_E_INVALID_LENGTH, "inconsistent sequence length");
    }
    auto count_strings = [&](const uint8_t *p, uint64_t n, const char *field) -> Failure {   // one NUL-terminated string per record
        ScanTotals tot{0, 0};
        uint8_t last_byte = 0;
        if (!reset_status()) return device_failure("host-to-device copy failed");
        launch_scan_nul(stream, p, n, d_dummy.as<uint64_t>(), 0, d_tmp.bytes(), d_totals.as<ScanTotals>(), d_status.as<uint32_t>());
        bool ok = hipGetLastError() == hipSuccess &&
                  hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess;
        if (n) ok = ok && hipMemcpyAsync(&last_byte, p + n - 1, 1, hipMemcpyDeviceToHost, stream) == hipSuccess;
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return device_failure("counting strings failed");
        if (tot.count != n_rec || last_byte != 0) return Failure::make(NAFGPU_E_MISSING_FIELD, std::string("missing record field: \"") + field + "\"");
        return Failure();
    };
    if (opts->id && !(f = count_strings(src->d_ids, src->n_ids_bytes, "id")).ok()) return f;
    if (opts->comment && !(f = count_strings(src->d_comments, src->n_comments_bytes, "comment")).ok()) return f;
    if (opts->sequence && nuc) {
        uint32_t status[4] = {0, 0, 0, 0};
        if (!d_packed.alloc((src->n_bases + 1) / 2 + 16) || !reset_status()) return device_failure("out of device memory");
        launch_enc_pack(stream, src->d_sequence, src->n_bases, opts->sequence_type, opts->mask != 0, d_packed.bytes(), d_status.as<uint32_t>());
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(status, d_status.bytes(), sizeof status, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return device_failure("packing the sequence failed");
        if (status[0] & kEncStBadLetter) {
            const unsigned long long at = ~((static_cast<unsigned long long>(status[3]) << 32) | status[2]);
            return Failure::make(NAFGPU_E_INVALID_SEQUENCE, "invalid character in sequence (letter " + std::to_string(at) + ")");
        }
    }
    // ---- the Length section: words per record, their offsets (k_scan_*), the words
    uint64_t n_words = 0;
    if (n_rec && (opts->sequence || opts->quality)) {
        ScanTotals tot{0, 0};
        if (!d_counts.alloc_items(n_rec, 8) || !d_offsets.alloc_items(n_rec, 8) || !reset_status()) return device_failure("out of device memory");
        launch_enc_length_counts(stream, src->d_record_end, n_rec, d_counts.as<uint64_t>());
        launch_scan_excl_u64(stream, d_counts.as<uint64_t>(), n_rec, d_offsets.as<uint64_t>(), d_tmp.bytes(), d_totals.as<ScanTotals>(),
                             d_status.as<uint32_t>());
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return device_failure("the length pass failed");
        n_words = tot.sum;
        if (!d_words.alloc_items(n_words, 4)) return device_failure("out of device memory");
        launch_enc_length_words(stream, src->d_record_end, n_rec, d_offsets.as<uint64_t>(), d_words.as<uint32_t>());
        if (hipGetLastError() != hipSuccess) return device_failure("the length pass failed");
    }
    // ---- the Mask section: edges per tile, their offsets, the edge positions; bytes per unit, their offsets, the bytes.
    // Two round trips: the host allocates by the number of edges, then by the number of bytes.
    uint64_t n_mask = 0;
    if (opts->mask && src->n_bases) {
        const uint64_t n = src->n_bases, n_tiles = enc_mask_tiles(n);
        DevBuf d_tile, d_mtmp, d_ends, d_sizes;                 // gone before the sections are compressed
        ScanTotals tot{0, 0};
        auto totals = [&]() {
            return hipGetLastError() == hipSuccess && hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
                   hipStreamSynchronize(stream) == hipSuccess;
        };
        if (!d_tile.alloc_items(n_tiles, 8) || !d_mtmp.alloc(scan_tmp_bytes(n_tiles)) || !reset_status()) return device_failure("out of device memory");
        launch_enc_mask_count(stream, src->d_sequence, n, d_tile.as<uint64_t>());
        launch_scan_excl_u64(stream, d_tile.as<uint64_t>(), n_tiles, d_tile.as<uint64_t>(), d_mtmp.bytes(), d_totals.as<ScanTotals>(),
                             d_status.as<uint32_t>());        // in place: a lane of k_scan_emit has read its items before it writes them
        if (!totals()) return device_failure("the mask pass failed");
        const uint64_t n_edges = tot.sum, n_units = n_edges + 1;
        if (!d_ends.alloc_items(n_units, 8) || !d_sizes.alloc_items(n_units, 8) || !d_mtmp.alloc(scan_tmp_bytes(n_units)))
            return device_failure("out of device memory");
        launch_enc_mask_edges(stream, src->d_sequence, n, d_tile.as<uint64_t>(), n_edges, d_ends.as<uint64_t>());
        launch_enc_mask_sizes(stream, d_ends.as<uint64_t>(), n_units, d_sizes.as<uint64_t>());
        launch_scan_excl_u64(stream, d_sizes.as<uint64_t>(), n_units, d_sizes.as<uint64_t>(), d_mtmp.bytes(), d_totals.as<ScanTotals>(),
                             d_status.as<uint32_t>());
        if (!totals()) return device_failure("the mask pass failed");
        n_mask = tot.sum;
        if (!d_mask.alloc(n_mask)) return device_failure("out of device memory");
        if (hipMemsetAsync(d_mask.bytes(), 0xFF, n_mask, stream) != hipSuccess) return device_failure("the mask pass failed");
        launch_enc_mask_bytes(stream, d_ends.as<uint64_t>(), n_units, d_sizes.as<uint64_t>(), n_mask, d_mask.bytes());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return device_failure("the mask pass failed");
    }
    // ---- the container (Encoder::write, mod.rs:325-384)
    put_archive_head(o, *opts, n_rec, line_length);
    auto block = [&](const uint8_t *d_data, uint64_t n, uint64_t original) {
        if (!f.ok()) return;
        std::vector<uint8_t> frame;
        f = se.compress(d_data, n, true, opts->threads, lz, frame);
        if (!f.ok()) return;
        put_varint(o, original);
        put_varint(o, frame.size());
        o.insert(o.end(), frame.begin(), frame.end());
    };
    if (opts->id) block(src->d_ids, src->n_ids_bytes, src->n_ids_bytes);
    if (opts->comment) block(src->d_comments, src->n_comments_bytes, src->n_comments_bytes);
    block(d_words.bytes(), n_words * 4, n_words * 4);
    if (opts->mask) block(d_mask.bytes(), n_mask, n_mask);
    if (opts->sequence) {
        if (nuc) block(d_packed.bytes(), (src->n_bases + 1) / 2, src->n_bases);      // letters, not bytes
        else block(src->d_sequence, src->n_bases, src->n_bases);
    }
    if (opts->quality) block(src->d_quality, src->n_quality, src->n_quality);
    se.times.total = now_ms() - t0;
    g_last_times = se.times;
    return f;
}

}  // namespace

Failure encode_device_archive(const nafgpu_encode_source *src, const nafgpu_encoder_opts *opts, int device, uint64_t line_length,
                              std::vector<uint8_t> &archive) {
    return encode_device(src, opts, device, line_length, archive);
}

}  // namespace enc
}  // namespace nafgpu

using namespace nafgpu;
using namespace nafgpu::enc;

extern "C" {

static int zstd_compress_c(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced, int device, bool lz, nafgpu_error *err) {
    if ((!src && n) || (!dst && cap) || !produced || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "invalid argument"));
    std::vector<uint8_t> frame;
    Failure f = compress_section_device(src, n, false, device, 0, lz, frame, nullptr);
    if (!f.ok()) return fail_c(err, f);
    *produced = frame.size();
    if (frame.size() > cap) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "destination buffer too small"));
    if (!frame.empty()) std::memcpy(dst, frame.data(), frame.size());
    return fail_c(err, Failure());
}

int nafgpu_zstd_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced, int device, nafgpu_error *err) {
    return zstd_compress_c(src, n, dst, cap, produced, device, false, err);
}

int nafgpu_zstd_compress_lz(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced, int device, nafgpu_error *err) {
    return zstd_compress_c(src, n, dst, cap, produced, device, true, err);
}

int nafgpu_encode_device(const nafgpu_encode_source *src, const nafgpu_encoder_opts *opts, int device, uint8_t **bytes, uint64_t *n,
                         nafgpu_error *err) {
    if (!src || !opts || !bytes || !n || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    *bytes = nullptr;
    *n = 0;
    std::vector<uint8_t> archive;
    Failure f = encode_device(src, opts, device, kDefaultLineLength, archive);
    if (!f.ok()) return fail_c(err, f);
    uint8_t *p = static_cast<uint8_t *>(std::malloc(archive.size() ? archive.size() : 1));
    if (!p) return fail_c(err, Failure::make(NAFGPU_E_IO, "out of memory"));
    std::memcpy(p, archive.data(), archive.size());
    *bytes = p;
    *n = archive.size();
    return fail_c(err, Failure());
}

void nafgpu_encode_free(uint8_t *bytes) { std::free(bytes); }

void nafgpu_encode_last_times(double *hist_ms, double *streams_ms, double *plan_ms, double *total_ms) {
    if (hist_ms) *hist_ms = g_last_times.hist;
    if (streams_ms) *streams_ms = g_last_times.streams;
    if (plan_ms) *plan_ms = g_last_times.plan;
    if (total_ms) *total_ms = g_last_times.total;
}

}  // extern "C"
