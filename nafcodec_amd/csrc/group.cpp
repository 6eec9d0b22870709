// group.cpp -- host side of nafgpu_group / nafgpu_group_decoder and the owner of the groups' buffers.  The kernels are in
// group.hip; the rules in include/nafgpu.h.
//
// Round trips: one per table round (the status words and the number of records that stay; one round unless hashes collided),
// one for the number of groups, by which the two group tables are allocated, and one for the largest group.  Beside the
// outputs: two hashes, a candidate, a flag word and a byte per record, and the table of at least two slots per record.
#include "group.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "device.h"
#include "select.h"
#include "summary.h"

using namespace nafgpu;
using namespace nafgpu::grp;

struct nafgpu_groups {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf d_representative, d_group_of, d_strand, d_group_first, d_group_size;
    nafgpu_group_result res{};
    ~nafgpu_groups() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            pooled_stream_put(device, stream);
        }
    }
};

namespace nafgpu {
namespace grp {

void group_tables(bool nucleotide, GroupTables *out) {
    for (int b = 0; b < 256; b++) out->canon[b] = out->comp[b] = static_cast<uint8_t>(b);
    if (!nucleotide) return;
    for (const char *p = "ACGTURYKMSWBDHVN"; *p; p++) {
        const uint8_t upper = static_cast<uint8_t>(*p == 'U' ? 'T' : *p);
        out->canon[static_cast<uint8_t>(*p)] = out->canon[static_cast<uint8_t>(*p) | 0x20] = upper;
    }
    // the format's 4-bit codes with their bits reversed, over the canonical letters (S, W and N are their own complements)
    const char *pairs = "ATCGRYKMBVDH";
    for (int i = 0; pairs[i]; i += 2) {
        out->comp[static_cast<uint8_t>(pairs[i])] = static_cast<uint8_t>(pairs[i + 1]);
        out->comp[static_cast<uint8_t>(pairs[i + 1])] = static_cast<uint8_t>(pairs[i]);
    }
}

}  // namespace grp
}  // namespace nafgpu

namespace {

Failure device_failure(const char *what) { return Failure::make(NAFGPU_E_DEVICE, std::string("group: ") + what); }

// a failure behind work that was enqueued: the stream is drained first, so that the buffers the work uses are idle when
// they are released
Failure drained_failure(hipStream_t stream, const char *what) {
    (void)hipStreamSynchronize(stream);
    return device_failure(what);
}

struct Events {
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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
Failure group(const nafgpu_encode_source &src, const nafgpu_group_opts &opts, int device, bool eof_beyond, std::unique_ptr<nafgpu_groups> &out) {
    auto refuse = [](const std::string &what) { return Failure::make(NAFGPU_E_INVALID_ARG, "group: " + what); };
    if (!src.d_sequence) return refuse("the sequence field is needed");
    if (src.n_records && !src.d_record_end) return refuse("records without their end table");
    if (opts.alphabet > 1) return refuse("alphabet " + std::to_string(opts.alphabet) + " (0 nucleotide, 1 bytes)");
    if (opts.alphabet == 1 && opts.both_strands) return refuse("both_strands needs the nucleotide alphabet");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return Failure::make(NAFGPU_E_DEVICE, "no HIP device available: the grouping runs on the GPU only");
    if (device >= count) return Failure::make(NAFGPU_E_INVALID_ARG, "no such device");
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return device_failure("hipSetDevice failed");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return device_failure("hipGetDevice failed");
    std::unique_ptr<nafgpu_groups> groups(new nafgpu_groups);
    groups->device = device;
    groups->stream = pooled_stream_get(device);
    if (!groups->stream) return device_failure("no stream");
    hipStream_t stream = groups->stream;
    Events ev;
    if (!ev.create()) return device_failure("hipEventCreate failed");

    const bool both = opts.both_strands != 0;
    const uint64_t n_section = src.n_bases, n_rec = src.n_records;
    nafgpu_group_result &r = groups->res;
    std::memset(&r, 0, sizeof r);
    r.n_bases = n_section;
    // the outputs are never empty, so that an empty table still has an address
    if (!groups->d_representative.alloc_items(std::max<uint64_t>(n_rec, 1), 8) || !groups->d_group_of.alloc_items(n_rec + 1, 8) ||
        (both && !groups->d_strand.alloc(std::max<uint64_t>(n_rec, 1))))
        return device_failure("out of device memory");
    uint64_t *representative = groups->d_representative.as<uint64_t>(), *group_of = groups->d_group_of.as<uint64_t>();
    uint8_t *strand = both ? groups->d_strand.bytes() : nullptr;
    r.d_representative = representative;
    r.d_group_of = group_of;
    r.d_strand = strand;
    if (!n_rec) {
        if (!groups->d_group_first.alloc(8) || !groups->d_group_size.alloc(8)) return device_failure("out of device memory");
        r.d_group_first = groups->d_group_first.as<uint64_t>();
        r.d_group_size = groups->d_group_size.as<uint64_t>();
        out = std::move(groups);
        return Failure();
    }

    uint64_t hash_mask = ~0ull;
    if (const char *e = hook_env("NAFGPU_GRP_HASH_BITS")) {   // tests: hashes that collide, so that the rounds are reached
        const unsigned long bits = std::strtoul(e, nullptr, 10);
        if (bits < 64) hash_mask = (1ull << bits) - 1;
    }
    uint64_t slots = 1024;
    while (slots < 2 * n_rec) slots <<= 1;
    GroupTables tables;
    group_tables(opts.alphabet == 0, &tables);
    uint32_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long words[2] = {0, 0};                    // [0]: the records a round leaves; [1]: the largest group
    ScanTotals tot{0, 0};
    DevBuf d_tables, d_status, d_hf, d_hr, d_cand, d_flags, d_active, d_table, d_words, d_scan_tmp, d_totals;
    if (!d_tables.alloc(sizeof tables) || !d_status.alloc(sizeof status) || !d_hf.alloc_items(n_rec, 8) || (both && !d_hr.alloc_items(n_rec, 8)) ||
        !d_cand.alloc_items(n_rec, 8) || !d_flags.alloc_items(n_rec, 4) || !d_active.alloc(n_rec) || !d_table.alloc_items(slots, 8) ||
        !d_words.alloc(sizeof words) || !d_scan_tmp.alloc(scan_tmp_bytes(n_rec + 1)) || !d_totals.alloc(sizeof tot))
        return device_failure("out of device memory");
    uint32_t *d_st = d_status.as<uint32_t>();
    unsigned long long *hf = d_hf.as<unsigned long long>(), *hr = both ? d_hr.as<unsigned long long>() : nullptr;
    unsigned long long *d_w = d_words.as<unsigned long long>();
    const GroupTables *dt = d_tables.as<GroupTables>();
    bool ok = hipEventRecord(ev.ev[0], stream) == hipSuccess &&
              hipMemcpyAsync(d_tables.bytes(), &tables, sizeof tables, hipMemcpyHostToDevice, stream) == hipSuccess &&
              hipMemsetAsync(d_st, 0, sizeof status, stream) == hipSuccess && hipMemsetAsync(hf, 0, n_rec * 8, stream) == hipSuccess &&
              (!both || hipMemsetAsync(hr, 0, n_rec * 8, stream) == hipSuccess) && hipMemsetAsync(d_active.bytes(), 1, n_rec, stream) == hipSuccess &&
              hipMemsetAsync(d_totals.bytes(), 0, sizeof tot, stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "host-to-device copy failed");
    // (k_sum_check is the check this needs, word for word: it is used as it is)
    sum::launch_sum_check(stream, src.d_record_end, n_rec, n_section, d_st);
    launch_grp_hash(stream, src.d_sequence, n_section, src.d_record_end, n_rec, dt, hf, hr, d_st);
    if (hash_mask != ~0ull) launch_grp_cut(stream, hf, hr, n_rec, hash_mask);
    ok = hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[1], stream) == hipSuccess;

    float ms_table = 0, ms_verify = 0;
    uint32_t rounds = 0;
    for (uint64_t left = n_rec; ok && left;) {
        ok =hipMemsetAsync(d_table.bytes(), 0, slots * 8, stream) == hipSuccess && hipMemsetAsync(d_w, 0, sizeof words, stream) == hipSuccess;
        if (!ok) break;
        launch_grp_table(stream, src.d_record_end, hf, hr, d_active.bytes(), n_rec, d_table.as<unsigned long long>(), slots, d_cand.as<uint64_t>(),
                         d_flags.as<uint32_t>());
        ok = hipEventRecord(ev.ev[2], stream) == hipSuccess;
        launch_grp_verify(stream, src.d_sequence, n_section, src.d_record_end, n_rec, dt, d_cand.as<uint64_t>(), d_active.bytes(), d_flags.as<uint32_t>(), d_st);
        ok = ok && hipEventRecord(ev.ev[3], stream) == hipSuccess;
        launch_grp_settle(stream, d_cand.as<uint64_t>(), d_flags.as<uint32_t>(), d_active.bytes(), n_rec, representative, strand, d_w);
        ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[4], stream) == hipSuccess &&
             hipMemcpyAsync(status, d_st, sizeof status, hipMemcpyDeviceToHost, stream) == hipSuccess &&
             hipMemcpyAsync(words, d_w, sizeof words, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        if (!ok) break;
        if (status[0] & (sum::kSumStDecreasing | sum::kSumStBeyond)) {
            const uint64_t down = status[0] & sum::kSumStDecreasing ? complement_at(status, 2) : UINT64_MAX;
            const uint64_t beyond = status[0] & sum::kSumStBeyond ? complement_at(status, 4) : UINT64_MAX;
            if (down <= beyond) return Failure::make(NAFGPU_E_INVALID_LENGTH, "group: the end of record " + std::to_string(down) + " lies below the end in front of it");
            const std::string what = "record " + std::to_string(beyond) + " ends beyond the " + std::to_string(n_section) + " letters of the section";
            return eof_beyond ? Failure::io(NAFGPU_IO_UNEXPECTED_EOF, what) : Failure::make(NAFGPU_E_INVALID_LENGTH, "group: " + what);
        }
        float a = 0, b = 0, c = 0;
        if (!rounds && hipEventElapsedTime(&a, ev.ev[1], ev.ev[2]) == hipSuccess) ms_table += a;
        if (hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]) == hipSuccess) ms_verify += b;
        if (hipEventElapsedTime(&c, ev.ev[3], ev.ev[4]) == hipSuccess) ms_table += c;
        rounds++;
        if (words[0] >= left) return device_failure("a table round settled no record");   // (every round settles the lowest record of a key)
        left = words[0];
    }
    if (!ok) return drained_failure(stream, "the table rounds failed");

    // ---- the groups: a flag per record, its exclusive sums in place (the scan that compacts search's hits), the two tables
    launch_grp_flag(stream, representative, n_rec, group_of);
    launch_scan_excl_u64(stream, group_of, n_rec + 1, group_of, d_scan_tmp.bytes(), d_totals.as<ScanTotals>(), d_st);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&tot, d_totals.bytes(), sizeof tot, hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the group count failed");
    const uint64_t n_groups = tot.sum;
    if (!n_groups || n_groups > n_rec) return device_failure("the group count is out of range");
    if (!groups->d_group_first.alloc_items(n_groups, 8) || !groups->d_group_size.alloc_items(n_groups, 8)) return device_failure("out of device memory");
    unsigned long long *group_size = groups->d_group_size.as<unsigned long long>();
    ok = hipMemsetAsync(group_size, 0, n_groups * 8, stream) == hipSuccess;
    launch_grp_fill(stream, representative, n_rec, group_of, groups->d_group_first.as<uint64_t>(), group_size);
    launch_grp_largest(stream, group_size, n_groups, d_w + 1);
    ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(ev.ev[5], stream) == hipSuccess &&
         hipMemcpyAsync(words, d_w, sizeof words, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) return drained_failure(stream, "the group tables failed");
    float ms = 0, ms_hash = 0, ms_groups = 0;
    (void)hipEventElapsedTime(&ms, ev.ev[0], ev.ev[5]);      // (with the read-backs between the rounds)
    if (hook_env("NAFGPU_DEBUG_TIMES") && hipEventElapsedTime(&ms_hash, ev.ev[0], ev.ev[1]) == hipSuccess &&
        hipEventElapsedTime(&ms_groups, ev.ev[4], ev.ev[5]) == hipSuccess)
        std::fprintf(stderr, "[nafgpu] group: hash %.3f ms, table %.3f, verify %.3f, groups %.3f; %u round(s)\n", ms_hash, ms_table, ms_verify, ms_groups, rounds);

    r.d_group_first = groups->d_group_first.as<uint64_t>();
    r.d_group_size = groups->d_group_size.as<uint64_t>();
    r.n_records = n_rec;
    r.n_groups = n_groups;
    r.largest_group = words[1];
    r.rounds = rounds;
    r.ms = ms;
    out = std::move(groups);
    return Failure();
}

}  // namespace

extern "C" {

int nafgpu_group(const nafgpu_encode_source *src, const nafgpu_group_opts *opts, int device, nafgpu_groups **out, nafgpu_group_result *res,
                 nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!src || !opts || !out || !res || device < -1) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    std::unique_ptr<nafgpu_groups> groups;
    const Failure f = group(*src, *opts, device, false, groups);
    if (!f.ok()) return fail_c(err, f);
    *res = groups->res;
    *out = groups.release();
    return fail_c(err, Failure());
}

int nafgpu_group_decoder(nafgpu_decoder *dec, const nafgpu_group_opts *opts, nafgpu_groups **out, nafgpu_group_result *res, nafgpu_error *err) {
    if (out) *out = nullptr;
    if (res) std::memset(res, 0, sizeof *res);
    if (!dec) return fail_c(err, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"));
    if (!out || !res) return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "null argument"), err);
    sel::SelSource s;
    Failure f = sel::decoder_source(dec, true, &s);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    const bool nucleotide = s.sequence_type <= 1;            // dna and rna; protein and text are grouped as bytes
    nafgpu_group_opts o;
    std::memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    else o.alphabet = nucleotide ? 0 : 1;
    if (o.alphabet == 0 && !nucleotide)
        return sel::decoder_fail(dec, Failure::make(NAFGPU_E_INVALID_ARG, "group: the nucleotide alphabet needs a nucleotide archive (dna or rna)"), err);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = s.seq;
    src.n_bases = s.seq ? s.n_seq : 0;
    src.d_record_end = s.rec_end;
    src.n_records = s.rec_end ? s.n_rec : 0;
    std::unique_ptr<nafgpu_groups> groups;
    f = group(src, o, s.device, true, groups);
    if (!f.ok()) return sel::decoder_fail(dec, f, err);
    *res = groups->res;
    *out = groups.release();
    return fail_c(err, Failure());
}

int nafgpu_groups_copy_to_host(nafgpu_groups *g, const void *d_ptr, uint64_t n, void *dst) {
    if (!g || (n && (!d_ptr || !dst))) return NAFGPU_E_INVALID_ARG;
    if (!n) return NAFGPU_OK;
    (void)hipSetDevice(g->device);
    if (hipMemcpyAsync(dst, d_ptr, n, hipMemcpyDeviceToHost, g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess) return NAFGPU_E_DEVICE;
    return NAFGPU_OK;
}

void nafgpu_groups_free(nafgpu_groups *g) { delete g; }

}  // extern "C"
