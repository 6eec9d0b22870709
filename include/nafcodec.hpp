// nafcodec.hpp -- header-only C++17 mirror of the reference's public decode API on top of the
// C-ABI (include/nafgpu.h).  Same names, defaults and error behaviour as
// nafcodec/src/decoder/mod.rs (DecoderBuilder :53-257, Decoder :285-461), data.rs (Record :29-40,
// Header :198-237, Flag(s) :80-189, SequenceType :56-73, FormatVersion :46-50) and error.rs.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nafgpu.h"

namespace nafcodec {

enum class FormatVersion : uint8_t { V1 = 1, V2 = 2 };
enum class SequenceType : uint8_t { Dna = 0, Rna = 1, Protein = 2, Text = 3 };
inline bool is_nucleotide(SequenceType t) { return t == SequenceType::Dna || t == SequenceType::Rna; }

enum class Flag : uint8_t { Quality = 0x1, Sequence = 0x2, Mask = 0x4, Length = 0x8, Comment = 0x10, Id = 0x20, Title = 0x40, Extended = 0x80 };
struct Flags {
    uint8_t bits = 0;
    bool test(Flag f) const { return (bits & static_cast<uint8_t>(f)) != 0; }
    void set(Flag f) { bits |= static_cast<uint8_t>(f); }
    void unset(Flag f) { bits &= static_cast<uint8_t>(~static_cast<uint8_t>(f)); }
    uint8_t as_byte() const { return bits; }
};
inline Flags operator|(Flag a, Flag b) { return Flags{static_cast<uint8_t>(static_cast<uint8_t>(a) | static_cast<uint8_t>(b))}; }
inline Flags operator|(Flags a, Flag b) { return Flags{static_cast<uint8_t>(a.bits | static_cast<uint8_t>(b))}; }

// error.rs:4-11 -- Io / Nom / Utf8 (+ the C-ABI's Panic and Device kinds)
struct Error : std::runtime_error {
    nafgpu_error raw;
    explicit Error(const nafgpu_error &e) : std::runtime_error(e.message), raw(e) {}
    bool is_io() const { return raw.status == NAFGPU_E_IO; }
    bool is_unexpected_eof() const { return is_io() && raw.io_kind == NAFGPU_IO_UNEXPECTED_EOF; }
    bool is_nom() const { return raw.status == NAFGPU_E_NOM; }
};

struct Record {   // data.rs:29-40: five public Option fields, owned strings (Record<'static>)
    std::optional<std::string> id, comment, sequence, quality;
    std::optional<uint64_t> length;
};

class Header {    // data.rs:198-237
public:
    explicit Header(const nafgpu_header &h) : h_(h) {}
    Flags flags() const { return Flags{h_.flags}; }
    uint64_t line_length() const { return h_.line_length; }
    char name_separator() const { return static_cast<char>(h_.name_separator); }
    uint64_t number_of_sequences() const { return h_.number_of_sequences; }
    SequenceType sequence_type() const { return static_cast<SequenceType>(h_.sequence_type); }
    FormatVersion format_version() const { return static_cast<FormatVersion>(h_.format_version); }

private:
    nafgpu_header h_;
};

// (no counterpart in the reference) one region of a decoded archive for Decoder::select: the letters [start, end) of a
// record, Region::npos = up to the record's end; reverse(): the reverse strand (nucleotide archives).  nafgpu.h has the rules.
struct Region {
    static constexpr uint64_t npos = NAFGPU_REGION_END;
    explicit Region(uint64_t record, uint64_t start = 0, uint64_t end = npos) : r{record, start, end, 0, {0, 0, 0, 0, 0, 0, 0}} {}
    Region slice(uint64_t start, uint64_t end) const {
        Region out = *this;
        out.r.start = start;
        out.r.end = end;
        return out;
    }
    Region reverse(bool on = true) const {
        Region out = *this;
        out.r.reverse_complement = on ? 1 : 0;
        return out;
    }
    nafgpu_region r;
};
static_assert(sizeof(Region) == sizeof(nafgpu_region), "a vector of Region is an array of nafgpu_region");

// What Decoder::select returns: records cut out of a decoded archive, in HBM; a copy that outlives the decoder.  Move-only.
class Selection {
public:
    Selection(Selection &&o) noexcept : s_(std::exchange(o.s_, nullptr)), res_(o.res_) {}
    Selection &operator=(Selection &&o) noexcept {
        if (this != &o) {
            nafgpu_selection_free(s_);
            s_ = std::exchange(o.s_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Selection(const Selection &) = delete;
    ~Selection() { nafgpu_selection_free(s_); }

    const nafgpu_encode_source &source() const { return res_.src; }   // device pointers: what encode_device takes
    const nafgpu_select_result &result() const { return res_; }
    uint64_t n_regions() const { return res_.n_regions; }
    uint64_t n_records() const { return res_.src.n_records; }
    uint64_t n_bases() const { return res_.src.n_bases; }
    // FASTA (FASTQ when the selection has qualities) in lines of line_length letters (0: one line), formatted on the GPU
    std::string to_text(uint64_t line_length = 60) {
        nafgpu_text_result t;
        check(nafgpu_selection_format(s_, line_length, &t), "nafgpu_selection_format", "the selection has no sequence field, so no text");
        std::string out(static_cast<size_t>(t.n_text), '\0');
        check(nafgpu_selection_copy_to_host(s_, t.d_text, t.n_text, out.data()), "nafgpu_selection_copy_to_host", "a null argument");
        return out;
    }
    nafgpu_selection *raw() const { return s_; }

private:
    friend class Decoder;
    Selection(nafgpu_selection *s, const nafgpu_select_result &r) : s_(s), res_(r) {}
    // the calls on a selection return a status alone: the message says which call it was and what that status means there
    static void check(int status, const char *call, const char *invalid_arg) {
        if (status == NAFGPU_OK) return;
        nafgpu_error e{};
        e.status = status;
        std::snprintf(e.message, sizeof e.message, "%s: %s", call,
                      status == NAFGPU_E_INVALID_ARG ? invalid_arg : status == NAFGPU_E_DEVICE ? "the device failed (allocation, copy or kernel)" : "failed");
        throw Error(e);
    }
    nafgpu_selection *s_ = nullptr;
    nafgpu_select_result res_{};
};

// (no counterpart in the reference) where patterns occur in records that are in HBM, matched on the GPU: nafgpu_search has the
// rules.  SearchOptions: alphabet -1 = by the archive for Decoder::search (nucleotide for dna and rna, bytes for protein and
// text) and nucleotide elsewhere; both_strands -1 = on for the nucleotide alphabet.
struct SearchOptions {
    int alphabet = -1;               // 0 nucleotide (IUPAC sets), 1 bytes (exact)
    int both_strands = -1;
    unsigned max_mismatches = 0;     // 0 .. 3 substitutions
    uint64_t max_hits = 0;           // 0: no cap
};
// What search returns: a Hits owns its device buffers and outlives its source; the accessors copy a table to the host.  Hits
// come in ascending order of (position, pattern, strand).  Move-only.
class Hits {
public:
    Hits(Hits &&o) noexcept : h_(std::exchange(o.h_, nullptr)), res_(o.res_), n_patterns_(o.n_patterns_) {}
    Hits &operator=(Hits &&o) noexcept {
        if (this != &o) {
            nafgpu_hits_free(h_);
            h_ = std::exchange(o.h_, nullptr);
            res_ = o.res_;
            n_patterns_ = o.n_patterns_;
        }
        return *this;
    }
    Hits(const Hits &) = delete;
    ~Hits() { nafgpu_hits_free(h_); }

    const nafgpu_search_result &result() const { return res_; }
    uint64_t n_hits() const { return res_.n_hits; }
    uint64_t n_records() const { return res_.n_records; }
    float ms() const { return res_.ms; }
    std::vector<uint64_t> pattern_hits() const { return std::vector<uint64_t>(res_.pattern_hits, res_.pattern_hits + n_patterns_); }   // both strands
    std::vector<nafgpu_region> regions() const { return table(res_.d_regions, res_.n_hits); }     // ready for nafgpu_select
    std::vector<nafgpu_hit_info> info() const { return table(res_.d_info, res_.n_hits); }
    std::vector<uint64_t> record_hit_begin() const { return table(res_.d_record_hit_begin, res_.n_records + 1); }   // CSR over the records

    // dec null: `src` is searched; else the decoder (it decodes first if nothing is decoded yet)
    static Hits of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const std::vector<std::string> &patterns, const SearchOptions &opts, int device) {
        std::string blob;
        for (const std::string &p : patterns) blob.append(p).push_back('\0');
        nafgpu_search_opts o{};
        bool nucleotide = opts.alphabet != 1;
        if (dec && opts.alphabet < 0) {
            nafgpu_header h;
            nafgpu_get_header(dec, &h);
            nucleotide = h.sequence_type <= 1;
        }
        o.alphabet = nucleotide ? 0 : 1;
        o.both_strands = opts.both_strands < 0 ? nucleotide : opts.both_strands != 0;
        o.max_mismatches = static_cast<uint8_t>(opts.max_mismatches > 255 ? 255 : opts.max_mismatches);
        o.max_hits = opts.max_hits;
        nafgpu_hits *h = nullptr;
        nafgpu_search_result r;
        nafgpu_error e{};
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(blob.data());
        const int rc = dec ? nafgpu_search_decoder(dec, bytes, blob.size(), patterns.size(), &o, &h, &r, &e)
                           : nafgpu_search(src, bytes, blob.size(), patterns.size(), &o, device, &h, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return Hits(h, r, patterns.size());
    }

private:
    Hits(nafgpu_hits *h, const nafgpu_search_result &r, size_t n_patterns) : h_(h), res_(r), n_patterns_(n_patterns) {}
    template <class T>
    std::vector<T> table(const T *d_ptr, uint64_t n) const {
        std::vector<T> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_hits_copy_to_host(h_, d_ptr, sizeof(T) * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_hits_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_hits *h_ = nullptr;
    nafgpu_search_result res_{};
    size_t n_patterns_ = 0;
};

// (no counterpart in the reference) which records that are in HBM have equal sequences, found on the GPU: nafgpu_group has the
// rules.  GroupOptions: alphabet -1 = by the archive for Decoder::group (nucleotide for dna and rna, bytes for protein and
// text) and nucleotide elsewhere.
struct GroupOptions {
    int alphabet = -1;               // 0 nucleotide (4-bit codes: case and T/U ignored), 1 bytes (exact)
    bool both_strands = false;       // nucleotide only: a record also equals its reverse complement
};
// What group returns: a Groups owns its device buffers and outlives its source; the accessors copy a table to the host.
// Move-only.
class Groups {
public:
    Groups(Groups &&o) noexcept : g_(std::exchange(o.g_, nullptr)), res_(o.res_) {}
    Groups &operator=(Groups &&o) noexcept {
        if (this != &o) {
            nafgpu_groups_free(g_);
            g_ = std::exchange(o.g_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Groups(const Groups &) = delete;
    ~Groups() { nafgpu_groups_free(g_); }

    const nafgpu_group_result &result() const { return res_; }
    uint64_t n_records() const { return res_.n_records; }
    uint64_t n_groups() const { return res_.n_groups; }
    uint64_t n_duplicates() const { return res_.n_records - res_.n_groups; }
    uint64_t largest_group() const { return res_.largest_group; }
    uint32_t rounds() const { return res_.rounds; }
    float ms() const { return res_.ms; }
    std::vector<uint64_t> representative() const { return table(res_.d_representative, res_.n_records); }   // the lowest record with an equal sequence
    std::vector<uint64_t> group_of() const { return table(res_.d_group_of, res_.n_records); }
    std::vector<uint8_t> strand() const { return table(res_.d_strand, res_.n_records); }                    // empty without both_strands
    std::vector<uint64_t> group_first() const { return table(res_.d_group_first, res_.n_groups); }         // the representatives, ascending
    std::vector<uint64_t> group_size() const { return table(res_.d_group_size, res_.n_groups); }

    // dec null: `src` is grouped; else the decoder (it decodes first if nothing is decoded yet)
    static Groups of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const GroupOptions &opts, int device) {
        nafgpu_group_opts o{};
        bool nucleotide = opts.alphabet != 1;
        if (dec && opts.alphabet < 0) {
            nafgpu_header h;
            nafgpu_get_header(dec, &h);
            nucleotide = h.sequence_type <= 1;
        }
        o.alphabet = nucleotide ? 0 : 1;
        o.both_strands = opts.both_strands ? 1 : 0;
        nafgpu_groups *g = nullptr;
        nafgpu_group_result r;
        nafgpu_error e{};
        const int rc = dec ? nafgpu_group_decoder(dec, &o, &g, &r, &e) : nafgpu_group(src, &o, device, &g, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return Groups(g, r);
    }

private:
    Groups(nafgpu_groups *g, const nafgpu_group_result &r) : g_(g), res_(r) {}
    template <class T>
    std::vector<T> table(const T *d_ptr, uint64_t n) const {
        std::vector<T> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_groups_copy_to_host(g_, d_ptr, sizeof(T) * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_groups_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_groups *g_ = nullptr;
    nafgpu_group_result res_{};
};

// (no counterpart in the reference) the window of every record that quality trimming keeps, found on the GPU: nafgpu_trim has
// the rules.  0 turns a step off.
struct TrimOptions {
    unsigned cut_front = 0, cut_tail = 0;   // step 1: the running-sum cutoffs of `cutadapt -q FRONT,TAIL`
    unsigned window = 0, window_quality = 0;   // step 2: the first window of W (1 .. 64) values whose mean is below Q
    bool trim_n = false;             // step 3: N at either end
    uint64_t min_length = 0;         // step 4: a record whose window is shorter is not kept
    bool interleaved = false;        //         records 2j and 2j + 1 are mates: both are kept only when both pass
    unsigned quality_base = 33;
};
// What trim returns: a Trims owns its device buffers and outlives its source; the accessors copy a table to the host.
// Move-only.
class Trims {
public:
    Trims(Trims &&o) noexcept : t_(std::exchange(o.t_, nullptr)), res_(o.res_) {}
    Trims &operator=(Trims &&o) noexcept {
        if (this != &o) {
            nafgpu_trims_free(t_);
            t_ = std::exchange(o.t_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Trims(const Trims &) = delete;
    ~Trims() { nafgpu_trims_free(t_); }

    const nafgpu_trim_result &result() const { return res_; }
    uint64_t n_records() const { return res_.n_records; }
    uint64_t n_kept() const { return res_.n_kept; }
    uint64_t n_changed() const { return res_.n_changed; }
    uint64_t bases_in_windows() const { return res_.bases_in_windows; }
    uint64_t bases_kept() const { return res_.bases_kept; }
    float ms() const { return res_.ms; }
    std::vector<nafgpu_region> regions() const { return table(res_.d_regions, res_.n_records); }            // {k, a, b, 0} per record
    std::vector<uint8_t> keep() const { return table(res_.d_keep, res_.n_records); }
    std::vector<nafgpu_region> kept_regions() const { return table(res_.d_kept_regions, res_.n_kept); }     // ready for nafgpu_select

    // dec null: `src` is trimmed; else the decoder (it decodes first if nothing is decoded yet)
    static Trims of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const TrimOptions &opts, int device) {
        nafgpu_trim_opts o{};
        auto byte = [](unsigned v) { return static_cast<uint8_t>(v > 255 ? 255 : v); };
        o.quality_base = byte(opts.quality_base);
        o.cut_front = byte(opts.cut_front);
        o.cut_tail = byte(opts.cut_tail);
        o.window = byte(opts.window);
        o.window_quality = byte(opts.window_quality);
        o.trim_n = opts.trim_n ? 1 : 0;
        o.interleaved = opts.interleaved ? 1 : 0;
        o.min_length = opts.min_length;
        nafgpu_trims *t = nullptr;
        nafgpu_trim_result r;
        nafgpu_error e{};
        const int rc = dec ? nafgpu_trim_decoder(dec, &o, &t, &r, &e) : nafgpu_trim(src, &o, device, &t, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return Trims(t, r);
    }

private:
    Trims(nafgpu_trims *t, const nafgpu_trim_result &r) : t_(t), res_(r) {}
    template <class T>
    std::vector<T> table(const T *d_ptr, uint64_t n) const {
        std::vector<T> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_trims_copy_to_host(t_, d_ptr, sizeof(T) * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_trims_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_trims *t_ = nullptr;
    nafgpu_trim_result res_{};
};

// (no counterpart in the reference) where read 1 and the reverse complement of read 2 of every pair of mates (records 2j and
// 2j + 1) overlap, found on the GPU: nafgpu_overlap has the rules.
struct OverlapOptions {
    unsigned min_overlap = 30;       // an accepted shift has so many matching letters
    unsigned max_mismatches = 5;     // at most so many mismatches
    unsigned max_mismatch_percent = 20;   // and at most this share of them among matches + mismatches
    unsigned quality_base = 33;      // what Decoder::merge writes the quality of disagreeing letters from
};
// What overlap returns: an Overlaps owns its device buffers and outlives its source; the accessors copy a table to the host.
// Move-only.
class Overlaps {
public:
    Overlaps(Overlaps &&o) noexcept : o_(std::exchange(o.o_, nullptr)), res_(o.res_) {}
    Overlaps &operator=(Overlaps &&o) noexcept {
        if (this != &o) {
            nafgpu_overlaps_free(o_);
            o_ = std::exchange(o.o_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Overlaps(const Overlaps &) = delete;
    ~Overlaps() { nafgpu_overlaps_free(o_); }

    const nafgpu_overlap_result &result() const { return res_; }
    const nafgpu_overlaps *raw() const { return o_; }
    uint64_t n_records() const { return res_.n_records; }
    uint64_t n_pairs() const { return res_.n_pairs; }
    uint64_t n_found() const { return res_.n_found; }
    uint64_t n_too_long() const { return res_.n_too_long; }
    uint64_t n_unmerged() const { return res_.n_unmerged; }
    uint64_t n_cut() const { return res_.n_cut; }
    uint64_t matches() const { return res_.matches; }
    uint64_t mismatches() const { return res_.mismatches; }
    uint64_t bases_merged() const { return res_.bases_merged; }
    uint64_t bases_after_cut() const { return res_.bases_after_cut; }
    float ms() const { return res_.ms; }
    std::vector<nafgpu_pair_overlap> pairs() const { return table(res_.d_pairs, res_.n_pairs); }
    std::vector<nafgpu_region> regions() const { return table(res_.d_regions, res_.n_records); }               // the adapter cut, ready for nafgpu_select
    std::vector<nafgpu_region> unmerged_regions() const { return table(res_.d_unmerged_regions, res_.n_unmerged); }

    // dec null: the pairs of `src`; else the decoder's (it decodes first if nothing is decoded yet)
    static Overlaps of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const OverlapOptions &opts, int device) {
        nafgpu_overlap_opts o{};
        o.min_overlap = opts.min_overlap;
        o.max_mismatches = opts.max_mismatches;
        o.max_mismatch_percent = static_cast<uint8_t>(opts.max_mismatch_percent > 255 ? 255 : opts.max_mismatch_percent);
        o.quality_base = static_cast<uint8_t>(opts.quality_base > 255 ? 255 : opts.quality_base);
        nafgpu_overlaps *h = nullptr;
        nafgpu_overlap_result r;
        nafgpu_error e{};
        const int rc = dec ? nafgpu_overlap_decoder(dec, &o, &h, &r, &e) : nafgpu_overlap(src, &o, device, &h, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return Overlaps(h, r);
    }

private:
    Overlaps(nafgpu_overlaps *o, const nafgpu_overlap_result &r) : o_(o), res_(r) {}
    template <class T>
    std::vector<T> table(const T *d_ptr, uint64_t n) const {
        std::vector<T> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_overlaps_copy_to_host(o_, d_ptr, sizeof(T) * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_overlaps_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_overlaps *o_ = nullptr;
    nafgpu_overlap_result res_{};
};

// (no counterpart in the reference) the k-mers of a reference as a set in HBM, and records screened against it:
// nafgpu_kmers_build and nafgpu_screen have the rules.
struct KmerOptions {
    unsigned k = 31;                 // 1 .. 31
    bool canonical = true;           // a k-mer and its reverse complement are one key
};
// What kmers returns: a KmerSet owns its table and outlives its source.  Move-only.
class KmerSet {
public:
    KmerSet(KmerSet &&o) noexcept : k_(std::exchange(o.k_, nullptr)), res_(o.res_) {}
    KmerSet &operator=(KmerSet &&o) noexcept {
        if (this != &o) {
            nafgpu_kmers_free(k_);
            k_ = std::exchange(o.k_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    KmerSet(const KmerSet &) = delete;
    ~KmerSet() { nafgpu_kmers_free(k_); }

    const nafgpu_kmers_result &result() const { return res_; }
    const nafgpu_kmers *raw() const { return k_; }
    unsigned k() const { return res_.k; }
    bool canonical() const { return res_.canonical != 0; }
    uint64_t n_windows() const { return res_.n_windows; }
    uint64_t n_kmers() const { return res_.n_kmers; }
    uint64_t slots() const { return res_.slots; }
    float ms() const { return res_.ms; }

    // dec null: the k-mers of `src`; else the decoder's (it decodes first if nothing is decoded yet)
    static KmerSet of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const KmerOptions &opts, int device) {
        nafgpu_kmer_opts o{};
        o.k = static_cast<uint8_t>(opts.k > 255 ? 255 : opts.k);
        o.canonical = opts.canonical ? 1 : 0;
        nafgpu_kmers *k = nullptr;
        nafgpu_kmers_result r;
        nafgpu_error e{};
        const int rc = dec ? nafgpu_kmers_build_decoder(dec, &o, &k, &r, &e) : nafgpu_kmers_build(src, &o, device, &k, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return KmerSet(k, r);
    }

private:
    KmerSet(nafgpu_kmers *k, const nafgpu_kmers_result &r) : k_(k), res_(r) {}
    nafgpu_kmers *k_ = nullptr;
    nafgpu_kmers_result res_{};
};

struct ScreenOptions {
    uint64_t min_hits = 1;           // a record matches with at least so many windows in the set
    unsigned min_percent = 0;        //   and so large a share of its windows, 0 .. 100
    bool interleaved = false;        // records 2j and 2j + 1 are mates: both match when either does
    bool keep_matched = false;       // false: what does not match is kept (decontamination); true: what matches (baiting)
};
// What screen returns: a Screens owns its device buffers and outlives its source and its set; the accessors copy a table to the
// host.  Move-only.
class Screens {
public:
    Screens(Screens &&o) noexcept : s_(std::exchange(o.s_, nullptr)), res_(o.res_) {}
    Screens &operator=(Screens &&o) noexcept {
        if (this != &o) {
            nafgpu_screens_free(s_);
            s_ = std::exchange(o.s_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Screens(const Screens &) = delete;
    ~Screens() { nafgpu_screens_free(s_); }

    const nafgpu_screen_result &result() const { return res_; }
    uint64_t n_records() const { return res_.n_records; }
    uint64_t n_matched() const { return res_.n_matched; }
    uint64_t n_kept() const { return res_.n_kept; }
    uint64_t n_windows() const { return res_.n_windows; }
    uint64_t n_hits() const { return res_.n_hits; }
    uint64_t bases_kept() const { return res_.bases_kept; }
    float ms() const { return res_.ms; }
    std::vector<uint64_t> windows() const { return table(res_.d_windows, res_.n_records); }
    std::vector<uint64_t> hits() const { return table(res_.d_hits, res_.n_records); }
    std::vector<nafgpu_region> regions() const { return table(res_.d_regions, res_.n_records); }            // {r, a, b, 0} per record
    std::vector<uint8_t> match() const { return table(res_.d_match, res_.n_records); }
    std::vector<uint8_t> keep() const { return table(res_.d_keep, res_.n_records); }
    std::vector<nafgpu_region> kept_regions() const { return table(res_.d_kept_regions, res_.n_kept); }     // ready for nafgpu_select

    // dec null: `src` is screened; else the decoder (it decodes first if nothing is decoded yet)
    static Screens of(nafgpu_decoder *dec, const nafgpu_encode_source *src, const KmerSet &set, const ScreenOptions &opts, int device) {
        nafgpu_screen_opts o{};
        o.keep_matched = opts.keep_matched ? 1 : 0;
        o.interleaved = opts.interleaved ? 1 : 0;
        o.min_percent = static_cast<uint8_t>(opts.min_percent > 255 ? 255 : opts.min_percent);
        o.min_hits = opts.min_hits;
        nafgpu_screens *s = nullptr;
        nafgpu_screen_result r;
        nafgpu_error e{};
        const int rc = dec ? nafgpu_screen_decoder(dec, set.raw(), &o, &s, &r, &e) : nafgpu_screen(src, set.raw(), &o, device, &s, &r, &e);
        if (rc != NAFGPU_OK) throw Error(e);
        return Screens(s, r);
    }

private:
    Screens(nafgpu_screens *s, const nafgpu_screen_result &r) : s_(s), res_(r) {}
    template <class T>
    std::vector<T> table(const T *d_ptr, uint64_t n) const {
        std::vector<T> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_screens_copy_to_host(s_, d_ptr, sizeof(T) * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_screens_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_screens *s_ = nullptr;
    nafgpu_screen_result res_{};
};

class Decoder {   // mod.rs:285-461
public:
    Decoder(Decoder &&o) noexcept
        : d_(std::exchange(o.d_, nullptr)), batch_(std::move(o.batch_)), at_(std::exchange(o.at_, 0)), n_(std::exchange(o.n_, 0)),
          pending_(std::exchange(o.pending_, NAFGPU_OK)), pending_err_(o.pending_err_) {}
    Decoder &operator=(Decoder &&o) noexcept {
        if (this != &o) {
            nafgpu_close(d_);
            d_ = std::exchange(o.d_, nullptr);
            batch_ = std::move(o.batch_);
            at_ = std::exchange(o.at_, 0);
            n_ = std::exchange(o.n_, 0);
            pending_ = std::exchange(o.pending_, NAFGPU_OK);
            pending_err_ = o.pending_err_;
        }
        return *this;
    }
    Decoder(const Decoder &) = delete;
    ~Decoder() { nafgpu_close(d_); }

    static Decoder from_path(const std::string &path);   // mod.rs:304-306
    Header header() const {
        nafgpu_header h;
        nafgpu_get_header(d_, &h);
        return Header(h);
    }
    SequenceType sequence_type() const { return header().sequence_type(); }
    size_t len() const { return static_cast<size_t>(nafgpu_remaining(d_)) + (n_ - at_); }   // ExactSizeIterator (records fetched ahead count)

    // Iterator::next: nullopt at the end; throws Error (the iterator stays usable, mod.rs:391).
    // Records cross the C boundary a batch at a time (nafgpu_next_batch); what the caller sees is what one nafgpu_next
    // per record gives: an error met by record k of a batch is thrown when record k is asked for, not before.
    std::optional<Record> next() {
        if (at_ == n_) {
            if (pending_ != NAFGPU_OK) {
                const int rc = std::exchange(pending_, NAFGPU_OK);
                if (rc == NAFGPU_END) return std::nullopt;
                throw Error(pending_err_);
            }
            if (batch_.empty()) batch_.resize(kBatch);
            uint64_t got = 0;
            const int rc = nafgpu_next_batch(d_, batch_.data(), kBatch, &got);
            at_ = 0;
            n_ = static_cast<size_t>(got);
            if (rc != NAFGPU_OK) {
                if (rc != NAFGPU_END) nafgpu_last_error(d_, &pending_err_);
                if (n_ == 0) {
                    if (rc == NAFGPU_END) return std::nullopt;
                    throw Error(pending_err_);
                }
                pending_ = rc;
            }
        }
        const nafgpu_record &r = batch_[at_++];
        auto own = [](const nafgpu_field &f) -> std::optional<std::string> {
            if (!f.present) return std::nullopt;
            return std::string(reinterpret_cast<const char *>(f.ptr), static_cast<size_t>(f.len));
        };
        Record out;
        out.id = own(r.id);
        out.comment = own(r.comment);
        out.sequence = own(r.sequence);
        out.quality = own(r.quality);
        if (r.has_length) out.length = r.length;
        return out;
    }
    // The whole archive as FASTA (FASTQ when it has qualities and `quality` is selected), formatted on
    // the GPU from the decoded buffers (nafgpu_format_device) and copied to the host: what `unnaf` prints.
    std::string to_text() {
        nafgpu_text_result t;
        if (nafgpu_format_device(d_, &t) != NAFGPU_OK) {
            nafgpu_error e;
            nafgpu_last_error(d_, &e);
            throw Error(e);
        }
        std::string out(static_cast<size_t>(t.n_text), '\0');
        if (t.n_text && nafgpu_copy_to_host(d_, t.d_text, t.n_text, out.data()) != NAFGPU_OK) {
            nafgpu_error e;
            nafgpu_last_error(d_, &e);
            throw Error(e);
        }
        return out;
    }
    // (no counterpart in the reference) for every name the index of the first record with that id, looked up on the GPU
    std::vector<std::optional<uint64_t>> find(const std::vector<std::string> &names) {
        std::string blob;
        for (const std::string &n : names) blob.append(n.c_str()).push_back('\0');
        std::vector<uint64_t> at(names.size() + 1);
        nafgpu_error e{};
        if (nafgpu_find_records(d_, reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), names.size(), at.data(), &e) != NAFGPU_OK) throw Error(e);
        std::vector<std::optional<uint64_t>> out(names.size());
        for (size_t k = 0; k < names.size(); k++)
            if (at[k] != UINT64_MAX) out[k] = at[k];
        return out;
    }
    // (no counterpart in the reference) regions -> records in HBM, region k the selection's record k; name_regions: ids
    // become id:START-END (and /rc).  Throws Error (NAFGPU_E_INVALID_ARG, naming the first region the rules refuse).
    Selection select(const std::vector<Region> &regions, bool name_regions = false) {
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.empty() ? nullptr : &regions[0].r, regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // the hits of a search as records of their own, a reverse-strand hit reversed and complemented: every record reads as its
    // pattern is written
    Selection select(const Hits &hits, bool name_regions = false) {
        const std::vector<nafgpu_region> regions = hits.regions();
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.data(), regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // (no counterpart in the reference) the window of every decoded record that quality trimming keeps (decodes first if nothing
    // is decoded yet)
    Trims trim(const TrimOptions &opts = TrimOptions()) { return Trims::of(d_, nullptr, opts, -1); }
    // the kept records cut to their windows, in order
    Selection select(const Trims &trims, bool name_regions = false) {
        const std::vector<nafgpu_region> regions = trims.kept_regions();
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.data(), regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // (no counterpart in the reference) the distinct k-mers of the decoded records as a set in HBM, and the decoded records
    // against such a set (either decodes first if nothing is decoded yet)
    KmerSet kmers(const KmerOptions &opts = KmerOptions()) { return KmerSet::of(d_, nullptr, opts, -1); }
    Screens screen(const KmerSet &set, const ScreenOptions &opts = ScreenOptions()) { return Screens::of(d_, nullptr, set, opts, -1); }
    // the kept records, whole and in order
    Selection select(const Screens &screens, bool name_regions = false) {
        const std::vector<nafgpu_region> regions = screens.kept_regions();
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.data(), regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // (no counterpart in the reference) where the mates of every decoded pair overlap (decodes first if nothing is decoded yet)
    Overlaps overlap(const OverlapOptions &opts = OverlapOptions()) { return Overlaps::of(d_, nullptr, opts, -1); }
    // every record, cut where it reads into the adapter
    Selection select(const Overlaps &overlaps, bool name_regions = false) {
        const std::vector<nafgpu_region> regions = overlaps.regions();
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.data(), regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // the found pairs of this decoder's overlaps joined into one record each, in pair order
    Selection merge(const Overlaps &overlaps) {
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_merge_pairs(d_, overlaps.raw(), &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    // (no counterpart in the reference) where `patterns` occur in the decoded records (decodes first if nothing is decoded yet)
    Hits search(const std::vector<std::string> &patterns, const SearchOptions &opts = SearchOptions()) { return Hits::of(d_, nullptr, patterns, opts, -1); }
    // (no counterpart in the reference) the decoded records whose sequences are equal (decodes first if nothing is decoded yet)
    Groups group(const GroupOptions &opts = GroupOptions()) { return Groups::of(d_, nullptr, opts, -1); }
    // the first record of every sequence, whole and in order: the archive without its duplicates
    Selection select(const Groups &groups, bool name_regions = false) {
        const std::vector<uint64_t> first = groups.group_first();
        std::vector<nafgpu_region> regions(first.size());
        for (size_t k = 0; k < first.size(); k++) {
            regions[k] = nafgpu_region{};
            regions[k].record = first[k];
            regions[k].end = NAFGPU_REGION_END;
        }
        nafgpu_select_opts o{};
        o.name_regions = name_regions ? 1 : 0;
        nafgpu_selection *s = nullptr;
        nafgpu_select_result r;
        nafgpu_error e{};
        if (nafgpu_select(d_, regions.data(), regions.size(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Selection(s, r);
    }
    nafgpu_decoder *raw() const { return d_; }

private:
    friend class DecoderBuilder;
    explicit Decoder(nafgpu_decoder *d) : d_(d) {}
    nafgpu_decoder *d_ = nullptr;
    static constexpr size_t kBatch = 1024;
    std::vector<nafgpu_record> batch_;
    size_t at_ = 0, n_ = 0;
    int pending_ = NAFGPU_OK;          // what the batch call returned behind its records (an error, or the end)
    nafgpu_error pending_err_{};
};

class DecoderBuilder {   // mod.rs:53-257
public:
    DecoderBuilder() { nafgpu_opts_default(&o_); }                                  // mod.rs:67-76
    static DecoderBuilder from_flags(Flags f) {                                     // mod.rs:93-101
        DecoderBuilder b;
        nafgpu_opts_from_flags(&b.o_, f.as_byte());
        return b;
    }
    DecoderBuilder &buffer_size(size_t n) { o_.buffer_size = n; return *this; }      // mod.rs:110
    DecoderBuilder &id(bool v) { o_.id = v; return *this; }
    DecoderBuilder &comment(bool v) { o_.comment = v; return *this; }
    DecoderBuilder &sequence(bool v) { o_.sequence = v; return *this; }
    DecoderBuilder &quality(bool v) { o_.quality = v; return *this; }
    DecoderBuilder &mask(bool v) { o_.mask = v; return *this; }
    DecoderBuilder &device(int ordinal) { o_.device = ordinal; return *this; }       // MI355X-specific knob

    Decoder with_bytes(const uint8_t *p, size_t n) const {                           // mod.rs:151-156
        nafgpu_decoder *d = nullptr;
        nafgpu_error e;
        if (nafgpu_open_bytes(p, n, &o_, &d, &e) != NAFGPU_OK) throw Error(e);
        return Decoder(d);
    }
    Decoder with_path(const std::string &path) const {                               // mod.rs:159-166
        nafgpu_decoder *d = nullptr;
        nafgpu_error e;
        if (nafgpu_open_path(path.c_str(), &o_, &d, &e) != NAFGPU_OK) throw Error(e);
        return Decoder(d);
    }
    Decoder with_reader(nafgpu_read_fn read, nafgpu_seek_fn seek, void *ctx) const {  // mod.rs:169-256
        nafgpu_decoder *d = nullptr;
        nafgpu_error e;
        if (nafgpu_open_io(read, seek, ctx, &o_, &d, &e) != NAFGPU_OK) throw Error(e);
        return Decoder(d);
    }

private:
    nafgpu_opts o_;
};

inline Decoder Decoder::from_path(const std::string &path) { return DecoderBuilder().with_path(path); }

// ---- Encoder (encoder/mod.rs:46-384).  Host code, as in the reference, unless EncoderBuilder::device() names a GPU:
// the sections of compression levels 1 and 2 are then compressed by the HIP kernels, to the same bytes.  See include/nafgpu.h.
class Encoder {      // mod.rs:215-384 (Memory storage)
public:
    Encoder(Encoder &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Encoder(const Encoder &) = delete;
    ~Encoder() { if (e_) nafgpu_encoder_free(e_); }
    void push(const Record &r) {                                                     // mod.rs:236-323
        nafgpu_record c{};
        auto field = [](const std::optional<std::string> &s, nafgpu_field *f) {
            if (!s) return;
            f->ptr = reinterpret_cast<const uint8_t *>(s->data());
            f->len = s->size();
            f->present = 1;
        };
        field(r.id, &c.id);
        field(r.comment, &c.comment);
        field(r.sequence, &c.sequence);
        field(r.quality, &c.quality);
        if (r.length) {
            c.length = *r.length;
            c.has_length = 1;
        }
        nafgpu_error err{};
        if (nafgpu_encoder_push(e_, &c, &err) != NAFGPU_OK) throw Error(err);
    }
    std::string write() {                                                            // mod.rs:325-384 into a string
        const uint8_t *p = nullptr;
        uint64_t n = 0;
        nafgpu_error err{};
        if (nafgpu_encoder_finish(e_, &p, &n, &err) != NAFGPU_OK) throw Error(err);
        return std::string(reinterpret_cast<const char *>(p), n);
    }

private:
    friend class EncoderBuilder;
    explicit Encoder(nafgpu_encoder *e) : e_(e) {}
    nafgpu_encoder *e_ = nullptr;
};

class EncoderBuilder {   // mod.rs:46-213
public:
    explicit EncoderBuilder(SequenceType t) { nafgpu_encoder_opts_default(static_cast<uint8_t>(t), &o_); }   // mod.rs:81-90
    static EncoderBuilder from_flags(SequenceType t, Flags f) {                      // mod.rs:92-110
        EncoderBuilder b(t);
        nafgpu_encoder_opts_from_flags(static_cast<uint8_t>(t), f.as_byte(), &b.o_);
        return b;
    }
    EncoderBuilder &id(bool v) { o_.id = v; return *this; }
    EncoderBuilder &comment(bool v) { o_.comment = v; return *this; }
    EncoderBuilder &sequence(bool v) { o_.sequence = v; return *this; }
    EncoderBuilder &quality(bool v) { o_.quality = v; return *this; }
    EncoderBuilder &compression_level(int v) { o_.compression_level = v; return *this; }
    // (no counterpart in the reference, whose mask writer is commented out, mod.rs:240) accept lower-case nucleotides and
    // write their runs as a Mask section; DNA / RNA with sequence(true) only, else with_memory() throws (NAFGPU_E_INVALID_ARG)
    EncoderBuilder &mask(bool v) { o_.mask = v; return *this; }
    // (no counterpart in the reference) compress the sections on that GPU (-1: the current one); compression_level 1 or 2
    EncoderBuilder &device(int v) { device_ = v; return *this; }
    // (no counterpart in the reference) with device(), encode_device() or encode_text(): compression_level 0 and >= 3 too,
    // the LZ matches found on the GPU (nafgpu_encoder_opts.device_lz); the host encoder ignores it
    EncoderBuilder &device_lz(bool v) { o_.device_lz = v; return *this; }
    Encoder with_memory() const {                                                    // mod.rs:161-163
        nafgpu_encoder *e = nullptr;
        nafgpu_error err{};
        if (nafgpu_encoder_new(&o_, &e, &err) != NAFGPU_OK) throw Error(err);
        Encoder enc(e);
        if (device_ >= -1) {
            err.status = nafgpu_encoder_set_device(e, device_);
            if (err.status != NAFGPU_OK) {
                std::snprintf(err.message, sizeof err.message, "%s",
                              err.status == NAFGPU_E_DEVICE ? "no usable HIP device" : "device encoding needs compression_level 1 or 2, or device_lz(true)");
                throw Error(err);
            }
        }
        return enc;
    }
    const nafgpu_encoder_opts &options() const { return o_; }

private:
    nafgpu_encoder_opts o_{};
    int device_ = -2;                                                                // -2: host code
};

// (no counterpart in the reference) records that are in HBM -> an archive, the bytes Encoder::write gives when the same
// records are pushed one by one: nafgpu_encode_device.  `fields` says what is written (id / comment / sequence / quality,
// mask, compression_level 1 or 2, or any level with device_lz(true)); the source's pointers must agree with it.
inline std::string encode_device(const nafgpu_encode_source &src, const EncoderBuilder &fields, int device = -1) {
    uint8_t *p = nullptr;
    uint64_t n = 0;
    nafgpu_error err{};
    if (nafgpu_encode_device(&src, &fields.options(), device, &p, &n, &err) != NAFGPU_OK) throw Error(err);
    std::string out(reinterpret_cast<const char *>(p), n);
    nafgpu_encode_free(p);
    return out;
}

// a selection -> an archive: the fields `fields` names (those the selection does not hold: nafgpu_encode_device refuses)
inline std::string encode_device(const Selection &sel, const EncoderBuilder &fields, int device = -1) {
    nafgpu_encode_source src = sel.source();
    const nafgpu_encoder_opts &o = fields.options();
    if (!o.id) src.d_ids = nullptr, src.n_ids_bytes = 0;
    if (!o.comment) src.d_comments = nullptr, src.n_comments_bytes = 0;
    if (!o.sequence) src.d_sequence = nullptr, src.n_bases = 0;
    if (!o.quality) src.d_quality = nullptr, src.n_quality = 0;
    return encode_device(src, fields, device);
}

// (no counterpart in the reference; what `ennaf` does) FASTA / FASTQ text -> an archive, parsed and encoded on the GPU:
// nafgpu_encode_text.  `fields` as for encode_device (quality needs FASTQ text); keep_line_length: the header carries the
// text's longest sequence line instead of 60.  The format is told by the text's first byte.
inline std::string encode_text(const std::string &text, const EncoderBuilder &fields, bool keep_line_length = true, int device = -1) {
    uint8_t *p = nullptr;
    uint64_t n = 0;
    nafgpu_error err{};
    if (nafgpu_encode_text(reinterpret_cast<const uint8_t *>(text.data()), text.size(), nullptr, &fields.options(), keep_line_length ? 1 : 0,
                           device, &p, &n, &err) != NAFGPU_OK)
        throw Error(err);
    std::string out(reinterpret_cast<const char *>(p), n);
    nafgpu_encode_free(p);
    return out;
}

// (no counterpart in the reference) per-record letter counts, quality sums and the sections' histograms of records that are
// in HBM, counted on the GPU: nafgpu_summarize has the rules.  A Summary owns its device buffers and outlives its source;
// the accessors copy a table to the host (empty when the source has no field for it).  Move-only.
class Summary {
public:
    enum Column { A = 0, C, G, T, N, Iupac, Other, Lower };   // the columns of the default table
    Summary(Summary &&o) noexcept : s_(std::exchange(o.s_, nullptr)), res_(o.res_) {}
    Summary &operator=(Summary &&o) noexcept {
        if (this != &o) {
            nafgpu_summary_free(s_);
            s_ = std::exchange(o.s_, nullptr);
            res_ = o.res_;
        }
        return *this;
    }
    Summary(const Summary &) = delete;
    ~Summary() { nafgpu_summary_free(s_); }

    const nafgpu_summary_result &result() const { return res_; }
    uint64_t n_records() const { return res_.n_records; }
    std::vector<uint64_t> totals() const { return std::vector<uint64_t>(res_.totals, res_.totals + 8); }
    uint64_t quality_total() const { return res_.quality_total; }
    float ms() const { return res_.ms; }
    std::vector<uint64_t> counts() const { return words(res_.d_counts, 8 * res_.n_records); }   // n_records rows of 8 columns
    std::vector<uint64_t> quality_sum() const { return words(res_.d_quality_sum, res_.n_records); }
    std::vector<uint64_t> letter_hist() const { return words(res_.d_letter_hist, 256); }
    std::vector<uint64_t> quality_hist() const { return words(res_.d_quality_hist, 256); }

    // classes: null = the default table, else 256 masks of eight columns
    static Summary of(const nafgpu_encode_source &src, int device = -1, const uint8_t *classes = nullptr) {
        nafgpu_summary_opts o = options(classes);
        nafgpu_summary *s = nullptr;
        nafgpu_summary_result r;
        nafgpu_error e{};
        if (nafgpu_summarize(&src, &o, device, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Summary(s, r);
    }
    static Summary of(const Decoder &dec, const uint8_t *classes = nullptr) {
        nafgpu_summary_opts o = options(classes);
        nafgpu_summary *s = nullptr;
        nafgpu_summary_result r;
        nafgpu_error e{};
        if (nafgpu_summarize_decoder(dec.raw(), &o, &s, &r, &e) != NAFGPU_OK) throw Error(e);
        return Summary(s, r);
    }

private:
    Summary(nafgpu_summary *s, const nafgpu_summary_result &r) : s_(s), res_(r) {}
    static nafgpu_summary_opts options(const uint8_t *classes) {
        nafgpu_summary_opts o{};
        if (classes) {
            std::memcpy(o.classes, classes, 256);
            o.use_classes = 1;
        }
        return o;
    }
    std::vector<uint64_t> words(const uint64_t *d_ptr, uint64_t n) const {
        std::vector<uint64_t> out(d_ptr ? static_cast<size_t>(n) : 0);
        const int rc = out.empty() ? NAFGPU_OK : nafgpu_summary_copy_to_host(s_, d_ptr, 8 * n, out.data());
        if (rc != NAFGPU_OK) {
            nafgpu_error e{};
            e.status = rc;
            std::snprintf(e.message, sizeof e.message, "nafgpu_summary_copy_to_host: %s", rc == NAFGPU_E_DEVICE ? "the copy failed" : "a null argument");
            throw Error(e);
        }
        return out;
    }
    nafgpu_summary *s_ = nullptr;
    nafgpu_summary_result res_{};
};
// decodes first if nothing is decoded yet
inline Summary summarize(const Decoder &dec, const uint8_t *classes = nullptr) { return Summary::of(dec, classes); }
inline Summary summarize(const Selection &sel, int device = -1, const uint8_t *classes = nullptr) { return Summary::of(sel.source(), device, classes); }
inline Summary summarize(const nafgpu_encode_source &src, int device, const uint8_t *classes = nullptr) { return Summary::of(src, device, classes); }

inline Hits search(const Selection &sel, const std::vector<std::string> &patterns, const SearchOptions &opts = SearchOptions(), int device = -1) {
    return Hits::of(nullptr, &sel.source(), patterns, opts, device);
}
inline Hits search(const nafgpu_encode_source &src, const std::vector<std::string> &patterns, const SearchOptions &opts = SearchOptions(), int device = -1) {
    return Hits::of(nullptr, &src, patterns, opts, device);
}

inline Groups group(const Selection &sel, const GroupOptions &opts = GroupOptions(), int device = -1) { return Groups::of(nullptr, &sel.source(), opts, device); }
inline Groups group(const nafgpu_encode_source &src, const GroupOptions &opts = GroupOptions(), int device = -1) { return Groups::of(nullptr, &src, opts, device); }
// the trims of a selection index the selection's records
inline Trims trim(const Selection &sel, const TrimOptions &opts = TrimOptions(), int device = -1) { return Trims::of(nullptr, &sel.source(), opts, device); }
inline Trims trim(const nafgpu_encode_source &src, const TrimOptions &opts = TrimOptions(), int device = -1) { return Trims::of(nullptr, &src, opts, device); }

// the k-mers of a selection or a source, and a selection or a source against a set: the screens of a selection index the
// selection's records
inline KmerSet kmers(const Selection &sel, const KmerOptions &opts = KmerOptions(), int device = -1) { return KmerSet::of(nullptr, &sel.source(), opts, device); }
inline KmerSet kmers(const nafgpu_encode_source &src, const KmerOptions &opts = KmerOptions(), int device = -1) { return KmerSet::of(nullptr, &src, opts, device); }
inline Screens screen(const Selection &sel, const KmerSet &set, const ScreenOptions &opts = ScreenOptions(), int device = -1) {
    return Screens::of(nullptr, &sel.source(), set, opts, device);
}
inline Screens screen(const nafgpu_encode_source &src, const KmerSet &set, const ScreenOptions &opts = ScreenOptions(), int device = -1) {
    return Screens::of(nullptr, &src, set, opts, device);
}

// the overlaps of a selection index the selection's records
inline Overlaps overlap(const Selection &sel, const OverlapOptions &opts = OverlapOptions(), int device = -1) { return Overlaps::of(nullptr, &sel.source(), opts, device); }
inline Overlaps overlap(const nafgpu_encode_source &src, const OverlapOptions &opts = OverlapOptions(), int device = -1) { return Overlaps::of(nullptr, &src, opts, device); }

// (no counterpart in the reference: the library keeps device memory of closed decoders for the next one -- nafgpu.h)
inline void trim_device_memory(int device = -1) { (void)nafgpu_trim_device_memory(device); }

}  // namespace nafcodec
