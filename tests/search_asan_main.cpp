// tests/search_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_search through the C-ABI, against expectations computed here in plain C++ (a loop over every window of every
// record): pattern lengths 1 .. 64, occurrences at the section's first and last letter, around tile and lane edges and at
// record ends, records of 0, 1, m - 1 and m letters and runs of empty ones, overlapping hits, the densest output there is,
// windows with exactly d substitutions, IUPAC letters in patterns and texts, both strands, both alphabets; and the refusals,
// hand-made end tables among them.  On the CPU harness host memory is device memory, so the sections are allocations of
// exactly their size at four alignments and the end tables vectors of exactly theirs: a read outside them is a finding.
// `make search-asan` (tests/test_search_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0, or
// says what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096;                 // search.h: kSearchTile

[[noreturn]] void die(const std::string &what) {
    std::printf("FAILED: %s\n", what.c_str());
    std::exit(1);
}
void expect(bool ok, const std::string &what) {
    if (!ok) die(what);
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return s >> 33;
    }
};

uint8_t set_of(uint8_t b) {
    const char *letters = "ACGTURYKMSWBDHVN";
    const uint8_t sets[] = {1, 2, 4, 8, 8, 5, 10, 12, 3, 6, 9, 14, 13, 11, 7, 15};
    for (int i = 0; letters[i]; i++)
        if (b == letters[i] || b == (letters[i] | 0x20)) return sets[i];
    return 0;
}
uint8_t reverse4(uint8_t s) { return static_cast<uint8_t>(((s & 1) << 3) | ((s & 2) << 1) | ((s & 4) >> 1) | ((s & 8) >> 3)); }

struct Hit {
    uint64_t at, pattern, strand, mismatches, record, start, end;
    bool operator<(const Hit &o) const { return std::tie(at, pattern, strand) < std::tie(o.at, o.pattern, o.strand); }
};

struct Options {
    bool nucleotide = true, both = true;
    uint32_t k = 0;
};

// the rules of include/nafgpu.h, window by window
std::vector<Hit> brute(const std::vector<uint8_t> &text, const std::vector<uint64_t> &ends_in, const std::vector<std::string> &patterns, const Options &o) {
    std::vector<uint64_t> ends = ends_in;
    if (ends.empty()) ends.push_back(text.size());
    std::vector<Hit> out;
    uint64_t begin = 0;
    for (size_t r = 0; r < ends.size(); begin = ends[r], r++)
        for (size_t p = 0; p < patterns.size(); p++) {
            const std::string &pat = patterns[p];
            const uint64_t m = pat.size();
            for (uint64_t s = begin; s + m <= ends[r]; s++)
                for (uint64_t strand = 0; strand < (o.both ? 2u : 1u); strand++) {
                    uint64_t miss = 0;
                    for (uint64_t j = 0; j < m; j++) {
                        const uint8_t t = text[s + j];
                        if (!o.nucleotide) {
                            miss += t != static_cast<uint8_t>(pat[j]);
                            continue;
                        }
                        const uint8_t want = strand ? reverse4(set_of(static_cast<uint8_t>(pat[m - 1 - j]))) : set_of(static_cast<uint8_t>(pat[j]));
                        miss += set_of(t) == 0 || (set_of(t) & ~want) != 0;
                    }
                    if (miss <= o.k) out.push_back(Hit{s, p, strand, miss, r, s - begin, s - begin + m});
                }
        }
    std::sort(out.begin(), out.end());
    return out;
}

// a copy in a block of exactly shift + n bytes, 16-byte aligned: the copy begins at an address with the low bits `shift`
// and the block ends with it
uint8_t *exact(const std::vector<uint8_t> &bytes, uint32_t shift) {
    void *p = nullptr;
    expect(posix_memalign(&p, 16, bytes.size() + shift ? bytes.size() + shift : 1) == 0, "posix_memalign");
    if (!bytes.empty()) std::memcpy(static_cast<uint8_t *>(p) + shift, bytes.data(), bytes.size());
    return static_cast<uint8_t *>(p) + shift;
}

std::string joined(const std::vector<std::string> &patterns) {
    std::string blob;
    for (const std::string &p : patterns) blob.append(p).push_back('\0');
    return blob;
}

nafgpu_search_opts c_options(const Options &o, uint64_t max_hits = 0) {
    nafgpu_search_opts c;
    std::memset(&c, 0, sizeof c);
    c.alphabet = o.nucleotide ? 0 : 1;
    c.both_strands = o.both;
    c.max_mismatches = static_cast<uint8_t>(o.k);
    c.max_hits = max_hits;
    return c;
}

// one call at four alignments, compared with the loop above; -> the number of hits
uint64_t check(const std::string &what, const std::vector<uint8_t> &text, const std::vector<uint64_t> &ends, const std::vector<std::string> &patterns,
               const Options &o = Options()) {
    const std::vector<Hit> want = brute(text, ends, patterns, o);
    const std::string blob = joined(patterns);
    for (uint32_t shift : {0u, 1u, 7u, 15u}) {
        const std::string where = what + ", shift " + std::to_string(shift);
        uint8_t *l = exact(text, shift);
        nafgpu_encode_source src;
        std::memset(&src, 0, sizeof src);
        src.d_sequence = l;
        src.n_bases = text.size();
        src.d_record_end = ends.empty() ? nullptr : ends.data();
        src.n_records = ends.size();
        const nafgpu_search_opts c = c_options(o);
        nafgpu_hits *h = nullptr;
        nafgpu_search_result r;
        nafgpu_error err;
        expect(nafgpu_search(&src, reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), patterns.size(), &c, 0, &h, &r, &err) == NAFGPU_OK,
               where + ": " + err.message);
        const uint64_t n_rec = ends.empty() ? 1 : ends.size();
        expect(r.n_hits == want.size() && r.n_records == n_rec && r.n_bases == text.size(),
               where + ": " + std::to_string(r.n_hits) + " hits, " + std::to_string(want.size()) + " expected");
        std::vector<nafgpu_region> regions(want.size());
        std::vector<nafgpu_hit_info> info(want.size());
        std::vector<uint64_t> begin(n_rec + 1), per_pattern(NAFGPU_SEARCH_MAX_PATTERNS, 0);
        expect(nafgpu_hits_copy_to_host(h, r.d_regions, regions.size() * sizeof(nafgpu_region), regions.data()) == NAFGPU_OK, where + ": copy");
        expect(nafgpu_hits_copy_to_host(h, r.d_info, info.size() * sizeof(nafgpu_hit_info), info.data()) == NAFGPU_OK, where + ": copy");
        expect(nafgpu_hits_copy_to_host(h, r.d_record_hit_begin, begin.size() * 8, begin.data()) == NAFGPU_OK, where + ": copy");
        for (size_t i = 0; i < want.size(); i++) {
            const Hit &w = want[i];
            const bool same = regions[i].record == w.record && regions[i].start == w.start && regions[i].end == w.end && regions[i].reverse_complement == w.strand &&
                              info[i].pattern == w.pattern && info[i].mismatches == w.mismatches;
            if (!same)
                die(where + ": hit " + std::to_string(i) + ": record " + std::to_string(regions[i].record) + " start " + std::to_string(regions[i].start) +
                    " pattern " + std::to_string(info[i].pattern) + " / record " + std::to_string(w.record) + " start " + std::to_string(w.start) + " pattern " +
                    std::to_string(w.pattern));
            per_pattern[w.pattern]++;
        }
        size_t at = 0;
        for (uint64_t k = 0; k <= n_rec; k++) {
            while (at < want.size() && want[at].record < k) at++;
            expect(begin[k] == at, where + ": record_hit_begin of record " + std::to_string(k));
        }
        for (size_t p = 0; p < NAFGPU_SEARCH_MAX_PATTERNS; p++) expect(r.pattern_hits[p] == per_pattern[p], where + ": pattern_hits");
        nafgpu_hits_free(h);
        std::free(l - shift);
    }
    return want.size();
}

std::vector<uint64_t> ends_of(const std::vector<uint64_t> &lengths) {
    std::vector<uint64_t> out;
    uint64_t at = 0;
    for (uint64_t l : lengths) out.push_back(at += l);
    return out;
}

std::vector<uint8_t> random_text(Rng &rng, size_t n, const char *alphabet) {
    const size_t k = std::strlen(alphabet);
    std::vector<uint8_t> out(n);
    for (uint8_t &b : out) b = static_cast<uint8_t>(alphabet[rng.next() % k]);
    return out;
}

void plant(std::vector<uint8_t> &text, uint64_t at, const std::string &pattern) { std::memcpy(text.data() + at, pattern.data(), pattern.size()); }

void refused(const std::string &what, const nafgpu_encode_source &src, const std::string &blob, uint64_t n_patterns, const nafgpu_search_opts *o, int status,
             const char *needle) {
    nafgpu_hits *h = reinterpret_cast<nafgpu_hits *>(1);
    nafgpu_search_result r;
    std::memset(&r, 0xFF, sizeof r);
    nafgpu_error err;
    const int rc = nafgpu_search(&src, reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), n_patterns, o, 0, &h, &r, &err);
    expect(rc == status && err.status == rc, what + ": status " + std::to_string(rc) + " " + err.message);
    expect(std::strstr(err.message, needle) != nullptr, what + ": " + err.message);
    expect(h == nullptr && r.d_regions == nullptr && r.n_hits == 0 && r.n_records == 0, what + ": something was produced");
}

void edges() {
    Rng rng{2024};
    // pattern lengths; the first and the last letter; around a tile edge and a lane edge; records cut at random
    for (uint64_t m : {1u, 2u, 15u, 16u, 17u, 63u, 64u}) {
        std::vector<uint8_t> text = random_text(rng, 2 * kTile + 100, "ACGT");
        const std::vector<uint8_t> p = random_text(rng, m, "ACGT");
        const std::string pattern(p.begin(), p.end());
        plant(text, 0, pattern);
        plant(text, text.size() - m, pattern);
        plant(text, kTile - m, pattern);                     // ends at a tile edge
        plant(text, kTile, pattern);                         // begins at one
        plant(text, 2 * kTile - m / 2 - 1, pattern);         // lies across one
        for (uint64_t i = 0; i <= 16; i++) plant(text, 112 + 81 * i, pattern);
        Options one;
        one.both = false;
        expect(check("m = " + std::to_string(m) + ", one record", text, {text.size()}, {pattern}, one) >= 22, "the planted occurrences");
        std::vector<uint64_t> lengths;
        for (uint64_t at = 0; at < text.size();) {
            lengths.push_back(std::min<uint64_t>(rng.next() % 700, text.size() - at));
            at += lengths.back();
        }
        Options k1;
        k1.k = m > 1 ? 1 : 0;
        check("m = " + std::to_string(m) + ", records", text, ends_of(lengths), {pattern, std::string(m, 'N')}, k1);
        check("m = " + std::to_string(m) + ", no record table", text, {}, {pattern});
    }
    // records of 0, 1, m - 1, m letters, runs of empty ones, a window at and one letter past a record end: every start (all-N)
    for (uint64_t m : {1u, 5u, 16u, 64u}) {
        std::vector<uint64_t> lengths = {0, 1, m - 1, m, 0, 0, 0, m + 1, 0};
        lengths.insert(lengths.end(), 300, 0);
        for (uint64_t l : {m, m, 2 * m, uint64_t(1), uint64_t(0), 3 * m + 7, kTile - 3 * m, m, kTile + 1, uint64_t(0), uint64_t(0)}) lengths.push_back(l);
        const std::vector<uint64_t> ends = ends_of(lengths);
        std::vector<uint8_t> text = random_text(rng, ends.back() + 37, "ACGTacgtNRY-");       // 37 letters behind the last record
        uint64_t n = 0;
        for (uint64_t l : lengths) n += l >= m ? l - m + 1 : 0;
        Options one;
        one.both = false;
        expect(check("record ends, m = " + std::to_string(m), text, ends, {std::string(m, 'N'), std::string(m, 'n')}, one) <= 2 * n, "all-N hits");
    }
    check("homopolymer", std::vector<uint8_t>(100, 'A'), {100}, {"AAAA"});
    // the densest output: sixteen all-N patterns on both strands over two full tiles
    {
        std::vector<std::string> patterns;
        uint64_t n = 0;
        for (uint64_t p = 0; p < 16; p++) patterns.push_back(std::string(1 + 4 * p, 'N')), n += 2 * (2 * kTile - 4 * p);
        expect(check("sixteen all-N patterns", random_text(rng, 2 * kTile, "ACGT"), {2 * kTile}, patterns) == n, "32 hits per position");
    }
    // exactly d substitutions, in the first and in the last position
    {
        const std::vector<uint8_t> p = random_text(rng, 24, "ACGT");
        const std::string pattern(p.begin(), p.end());
        std::vector<uint8_t> text = random_text(rng, kTile + 900, "ACGT");
        for (uint64_t d = 0; d < 5; d++)
            for (uint64_t side = 0; side < 2; side++) {
                std::string w = pattern;
                for (uint64_t i = 0; i < d; i++) {
                    const size_t j = i == 0 ? (side ? w.size() - 1 : 0) : 3 + 4 * (i - 1);
                    w[j] = w[j] == 'A' ? 'C' : 'A';
                }
                plant(text, kTile - 300 + 61 * (2 * d + side), w);
            }
        for (uint32_t k = 0; k < 4; k++) {
            Options o;
            o.k = k;
            o.both = false;
            expect(check("substitutions, k = " + std::to_string(k), text, {text.size()}, {pattern}, o) >= 2 * (k + 1), "planted windows");
        }
    }
    // IUPAC both ways, U and T, the reverse strand, duplicates, zero hits, the bytes alphabet
    {
        const std::string t = "AGRN-CTYacgtrynWSKMBDHVUu";
        std::vector<uint8_t> text(t.begin(), t.end());
        const std::vector<uint8_t> more = random_text(rng, 700, "AGRN-CTYUWSKMBDHVacgt");
        text.insert(text.end(), more.begin(), more.end());
        Options k1;
        k1.k = 1;
        check("IUPAC", text, {25, 25, text.size()}, {"R", "N", "RYN", "NRY", "ARN", "UU", "TT", "GATTACA", "GATTACA", "BDHV"});
        check("IUPAC, one substitution", text, {25, 25, text.size()}, {"RYN", "NRY", "ARN", "UU", "acgu"}, k1);
        check("zero hits", random_text(rng, 500, "AC"), {100, 500}, {"GGGGGGGG", "TTTTTTTTTTTT"});
        Options bytes;
        bytes.nucleotide = false;
        bytes.both = false;
        std::vector<uint8_t> protein = random_text(rng, 3 * kTile + 5, "ACDEFGHIKLMNPQRSTVWY*acgt \xff\x01");
        const std::string cut(protein.begin() + 4090, protein.begin() + 4101);
        check("bytes", protein, {4000, 4095, 4095, protein.size()}, {cut, "MK", "a", "\xff\x01", std::string(64, 'L')}, bytes);
        bytes.k = 3;
        check("bytes, three substitutions", protein, {4000, 4095, 4095, protein.size()}, {cut, "MKLV", std::string(64, 'L')}, bytes);
    }
    check("nothing", {}, {0, 0}, {"ACGT"});
    check("one letter", {uint8_t('g')}, {0, 0, 1, 1}, {"G", "C", "N"});
}

void refusals() {
    Rng rng{7};
    const std::vector<uint8_t> text = random_text(rng, 10000, "ACGT");
    std::vector<uint64_t> good;
    for (uint64_t k = 1; k <= 1000; k++) good.push_back(10 * k);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = text.data();
    src.n_bases = text.size();
    src.d_record_end = good.data();
    src.n_records = good.size();
    const int bad = NAFGPU_E_INVALID_ARG;
    refused("no pattern", src, "", 0, nullptr, bad, "0 patterns");
    refused("seventeen patterns", src, joined(std::vector<std::string>(17, "ACGT")), 17, nullptr, bad, "17 patterns");
    refused("no NUL at the end", src, "ACGT", 1, nullptr, bad, "NUL-terminated");
    refused("a string too few", src, joined({"ACGT"}), 2, nullptr, bad, "NUL-terminated");
    refused("a string too many", src, joined({"ACGT", "GG"}), 1, nullptr, bad, "NUL-terminated");
    refused("an empty pattern", src, joined({"ACGT", "", "GG", ""}), 4, nullptr, bad, "pattern 1:");
    refused("a long pattern", src, joined({"ACGT", "AC", std::string(65, 'A'), ""}), 4, nullptr, bad, "pattern 2:");
    refused("a letter that is none", src, joined({"ACGT", "ACGX", "AC-T"}), 3, nullptr, bad, "pattern 1:");
    nafgpu_search_opts o = c_options(Options());
    o.max_mismatches = 4;
    refused("four substitutions", src, joined({"ACGTACGT"}), 1, &o, bad, "max_mismatches");
    o.max_mismatches = 2;
    refused("as many substitutions as letters", src, joined({"ACGTACGT", "AC"}), 2, &o, bad, "max_mismatches");
    o = c_options(Options());
    o.alphabet = 1;
    refused("both strands of bytes", src, joined({"ACGT"}), 1, &o, bad, "both_strands");
    o.alphabet = 2;
    refused("an alphabet that is none", src, joined({"ACGT"}), 1, &o, bad, "alphabet");
    nafgpu_encode_source none = src;
    none.d_sequence = nullptr;
    refused("no letters", none, joined({"ACGT"}), 1, nullptr, bad, "sequence");
    // max_hits: one below the count is refused, the count is accepted
    Options both;
    const uint64_t n = brute(text, good, {"ACG"}, both).size();
    expect(n > 50, "hits of ACG");
    o = c_options(both, n - 1);
    refused("max_hits one below", src, joined({"ACG"}), 1, &o, bad, std::to_string(n).c_str());
    o.max_hits = n;
    nafgpu_hits *h = nullptr;
    nafgpu_search_result r;
    nafgpu_error err;
    expect(nafgpu_search(&src, reinterpret_cast<const uint8_t *>("ACG"), 4, 1, &o, 0, &h, &r, &err) == NAFGPU_OK && r.n_hits == n, "max_hits equal to the count");
    nafgpu_hits_free(h);
    expect(nafgpu_search(nullptr, reinterpret_cast<const uint8_t *>("ACG"), 4, 1, &o, 0, &h, &r, &err) == bad, "src NULL");
    expect(nafgpu_search(&src, reinterpret_cast<const uint8_t *>("ACG"), 4, 1, &o, 0, nullptr, &r, &err) == bad, "out NULL");
    expect(nafgpu_search(&src, reinterpret_cast<const uint8_t *>("ACG"), 4, 1, &o, 0, &h, nullptr, &err) == bad, "res NULL");
    expect(nafgpu_search(&src, nullptr, 4, 1, &o, 0, &h, &r, &err) == bad, "patterns NULL");
    expect(nafgpu_hits_copy_to_host(nullptr, text.data(), 2, &r) == bad, "copy_to_host of nothing");
    nafgpu_hits_free(nullptr);

    // hand-made end tables: decreasing, beyond the section, the first record bad, the last record bad
    const std::string blob = joined({"ACGT"});
    const int len = NAFGPU_E_INVALID_LENGTH;
    auto with = [&](const std::vector<uint64_t> &ends) {
        nafgpu_encode_source s = src;
        s.d_record_end = ends.data();
        s.n_records = ends.size();
        return s;
    };
    std::vector<uint64_t> table = good;
    table[500] = 4000;
    refused("decreasing", with(table), blob, 1, nullptr, len, "record 500 ");
    table[300] = 2000;
    table[999] = 1;
    refused("decreasing, three of them", with(table), blob, 1, nullptr, len, "record 300 ");
    table = good;
    table[999] = 10001;
    refused("the last record beyond the section", with(table), blob, 1, nullptr, len, "record 999 ");
    table[999] = ~0ull;
    refused("the last record far beyond", with(table), blob, 1, nullptr, len, "record 999 ");
    table = good;
    table[0] = 1ull << 40;
    refused("the first record bad", with(table), blob, 1, nullptr, len, "record 0 ");
    table = good;
    for (uint64_t k = 700; k < 1000; k++) table[k] = (1ull << 33) + k;
    refused("beyond from record 700 on", with(table), blob, 1, nullptr, len, "record 700 ");
    table = good;
    table[999] = 9989;
    refused("the last record below the one in front", with(table), blob, 1, nullptr, len, "record 999 ");
    const std::vector<uint8_t> letter = {uint8_t('A')};
    const std::vector<uint64_t> two = {2};
    nafgpu_encode_source tiny = with(two);
    tiny.d_sequence = letter.data();
    tiny.n_bases = 1;
    refused("one record beyond a section of one letter", tiny, joined({"A"}), 1, nullptr, len, "record 0 ");
    check("after the refusals", text, good, {"ACGT", "NNNNNNNNNN"});
}

}  // namespace

int main() {
    edges();
    refusals();
    std::printf("OK\n");
    return 0;
}
