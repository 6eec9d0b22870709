// tests/group_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_group through the C-ABI, against expectations computed here in plain C++ (a map from the canonicalised letters of a
// record to the first record that has them): every record length the kernels take another path at, equal records at every
// residue of their start, records one letter apart (first, last, at a tile edge) or one letter shorter, empty records, every
// record equal and no two equal, a duplicate around a long record, letters outside the alphabet, both strands, both
// alphabets, hashes cut to 0 bits; and the refusals, hand-made end tables among them.  On the CPU harness host memory is
// device memory, so the sections are allocations of exactly their size at four alignments and the end tables vectors of
// exactly theirs: a read outside them is a finding.
// `make group-asan` (tests/test_group_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0, or
// says what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096, kRun = 16;      // group.h: kGrpTile, kGrpRun

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

std::string letters(Rng &rng, uint64_t n, const char *alphabet = "ACGT") {
    const size_t k = std::strlen(alphabet);
    std::string out(n, ' ');
    for (char &c : out) c = alphabet[rng.next() % k];
    return out;
}

// the rules of include/nafgpu.h: what a letter is compared as, and its complement
char canon(char c) {
    for (const char *p = "ACGTURYKMSWBDHVN"; *p; p++)
        if (c == *p || c == (*p | 0x20)) return *p == 'U' ? 'T' : *p;
    return c;
}
char complement(char c) {
    const char *pairs = "ATCGRYKMBVDH";
    for (int i = 0; pairs[i]; i += 2) {
        if (c == pairs[i]) return pairs[i + 1];
        if (c == pairs[i + 1]) return pairs[i];
    }
    return c;
}
std::string canonical(const std::string &s, bool nucleotide) {
    std::string out = s;
    if (nucleotide)
        for (char &c : out) c = canon(c);
    return out;
}
std::string reverse_complement(const std::string &s) {
    std::string out(s.rbegin(), s.rend());
    for (char &c : out) c = complement(canon(c));
    return out;
}

struct Options {
    bool nucleotide = true, both = false;
};

struct Want {
    std::vector<uint64_t> representative, group_of, group_first, group_size;
    std::vector<uint8_t> strand;
};

Want brute(const std::vector<std::string> &records, const Options &o) {
    Want w;
    std::map<std::string, uint64_t> first;
    std::vector<std::string> seen;
    for (uint64_t k = 0; k < records.size(); k++) {
        const std::string c = canonical(records[k], o.nucleotide);
        seen.push_back(c);
        const std::string key = o.both ? std::min(c, reverse_complement(c)) : c;
        const uint64_t at = first.emplace(key, k).first->second;
        w.representative.push_back(at);
        w.strand.push_back(c != seen[at]);
        if (at == k) w.group_first.push_back(k);
    }
    w.group_size.assign(w.group_first.size(), 0);
    for (uint64_t at : w.representative) {
        const uint64_t g = std::lower_bound(w.group_first.begin(), w.group_first.end(), at) - w.group_first.begin();
        w.group_of.push_back(g);
        w.group_size[g]++;
    }
    return w;
}

// a copy in a block of exactly shift + n bytes, 16-byte aligned: the copy begins at an address with the low bits `shift`
// and the block ends with it
uint8_t *exact(const std::string &bytes, uint32_t shift) {
    void *p = nullptr;
    expect(posix_memalign(&p, 16, bytes.size() + shift ? bytes.size() + shift : 1) == 0, "posix_memalign");
    if (!bytes.empty()) std::memcpy(static_cast<uint8_t *>(p) + shift, bytes.data(), bytes.size());
    return static_cast<uint8_t *>(p) + shift;
}

template <class T>
void same(nafgpu_groups *g, const T *d_ptr, const std::vector<T> &want, const std::string &what) {
    expect(d_ptr != nullptr, what + ": no table");
    std::vector<T> got(want.size());
    expect(nafgpu_groups_copy_to_host(g, d_ptr, sizeof(T) * want.size(), got.data()) == NAFGPU_OK, what + ": copy");
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i])
            die(what + " differs at " + std::to_string(i) + ": " + std::to_string(static_cast<uint64_t>(got[i])) + " / " +
                std::to_string(static_cast<uint64_t>(want[i])));
}

// one call at four alignments, compared with the map above; -> the number of groups.  rounds 0: any number
uint64_t check(const std::string &what, const std::vector<std::string> &records, const Options &o = Options(), uint32_t rounds = 1) {
    const Want want = brute(records, o);
    std::string text;
    std::vector<uint64_t> ends;
    for (const std::string &r : records) {
        text += r;
        ends.push_back(text.size());
    }
    for (uint32_t shift : {0u, 1u, 7u, 15u}) {
        const std::string where = what + ", shift " + std::to_string(shift);
        uint8_t *l = exact(text, shift);
        nafgpu_encode_source src;
        std::memset(&src, 0, sizeof src);
        src.d_sequence = l;
        src.n_bases = text.size();
        src.d_record_end = ends.empty() ? nullptr : ends.data();
        src.n_records = ends.size();
        nafgpu_group_opts c;
        std::memset(&c, 0, sizeof c);
        c.alphabet = o.nucleotide ? 0 : 1;
        c.both_strands = o.both;
        nafgpu_groups *g = nullptr;
        nafgpu_group_result r;
        nafgpu_error err;
        expect(nafgpu_group(&src, &c, 0, &g, &r, &err) == NAFGPU_OK, where + ": " + err.message);
        expect(r.n_records == records.size() && r.n_groups == want.group_first.size() && r.n_bases == text.size(),
               where + ": " + std::to_string(r.n_groups) + " groups, " + std::to_string(want.group_first.size()) + " expected");
        same(g, r.d_representative, want.representative, where + ": representative");
        same(g, r.d_group_of, want.group_of, where + ": group_of");
        same(g, r.d_group_first, want.group_first, where + ": group_first");
        same(g, r.d_group_size, want.group_size, where + ": group_size");
        if (o.both) same(g, r.d_strand, want.strand, where + ": strand");
        else expect(r.d_strand == nullptr, where + ": a strand table on one strand");
        const uint64_t largest = want.group_size.empty() ? 0 : *std::max_element(want.group_size.begin(), want.group_size.end());
        expect(r.largest_group == largest, where + ": largest_group");
        expect(records.empty() ? r.rounds == 0 : (rounds ? r.rounds == rounds : r.rounds >= 1), where + ": " + std::to_string(r.rounds) + " rounds");
        nafgpu_groups_free(g);
        std::free(l - shift);
    }
    return want.group_first.size();
}

std::string changed(std::string s, uint64_t at) {
    s[at] = s[at] == 'C' ? 'A' : 'C';
    return s;
}

std::vector<std::string> edge_records(Rng &rng) {
    std::vector<std::string> records;
    // the lengths, each twice with other records between; a copy in lower case, one reversed and complemented
    const uint64_t lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, kTile - 1, kTile, kTile + 1, kRun * kTile - 1, kRun * kTile + 1, 3 * kRun * kTile + 5};
    for (uint64_t l : lengths) records.push_back(letters(rng, l));
    const size_t n = records.size();
    for (size_t k = 0; k < n; k++) {
        std::string copy = records[(k * 5) % n];
        if (k % 3 == 1)
            for (char &c : copy) c = static_cast<char>(c | 0x20);
        if (k % 3 == 2) copy = reverse_complement(copy);
        records.push_back(copy);
        records.push_back(letters(rng, rng.next() % 40));
    }
    // one letter apart: first, last, at the tile edges of the record and of the section; one letter shorter, one longer
    const std::string base = letters(rng, 2 * kTile + 7);
    for (const std::string &v : {base, changed(base, 0), changed(base, base.size() - 1), base.substr(0, base.size() - 1), base + "A", base.substr(1), base})
        records.push_back(v);
    for (int k = 0; k < 4; k++) {
        uint64_t start = 0;
        for (const std::string &r : records) start += r.size();
        const uint64_t index = (kTile - start % kTile) % kTile + (k % 2 == 0 ? kTile - 1 : 0);
        records.push_back(changed(base, index % base.size()));
    }
    records.push_back(reverse_complement(base));
    // empty records, the last among them (the first one is: length 0 leads the list); letters outside the alphabet
    for (const char *s : {"", "AC-GT", "ac-gu", "AC.GT", "ACXGT", "acxgt", "ACxGT", "ARG", "CYT", "GAATTC", "gaauuc", "ACGTA", "TACGT", "A-C", "G-T", "N", "", ""})
        records.push_back(s);
    return records;
}

void edges() {
    Rng rng{20241019};
    const std::vector<std::string> records = edge_records(rng);
    Options one, both, bytes;
    both.both = true;
    bytes.nucleotide = false;
    const uint64_t a = check("edges, one strand", records, one), b = check("edges, both strands", records, both), c = check("edges, bytes", records, bytes);
    expect(b < a && a < c, "edges: " + std::to_string(b) + " < " + std::to_string(a) + " < " + std::to_string(c) + " groups expected");
    // equal records whose starts take every residue
    for (uint64_t l : {5u, 77u}) {
        std::vector<std::string> recs;
        const std::string seq = letters(rng, l);
        uint64_t at = 0;
        for (uint64_t residue = 0; residue < 16; residue++) {
            if (residue) {
                const uint64_t pad = (residue + 16 - at % 16) % 16 ? (residue + 16 - at % 16) % 16 : 16;
                recs.push_back(letters(rng, pad));
                at += pad;
            }
            expect(at % 16 == residue, "residue");
            recs.push_back(residue % 3 == 2 ? reverse_complement(seq) : seq);
            at += l;
        }
        check("every residue", recs, both);
        check("every residue, one strand", recs, one);
    }
    // around the 8-letter words
    for (const std::string &word : {std::string("ACGTACGTA"), std::string("ACGTACGTACGTACGTA")}) {
        std::vector<std::string> near{word};
        for (size_t i = 0; i < word.size(); i++) {
            near.push_back(changed(word, i));
            near.push_back(word.substr(0, i));
            near.push_back(reverse_complement(word.substr(i)));
        }
        near.push_back(word);
        check("words", near, one);
        check("words, both strands", near, both);
    }
    expect(check("every record equal", std::vector<std::string>(700, "ACGTTGCATT"), both) == 1, "every record equal");
    std::vector<std::string> distinct;
    for (int k = 0; k < 1500; k++) distinct.push_back(std::to_string(k) + ".");
    expect(check("no two equal", distinct, one) == 1500, "no two equal");
    expect(check("only empty records", std::vector<std::string>(5, ""), both) == 1, "only empty records");
    check("no records", {}, one);
    // hashes cut to 0 bits: every length is one key, so the table rounds are reached, and the answer is the same
    setenv("NAFGPU_GRP_HASH_BITS", "0", 1);
    nafgpu_test_hooks(1);
    std::vector<std::string> few(records.begin(), records.begin() + 20);
    few.insert(few.end(), records.end() - 30, records.end());
    check("0 hash bits", few, both, 0);
    check("0 hash bits, one strand", few, one, 0);
    nafgpu_test_hooks(0);
    unsetenv("NAFGPU_GRP_HASH_BITS");
}

void refusals() {
    Rng rng{7};
    const std::string text = letters(rng, 2100);
    uint8_t *l = exact(text, 0);
    std::vector<uint64_t> good(200);
    for (size_t k = 0; k < good.size(); k++) good[k] = 10 * (k + 1);
    auto call = [&](const uint8_t *seq, const std::vector<uint64_t> *ends, uint64_t n_records, uint8_t alphabet, uint8_t both, std::string *message) {
        nafgpu_encode_source src;
        std::memset(&src, 0, sizeof src);
        src.d_sequence = seq;
        src.n_bases = text.size();
        src.d_record_end = ends ? ends->data() : nullptr;
        src.n_records = n_records;
        nafgpu_group_opts c;
        std::memset(&c, 0, sizeof c);
        c.alphabet = alphabet;
        c.both_strands = both;
        nafgpu_groups *g = nullptr;
        nafgpu_group_result r;
        nafgpu_error err;
        const int rc = nafgpu_group(&src, &c, 0, &g, &r, &err);
        if (message) *message = err.message;
        if (rc == NAFGPU_OK) nafgpu_groups_free(g);
        else expect(g == nullptr && r.n_records == 0 && r.d_representative == nullptr, "a refusal produced something");
        return rc;
    };
    expect(call(l, &good, 200, 0, 1, nullptr) == NAFGPU_OK, "a good table");
    expect(call(nullptr, &good, 200, 0, 0, nullptr) == NAFGPU_E_INVALID_ARG, "no letters");
    expect(call(l, nullptr, 200, 0, 0, nullptr) == NAFGPU_E_INVALID_ARG, "records without a table");
    expect(call(l, &good, 200, 2, 0, nullptr) == NAFGPU_E_INVALID_ARG, "alphabet 2");
    expect(call(l, &good, 200, 1, 1, nullptr) == NAFGPU_E_INVALID_ARG, "both strands as bytes");
    expect(call(l, nullptr, 0, 0, 0, nullptr) == NAFGPU_OK, "no records");
    struct Bad {
        std::vector<std::pair<size_t, uint64_t>> change;
        const char *needle;
    };
    const std::vector<Bad> bad = {{{{100, 500}}, "record 100 "}, {{{100, 500}, {60, 300}, {199, 1}}, "record 60 "}, {{{199, text.size() + 1}}, "record 199 "},
                                  {{{199, UINT64_MAX}}, "record 199 "}, {{{0, 1ull << 40}}, "record 0 "}, {{{199, 1989}}, "record 199 "},
                                  {{{50, 1ull << 50}, {51, 510}}, "record 50 "}};
    for (const Bad &b : bad)
        for (uint8_t both : {0, 1}) {
            std::vector<uint64_t> table = good;
            for (const auto &c : b.change) table[c.first] = c.second;
            std::string message;
            expect(call(l, &table, 200, 0, both, &message) == NAFGPU_E_INVALID_LENGTH && message.find(b.needle) != std::string::npos,
                   std::string("end table, ") + b.needle + ": " + message);
        }
    nafgpu_groups *g = nullptr;
    nafgpu_group_result r;
    nafgpu_group_opts c{};
    nafgpu_encode_source src{};
    src.d_sequence = l;
    src.n_bases = text.size();
    expect(nafgpu_group(nullptr, &c, 0, &g, &r, nullptr) == NAFGPU_E_INVALID_ARG && nafgpu_group(&src, nullptr, 0, &g, &r, nullptr) == NAFGPU_E_INVALID_ARG &&
               nafgpu_group(&src, &c, 0, nullptr, &r, nullptr) == NAFGPU_E_INVALID_ARG && nafgpu_group(&src, &c, 0, &g, nullptr, nullptr) == NAFGPU_E_INVALID_ARG,
           "null arguments");
    expect(nafgpu_groups_copy_to_host(nullptr, nullptr, 1, nullptr) == NAFGPU_E_INVALID_ARG, "copy from nothing");
    nafgpu_groups_free(nullptr);
    std::free(l);
}

}  // namespace

int main() {
    edges();
    refusals();
    std::printf("OK\n");
    return 0;
}
