// tests/summary_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_summarize through the C-ABI, against expectations computed here in plain C++: the edges of the per-record pass
// (record lengths around 16 and around a tile, starts at every residue, tile edges, runs of empty records, long records
// between short ones) under the default table and a table of its own, by every route, with sections at every alignment;
// and the refusals of hand-made end tables.  On the CPU harness host memory is device memory, so the sections and the end
// tables are vectors of exactly their size: a read outside them is a finding.
// `make summary-asan` (tests/test_summary_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0,
// or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096, kRun = 16;      // summary.h: kSumTile, kSumRun

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

void default_table(uint8_t *t) {
    for (int b = 0; b < 256; b++) t[b] = 64;
    const char *cols[6] = {"A", "C", "G", "TU", "N", "RYKMSWBDHV"};
    for (int c = 0; c < 6; c++)
        for (const char *p = cols[c]; *p; p++) t[static_cast<uint8_t>(*p)] = t[static_cast<uint8_t>(*p) | 0x20] = static_cast<uint8_t>(1 << c);
    for (int b = 'a'; b <= 'z'; b++) t[b] |= 128;
}

std::vector<uint64_t> fetch(nafgpu_summary *s, const uint64_t *d_ptr, uint64_t n) {
    std::vector<uint64_t> out(static_cast<size_t>(n));
    expect(d_ptr != nullptr, "a table is missing");
    expect(nafgpu_summary_copy_to_host(s, d_ptr, 8 * n, out.data()) == NAFGPU_OK, "summary_copy_to_host");
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

// one call, compared with a plain loop
void check(const std::string &what, const std::vector<uint8_t> &letters, const std::vector<uint8_t> *quals, const std::vector<uint64_t> &ends,
           const uint8_t *table, uint32_t shift) {
    const uint64_t n = letters.size();
    uint8_t *l = exact(letters, shift), *q = quals ? exact(*quals, shift) : nullptr;
    const uint8_t *lp = l, *qp = q;
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = lp;
    src.n_bases = n;
    src.d_quality = qp;
    src.n_quality = qp ? n : 0;
    src.d_record_end = ends.data();
    src.n_records = ends.size();
    nafgpu_summary_opts o;
    std::memset(&o, 0, sizeof o);
    uint8_t def[256];
    default_table(def);
    if (table) {
        std::memcpy(o.classes, table, 256);
        o.use_classes = 1;
    }
    const uint8_t *t = table ? table : def;
    nafgpu_summary *s = nullptr;
    nafgpu_summary_result r;
    nafgpu_error err;
    expect(nafgpu_summarize(&src, table ? &o : nullptr, 0, &s, &r, &err) == NAFGPU_OK, what + ": " + err.message);
    expect(r.n_records == ends.size() && r.n_bases == n && r.n_quality == (qp ? n : 0), what + ": sizes");
    std::vector<uint64_t> want(ends.size() * 8, 0), want_q(ends.size(), 0), want_h(256, 0), want_qh(256, 0), totals(8, 0);
    uint64_t at = 0, q_total = 0;
    for (size_t k = 0; k < ends.size(); k++)
        for (; at < ends[k]; at++) {
            for (int c = 0; c < 8; c++) want[8 * k + c] += t[letters[at]] >> c & 1, totals[c] += t[letters[at]] >> c & 1;
            if (quals) want_q[k] += (*quals)[at], q_total += (*quals)[at];
        }
    for (uint64_t i = 0; i < n; i++) want_h[letters[i]]++;
    if (quals)
        for (uint64_t i = 0; i < n; i++) want_qh[(*quals)[i]]++;
    if (!ends.empty()) {
        const std::vector<uint64_t> got = fetch(s, r.d_counts, 8 * ends.size());
        for (size_t i = 0; i < got.size(); i++)
            if (got[i] != want[i]) die(what + ": record " + std::to_string(i / 8) + " column " + std::to_string(i % 8) + ": " + std::to_string(got[i]) + " / " + std::to_string(want[i]));
        if (quals) expect(fetch(s, r.d_quality_sum, ends.size()) == want_q, what + ": quality sums");
        for (int c = 0; c < 8; c++) expect(r.totals[c] == totals[c], what + ": totals");
        expect(r.quality_total == q_total, what + ": quality total");
    } else {
        expect(!r.d_counts && !r.d_quality_sum, what + ": tables without records");
    }
    expect(fetch(s, r.d_letter_hist, 256) == want_h, what + ": letter histogram");
    if (quals) expect(fetch(s, r.d_quality_hist, 256) == want_qh, what + ": quality histogram");
    else expect(!r.d_quality_hist, what + ": a quality histogram without qualities");
    nafgpu_summary_free(s);
    std::free(l - shift);
    if (q) std::free(q - shift);
}

std::vector<uint64_t> ends_of(const std::vector<uint64_t> &lengths) {
    std::vector<uint64_t> out;
    uint64_t at = 0;
    for (uint64_t l : lengths) out.push_back(at += l);
    return out;
}

std::vector<uint64_t> edge_lengths() {
    std::vector<uint64_t> l = {0, 0, 1, 15, 16, 17, kTile - 1, kTile, kTile + 1};
    uint64_t pos = 0;
    for (uint64_t v : l) pos += v;
    for (uint64_t r = 0; r < 16; r++) l.push_back(16 + r + (r % 3 == 0)), pos += l.back();   // starts at every residue mod 16
    l.push_back(kTile - pos % kTile), pos += l.back();                                          // ends on a tile edge
    l.push_back(kTile), pos += kTile;                                                           // begins and ends on one
    for (int i = 0; i < 600; i++) {                                                             // one-letter records, empty ones among them
        l.push_back(1);
        if (i % 50 == 7) l.push_back(0), l.push_back(0);
    }
    for (int i = 0; i < 300; i++) l.push_back(0);                                               // a run of empty records, then one letter
    l.push_back(1);
    for (int i = 0; i < 40; i++) l.push_back(90 + i);
    l.push_back(3 * kTile + 5);                                                                 // a few tiles between runs of short ones
    for (int i = 0; i < 40; i++) l.push_back(1 + 3 * i);
    l.push_back(kRun * kTile + 77);                                                             // longer than a workgroup's run
    l.push_back(2 * kTile);
    l.push_back(0);
    return l;
}

void refused(const std::string &what, const std::vector<uint8_t> &letters, const std::vector<uint64_t> &ends, const char *needle) {
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = letters.data();
    src.n_bases = letters.size();
    src.d_quality = letters.data();
    src.n_quality = letters.size();
    src.d_record_end = ends.data();
    src.n_records = ends.size();
    nafgpu_summary *s = reinterpret_cast<nafgpu_summary *>(1);
    nafgpu_summary_result r;
    std::memset(&r, 0xFF, sizeof r);
    nafgpu_error err;
    const int rc = nafgpu_summarize(&src, nullptr, 0, &s, &r, &err);
    expect(rc == NAFGPU_E_INVALID_LENGTH && err.status == rc, what + ": status " + std::to_string(rc));
    expect(std::strstr(err.message, needle) != nullptr, what + ": " + err.message);
    expect(s == nullptr && r.d_counts == nullptr && r.n_records == 0, what + ": something was produced");
}

void all_checks(const std::string &route) {
    Rng rng{2024};
    const std::vector<uint64_t> lengths = edge_lengths();
    const std::vector<uint64_t> ends = ends_of(lengths);
    const char *alphabet = "ACGTUNRYKMSWBDHVacgtunrykmswbdhv-*Xx";
    std::vector<uint8_t> letters(ends.back() + 37), quals(ends.back() + 37);                     // 37 letters behind the last record
    for (size_t i = 0; i < letters.size(); i++) {
        letters[i] = i % 97 == 0 ? static_cast<uint8_t>(rng.next()) : static_cast<uint8_t>(alphabet[rng.next() % 36]);
        quals[i] = static_cast<uint8_t>(rng.next());
    }
    uint8_t custom[256];
    for (int b = 0; b < 256; b++) custom[b] = static_cast<uint8_t>(rng.next());
    custom[0] = 0xFF;
    for (uint32_t shift : {0u, 1u, 7u, 15u}) {
        check(route + ": edges, shift " + std::to_string(shift), letters, &quals, ends, nullptr, shift);
        check(route + ": edges, a table of its own, shift " + std::to_string(shift), letters, nullptr, ends, custom, shift);
    }
    std::vector<uint8_t> whole(letters.begin(), letters.begin() + static_cast<long>(ends.back() / 16 * 16));
    std::vector<uint8_t> whole_q(quals.begin(), quals.begin() + static_cast<long>(whole.size()));
    check(route + ": one record, the section of exactly its size", whole, &whole_q, {whole.size()}, custom, 0);
    check(route + ": every record empty", letters, &quals, std::vector<uint64_t>(700, 0), nullptr, 0);
    check(route + ": no records", letters, &quals, {}, nullptr, 0);
    check(route + ": one letter", {uint8_t('g')}, nullptr, {0, 0, 1, 1}, nullptr, 0);
    check(route + ": nothing", {}, nullptr, {0, 0}, nullptr, 0);

    // hand-made end tables: decreasing, beyond the section, the first record bad, the last record bad
    std::vector<uint8_t> small(letters.begin(), letters.begin() + 10000);
    std::vector<uint64_t> good;
    for (uint64_t k = 1; k <= 1000; k++) good.push_back(10 * k);
    std::vector<uint64_t> bad = good;
    bad[500] = 4000;
    refused(route + ": decreasing", small, bad, "record 500 ");
    bad[300] = 2000;
    bad[999] = 1;
    refused(route + ": decreasing, three of them", small, bad, "record 300 ");
    bad = good;
    bad[999] = 10001;
    refused(route + ": the last record beyond the section", small, bad, "record 999 ");
    bad[999] = ~0ull;
    refused(route + ": the last record far beyond", small, bad, "record 999 ");
    bad = good;
    bad[0] = 1ull << 40;
    refused(route + ": the first record bad", small, bad, "record 0 ");
    bad = good;
    for (uint64_t k = 700; k < 1000; k++) bad[k] = (1ull << 33) + k;
    refused(route + ": beyond from record 700 on", small, bad, "record 700 ");
    bad = good;
    bad[999] = 9989;
    refused(route + ": the last record below the one in front", small, bad, "record 999 ");
    refused(route + ": one record beyond a section of one letter", {uint8_t('A')}, {2}, "record 0 ");
    check(route + ": after the refusals", small, nullptr, good, nullptr, 0);
}

}  // namespace

int main() {
    int count = 0;
    nafgpu_error err;
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    nafgpu_summary *s = nullptr;
    nafgpu_summary_result r;
    expect(nafgpu_summarize(&src, nullptr, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG, "both sections absent");
    expect(nafgpu_summarize(nullptr, nullptr, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG, "src NULL");
    const uint8_t two[2] = {'A', 'C'};
    src.d_sequence = src.d_quality = two;
    src.n_bases = 2;
    src.n_quality = 1;
    expect(nafgpu_summarize(&src, nullptr, 0, &s, &r, &err) == NAFGPU_E_INVALID_LENGTH, "n_quality != n_bases");
    src.n_quality = 2;
    expect(nafgpu_summarize(&src, nullptr, 0, nullptr, &r, &err) == NAFGPU_E_INVALID_ARG, "out NULL");
    expect(nafgpu_summarize(&src, nullptr, 0, &s, nullptr, &err) == NAFGPU_E_INVALID_ARG, "res NULL");
    expect(nafgpu_summary_copy_to_host(nullptr, two, 2, &count) == NAFGPU_E_INVALID_ARG, "copy_to_host of nothing");
    nafgpu_summary_free(nullptr);

    all_checks("auto");
    nafgpu_test_hooks(1);
    for (const char *route : {"long", "short"}) {
        setenv("NAFGPU_SUM_ROUTE", route, 1);
        all_checks(route);
    }
    std::printf("OK\n");
    return 0;
}
