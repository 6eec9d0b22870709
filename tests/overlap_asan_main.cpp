// tests/overlap_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_overlap and nafgpu_merge_pairs through the C-ABI, against expectations computed here in plain C++ (the rules of
// include/nafgpu.h as a loop over every shift of every pair): mates of 0, 1, 63 .. 65, 127 .. 129, 1 023, 1 024 and 1 025
// letters both ways, a planted overlap at every shift of a 70 + 66 pair, the outermost shifts of the longest pair, the three
// limits at and one off, ties, N, lower case and U, runs of empty records, letters behind the last end, a pair that is too long
// at every place of a workgroup's pairs; pairs joined through a decoder with the qualities above, equal and below on agreeing and
// disagreeing letters and shifts below, at and above 0; and the refusals, hand-made end tables among them.  On the CPU harness
// host memory is device memory, so the letters are an allocation of exactly their size at four alignments and the end table a
// vector of exactly its size: a read outside them is a finding.
// `make overlap-asan` (tests/test_overlap_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0, or says
// what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr int64_t kCap = NAFGPU_OVERLAP_MAX_LENGTH;

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

int code(char c) {
    switch (c & 0xDF) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': case 'U': return 3;
    default: return 4;
    }
}
char complement(char c) {
    const char *from = "ACGTacgt", *to = "TGCAtgca";
    for (int i = 0; from[i]; i++)
        if (c == from[i]) return to[i];
    return c;
}
std::string rc(const std::string &s) {
    std::string out(s.rbegin(), s.rend());
    for (char &c : out) c = complement(c);
    return out;
}
std::string random_letters(Rng &rng, size_t n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGT"[rng.next() & 3];
    return s;
}

nafgpu_overlap_opts options(unsigned min_overlap = 30, unsigned max_mismatches = 5, unsigned percent = 20, unsigned base = 33) {
    nafgpu_overlap_opts o;
    std::memset(&o, 0, sizeof o);
    o.min_overlap = min_overlap;
    o.max_mismatches = max_mismatches;
    o.max_mismatch_percent = static_cast<uint8_t>(percent);
    o.quality_base = static_cast<uint8_t>(base);
    return o;
}

// the rules, one pair at a time
nafgpu_pair_overlap rules(const std::string &r1, const std::string &r2, const nafgpu_overlap_opts &o) {
    nafgpu_pair_overlap best;
    std::memset(&best, 0, sizeof best);
    const int64_t n1 = static_cast<int64_t>(r1.size()), n2 = static_cast<int64_t>(r2.size());
    if (n1 > kCap || n2 > kCap) {
        best.too_long = 1;
        return best;
    }
    for (int64_t d = -(n2 - 1); d < n1 && n1 && n2; d++) {
        uint32_t m = 0, mm = 0;
        const int64_t lo = std::max<int64_t>(0, d), hi = std::min(n1, d + n2);
        for (int64_t p = lo; p < hi; p++) {
            const int a = code(r1[p]);
            int b = code(r2[n2 - 1 - (p - d)]);
            if (b < 4) b = 3 - b;
            if (a < 4 && b < 4) (a == b ? m : mm)++;
        }
        if (m < std::max(o.min_overlap, 1u) || mm > o.max_mismatches || mm * 100u > o.max_mismatch_percent * (m + mm)) continue;
        if (best.found && (mm > best.mismatches || (mm == best.mismatches && m <= best.matches))) continue;      // (d ascends: the lowest of equals stays)
        best.shift = d;
        best.insert = static_cast<uint64_t>(d + n2);
        best.matches = m;
        best.mismatches = mm;
        best.compared = static_cast<uint32_t>(hi - lo);
        best.found = 1;
    }
    return best;
}

// the reads in a section of exactly its size (plus `behind`), the pointer at residue `pad` of 16
std::vector<nafgpu_pair_overlap> run(const std::string &what, const std::vector<std::string> &reads, const nafgpu_overlap_opts &o, unsigned pad = 0,
                                     const std::string &behind = "") {
    std::string letters;
    std::vector<uint64_t> ends;
    for (const std::string &r : reads) {
        letters += r;
        ends.push_back(letters.size());
    }
    letters += behind;
    const size_t n = letters.size();
    uint8_t *block = static_cast<uint8_t *>(std::malloc(pad + n ? pad + n : 1));
    expect(block != nullptr, "out of memory");
    std::memcpy(block + pad, letters.data(), n);
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = block + pad;
    src.n_bases = n;
    src.d_record_end = ends.data();
    src.n_records = ends.size();
    nafgpu_overlaps *h = nullptr;
    nafgpu_overlap_result res;
    nafgpu_error err;
    const int rc = nafgpu_overlap(&src, &o, 0, &h, &res, &err);
    expect(rc == NAFGPU_OK, what + ": status " + std::to_string(rc) + " " + err.message);
    expect(res.n_records == reads.size() && res.n_pairs == reads.size() / 2 && res.n_bases == n, what + ": n_records / n_pairs / n_bases");
    std::vector<nafgpu_pair_overlap> pairs(res.n_pairs);
    std::vector<nafgpu_region> regions(res.n_records), unmerged(res.n_unmerged);
    expect(nafgpu_overlaps_copy_to_host(h, res.d_pairs, pairs.size() * sizeof pairs[0], pairs.data()) == NAFGPU_OK &&
               nafgpu_overlaps_copy_to_host(h, res.d_regions, regions.size() * sizeof regions[0], regions.data()) == NAFGPU_OK &&
               nafgpu_overlaps_copy_to_host(h, res.d_unmerged_regions, unmerged.size() * sizeof unmerged[0], unmerged.data()) == NAFGPU_OK,
           what + ": copy to host");
    uint64_t found = 0, too_long = 0, cut = 0, matches = 0, mismatches = 0, inserts = 0, left = 0;
    size_t at = 0;
    for (size_t j = 0; j < pairs.size(); j++) {
        const nafgpu_pair_overlap want = rules(reads[2 * j], reads[2 * j + 1], o);
        if (std::memcmp(&pairs[j], &want, sizeof want))
            die(what + ": pair " + std::to_string(j) + " is shift " + std::to_string(pairs[j].shift) + " matches " + std::to_string(pairs[j].matches) + " mismatches " +
                std::to_string(pairs[j].mismatches) + " found " + std::to_string(pairs[j].found) + ", expected shift " + std::to_string(want.shift) + " matches " +
                std::to_string(want.matches) + " mismatches " + std::to_string(want.mismatches) + " found " + std::to_string(want.found));
        found += want.found;
        too_long += want.too_long;
        matches += want.matches;
        mismatches += want.mismatches;
        inserts += want.insert;
        for (size_t m = 0; m < 2; m++) {
            const uint64_t L = reads[2 * j + m].size();
            nafgpu_region r;
            std::memset(&r, 0, sizeof r);
            r.record = 2 * j + m;
            r.end = want.found ? std::min<uint64_t>(L, want.insert) : L;
            expect(!std::memcmp(&regions[2 * j + m], &r, sizeof r), what + ": the region of record " + std::to_string(2 * j + m));
            cut += r.end < L;
            left += r.end;
            if (!want.found) expect(at < unmerged.size() && !std::memcmp(&unmerged[at++], &r, sizeof r), what + ": unmerged regions");
        }
    }
    expect(at == unmerged.size(), what + ": the number of unmerged regions");
    expect(res.n_found == found && res.n_too_long == too_long && res.n_cut == cut && res.matches == matches && res.mismatches == mismatches &&
               res.bases_merged == inserts && res.bases_after_cut == left,
           what + ": totals");
    nafgpu_overlaps_free(h);
    std::free(block);
    return pairs;
}

// a fragment read from both ends; what lies behind its end is adapter
void add_pair(Rng &rng, std::vector<std::string> &reads, size_t n1, size_t n2, const std::string &fragment) {
    const std::string back = rc(fragment);
    reads.push_back(fragment.substr(0, n1) + random_letters(rng, n1 > fragment.size() ? n1 - fragment.size() : 0));
    reads.push_back(back.substr(0, n2) + random_letters(rng, n2 > back.size() ? n2 - back.size() : 0));
}

void analysis(Rng &rng) {
    const size_t lengths[] = {0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025};
    std::vector<std::string> reads;
    for (size_t n1 : lengths)
        for (size_t n2 : lengths) add_pair(rng, reads, n1, n2, random_letters(rng, std::max<size_t>(1, std::max(n1, n2) / 2 + rng.next() % (n1 / 2 + n2 + 2))));
    for (unsigned pad : {0u, 1u, 7u, 15u}) run("lengths", reads, options(1, 3, 20), pad, pad ? "ACGTAC" : "");
    // a too long pair at every place among the pairs of a workgroup; runs of empty records
    std::vector<std::string> some;
    add_pair(rng, some, 70, 80, random_letters(rng, 100));
    for (size_t k = 0; k <= 4; k++) {
        reads.clear();
        for (size_t i = 0; i < 9; i++) {
            if (i == k) {
                reads.push_back(random_letters(rng, 30));
                reads.push_back(random_letters(rng, 1025));
            }
            reads.insert(reads.end(), some.begin(), some.end());
        }
        const std::vector<nafgpu_pair_overlap> pairs = run("too long", reads, options(10), 3, random_letters(rng, 99));
        for (size_t j = 0; j < pairs.size(); j++) expect(pairs[j].too_long == (j == k) && pairs[j].found == (j != k), "too long: which pair");
    }
    reads.assign(6, "");
    reads.insert(reads.end(), some.begin(), some.end());
    for (const char *s : {"", "ACGT", "ACGT", ""}) reads.push_back(s);
    reads.insert(reads.end(), 20, "");
    reads.insert(reads.end(), some.begin(), some.end());
    run("empty records", reads, options(3), 9);

    // a planted overlap at every shift of a 70 + 66 pair
    reads.clear();
    const int64_t n1 = 70, n2 = 66;
    for (int64_t d = -(n2 - 1); d < n1; d++) {
        const std::string x = random_letters(rng, n1);
        std::string y = random_letters(rng, n2);
        for (int64_t p = std::max<int64_t>(0, d); p < std::min(n1, d + n2); p++) y[p - d] = x[p];
        reads.push_back(x);
        reads.push_back(rc(y));
    }
    std::vector<nafgpu_pair_overlap> pairs = run("a plant at every shift", reads, options(8, 0, 20), 5);
    for (int64_t d = -(n2 - 1); d < n1; d++) {
        const int64_t size = std::min(n1, d + n2) - std::max<int64_t>(0, d);
        const nafgpu_pair_overlap &p = pairs[static_cast<size_t>(d + n2 - 1)];
        expect(size >= 8 ? p.found && p.shift == d && p.matches == size : !p.found, "the plant at shift " + std::to_string(d));
    }
    // the outermost shifts of the longest pair
    reads = {"A" + std::string(kCap - 1, 'C'), rc(std::string(kCap - 1, 'G') + "A"), std::string(kCap - 1, 'C') + "A", rc("A" + std::string(kCap - 1, 'G'))};
    pairs = run("the outermost shifts", reads, options(1, 0, 0));
    expect(pairs[0].shift == -(kCap - 1) && pairs[0].insert == 1 && pairs[1].shift == kCap - 1 && pairs[1].insert == 2 * kCap - 1, "the outermost shifts");
    // the three limits: 45 matches and 5 mismatches
    const std::string frag = random_letters(rng, 50);
    std::string r1 = frag;
    for (size_t at : {3u, 11u, 24u, 37u, 49u}) r1[at] = complement(r1[at]);
    const struct { unsigned min_overlap, max_mismatches, percent; bool found; } limits[] = {{45, 5, 20, true}, {46, 5, 20, false}, {40, 4, 20, false},
                                                                                           {40, 5, 10, true}, {40, 5, 9, false}, {0, 5, 100, true}};
    for (const auto &l : limits) expect(run("limits", {r1, rc(frag)}, options(l.min_overlap, l.max_mismatches, l.percent))[0].found == l.found, "a limit");
    // ties, and N, lower case and U
    pairs = run("ties", {std::string(50, 'A'), std::string(40, 'T'), std::string(40, 'A'), std::string(50, 'T'), "ACACACACACACACACACACACACAC", rc("ACACACACACACACAC")},
                options(10));
    expect(pairs[0].shift == 0 && pairs[1].shift == -10 && pairs[2].shift == 0 && pairs[2].matches == 16, "ties");
    std::string marked = frag;
    marked[5] = 'N';
    marked[6] = static_cast<char>(marked[6] | 0x20);
    marked[7] = '-';
    for (char &c : marked)
        if (c == 'T') c = 'U';
    pairs = run("other bytes", {marked, rc(frag)}, options(40));
    expect(pairs[0].found && pairs[0].matches == 48 && pairs[0].mismatches == 0 && pairs[0].compared == 50, "N and '-' are neutral, case and U play no part");
}

void refused(const std::string &what, const nafgpu_encode_source *src, const nafgpu_overlap_opts *o, int status, const char *needle, bool null_out = false) {
    nafgpu_overlaps *h = reinterpret_cast<nafgpu_overlaps *>(1);
    nafgpu_overlap_result res;
    nafgpu_error err;
    std::memset(&err, 0, sizeof err);
    const int rc = nafgpu_overlap(src, o, 0, null_out ? nullptr : &h, &res, &err);
    expect(rc == status && (null_out || h == nullptr) && std::strstr(err.message, needle), what + ": status " + std::to_string(rc) + " " + err.message);
}

void refusals(Rng &rng) {
    const std::string letters = random_letters(rng, 2000);
    std::vector<uint64_t> ends;
    for (uint64_t k = 1; k <= 200; k++) ends.push_back(10 * k);
    uint8_t *block = static_cast<uint8_t *>(std::malloc(letters.size()));
    expect(block != nullptr, "out of memory");
    std::memcpy(block, letters.data(), letters.size());
    nafgpu_encode_source good;
    std::memset(&good, 0, sizeof good);
    good.d_sequence = block;
    good.n_bases = letters.size();
    good.d_record_end = ends.data();
    good.n_records = ends.size();
    const nafgpu_overlap_opts o = options(3);
    refused("null source", nullptr, &o, NAFGPU_E_INVALID_ARG, "null");
    refused("null options", &good, nullptr, NAFGPU_E_INVALID_ARG, "null");
    refused("null out", &good, &o, NAFGPU_E_INVALID_ARG, "null", true);
    nafgpu_encode_source src = good;
    src.d_sequence = nullptr;
    refused("no sequence", &src, &o, NAFGPU_E_INVALID_ARG, "sequence");
    src = good;
    src.d_record_end = nullptr;
    refused("no table", &src, &o, NAFGPU_E_INVALID_ARG, "record table");
    src = good;
    src.n_records = 0;
    refused("no records", &src, &o, NAFGPU_E_INVALID_ARG, "record table");
    src.n_records = 199;
    refused("odd", &src, &o, NAFGPU_E_INVALID_ARG, "odd");
    const nafgpu_overlap_opts wide = options(3, 5, 101);
    refused("percent", &good, &wide, NAFGPU_E_INVALID_ARG, "percent");
    const struct { size_t at; uint64_t value; const char *needle; } tables[] = {{100, 500, "record 100 "}, {199, 2001, "record 199 "}, {199, ~0ull, "record 199 "},
                                                                                  {0, 1ull << 40, "record 0 "}, {60, 300, "record 60 "}};
    for (const auto &t : tables) {
        std::vector<uint64_t> bad(ends);
        bad[t.at] = t.value;
        src = good;
        src.d_record_end = bad.data();
        refused("a bad end table", &src, &o, NAFGPU_E_INVALID_LENGTH, t.needle);
    }
    expect(nafgpu_overlaps_copy_to_host(nullptr, nullptr, 1, nullptr) == NAFGPU_E_INVALID_ARG, "copy_to_host of nothing");
    nafgpu_overlaps_free(nullptr);
    std::free(block);
}

// pairs with qualities through an archive and a decoder: nafgpu_overlap_decoder, nafgpu_merge_pairs
void merge(Rng &rng) {
    std::vector<std::string> reads, quals;
    const std::string frag = random_letters(rng, 5000);
    const struct { size_t n1, n2, F; } shapes[] = {{60, 60, 40}, {60, 60, 60}, {60, 60, 90}, {70, 45, 80}, {45, 70, 80}, {60, 50, 30}};
    for (size_t k = 0; k < 60; k++) {                        // (9 000 letters of merged output: tile edges inside overlaps)
        const auto &s = shapes[k % 6];
        std::vector<std::string> two;
        add_pair(rng, two, k < 6 ? s.n1 : 150, k < 6 ? s.n2 : 150, frag.substr(70 * k, k < 6 ? s.F : 150));
        for (size_t at : {2u, 7u, 12u, 17u}) two[0][at] = complement(two[0][at]);
        two[0][22] = 'N';
        for (const std::string &r : two) {
            std::string q(r.size(), 'I');
            for (char &c : q) c = static_cast<char>(40 + rng.next() % 35);
            reads.push_back(r);
            quals.push_back(q);
        }
        if (k < 6) {                                         // position p of R1 lies at n2 - 1 - (p - d) of R2: above, equal, below, far below
            std::string &q1 = quals[2 * k], &q2 = quals[2 * k + 1];
            const int64_t d = static_cast<int64_t>(s.F) - static_cast<int64_t>(s.n2);
            const int deltas[] = {9, 0, -1, -5};
            const size_t spots[] = {2, 7, 12, 17};
            for (size_t i = 0; i < 4; i++) {
                const int64_t at = static_cast<int64_t>(s.n2) - 1 - (static_cast<int64_t>(spots[i]) - d);
                if (at >= 0 && at < static_cast<int64_t>(s.n2)) q2[at] = static_cast<char>(q1[spots[i]] + deltas[i]);
            }
        }
    }
    nafgpu_encoder_opts eo;
    nafgpu_encoder_opts_default(0, &eo);
    eo.id = eo.comment = eo.sequence = eo.quality = 1;
    eo.compression_level = 1;
    nafgpu_encoder *enc = nullptr;
    nafgpu_error err;
    expect(nafgpu_encoder_new(&eo, &enc, &err) == NAFGPU_OK, "encoder_new");
    for (size_t k = 0; k < reads.size(); k++) {
        const std::string id = "r" + std::to_string(k), comment = "c";
        nafgpu_record rec;
        std::memset(&rec, 0, sizeof rec);
        rec.id = {reinterpret_cast<const uint8_t *>(id.data()), id.size(), 1, {}};
        rec.comment = {reinterpret_cast<const uint8_t *>(comment.data()), comment.size(), 1, {}};
        rec.sequence = {reinterpret_cast<const uint8_t *>(reads[k].data()), reads[k].size(), 1, {}};
        rec.quality = {reinterpret_cast<const uint8_t *>(quals[k].data()), quals[k].size(), 1, {}};
        expect(nafgpu_encoder_push(enc, &rec, &err) == NAFGPU_OK, std::string("encoder_push: ") + err.message);
    }
    const uint8_t *archive = nullptr;
    uint64_t n_archive = 0;
    expect(nafgpu_encoder_finish(enc, &archive, &n_archive, &err) == NAFGPU_OK, "encoder_finish");
    nafgpu_opts dopts;
    nafgpu_opts_default(&dopts);
    nafgpu_decoder *dec = nullptr;
    expect(nafgpu_open_bytes(archive, n_archive, &dopts, &dec, &err) == NAFGPU_OK, std::string("open: ") + err.message);
    for (unsigned base : {33u, 64u}) {
        const nafgpu_overlap_opts o = options(15, 8, 20, base);
        nafgpu_overlaps *h = nullptr;
        nafgpu_overlap_result res;
        expect(nafgpu_overlap_decoder(dec, &o, &h, &res, &err) == NAFGPU_OK, std::string("overlap_decoder: ") + err.message);
        std::string letters, quality;
        std::vector<uint64_t> rec_end, id_end;
        uint64_t found = 0;
        for (size_t j = 0; j < reads.size() / 2; j++) {
            const std::string &r1 = reads[2 * j], &r2 = reads[2 * j + 1], &q1 = quals[2 * j], &q2 = quals[2 * j + 1];
            const nafgpu_pair_overlap p = rules(r1, r2, o);
            if (!p.found) continue;
            found++;
            const int64_t n1 = static_cast<int64_t>(r1.size()), n2 = static_cast<int64_t>(r2.size());
            for (int64_t pos = 0; pos < static_cast<int64_t>(p.insert); pos++) {
                const int64_t at = n2 - 1 - (pos - p.shift);
                if (pos < p.shift) {
                    letters += r1[pos];
                    quality += q1[pos];
                } else if (pos >= n1) {
                    letters += complement(r2[at]);
                    quality += q2[at];
                } else {
                    const char a = r1[pos], b = complement(r2[at]);
                    const int qa = static_cast<uint8_t>(q1[pos]), qb = static_cast<uint8_t>(q2[at]);
                    letters += qb > qa ? b : a;
                    quality += static_cast<char>(code(a) < 4 && code(a) == code(b) ? std::max(qa, qb) : std::min(255, static_cast<int>(base) + std::max(std::abs(qa - qb), 2)));
                }
            }
            rec_end.push_back(letters.size());
        }
        expect(res.n_found == found && found >= 58, "merge: the pairs found");
        nafgpu_selection *sel = nullptr;
        nafgpu_select_result sr;
        expect(nafgpu_merge_pairs(dec, h, &sel, &sr, &err) == NAFGPU_OK, std::string("merge_pairs: ") + err.message);
        expect(sr.src.n_records == found && sr.src.n_bases == letters.size() && sr.src.n_quality == letters.size() && letters.size() > 8192, "merge: sizes");
        std::string got(letters.size(), 0), got_q(letters.size(), 0);
        std::vector<uint64_t> got_end(found);
        expect(nafgpu_selection_copy_to_host(sel, sr.src.d_sequence, got.size(), &got[0]) == NAFGPU_OK &&
                   nafgpu_selection_copy_to_host(sel, sr.src.d_quality, got_q.size(), &got_q[0]) == NAFGPU_OK &&
                   nafgpu_selection_copy_to_host(sel, sr.src.d_record_end, 8 * found, got_end.data()) == NAFGPU_OK,
               "merge: copy to host");
        expect(got_end == rec_end, "merge: record ends");
        for (size_t i = 0; i < got.size(); i++)
            if (got[i] != letters[i] || got_q[i] != quality[i]) die("merge: position " + std::to_string(i) + " of the merged output differs (base " + std::to_string(base) + ")");
        std::string ids(sr.src.n_ids_bytes, 0);
        expect(nafgpu_selection_copy_to_host(sel, sr.src.d_ids, ids.size(), &ids[0]) == NAFGPU_OK && ids.compare(0, 3, std::string("r0\0", 3)) == 0, "merge: ids are R1's");
        // refusals of the merge
        nafgpu_selection *none = reinterpret_cast<nafgpu_selection *>(1);
        expect(nafgpu_merge_pairs(dec, nullptr, &none, &sr, &err) == NAFGPU_E_INVALID_ARG && none == nullptr, "merge: null overlaps");
        expect(nafgpu_merge_pairs(nullptr, h, &none, &sr, &err) == NAFGPU_E_INVALID_ARG, "merge: null decoder");
        expect(nafgpu_merge_pairs(dec, h, nullptr, &sr, &err) == NAFGPU_E_INVALID_ARG, "merge: null out");
        nafgpu_selection_free(sel);
        nafgpu_overlaps_free(h);
    }
    nafgpu_close(dec);
    nafgpu_encoder_free(enc);
}

}  // namespace

int main() {
    Rng rng{20250303};
    analysis(rng);
    refusals(rng);
    merge(rng);
    std::printf("OK\n");
    return 0;
}
