// tests/select_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_select and nafgpu_find_records through the C-ABI, against expectations computed here in plain C++: the edges of
// the gather (tests/select_checks.py: edge_regions) and the id lookup, also with every id in one of four probe chains.
// `make select-asan` (tests/test_select_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0,
// or says what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096, kLane = 16;     // select.h: kSelTile; select.hip: 16 output bytes per lane

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

struct Rec {
    std::string id, comment, seq;
};

std::string archive_of(const std::vector<Rec> &recs) {
    nafgpu_encoder_opts o;
    nafgpu_encoder_opts_default(0, &o);
    o.id = o.comment = o.sequence = o.mask = 1;
    o.compression_level = 1;
    nafgpu_encoder *enc = nullptr;
    nafgpu_error err;
    expect(nafgpu_encoder_new(&o, &enc, &err) == NAFGPU_OK, "encoder_new");
    for (const Rec &r : recs) {
        nafgpu_record rec;
        std::memset(&rec, 0, sizeof rec);
        rec.id = {reinterpret_cast<const uint8_t *>(r.id.data()), r.id.size(), 1, {}};
        rec.comment = {reinterpret_cast<const uint8_t *>(r.comment.data()), r.comment.size(), 1, {}};
        rec.sequence = {reinterpret_cast<const uint8_t *>(r.seq.data()), r.seq.size(), 1, {}};
        expect(nafgpu_encoder_push(enc, &rec, &err) == NAFGPU_OK, std::string("encoder_push: ") + err.message);
    }
    const uint8_t *bytes = nullptr;
    uint64_t n = 0;
    expect(nafgpu_encoder_finish(enc, &bytes, &n, &err) == NAFGPU_OK, "encoder_finish");
    std::string out(reinterpret_cast<const char *>(bytes), n);
    nafgpu_encoder_free(enc);
    return out;
}

nafgpu_decoder *open_archive(const std::string &blob) {
    nafgpu_opts o;
    nafgpu_opts_default(&o);
    o.spec_mask = 1;                             // every masked letter lower case: the letters that were pushed
    nafgpu_decoder *dec = nullptr;
    nafgpu_error err;
    expect(nafgpu_open_bytes(reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), &o, &dec, &err) == NAFGPU_OK, "open_bytes");
    return dec;
}

uint8_t complement(uint8_t c) {
    static const char *pairs = "ATCGRYKMBVDH";
    for (int i = 0; pairs[i]; i++) {
        if (c == static_cast<uint8_t>(pairs[i])) return static_cast<uint8_t>(pairs[i ^ 1]);
        if (c == static_cast<uint8_t>(pairs[i] | 0x20)) return static_cast<uint8_t>(pairs[i ^ 1] | 0x20);
    }
    return c;
}

std::string fetch(nafgpu_selection *sel, const void *d_ptr, uint64_t n) {
    std::string out(static_cast<size_t>(n), '\0');
    expect(nafgpu_selection_copy_to_host(sel, d_ptr, n, out.data()) == NAFGPU_OK, "selection_copy_to_host");
    return out;
}

std::string ends_of(const std::vector<uint64_t> &sizes) {
    std::string out;
    uint64_t at = 0;
    for (uint64_t v : sizes) {
        at += v;
        out.append(reinterpret_cast<const char *>(&at), 8);
    }
    return out;
}

void check_select(nafgpu_decoder *dec, const std::vector<Rec> &recs, const std::vector<nafgpu_region> &regions, bool named, const char *what) {
    std::string seq, ids, coms;
    std::vector<uint64_t> lens, id_sizes, com_sizes;
    for (const nafgpu_region &g : regions) {
        const Rec &r = recs[g.record];
        const uint64_t end = g.end == NAFGPU_REGION_END ? r.seq.size() : g.end;
        std::string s = r.seq.substr(g.start, end - g.start);
        if (g.reverse_complement) {
            std::reverse(s.begin(), s.end());
            for (char &c : s) c = static_cast<char>(complement(static_cast<uint8_t>(c)));
        }
        std::string id = r.id;
        if (named) id += ":" + std::to_string(g.start + 1) + "-" + std::to_string(end) + (g.reverse_complement ? "/rc" : "");
        seq += s;
        ids += id;
        ids.push_back('\0');
        coms += r.comment;
        coms.push_back('\0');
        lens.push_back(s.size());
        id_sizes.push_back(id.size() + 1);
        com_sizes.push_back(r.comment.size() + 1);
    }
    nafgpu_select_opts so;
    std::memset(&so, 0, sizeof so);
    so.name_regions = named ? 1 : 0;
    nafgpu_selection *sel = nullptr;
    nafgpu_select_result res;
    nafgpu_error err;
    const int rc = nafgpu_select(dec, regions.data(), regions.size(), &so, &sel, &res, &err);
    expect(rc == NAFGPU_OK, std::string(what) + ": nafgpu_select: " + err.message);
    const uint64_t n = regions.size();
    expect(res.n_regions == n && res.src.n_records == n && res.src.n_bases == seq.size() && res.src.n_ids_bytes == ids.size() &&
               res.src.n_comments_bytes == coms.size() && res.src.d_quality == nullptr && res.src.n_quality == 0,
           std::string(what) + ": counts");
    expect(fetch(sel, res.src.d_sequence, seq.size()) == seq, std::string(what) + ": letters");
    expect(fetch(sel, res.src.d_ids, ids.size()) == ids, std::string(what) + ": ids");
    expect(fetch(sel, res.src.d_comments, coms.size()) == coms, std::string(what) + ": comments");
    expect(fetch(sel, res.src.d_record_end, 8 * n) == ends_of(lens), std::string(what) + ": record ends");
    expect(fetch(sel, res.d_id_end, 8 * n) == ends_of(id_sizes), std::string(what) + ": id ends");
    expect(fetch(sel, res.d_comment_end, 8 * n) == ends_of(com_sizes), std::string(what) + ": comment ends");
    uint64_t h = 0;
    expect(nafgpu_selection_hash64(sel, res.src.d_sequence, seq.size(), 0, &h) == NAFGPU_OK &&
               h == nafgpu_hash64_host(reinterpret_cast<const uint8_t *>(seq.data()), seq.size()),
           std::string(what) + ": checksum");
    nafgpu_selection_free(sel);
}

void check_edges() {
    Rng rng{20241019};
    std::vector<uint64_t> lens = {0, 9000, 1, 15, 16, 17, kTile - 1, kTile, kTile + 1};
    while (lens.size() < 62) lens.push_back(rng.next() % 9001);
    lens.push_back(0);
    lens.push_back(33);
    static const char letters[] = "ACGTRYSWKMBDHVN-acgtryswkmbdhvn";
    std::vector<Rec> recs;
    for (size_t k = 0; k < lens.size(); k++) {
        Rec r;
        r.id = "e" + std::to_string(k);
        r.comment = k % 3 ? "edge " + std::to_string(k) : "";
        for (uint64_t i = 0; i < lens[k]; i++) r.seq.push_back(letters[rng.next() % (sizeof letters - 1)]);
        recs.push_back(r);
    }
    const std::string blob = archive_of(recs);
    nafgpu_decoder *dec = open_archive(blob);
    nafgpu_device_result all;
    expect(nafgpu_decode_all_device(dec, &all) == NAFGPU_OK, "decode_all_device");
    std::string joined, decoded(static_cast<size_t>(all.n_bases), '\0');
    for (const Rec &r : recs) joined += r.seq;
    expect(nafgpu_copy_to_host(dec, all.d_sequence, all.n_bases, decoded.data()) == NAFGPU_OK && decoded == joined, "the archive decodes to what was pushed");

    const uint64_t big = 1, first = 1, last = lens.size() - 1;
    std::vector<nafgpu_region> regions;
    uint64_t pos = 0;
    auto add = [&](uint64_t record, uint64_t start, uint64_t length, int strand) {
        expect(start + length <= lens[record], "a region of the test leaves its record");
        nafgpu_region g;
        std::memset(&g, 0, sizeof g);
        g.record = record;
        g.start = start;
        g.end = start + length == lens[record] && (regions.size() & 1) ? NAFGPU_REGION_END : start + length;
        g.reverse_complement = static_cast<uint8_t>(strand);
        regions.push_back(g);
        pos += length;
    };
    const uint64_t edge_lengths[] = {0, 1, 15, 16, 17, kTile - 1, kTile, kTile + 1};
    for (int strand = 0; strand < 2; strand++) {
        add(first, 0, 1, strand);                                     // the section's first letter
        add(last, lens[last] - 1, 1, strand);                         // ... and its last one
        for (uint64_t l : edge_lengths) add(big, 101, l, strand);
        for (uint64_t k = 2; k < 9; k++) add(k, 0, lens[k], strand);  // whole records of the edge lengths
        for (uint64_t r = 0; r < kLane; r++) add(big, 200 + r, 37, strand);
        add(big, 5, (kTile - pos % kTile) % kTile ? (kTile - pos % kTile) % kTile : kTile, strand);   // ends on an output tile edge
        expect(pos % kTile == 0, "tile edge");
        add(big, 3, 100, strand);                                     // starts on one
        for (uint64_t i = 0; i < 600; i++) {                          // more one-letter regions than a tile has lanes
            add(big, (i * 7) % 9000, 1, i % 3 == 0 ? static_cast<int>((i + strand) & 1) : strand);
            if (i % 50 == 7) {
                add(big, 10, 0, strand);
                add(0, 0, 0, 0);
            }
        }
        for (uint64_t i = 0; i < 300; i++) add((i * 5) % lens.size(), 0, 0, strand);   // a run of empty regions, then one letter
        add(big, 8999, 1, strand);
        add(first, 0, lens[first], strand);
        add(last, 0, lens[last], strand);
    }
    expect(pos > 4 * kTile, "several tiles");
    check_select(dec, recs, regions, false, "edges");
    std::reverse(regions.begin(), regions.end());
    check_select(dec, recs, regions, true, "edges, reversed list, named");
    std::vector<nafgpu_region> empty_ones;
    for (uint64_t k = 0; k < 700; k++) {
        nafgpu_region g;
        std::memset(&g, 0, sizeof g);
        g.record = k % 64;
        g.reverse_complement = k & 1;
        empty_ones.push_back(g);
    }
    check_select(dec, recs, empty_ones, false, "every region empty");
    check_select(dec, recs, {}, false, "no region");
    // a refusal produces nothing
    regions[40].start = 9001;
    regions[900].record = 64;
    nafgpu_selection *sel = nullptr;
    nafgpu_select_result res;
    nafgpu_error err;
    expect(nafgpu_select(dec, regions.data(), regions.size(), nullptr, &sel, &res, &err) == NAFGPU_E_INVALID_ARG && !sel && !res.src.d_sequence &&
               std::strncmp(err.message, "region 40:", 10) == 0,
           std::string("refusal: ") + err.message);
    nafgpu_close(dec);
}

void check_find(const char *what) {
    std::vector<Rec> recs;
    const char *head[] = {"dup", "x1", "dup", "", "x2", "", "dup", "x"};
    for (const char *h : head) recs.push_back({h, "", "A"});
    for (int k = 0; k < 1300; k++) recs.push_back({"n" + std::to_string(k % 500), "", "AC"});
    const std::string blob = archive_of(recs);
    nafgpu_decoder *dec = open_archive(blob);
    std::vector<std::string> probes = {"dup", "", "x1", "x2", "x", "n0", "n499", "n500", "du", "dupp", "n49", "N0", "x1 "};
    for (int k = 0; k < 500; k += 7) probes.push_back("n" + std::to_string(k));
    std::string names;
    for (const std::string &p : probes) names.append(p).push_back('\0');
    std::vector<uint64_t> got(probes.size(), 12345);
    nafgpu_error err;
    expect(nafgpu_find_records(dec, reinterpret_cast<const uint8_t *>(names.data()), names.size(), probes.size(), got.data(), &err) == NAFGPU_OK,
           std::string(what) + ": find_records: " + err.message);
    for (size_t j = 0; j < probes.size(); j++) {
        uint64_t want = UINT64_MAX;
        for (size_t k = 0; k < recs.size() && want == UINT64_MAX; k++)
            if (recs[k].id == probes[j]) want = k;
        expect(got[j] == want, std::string(what) + ": name '" + probes[j] + "' -> " + std::to_string(got[j]) + ", expected " + std::to_string(want));
    }
    // the blob's own rules: a missing NUL, a count that disagrees
    expect(nafgpu_find_records(dec, reinterpret_cast<const uint8_t *>("abc"), 3, 1, got.data(), &err) == NAFGPU_E_INVALID_ARG, "a missing NUL");
    expect(nafgpu_find_records(dec, reinterpret_cast<const uint8_t *>("abc\0de"), 7, 1, got.data(), &err) == NAFGPU_E_INVALID_ARG, "two names for one");
    expect(nafgpu_find_records(dec, nullptr, 0, 0, got.data(), &err) == NAFGPU_OK, "no names");
    nafgpu_close(dec);
}

}  // namespace

int main() {
    int units = 0;
    uint64_t memory = 0;
    char name[64];
    if (nafgpu_device_info(0, name, sizeof name, &memory, &units) != NAFGPU_OK) die("no device");
    check_edges();
    check_find("find");
    setenv("NAFGPU_SEL_HASH_BITS", "2", 1);      // every id in one of four probe chains
    nafgpu_test_hooks(1);
    check_find("find, colliding");
    std::printf("OK\n");
    return 0;
}
