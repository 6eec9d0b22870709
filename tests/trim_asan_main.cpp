// tests/trim_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_trim through the C-ABI, against expectations computed here in plain C++ (the four steps of include/nafgpu.h as loops
// over every record): window lengths 1 .. 64 with the failing window at the section's first and last start, around tile and
// lane edges and at record ends, records of 0, 1, W - 1, W and W + 1 letters and runs of empty ones, running sums that stop at
// once, never, and on either side of a chunk edge on both routes, three tiles of all-low qualities, N ends on chunk edges,
// min_length and mates, letters behind the last end, no record table; and the refusals, hand-made end tables among them.  On
// the CPU harness host memory is device memory, so the sections are allocations of exactly their size at four alignments and
// the end tables vectors of exactly theirs: a read outside them is a finding.
// `make trim-asan` (tests/test_trim_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0, or
// says what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096, kChunk = 256;   // trim.h: kTrimTile, 16 bytes of kTrimShortLanes lanes

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

struct Record {
    std::string letters, quality;
};

struct Want {
    std::vector<nafgpu_region> regions;
    std::vector<uint8_t> keep;
    uint64_t changed = 0, in_windows = 0, kept_letters = 0, n_kept = 0;
};

bool is_n(char c) { return c == 'N' || c == 'n'; }

// the rules, one record at a time
Want rules(const std::string &letters, const std::string &quality, const std::vector<uint64_t> &ends, const nafgpu_trim_opts &o) {
    Want w;
    uint64_t lo = 0;
    std::vector<bool> pass;
    for (size_t k = 0; k < ends.size(); lo = ends[k], k++) {
        const int64_t L = static_cast<int64_t>(ends[k] - lo);
        auto v = [&](int64_t i) { return static_cast<int64_t>(static_cast<uint8_t>(quality[lo + i])) - o.quality_base; };
        int64_t a = 0, b = L;
        if (o.cut_front) {
            int64_t sum = 0, best = 0;
            for (int64_t i = 0; i < L; i++) {
                sum += o.cut_front - v(i);
                if (sum < 0) break;
                if (sum > best) best = sum, a = i + 1;
            }
        }
        if (o.cut_tail) {
            int64_t sum = 0, best = 0;
            for (int64_t i = L - 1; i >= 0; i--) {
                sum += o.cut_tail - v(i);
                if (sum < 0) break;
                if (sum > best) best = sum, b = i;
            }
        }
        if (o.window) {
            const int64_t W = o.window;
            for (int64_t i = a; i + W <= b; i++) {
                int64_t sum = 0;
                for (int64_t j = 0; j < W; j++) sum += v(i + j);
                if (sum < W * o.window_quality) {
                    b = i;
                    break;
                }
            }
        }
        if (o.trim_n) {
            while (a < b && is_n(letters[lo + a])) a++;
            while (a < b && is_n(letters[lo + b - 1])) b--;
        }
        if (a >= b) a = b = 0;
        nafgpu_region r;
        std::memset(&r, 0, sizeof r);
        r.record = k;
        r.start = static_cast<uint64_t>(a);
        r.end = static_cast<uint64_t>(b);
        w.regions.push_back(r);
        pass.push_back(static_cast<uint64_t>(b - a) >= o.min_length);
        w.changed += a != 0 || b != L;
        w.in_windows += static_cast<uint64_t>(b - a);
    }
    for (size_t k = 0; k < pass.size(); k++) {
        const bool keep = pass[k] && (!o.interleaved || pass[k ^ 1]);
        w.keep.push_back(keep);
        if (keep) w.n_kept++, w.kept_letters += w.regions[k].end - w.regions[k].start;
    }
    return w;
}

nafgpu_trim_opts options(unsigned front, unsigned tail, unsigned W, unsigned Q, bool n, uint64_t min_length = 0, bool mates = false, unsigned base = 33) {
    nafgpu_trim_opts o;
    std::memset(&o, 0, sizeof o);
    o.quality_base = static_cast<uint8_t>(base);
    o.cut_front = static_cast<uint8_t>(front);
    o.cut_tail = static_cast<uint8_t>(tail);
    o.window = static_cast<uint8_t>(W);
    o.window_quality = static_cast<uint8_t>(Q);
    o.trim_n = n;
    o.interleaved = mates;
    o.min_length = min_length;
    return o;
}

// the records in sections of exactly their size, the pointers at residue `pad` of 16; n_records < 0: every record
void run(const std::string &what, const std::vector<Record> &records, const nafgpu_trim_opts &o, unsigned pad = 0, long n_records = -1,
         const std::string &behind = "", bool with_letters = true, bool with_quality = true) {
    std::string letters, quality;
    std::vector<uint64_t> ends;
    for (const Record &r : records) {
        expect(r.letters.size() == r.quality.size(), what + ": a record's letters and qualities differ in length");
        letters += r.letters;
        quality += r.quality;
        ends.push_back(letters.size());
    }
    letters += behind;
    quality += behind;
    if (n_records >= 0) ends.resize(static_cast<size_t>(n_records));
    const size_t n = letters.size();
    // (malloc's blocks are 16-byte aligned: the section begins at residue `pad` and ends where its block ends)
    uint8_t *s_block = static_cast<uint8_t *>(std::malloc(pad + n ? pad + n : 1)), *q_block = static_cast<uint8_t *>(std::malloc(pad + n ? pad + n : 1));
    expect(s_block && q_block, "out of memory");
    std::memcpy(s_block + pad, letters.data(), n);
    std::memcpy(q_block + pad, quality.data(), n);
    std::vector<uint64_t> table(ends);                       // exactly its size
    nafgpu_encode_source src;
    std::memset(&src, 0, sizeof src);
    src.d_sequence = with_letters ? s_block + pad : nullptr;
    src.n_bases = n;
    src.d_quality = with_quality ? q_block + pad : nullptr;
    src.n_quality = n;
    src.d_record_end = table.empty() ? nullptr : table.data();
    src.n_records = table.size();
    const Want want = rules(letters, quality, ends.empty() ? std::vector<uint64_t>{n} : ends, o);
    nafgpu_trims *t = nullptr;
    nafgpu_trim_result res;
    nafgpu_error err;
    const int rc = nafgpu_trim(&src, &o, 0, &t, &res, &err);
    expect(rc == NAFGPU_OK, what + ": status " + std::to_string(rc) + " " + err.message);
    expect(res.n_records == want.regions.size() && res.n_bases == n, what + ": n_records / n_bases");
    expect(res.n_kept == want.n_kept && res.n_changed == want.changed && res.bases_in_windows == want.in_windows && res.bases_kept == want.kept_letters,
           what + ": totals " + std::to_string(res.n_kept) + "/" + std::to_string(want.n_kept) + " " + std::to_string(res.n_changed) + "/" +
               std::to_string(want.changed) + " " + std::to_string(res.bases_in_windows) + "/" + std::to_string(want.in_windows));
    std::vector<nafgpu_region> regions(res.n_records), kept(res.n_kept);
    std::vector<uint8_t> keep(res.n_records);
    expect(nafgpu_trims_copy_to_host(t, res.d_regions, regions.size() * sizeof(nafgpu_region), regions.data()) == NAFGPU_OK &&
               nafgpu_trims_copy_to_host(t, res.d_keep, keep.size(), keep.data()) == NAFGPU_OK &&
               nafgpu_trims_copy_to_host(t, res.d_kept_regions, kept.size() * sizeof(nafgpu_region), kept.data()) == NAFGPU_OK,
           what + ": copy to host");
    size_t at = 0;
    for (size_t k = 0; k < regions.size(); k++) {
        if (std::memcmp(&regions[k], &want.regions[k], sizeof(nafgpu_region)) || keep[k] != want.keep[k])
            die(what + ": record " + std::to_string(k) + " is [" + std::to_string(regions[k].start) + ", " + std::to_string(regions[k].end) + ") keep " +
                std::to_string(keep[k]) + ", expected [" + std::to_string(want.regions[k].start) + ", " + std::to_string(want.regions[k].end) + ") keep " +
                std::to_string(want.keep[k]));
        if (keep[k]) expect(at < kept.size() && !std::memcmp(&kept[at++], &regions[k], sizeof(nafgpu_region)), what + ": kept regions");
    }
    expect(at == kept.size(), what + ": the number of kept regions");
    nafgpu_trims_free(t);
    std::free(s_block);
    std::free(q_block);
}

std::string random_letters(Rng &rng, size_t n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGT"[rng.next() & 3];
    return s;
}

void windows(Rng &rng) {
    // base 34, Q 0, low '!' (v = -1), high '~' (v = 92): a window fails when and only when all of it is low
    for (unsigned W : {1u, 2u, 15u, 16u, 17u, 63u, 64u}) {
        const nafgpu_trim_opts o = options(0, 0, W, 0, false, 0, false, 34);
        const size_t n = kTile * (W + 1) + 200;
        std::vector<size_t> starts = {0, n - W};
        for (size_t j = 1; j <= W + 1; j++) starts.push_back(kTile * j - W + (j - 1));
        for (size_t i = 0; i <= 16; i++) starts.push_back(112 + 81 * i);
        std::sort(starts.begin(), starts.end());
        std::string quality(n, '~');
        for (size_t s : starts) quality.replace(s, W, std::string(W, '!'));
        std::vector<Record> records;                         // every planted window in a record of its own
        size_t lo = 0;
        for (size_t i = 0; i < starts.size(); i++) {
            const size_t hi = i + 1 < starts.size() ? starts[i] + W + rng.next() % (starts[i + 1] - starts[i] - W + 1) : n;
            records.push_back({random_letters(rng, hi - lo), quality.substr(lo, hi - lo)});
            lo = hi;
        }
        for (unsigned pad : {0u, 1u, 7u, 15u}) run("planted windows, W = " + std::to_string(W), records, o, pad);
        run("one record, W = " + std::to_string(W), {{random_letters(rng, n), quality}}, o, W % 16);
        std::vector<Record> lengths;
        for (size_t l : {size_t(0), size_t(1), size_t(W - 1), size_t(W), size_t(W + 1), size_t(0), size_t(0), size_t(W), size_t(0)})
            lengths.push_back({random_letters(rng, l), std::string(l, '!')});
        for (int i = 0; i < 70; i++) lengths.push_back({"", ""});
        lengths.push_back({random_letters(rng, 2 * W), std::string(2 * W, '!')});
        run("record lengths, W = " + std::to_string(W), lengths, o, 3);
        run("a low run split by a record end, W = " + std::to_string(W),
            {{random_letters(rng, 64), std::string(65 - W, '~') + std::string(W - 1, '!')}, {random_letters(rng, 20), "!" + std::string(19, '~')},
             {random_letters(rng, W + 5), std::string(5, '~') + std::string(W, '!')}},
            o, 9);
    }
}

std::string q(const std::vector<int> &values) {
    std::string s;
    for (int v : values) s.push_back(static_cast<char>(33 + v));
    return s;
}

void sums(Rng &rng) {
    const nafgpu_trim_opts both = options(10, 10, 0, 0, false);
    for (const std::vector<int> &values : std::vector<std::vector<int>>{std::vector<int>(12, 30), std::vector<int>(12, 5), {5, 15, 5, 15, 30, 30, 30, 15, 5, 15, 5},
                                                                        {5, 5, 0, 40, 40, 0, 5, 5}, {9, 9, 9, 11, 9, 9, 9}, {3}, {30}})
        run("a running sum of " + std::to_string(values.size()), {{random_letters(rng, values.size()), q(values)}}, both, 5);
    run("values below the base", {{random_letters(rng, 6), std::string("\x3c\x3c\x7e\x7e\x3c\x32")}}, options(1, 1, 0, 0, false, 0, false, 64));
    for (size_t chunk : {kChunk, kTile}) {
        const size_t length = 3 * chunk + 77;
        std::vector<Record> records;
        for (int d = -2; d <= 2; d++)
            for (size_t stop : {size_t(1), size_t(2), size_t(17)}) {
                std::vector<int> values(length, 40);
                for (size_t i = 0; i < chunk + d; i++) values[i] = 5;
                for (size_t i = chunk + d; i + 1 < chunk + d + stop; i++) values[i] = 12;
                records.push_back({random_letters(rng, length), q(values)});
                std::reverse(values.begin(), values.end());
                records.push_back({random_letters(rng, length), q(values)});
            }
        for (unsigned pad : {0u, 1u, 7u, 15u}) run("chunk edges of " + std::to_string(chunk), records, both, pad);
    }
    std::string low(3 * kTile, static_cast<char>(35));
    run("three tiles, all low", {{random_letters(rng, low.size()), low}}, both, 7);
    low[kTile + 7] = static_cast<char>(120);
    run("three tiles, low but for one letter", {{random_letters(rng, low.size()), low}, {"ACG", q({1, 2, 3})}}, both, 15);
}

void everything(Rng &rng) {
    for (unsigned pad = 0; pad < 16; pad += 5) {
        std::vector<Record> records;
        for (int k = 0; k < 60; k++) {
            const size_t l = std::vector<size_t>{0, 1, 40, 300, 2000, 5000}[rng.next() % 6] + rng.next() % 9;
            Record r{random_letters(rng, l), std::string(l, ' ')};
            for (char &c : r.quality) c = static_cast<char>(rng.next() & 255);
            for (size_t i = 0; i < l && i < rng.next() % 5; i++) r.letters[i] = 'N';
            for (size_t i = 0; i < l && i < rng.next() % 5; i++) r.letters[l - 1 - i] = 'n';
            records.push_back(r);
        }
        run("all byte values", records, options(100, 140, 1 + 4 * pad, 120, true, pad, true, 33 + pad), pad, -1, std::string(pad % 3, '\1'));
    }
    std::vector<Record> ns = {{"NNNNNNNN", std::string(8, '~')}, {"nNnACGTNACGnn", std::string(13, '~')}, {"ACNNNGT", std::string(7, '~')}, {"N", "~"}, {"", ""},
                              {std::string(kChunk, 'N') + "A" + std::string(kChunk, 'N'), std::string(2 * kChunk + 1, '~')},
                              {std::string(kTile, 'N') + "ACG" + std::string(2 * kTile, 'N'), std::string(3 * kTile + 3, '~')},
                              {std::string(2 * kTile + 9, 'N'), std::string(2 * kTile + 9, '~')}};
    for (unsigned pad : {0u, 1u, 7u, 15u}) run("N ends", ns, options(0, 0, 0, 0, true, 2), pad);
    run("N ends without qualities", ns, options(0, 0, 0, 0, true), 3, -1, "", true, false);
    std::vector<Record> reads;
    for (int tail : {8, 0, 0, 8, 8, 9, 0, 0}) reads.push_back({random_letters(rng, 20), q(std::vector<int>(20 - tail, 30)) + q(std::vector<int>(tail, 2))});
    for (uint64_t min_length : {0, 11, 12, 13, 21})
        for (bool mates : {false, true}) run("min_length " + std::to_string(min_length), reads, options(0, 10, 0, 0, false, min_length, mates), 1);
    run("letters behind the last end", reads, options(10, 10, 4, 20, true), 7, 5, std::string(70, '!'));
    run("no records", reads, options(0, 10, 4, 20, true), 7, 0);
    run("qualities only", reads, options(10, 10, 4, 20, false, 3), 2, -1, "", false, true);
    run("all options off", reads, options(0, 0, 0, 0, false));
}

int refused(const nafgpu_encode_source &src, const nafgpu_trim_opts *o, std::string *message = nullptr) {
    nafgpu_trims *t = reinterpret_cast<nafgpu_trims *>(1);
    nafgpu_trim_result res;
    nafgpu_error err;
    std::memset(&err, 0, sizeof err);
    const int rc = nafgpu_trim(&src, o, 0, &t, &res, &err);
    if (rc == NAFGPU_OK) {
        nafgpu_trims_free(t);
    } else {
        expect(t == nullptr && res.n_records == 0 && res.d_regions == nullptr, "a refusal produced something");
    }
    if (message) *message = err.message;
    return rc;
}

void refusals() {
    std::string letters(2000, 'A'), quality(2000, 'I');
    std::vector<uint64_t> ends;
    for (uint64_t k = 1; k <= 200; k++) ends.push_back(10 * k);
    nafgpu_encode_source good;
    std::memset(&good, 0, sizeof good);
    good.d_sequence = reinterpret_cast<const uint8_t *>(letters.data());
    good.n_bases = letters.size();
    good.d_quality = reinterpret_cast<const uint8_t *>(quality.data());
    good.n_quality = quality.size();
    good.d_record_end = ends.data();
    good.n_records = ends.size();
    const nafgpu_trim_opts all = options(20, 20, 4, 20, true, 3);
    expect(refused(good, &all) == NAFGPU_OK, "a good source");
    expect(refused(good, nullptr) == NAFGPU_E_INVALID_ARG, "opts NULL");
    nafgpu_encode_source src = good;
    src.d_sequence = src.d_quality = nullptr;
    expect(refused(src, &all) == NAFGPU_E_INVALID_ARG, "both sections NULL");
    src = good;
    src.d_quality = nullptr;
    for (const nafgpu_trim_opts &o : {options(1, 0, 0, 0, false), options(0, 1, 0, 0, false), options(0, 0, 4, 0, false)})
        expect(refused(src, &o) == NAFGPU_E_INVALID_ARG, "a quality step without d_quality");
    src = good;
    src.d_sequence = nullptr;
    const nafgpu_trim_opts n_only = options(0, 0, 0, 0, true);
    expect(refused(src, &n_only) == NAFGPU_E_INVALID_ARG, "trim_n without d_sequence");
    const nafgpu_trim_opts wide = options(0, 0, 65, 0, false);
    expect(refused(good, &wide) == NAFGPU_E_INVALID_ARG, "window 65");
    src = good;
    src.n_records = 199;
    const nafgpu_trim_opts mates = options(0, 0, 0, 0, false, 0, true);
    expect(refused(src, &mates) == NAFGPU_E_INVALID_ARG && refused(good, &mates) == NAFGPU_OK, "interleaved with an odd number of records");
    src = good;
    src.n_quality--;
    expect(refused(src, &all) == NAFGPU_E_INVALID_LENGTH, "n_quality != n_bases");
    // hand-made end tables: the lowest offender is named
    struct Bad {
        std::vector<std::pair<size_t, uint64_t>> change;
        const char *needle;
    };
    for (const Bad &bad : {Bad{{{100, 500}}, "record 100 "}, Bad{{{100, 500}, {60, 300}, {199, 1}}, "record 60 "}, Bad{{{199, 2001}}, "record 199 "},
                           Bad{{{199, UINT64_MAX}}, "record 199 "}, Bad{{{0, 1ull << 40}}, "record 0 "}, Bad{{{199, 1989}}, "record 199 "}}) {
        std::vector<uint64_t> table(ends);
        for (const auto &c : bad.change) table[c.first] = c.second;
        src = good;
        src.d_record_end = table.data();
        std::string message;
        expect(refused(src, &all, &message) == NAFGPU_E_INVALID_LENGTH && message.find(bad.needle) != std::string::npos, std::string("an end table: ") + message);
    }
    expect(nafgpu_trims_copy_to_host(nullptr, nullptr, 1, nullptr) == NAFGPU_E_INVALID_ARG, "copy_to_host(NULL)");
    nafgpu_trims_free(nullptr);
}

}  // namespace

int main() {
    Rng rng{20250101};
    windows(rng);
    sums(rng);
    everything(rng);
    refusals();
    std::printf("OK\n");
    return 0;
}
