// tests/screen_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// nafgpu_kmers_build and nafgpu_screen through the C-ABI, against expectations computed here in plain C++ (the rules of
// include/nafgpu.h as loops over every window of every record, the keys in a std::set): every k of 1, 2, 15, 16, 17, 30, 31 on
// both kinds of key with a planted window at the section's first and last start, around tile and lane edges and at record
// ends, records of 0, 1, k - 1, k and k + 1 letters and runs of empty ones, an N at every position, all byte values, letters
// behind the last end, no record table, an empty set, thresholds and mates, tables that the hooks make nearly full with the
// hash cut to 0, 3 and 8 bits; and the refusals, hand-made end tables among them.  On the CPU harness host memory is device
// memory, so the sections are allocations of exactly their size at four alignments and the end tables vectors of exactly
// theirs: a read outside them is a finding.
// `make screen-asan` (tests/test_screen_emu.py) compiles it and the CPU harness into one program with
// -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and returns 0, or
// says what differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "nafgpu.h"

namespace {

constexpr uint64_t kTile = 4096;                 // screen.h: kScreenTile

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

std::string random_letters(Rng &rng, size_t n) {
    std::string out(n, 'A');
    for (char &c : out) c = "ACGT"[rng.next() & 3];
    return out;
}

int code_of(unsigned char b) {
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}

std::string revcomp(const std::string &s) {
    std::string out(s.rbegin(), s.rend());
    for (char &c : out) c = "TGCA"[code_of(static_cast<unsigned char>(c))];
    return out;
}

// the key of the window at s[at .. at + k), or false: it holds a non-letter
bool key_at(const std::string &s, size_t at, unsigned k, bool canonical, uint64_t *key) {
    uint64_t f = 0, r = 0;
    for (unsigned j = 0; j < k; j++) {
        const int c = code_of(static_cast<unsigned char>(s[at + j]));
        if (c > 3) return false;
        f = f * 4 + static_cast<uint64_t>(c);
        r |= static_cast<uint64_t>(3 - c) << (2 * j);
    }
    *key = canonical && r < f ? r : f;
    return true;
}

struct Section {
    std::string letters;
    std::vector<uint64_t> ends;          // empty: no table, the section is record 0
};

Section section_of(const std::vector<std::string> &records, const std::string &behind = "", long n_records = -1) {
    Section s;
    for (const std::string &r : records) {
        s.letters += r;
        s.ends.push_back(s.letters.size());
    }
    s.letters += behind;
    if (n_records >= 0) s.ends.resize(static_cast<size_t>(n_records));
    return s;
}

// calls visit(record, start relative to the record, key) for every window, ascending
template <class F>
void windows_of(const Section &s, unsigned k, bool canonical, F visit) {
    std::vector<uint64_t> ends = s.ends;
    if (ends.empty()) ends.push_back(s.letters.size());
    uint64_t lo = 0;
    for (size_t rec = 0; rec < ends.size(); lo = ends[rec], rec++)
        for (uint64_t at = lo; at + k <= ends[rec]; at++) {
            uint64_t key;
            if (key_at(s.letters, at, k, canonical, &key)) visit(rec, at - lo, key);
        }
}

// a section in an allocation of exactly its size, the pointer at residue `pad` of 16 (malloc's blocks are 16-byte aligned: the
// section begins at residue `pad` and ends where its block ends), and a table of exactly its size
struct OnDevice {
    uint8_t *block;
    std::vector<uint64_t> table;
    nafgpu_encode_source src;
    OnDevice(const Section &s, unsigned pad) : block(static_cast<uint8_t *>(std::malloc(pad + s.letters.size() ? pad + s.letters.size() : 1))), table(s.ends) {
        expect(block != nullptr, "out of memory");
        std::memcpy(block + pad, s.letters.data(), s.letters.size());
        std::memset(&src, 0, sizeof src);
        src.d_sequence = block + pad;
        src.n_bases = s.letters.size();
        src.d_record_end = table.empty() ? nullptr : table.data();
        src.n_records = table.size();
    }
    ~OnDevice() { std::free(block); }
};

nafgpu_screen_opts options(uint64_t min_hits = 1, unsigned min_percent = 0, bool mates = false, bool keep_matched = false) {
    nafgpu_screen_opts o;
    std::memset(&o, 0, sizeof o);
    o.min_hits = min_hits;
    o.min_percent = static_cast<uint8_t>(min_percent);
    o.interleaved = mates;
    o.keep_matched = keep_matched;
    return o;
}

template <class T>
std::vector<T> fetch(nafgpu_screens *s, const T *d_ptr, uint64_t n) {
    std::vector<T> out(static_cast<size_t>(n));
    expect(nafgpu_screens_copy_to_host(s, d_ptr, n * sizeof(T), out.data()) == NAFGPU_OK, "copy_to_host failed");
    return out;
}

// -> the hits of every record
std::vector<uint64_t> run(const std::string &what, const Section &ref, const Section &query, unsigned k, bool canonical, const nafgpu_screen_opts &o = options(),
                          unsigned pad = 0) {
    std::set<uint64_t> keys;
    uint64_t ref_windows = 0;
    windows_of(ref, k, canonical, [&](size_t, uint64_t, uint64_t key) {
        ref_windows++;
        keys.insert(key);
    });
    const size_t n = query.ends.empty() ? 1 : query.ends.size();
    std::vector<uint64_t> windows(n, 0), hits(n, 0), first(n, 0), last(n, 0);
    windows_of(query, k, canonical, [&](size_t rec, uint64_t at, uint64_t key) {
        windows[rec]++;
        if (!keys.count(key)) return;
        if (!hits[rec]) first[rec] = at;
        hits[rec]++;
        last[rec] = at + k;
    });

    OnDevice d_ref(ref, pad), d_query(query, (pad * 5 + 3) % 16);
    nafgpu_kmer_opts ko;
    std::memset(&ko, 0, sizeof ko);
    ko.k = static_cast<uint8_t>(k);
    ko.canonical = canonical;
    nafgpu_kmers *set = nullptr;
    nafgpu_kmers_result kr;
    nafgpu_error err;
    int rc = nafgpu_kmers_build(&d_ref.src, &ko, 0, &set, &kr, &err);
    expect(rc == NAFGPU_OK && set, what + ": nafgpu_kmers_build failed: " + err.message);
    expect(kr.n_windows == ref_windows && kr.n_kmers == keys.size() && kr.k == k && (kr.canonical != 0) == canonical && kr.n_bases == ref.letters.size() &&
               kr.n_records == (ref.ends.empty() ? 1 : ref.ends.size()) && !(kr.slots & (kr.slots - 1)),
           what + ": the set's figures differ: " + std::to_string(kr.n_windows) + " windows, " + std::to_string(kr.n_kmers) + " keys for " +
               std::to_string(ref_windows) + ", " + std::to_string(keys.size()));
    nafgpu_screens *s = nullptr;
    nafgpu_screen_result r;
    rc = nafgpu_screen(&d_query.src, set, &o, 0, &s, &r, &err);
    expect(rc == NAFGPU_OK && s, what + ": nafgpu_screen failed: " + err.message);
    expect(r.n_records == n && r.n_bases == query.letters.size(), what + ": the screen's sizes differ");
    const std::vector<uint64_t> got_windows = fetch(s, r.d_windows, n), got_hits = fetch(s, r.d_hits, n);
    const std::vector<nafgpu_region> regions = fetch(s, r.d_regions, n), kept = fetch(s, r.d_kept_regions, r.n_kept);
    const std::vector<uint8_t> match = fetch(s, r.d_match, n), keep = fetch(s, r.d_keep, n);
    uint64_t n_matched = 0, n_kept = 0, n_windows = 0, n_hits = 0, bases_kept = 0, lo = 0;
    for (size_t rec = 0; rec < n; rec++) {
        const std::string at = what + ": record " + std::to_string(rec);
        auto matches = [&](size_t i) { return hits[i] >= std::max<uint64_t>(o.min_hits, 1) && hits[i] * 100 >= static_cast<uint64_t>(o.min_percent) * windows[i]; };
        const bool m = matches(rec) || (o.interleaved && matches(rec ^ 1)), kp = m == (o.keep_matched != 0);
        const uint64_t hi = query.ends.empty() ? query.letters.size() : query.ends[rec];
        expect(got_windows[rec] == windows[rec] && got_hits[rec] == hits[rec],
               at + ": " + std::to_string(got_hits[rec]) + " of " + std::to_string(got_windows[rec]) + " for " + std::to_string(hits[rec]) + " of " + std::to_string(windows[rec]));
        nafgpu_region want;
        std::memset(&want, 0, sizeof want);
        want.record = rec;
        want.start = hits[rec] ? first[rec] : 0;
        want.end = hits[rec] ? last[rec] : 0;
        expect(!std::memcmp(&regions[rec], &want, sizeof want), at + ": the region differs");
        expect(match[rec] == (m ? 1 : 0) && keep[rec] == (kp ? 1 : 0), at + ": the flags differ");
        if (kp) {
            want.start = 0;
            want.end = hi - lo;
            expect(n_kept < kept.size() && !std::memcmp(&kept[n_kept], &want, sizeof want), at + ": the kept region differs");
            n_kept++;
            bases_kept += hi - lo;
        }
        n_matched += m;
        n_windows += windows[rec];
        n_hits += hits[rec];
        lo = hi;
    }
    expect(r.n_matched == n_matched && r.n_kept == n_kept && r.n_windows == n_windows && r.n_hits == n_hits && r.bases_kept == bases_kept, what + ": the totals differ");
    nafgpu_screens_free(s);
    nafgpu_kmers_free(set);
    return hits;
}

void refusals() {
    Rng rng{11};
    const Section good = section_of({random_letters(rng, 40), random_letters(rng, 60)});
    OnDevice d(good, 0);
    nafgpu_kmer_opts ko;
    std::memset(&ko, 0, sizeof ko);
    ko.k = 9;
    ko.canonical = 1;
    nafgpu_kmers *set = nullptr, *none = nullptr;
    nafgpu_kmers_result kr;
    nafgpu_screens *s = nullptr;
    nafgpu_screen_result r;
    nafgpu_error err;
    expect(nafgpu_kmers_build(&d.src, &ko, 0, &set, &kr, &err) == NAFGPU_OK, "the good set");
    for (unsigned k : {0u, 32u, 255u}) {
        nafgpu_kmer_opts bad = ko;
        bad.k = static_cast<uint8_t>(k);
        expect(nafgpu_kmers_build(&d.src, &bad, 0, &none, &kr, &err) == NAFGPU_E_INVALID_ARG && !none, "k " + std::to_string(k) + " was taken");
    }
    nafgpu_encode_source src = d.src;
    src.d_sequence = nullptr;
    nafgpu_screen_opts o = options();
    expect(nafgpu_kmers_build(&src, &ko, 0, &none, &kr, &err) == NAFGPU_E_INVALID_ARG, "a set without letters");
    expect(nafgpu_kmers_build(nullptr, &ko, 0, &none, &kr, &err) == NAFGPU_E_INVALID_ARG && nafgpu_kmers_build(&d.src, nullptr, 0, &none, &kr, &err) == NAFGPU_E_INVALID_ARG &&
               nafgpu_kmers_build(&d.src, &ko, 0, nullptr, &kr, &err) == NAFGPU_E_INVALID_ARG && nafgpu_kmers_build(&d.src, &ko, 0, &none, nullptr, &err) == NAFGPU_E_INVALID_ARG,
           "null arguments of the build");
    expect(nafgpu_screen(&src, set, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG && nafgpu_screen(&d.src, nullptr, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG &&
               nafgpu_screen(&d.src, set, nullptr, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG && nafgpu_screen(nullptr, set, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG &&
               nafgpu_screen(&d.src, set, &o, 0, nullptr, &r, &err) == NAFGPU_E_INVALID_ARG && nafgpu_screen(&d.src, set, &o, 0, &s, nullptr, &err) == NAFGPU_E_INVALID_ARG,
           "null arguments of the screen");
    o.min_percent = 101;
    expect(nafgpu_screen(&d.src, set, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG && std::strstr(err.message, "min_percent"), "min_percent 101");
    o = options(1, 0, true);
    src = d.src;
    src.n_records = 1;
    expect(nafgpu_screen(&src, set, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_ARG && std::strstr(err.message, "odd"), "mates of one record");
    expect(nafgpu_screens_copy_to_host(nullptr, nullptr, 1, nullptr) == NAFGPU_E_INVALID_ARG, "copy_to_host of nothing");
    nafgpu_screens_free(nullptr);
    nafgpu_kmers_free(nullptr);
    // hand-made end tables: the lowest offender is named, and nothing is read outside the section or the table
    o = options();
    struct Bad {
        std::vector<uint64_t> ends;
        const char *needle;
    };
    for (const Bad &bad : {Bad{{40, 30, 100}, "record 1 "}, Bad{{40, 101}, "record 1 "}, Bad{{1ull << 40, 100}, "record 0 "}, Bad{{40, 30, 20, ~0ull}, "record 1 "},
                           Bad{{10, 20, 30, 29, 100, 99}, "record 3 "}}) {
        Section sec = good;
        sec.ends = bad.ends;
        OnDevice b(sec, 3);
        expect(nafgpu_kmers_build(&b.src, &ko, 0, &none, &kr, &err) == NAFGPU_E_INVALID_LENGTH && std::strstr(err.message, bad.needle), std::string("a bad table, build: ") + err.message);
        expect(nafgpu_screen(&b.src, set, &o, 0, &s, &r, &err) == NAFGPU_E_INVALID_LENGTH && std::strstr(err.message, bad.needle) && !s, std::string("a bad table, screen: ") + err.message);
    }
    nafgpu_kmers_free(set);
}

}  // namespace

int main() {
    Rng rng{20250303};
    const std::string R = random_letters(rng, 600);
    for (unsigned k : {1u, 2u, 15u, 16u, 17u, 30u, 31u}) {
        const std::string tag = ", k = " + std::to_string(k);
        const std::string P = random_letters(rng, k);
        // a planted window (its reverse complement at every other place) at the section's first and last start, around two tile
        // edges at every offset, at every residue of a lane
        const size_t n = 2 * kTile + 300;
        std::vector<size_t> starts = {0, n - k};
        for (size_t i = 0; i <= 16; i++) starts.push_back(112 + 81 * i);
        starts.push_back(kTile - k + (k & 3));
        starts.push_back(2 * kTile - (k >> 1));
        std::sort(starts.begin(), starts.end());
        std::string section = random_letters(rng, n);
        for (size_t i = 0; i < starts.size(); i++) section.replace(starts[i], k, i & 1 ? revcomp(P) : P);
        for (unsigned pad : {0u, 1u, 7u, 15u}) {
            const std::vector<uint64_t> hits = run("one record" + tag, section_of({P}), section_of({section}), k, true, options(), pad);
            expect(k < 15 || hits[0] == starts.size(), "one record" + tag + ": a planted window was missed");
        }
        for (size_t at = kTile - k; at <= kTile; at++) {     // every offset around a tile edge, the window in a record of its own
            std::string edge = random_letters(rng, kTile + 64);
            edge.replace(at, k, P);
            const std::vector<uint64_t> hits = run("a tile edge" + tag, section_of({P}), section_of({edge.substr(0, at), edge.substr(at, k), edge.substr(at + k)}), k, false);
            expect(hits[1] == 1, "a tile edge" + tag + ": the window at " + std::to_string(at) + " was missed");
        }
        // the same letters cut into random records, forward keys, letters behind the last end, and without a table
        std::vector<std::string> pieces;
        for (size_t at = 0; at < n;) {
            const size_t l = std::min<size_t>(rng.next() % (3 * k + 40), n - at);
            pieces.push_back(section.substr(at, l));
            at += l;
        }
        run("random records" + tag, section_of({P, revcomp(P)}, R.substr(0, 40)), section_of(pieces, R.substr(100, 77)), k, false, options(2, 10, !(pieces.size() & 1)), 5);
        run("fewer records announced" + tag, section_of({R.substr(0, 100), R.substr(100, 100)}, "", 1), section_of(pieces, "", static_cast<long>(pieces.size() / 2)), k, true);
        run("no tables" + tag, section_of({R}, "", 0), section_of({R.substr(50, 300) + "N" + revcomp(R.substr(10, 200))}, "", 0), k, true, options(), 9);
        // records of 0, 1, k - 1, k, k + 1 letters and runs of empty ones; a window across a record end on either side
        std::vector<std::string> shapes;
        const size_t lengths[] = {0, 1, k - 1, k, k + 1, 0, 0, 0, k, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, k, k - 1, 2 * k, 1};
        for (size_t i = 0; i < sizeof lengths / sizeof *lengths; i++) shapes.push_back(R.substr(3 * i, lengths[i]));
        run("record shapes" + tag, section_of({R}), section_of(shapes), k, true, options(1, 0, false, true));
        run("split windows" + tag, section_of({P.substr(0, k / 2), P.substr(k / 2)}), section_of({P, P.substr(0, k / 2), P.substr(k / 2), P + P}), k, true);
        // an N at every position of a record of 2 k letters
        std::vector<std::string> with_n;
        for (size_t p = 0; p < 2 * k; p++) {
            std::string rec = R.substr(100, 2 * k);
            rec[p] = "NnRY-\x80"[p % 6];
            with_n.push_back(rec);
        }
        run("an N at every position" + tag, section_of({R.substr(100, 2 * k)}), section_of(with_n), k, true, options(1, 100));
    }
    // all byte values; lower case and U
    std::string everything(256 * 24, 0);
    for (size_t i = 0; i < everything.size(); i++) everything[i] = static_cast<char>((i * 167 + (i >> 8)) & 0xFF);
    run("all byte values", section_of({everything.substr(0, 2000)}), section_of({everything.substr(0, 3000), "", everything.substr(3000)}), 2, false);
    std::string lower = R.substr(0, 200), rna = lower;
    for (char &c : lower) c = static_cast<char>(c | 0x20);
    for (char &c : rna) c = c == 'T' ? 'U' : c;
    expect(run("lower case and U", section_of({R.substr(0, 200)}), section_of({lower, rna}), 21, true) == std::vector<uint64_t>({180, 180}), "lower case and U");
    // the ends of the key range, an empty set, thousands of inserts of one key
    expect(run("poly-A", section_of({std::string(40, 'A')}), section_of({std::string(31, 'A'), std::string(31, 'T'), std::string(31, 'C')}), 31, false) == std::vector<uint64_t>({1, 0, 0}), "poly-A");
    expect(run("poly-T", section_of({std::string(40, 'T')}), section_of({std::string(31, 'A'), std::string(31, 'T'), std::string(31, 'C')}), 31, false) == std::vector<uint64_t>({0, 1, 0}), "poly-T");
    run("poly-A over three tiles", section_of({std::string(3 * kTile, 'A')}), section_of({std::string(50, 'T'), std::string(29, 'A') + "CA"}), 31, true);
    run("an empty set", section_of({R.substr(0, 10), R.substr(10, 10), ""}), section_of({R.substr(0, 100), R.substr(100, 7)}), 11, true);
    // a record over three tiles with hits in the first and the last; thresholds and mates
    run("three tiles", section_of({R}), section_of({R.substr(300, 30), R.substr(0, 40) + random_letters(rng, 3 * kTile) + R.substr(100, 40), R.substr(0, 29)}), 30, true, options(), 5);
    const std::vector<std::string> reads = {R.substr(0, 60), random_letters(rng, 60), random_letters(rng, 60), R.substr(100, 30) + random_letters(rng, 30), random_letters(rng, 60),
                                            random_letters(rng, 60), R.substr(200, 60), "ACGTN", std::string(60, 'N'), R.substr(400, 60)};
    for (uint64_t min_hits : {0, 10, 11, 12})
        for (unsigned min_percent : {0u, 25u, 26u, 28u, 100u})
            for (int flags = 0; flags < 4; flags++) run("thresholds", section_of({R}), section_of(reads), 21, true, options(min_hits, min_percent, flags & 1, flags & 2));
    // nearly full tables and long probe chains (the hooks are read only after nafgpu_test_hooks(1))
    nafgpu_test_hooks(1);
    for (const char *bits : {"0", "3", "8"})
        for (const char *slots : {"128", "256"}) {
            setenv("NAFGPU_KMER_HASH_BITS", bits, 1);
            setenv("NAFGPU_KMER_SLOTS", slots, 1);
            run(std::string("hash bits ") + bits + ", slots " + slots, section_of({R.substr(0, 141)}), section_of({R.substr(0, 100), R.substr(100, 100), revcomp(R.substr(20, 90)), random_letters(rng, 80)}),
                15, true, options(3));
        }
    unsetenv("NAFGPU_KMER_HASH_BITS");
    unsetenv("NAFGPU_KMER_SLOTS");
    nafgpu_test_hooks(0);
    refusals();
    std::printf("OK\n");
    return 0;
}
