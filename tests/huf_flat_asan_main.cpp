// tests/huf_flat_asan_main.cpp -- TEST PROGRAM, NOT PRODUCT CODE.
//
// The plan level of flat Huffman trees (plan.h: kTblFlat) and k_huf_flat through the C-ABI, on the CPU harness.  Arguments,
// written by tests/huf_flat_checks.py (write_plan_inputs):
//   flat:BASE     BASE.zst is a section payload all of whose Huffman streams qualify, BASE.bin what it decodes to
//   mixed:BASE    ... some of whose streams qualify and some do not
//   refuse:BASE   BASE.zst holds a flat stream that does not end where it must
//   fixture:PATH  a NAF archive of the reference's: none of its sections may yield a flat class
// For flat / mixed: pack_tasks yields kTblFlat classes (only such classes for flat); with the switch off it yields none; with
// streams in parts the plan is byte for byte the one the switch-off plan is; nafgpu_zstd_decompress gives BASE.bin into a
// buffer of exactly its size.  `make huf-flat-asan` (tests/test_huf_flat_emu.py) compiles it and the CPU harness into one
// program with -fsanitize=address,undefined, the runtimes linked statically; it runs as an ordinary process.  Prints OK and
// returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../nafcodec_amd/csrc/container.h"
#include "../nafcodec_amd/csrc/zplan.h"
#include "nafgpu.h"

using namespace nafgpu;

namespace {

[[noreturn]] void die(const std::string &what) {
    std::printf("FAILED: %s\n", what.c_str());
    std::exit(1);
}
void expect(bool ok, const std::string &what) {
    if (!ok) die(what);
}

std::vector<uint8_t> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    expect(f.good(), "cannot read " + path);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// walk + pack with the given switches
ZPlan plan_of(const std::vector<uint8_t> &payload, bool flat, uint32_t force_split, const std::string &what) {
    ZPlan p;
    bool truncated = false;
    const std::string err = walk_zstd(payload.data(), payload.size(), &p, &truncated);
    expect(err.empty(), what + ": walk: " + err);
    set_huf_flat(flat);
    set_huf_split(0, force_split);
    pack_tasks_public(&p);
    set_huf_flat(true);
    set_huf_split(0, 0);
    return p;
}

void count_classes(const ZPlan &p, size_t *n_flat, size_t *n_other) {
    *n_flat = *n_other = 0;
    for (const HufClass &c : p.classes) (c.tbl == kTblFlat ? *n_flat : *n_other)++;
}

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

void check_plans(const std::string &what, const std::vector<uint8_t> &payload, bool all_flat) {
    size_t n_flat, n_other;
    const ZPlan on = plan_of(payload, true, 0, what);
    count_classes(on, &n_flat, &n_other);
    expect(n_flat > 0, what + ": no flat class");
    expect(all_flat ? n_other == 0 : n_other > 0, what + ": classes of the other kinds: " + std::to_string(n_other));
    for (const HufClass &c : on.classes) {
        if (c.tbl != kTblFlat) continue;
        expect(c.seg == 0 && c.split == 1 && c.lds_bytes == 0 && c.sync_lds == 0, what + ": a flat class with seg, parts or LDS");
        for (uint32_t t = c.first_task; t < c.first_task + c.n_tasks; t++) {
            const HufTask &task = on.tasks[t];
            for (uint32_t s = task.first_stream; s < task.first_stream + task.n_streams; s++) {
                const HufStream &hs = on.streams[s];
                expect(hs.tbl_lds < task.n_copies, what + ": tree index outside the task's copies");
                const HufTblCopy &cp = on.tbl_copies[task.first_copy + hs.tbl_lds];
                expect(hs.max_bits >= 1 && hs.max_bits <= 8 && cp.n_entries == (1u << hs.max_bits), what + ": code length");
                expect(size_t(cp.pool_off) + cp.n_entries <= on.huf_pool.size(), what + ": pool range");
                for (uint32_t i = 0; i < cp.n_entries; i++)
                    expect((on.huf_pool[cp.pool_off + i] >> 8) == hs.max_bits, what + ": a code of another length");
                expect(!(hs.flags & 2) && hs.sub == 0, what + ": a flat stream with segments or in parts");
            }
        }
    }
    const ZPlan off = plan_of(payload, false, 0, what);
    count_classes(off, &n_flat, &n_other);
    expect(n_flat == 0, what + ": a flat class with the switch off");
    const ZPlan parts_on = plan_of(payload, true, 2, what), parts_off = plan_of(payload, false, 2, what);
    count_classes(parts_on, &n_flat, &n_other);
    expect(n_flat == 0, what + ": a flat class of streams in parts");
    expect(same(parts_on.streams, parts_off.streams) && same(parts_on.tasks, parts_off.tasks) && same(parts_on.classes, parts_off.classes) &&
               same(parts_on.tbl_copies, parts_off.tbl_copies) && same(parts_on.dict_pool, parts_off.dict_pool),
           what + ": the plan of streams in parts differs with the switch");
}

void check_decode(const std::string &what, const std::vector<uint8_t> &payload, const std::vector<uint8_t> &want) {
    for (const char *flat : {"1", "0"}) {
        setenv("NAFGPU_HUF_FLAT", flat, 1);
        std::vector<uint8_t> got(want.size() ? want.size() : 1);
        size_t produced = 0;
        nafgpu_error err;
        const int rc = nafgpu_zstd_decompress(payload.data(), payload.size(), got.data(), want.size(), &produced, -1, &err);
        expect(rc == NAFGPU_OK, what + ": decode failed (flat " + flat + "): " + err.message);
        expect(produced == want.size() && std::memcmp(got.data(), want.data(), want.size()) == 0, what + ": other bytes (flat " + flat + ")");
    }
}

void check_refused(const std::string &what, const std::vector<uint8_t> &payload) {
    for (const char *flat : {"1", "0"}) {
        setenv("NAFGPU_HUF_FLAT", flat, 1);
        std::vector<uint8_t> got(1 << 16);
        size_t produced = 0;
        nafgpu_error err;
        const int rc = nafgpu_zstd_decompress(payload.data(), payload.size(), got.data(), got.size(), &produced, -1, &err);
        expect(rc == NAFGPU_E_IO && err.io_kind == NAFGPU_IO_INVALID_DATA, what + ": not refused as invalid data (flat " + flat + ")");
    }
}

void check_fixture(const std::string &path) {
    const std::vector<uint8_t> blob = slurp(path);
    nafgpu_header h;
    SectionInfo sec[kNumSections];
    expect(parse_archive(blob.data(), blob.size(), &h, sec).ok(), path + ": parse_archive");
    size_t walked = 0;
    for (int s = 0; s < kNumSections; s++) {
        if (!sec[s].present || !sec[s].compressed_size) continue;
        const std::vector<uint8_t> payload(blob.begin() + sec[s].offset, blob.begin() + sec[s].offset + sec[s].compressed_size);
        size_t n_flat, n_other;
        count_classes(plan_of(payload, true, 0, path), &n_flat, &n_other);
        expect(n_flat == 0, path + ": section " + std::to_string(s) + " yields a flat class");
        walked++;
    }
    expect(walked > 0, path + ": no section walked");
}

}  // namespace

int main(int argc, char **argv) {
    nafgpu_test_hooks(1);
    setenv("NAFGPU_HUF_SPLIT", "0", 1);
    size_t n = 0;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        const size_t colon = arg.find(':');
        expect(colon != std::string::npos, "argument " + arg);
        const std::string kind = arg.substr(0, colon), base = arg.substr(colon + 1);
        if (kind == "flat" || kind == "mixed") {
            const std::vector<uint8_t> payload = slurp(base + ".zst");
            check_plans(base, payload, kind == "flat");
            check_decode(base, payload, slurp(base + ".bin"));
        } else if (kind == "refuse") {
            check_refused(base, slurp(base + ".zst"));
        } else if (kind == "fixture") {
            check_fixture(base);
        } else {
            die("argument " + arg);
        }
        n++;
    }
    expect(n > 0, "no arguments");
    std::printf("%zu inputs\nOK\n", n);
    return 0;
}
