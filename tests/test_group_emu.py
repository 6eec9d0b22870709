"""Decoder.group, Selection.group, ParsedText.group and group() on the CPU harness (libnafgpu_emu.so: the same group.hip /
group.cpp, one fibre per work-item): representatives, strands and groups against a Python dict over what the CPU oracle
decodes (tests/group_checks.py holds the checks, shared with tests/test_gpu_group.py)."""
import os
import subprocess

import pytest

import group_checks as gc
import select_checks as sc
from conftest import ROOT, golden_bytes

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
EMU_LIB = os.path.join(EMU_DIR, "libnafgpu_emu.so")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def make(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def emu():
    make("emu")
    from nafcodec_amd import _ffi
    return gc.bind(_ffi.Library(EMU_LIB))


def test_fixtures(emu):
    gc.check_fixtures(emu)


def test_edges(emu):
    gc.check_edges(emu)


def test_random(emu):
    gc.check_random(emu, 2 ** 18)


def test_collisions(emu):
    """hashes cut to 0, 1 and 4 bits (NAFGPU_GRP_HASH_BITS behind nafgpu_test_hooks): the same tables, and the rounds are reached;
    in a process of its own, since the hook is process-wide"""
    gc.run_in_process(EMU_LIB, "check_collisions", timeout=600)


def test_composition(emu):
    gc.check_composition(emu)


def test_refusals(emu):
    gc.check_refusals(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
static void print(const char *name, const std::vector<uint64_t> &v) {
    std::printf(" | %s", name);
    for (uint64_t x : v) std::printf(" %llu", static_cast<unsigned long long>(x));
}
int main(int argc, char **argv) {
    using namespace nafcodec;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    Groups whole = dec.group();
    std::printf("records %llu groups %llu duplicates %llu largest %llu rounds %u strand %d", static_cast<unsigned long long>(whole.n_records()),
                static_cast<unsigned long long>(whole.n_groups()), static_cast<unsigned long long>(whole.n_duplicates()),
                static_cast<unsigned long long>(whole.largest_group()), whole.rounds(), int(whole.strand().size()));
    print("first", whole.group_first());
    // record 0, record 1, record 0 again, its reverse strand, record 1 again: a selection with duplicates
    Selection five = dec.select({Region(0), Region(1), Region(0), Region(0).reverse(), Region(1)});
    GroupOptions both;
    both.both_strands = true;
    Groups g = group(five, both);
    dec = DecoderBuilder().with_path(argv[1]);              // groups and selections outlive their source
    std::printf("\nrecords %llu groups %llu duplicates %llu largest %llu rounds %u", static_cast<unsigned long long>(g.n_records()),
                static_cast<unsigned long long>(g.n_groups()), static_cast<unsigned long long>(g.n_duplicates()),
                static_cast<unsigned long long>(g.largest_group()), g.rounds());
    print("representative", g.representative());
    print("group_of", g.group_of());
    std::printf(" | strand");
    for (uint8_t s : g.strand()) std::printf(" %u", unsigned(s));
    print("first", g.group_first());
    print("size", g.group_size());
    Groups one = group(five.source());
    print("one strand", one.representative());
    GroupOptions bytes;
    bytes.alphabet = 1;
    print("bytes", group(five, bytes).representative());
    Selection unique = dec.select(whole);                   // the first record of every sequence
    std::printf(" | unique %llu", static_cast<unsigned long long>(unique.n_records()));
    int refused = 0;
    bytes.both_strands = true;
    try { group(five, bytes); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    nafgpu_encode_source none{};
    try { group(none); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""


def cpp_expected():
    """the program's two lines, from what the oracle decodes of masked.naf"""
    recs = [r[2] for r in sc.oracle_records(golden_bytes("masked.naf"))]
    whole = gc.expected(recs)
    five = [recs[0], recs[1], recs[0], gc.reverse_complement(recs[0]), recs[1]]
    rep, of, strand, first, size = gc.expected(five, both_strands=True)

    def words(name, v):
        return " | %s %s" % (name, " ".join(str(int(x)) for x in v))
    return "records %d groups %d duplicates %d largest %d rounds 1 strand 0%s\n" % (len(recs), len(whole[3]), len(recs) - len(whole[3]), int(whole[4].max()),
                                                                                   words("first", whole[3])) + \
           "records 5 groups %d duplicates %d largest %d rounds 1%s%s%s%s%s%s%s | unique %d refused 2\n" % (
               len(first), 5 - len(first), int(size.max()), words("representative", rep), words("group_of", of), words("strand", strand), words("first", first),
               words("size", size), words("one strand", gc.expected(five)[0]), words("bytes", gc.expected(five, nucleotide=False)[0]), len(whole[3]))


def test_cpp_group(tmp_path):
    """include/nafcodec.hpp: group of a decoder, of a selection and of a source, select of the groups, compiled and run against
    the CPU harness build; the expected output is computed here from masked.naf by the checks' dict."""
    make("emu")
    src, exe = tmp_path / "group.cpp", tmp_path / "group"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "masked.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = cpp_expected()
    assert "representative 0 1 0 0 1" in want and "strand 0 0 0 1 0" in want
    assert out.stdout == want, out.stdout + want


def test_c_abi_under_sanitizers():
    """tests/group_asan_main.cpp: a program of its own drives the edges (record lengths, every residue of a record's start,
    records one letter apart, empty records, both strands, both alphabets, hashes cut to 0 bits) and the refusals through the
    C-ABI against expectations it computes itself, the sections in allocations of exactly their size at four alignments.
    `make group-asan` compiles it together with the CPU harness with -fsanitize=address,undefined and the sanitizer runtimes
    linked statically, so it runs as an ordinary child process in the environment it is given: nothing is preloaded and
    nothing is taken out."""
    make("group-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "group_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
