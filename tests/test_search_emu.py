"""Decoder.search, Selection.search, ParsedText.search and search() on the CPU harness (libnafgpu_emu.so: the same search.hip /
search.cpp, one fibre per work-item): hits, their mismatch counts and the records' rows against numpy over what the CPU oracle
decodes (tests/search_checks.py holds the checks, shared with tests/test_gpu_search.py)."""
import os
import subprocess

import pytest

import search_checks as sk
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def make(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def emu():
    make("emu")
    from nafcodec_amd import _ffi
    return sk.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_fixtures(emu):
    sk.check_fixtures(emu)


def test_edges(emu):
    sk.check_edges(emu)


def test_random(emu):
    sk.check_random(emu, 2 ** 18)


def test_composition(emu):
    sk.check_composition(emu)


def test_refusals(emu):
    sk.check_refusals(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    SearchOptions both;
    both.both_strands = true;
    Hits site = dec.search({"GAATTC"}, both);
    std::printf("hits %llu records %llu", static_cast<unsigned long long>(site.n_hits()), static_cast<unsigned long long>(site.n_records()));
    const std::vector<nafgpu_region> regions = site.regions();
    const std::vector<nafgpu_hit_info> info = site.info();
    for (size_t i = 0; i < regions.size(); i++)
        std::printf(" | %llu %llu %llu %c %u %u", static_cast<unsigned long long>(regions[i].record), static_cast<unsigned long long>(regions[i].start),
                    static_cast<unsigned long long>(regions[i].end), regions[i].reverse_complement ? '-' : '+', info[i].pattern, unsigned(info[i].mismatches));
    std::printf(" | begin");
    for (uint64_t v : site.record_hit_begin()) std::printf(" %llu", static_cast<unsigned long long>(v));
    std::printf(" | per pattern");
    for (uint64_t v : site.pattern_hits()) std::printf(" %llu", static_cast<unsigned long long>(v));
    Selection windows = dec.select(site);                   // the hits as records: both read GAATTC
    dec = DecoderBuilder().with_path(argv[1]);              // hits and selections outlive their source
    SearchOptions one;
    one.max_mismatches = 1;
    one.both_strands = 0;
    Hits again = search(windows, {"GAATTC", "GAATTG"}, one);
    std::printf("\nwindows %llu hits %llu:", static_cast<unsigned long long>(windows.n_records()), static_cast<unsigned long long>(again.n_hits()));
    const std::vector<nafgpu_hit_info> how = again.info();
    for (const nafgpu_hit_info &h : how) std::printf(" %u/%u", h.pattern, unsigned(h.mismatches));
    Hits same = search(windows.source(), {"GAATTC", "GAATTG"}, one);
    std::printf(" same %d", int(same.n_hits() == again.n_hits() && same.record_hit_begin() == again.record_hit_begin()));
    int refused = 0;
    try { dec.search({"GAXTTC"}); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    try { dec.search({}); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    nafgpu_encode_source none{};
    try { search(none, {"GAATTC"}); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""


def test_cpp_search(tmp_path):
    """include/nafcodec.hpp: search of a decoder, of a selection and of a source, compiled and run against the CPU harness
    build.  masked.naf: GAATTC lies once, in record 0 at 1295, and is its own reverse complement: one hit per strand; the two
    windows selected read GAATTC, which GAATTG matches with one substitution."""
    make("emu")
    src, exe = tmp_path / "search.cpp", tmp_path / "search"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "masked.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED, out.stdout


CPP_EXPECTED = "hits 2 records 2 | 0 1295 1301 + 0 0 | 0 1295 1301 - 0 0 | begin 0 2 2 | per pattern 2\n" \
               "windows 2 hits 4: 0/0 1/1 0/0 1/1 same 1 refused 3\n"


def test_c_abi_under_sanitizers():
    """tests/search_asan_main.cpp: a program of its own drives the edges of the match (pattern lengths, tile and lane edges,
    record ends, dense output, substitutions, both alphabets) and the refusals through the C-ABI against expectations it computes
    itself, the sections in allocations of exactly their size at four alignments.  `make search-asan` compiles it together with
    the CPU harness with -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an ordinary
    child process in the environment it is given: nothing is preloaded and nothing is taken out."""
    make("search-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "search_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
