"""Decoder.overlap, Selection.overlap, ParsedText.overlap, overlap() and Decoder.merge on the CPU harness (libnafgpu_emu.so: the
same overlap.hip / overlap.cpp / select.cpp, one fibre per work-item, one wave per workgroup): every table against a plain loop
over all shifts of every pair (tests/overlap_checks.py holds the checks, shared with tests/test_gpu_overlap.py)."""
import os
import subprocess

import pytest

import overlap_checks as oc
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def make(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def emu():
    make("emu")
    from nafcodec_amd import _ffi
    return oc.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_fixtures(emu):
    oc.check_fixtures(emu)


def test_edges(emu):
    oc.check_edges(emu)


def test_random(emu):
    oc.check_random(emu, 2 ** 18)


def test_composition(emu):
    oc.check_composition(emu)


def test_refusals(emu):
    oc.check_refusals(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    typedef unsigned long long ull;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    Overlaps o = dec.overlap();
    std::printf("pairs %llu found %llu unmerged %llu cut %llu", ull(o.n_pairs()), ull(o.n_found()), ull(o.n_unmerged()), ull(o.n_cut()));
    const std::vector<nafgpu_pair_overlap> pairs = o.pairs();
    std::printf(" | pair 14: %lld %llu %u %u", (long long)pairs[14].shift, ull(pairs[14].insert), pairs[14].matches, pairs[14].mismatches);
    Selection merged = dec.merge(o);
    Selection cut = dec.select(o);
    std::printf("\nmerged %llu of %llu letters, cut %llu of %llu letters", ull(merged.n_records()), ull(merged.source().n_bases), ull(cut.n_records()),
                ull(cut.source().n_bases));
    std::vector<Region> list;
    for (unsigned k : {0, 34, 1, 14, 2, 28, 3, 20, 5, 16, 6, 13, 8, 23, 9, 29, 15, 19, 21, 30, 4, 7}) list.push_back(Region(k));
    Selection picked = dec.select(list);
    dec = DecoderBuilder().with_path(argv[1]);              // overlaps and selections outlive their source
    Overlaps of_list = overlap(picked);
    Overlaps again = overlap(picked.source());
    OverlapOptions strict;
    strict.max_mismatches = 0;
    std::printf("\nlist: found %llu matches %llu mismatches %llu merged %llu same %d strict %llu", ull(of_list.n_found()), ull(of_list.matches()),
                ull(of_list.mismatches()), ull(of_list.bases_merged()), int(again.n_found() == of_list.n_found() && again.regions().size() == 22),
                ull(overlap(picked, strict).n_found()));
    int refused = 0;
    OverlapOptions wide;
    wide.max_mismatch_percent = 101;
    try { dec.overlap(wide); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    try { dec.merge(of_list); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }     // 22 records, not 42
    nafgpu_encode_source nothing{};
    try { overlap(nothing); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""

CPP_EXPECTED = "pairs 21 found 1 unmerged 40 cut 2 | pair 14: -251 50 48 0\n" \
               "merged 1 of 50 letters, cut 42 of %d letters\n" \
               "list: found 10 matches 1937 mismatches 8 merged 3495 same 1 strict 6 refused 3\n"


def test_cpp_overlap(tmp_path):
    """include/nafcodec.hpp: overlap of a decoder, of a selection and of a source, merge and select(overlaps), compiled and run
    against the CPU harness build on phix.naf.  The figures are the issue's tables; the letters left by the cut come from the
    loop of tests/overlap_checks.py."""
    make("emu")
    from conftest import golden_bytes
    import select_checks as sc
    recs = sc.oracle_records(golden_bytes("phix.naf"))
    letters, ends = oc.layout(recs)
    pairs, regions, _, totals = oc.expected(letters, ends)
    assert totals["n_cut"] == 2 and int(pairs[14]["insert"]) == 50
    src, exe = tmp_path / "overlap.cpp", tmp_path / "overlap"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "phix.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED % totals["bases_after_cut"], out.stdout


def test_c_abi_under_sanitizers():
    """tests/overlap_asan_main.cpp: a program of its own drives the edges of the analysis, the merge through a decoder and the
    refusals through the C-ABI against a loop of its own, the letters in allocations of exactly their size at four alignments.
    `make overlap-asan` compiles it together with the CPU harness with -fsanitize=address,undefined and the sanitizer runtimes
    linked statically, so it runs as an ordinary child process in the environment it is given: nothing is preloaded and nothing
    is taken out."""
    make("overlap-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "overlap_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
