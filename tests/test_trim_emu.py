"""Decoder.trim, Selection.trim, ParsedText.trim and trim() on the CPU harness (libnafgpu_emu.so: the same trim.hip / trim.cpp,
one fibre per work-item): the kept window, the keep flag and the compacted regions of every record against a plain loop over what
the CPU oracle decodes (tests/trim_checks.py holds the checks, shared with tests/test_gpu_trim.py)."""
import os
import subprocess

import pytest

import trim_checks as tk
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


def make(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def emu():
    make("emu")
    from nafcodec_amd import _ffi
    return tk.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_fixtures(emu):
    tk.check_fixtures(emu)


def test_edges(emu):
    tk.check_edges(emu)


def test_random(emu):
    tk.check_random(emu, 2 ** 18)


def test_composition(emu):
    tk.check_composition(emu)


def test_refusals(emu):
    tk.check_refusals(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    typedef unsigned long long ull;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    TrimOptions sums;
    sums.cut_front = sums.cut_tail = 20;
    Trims t = dec.trim(sums);
    std::printf("records %llu kept %llu changed %llu left %llu", ull(t.n_records()), ull(t.n_kept()), ull(t.n_changed()), ull(t.bases_in_windows()));
    const std::vector<nafgpu_region> regions = t.regions();
    for (size_t k = 0; k < 3; k++) std::printf(" | %llu %llu %llu", ull(regions[k].record), ull(regions[k].start), ull(regions[k].end));
    TrimOptions all = sums;
    all.window = 10;
    all.window_quality = 30;
    all.trim_n = true;
    all.min_length = 60;
    Trims cleaned = dec.trim(all);
    std::printf("\nall: kept %llu changed %llu left %llu kept letters %llu", ull(cleaned.n_kept()), ull(cleaned.n_changed()), ull(cleaned.bases_in_windows()),
                ull(cleaned.bases_kept()));
    Selection sel = dec.select(cleaned);                    // the kept reads cut to their windows
    dec = DecoderBuilder().with_path(argv[1]);              // trims and selections outlive their source
    uint64_t keep = 0;
    for (uint8_t k : cleaned.keep()) keep += k;
    std::printf(" selected %llu of %llu letters, flags %llu", ull(sel.n_records()), ull(sel.source().n_bases), ull(keep));
    TrimOptions none;
    Trims same = trim(sel, none);
    Trims again = trim(sel.source(), none);
    std::printf("\nselection: records %llu changed %llu left %llu same %d", ull(same.n_records()), ull(same.n_changed()), ull(same.bases_in_windows()),
                int(again.n_records() == same.n_records() && again.bases_kept() == same.bases_kept()));
    int refused = 0;
    TrimOptions wide;
    wide.window = 65;
    try { dec.trim(wide); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    nafgpu_encode_source nothing{};
    try { trim(nothing); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""


def test_cpp_trim(tmp_path):
    """include/nafcodec.hpp: trim of a decoder, of a selection and of a source, compiled and run against the CPU harness build on
    phix.naf.  The first line is the issue's table (42 reads changed, 12 175 letters left under cut_front = cut_tail = 20); the
    others are what tests/trim_checks.py's loop gives for the same options."""
    make("emu")
    src, exe = tmp_path / "trim.cpp", tmp_path / "trim"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "phix.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED == cpp_expected(), out.stdout


CPP_EXPECTED = "records 42 kept 42 changed 42 left 12175 | 0 1 300 | 1 1 300 | 2 1 301\n" \
               "all: kept 39 changed 42 left 9833 kept letters 9774 selected 39 of 9774 letters, flags 39\n" \
               "selection: records 39 changed 0 left 9774 same 1 refused 2\n"


def cpp_expected():
    """the same lines from the loop of tests/trim_checks.py"""
    from conftest import golden_bytes
    import select_checks as sc
    recs = sc.oracle_records(golden_bytes("phix.naf"))
    letters, quality, ends = tk.layout(recs)
    sums, _ = tk.expected(letters, quality, ends, cut_front=20, cut_tail=20)
    regions, keep = tk.expected(letters, quality, ends, cut_front=20, cut_tail=20, window=(10, 30), trim_n=True, min_length=60)
    size = (regions["end"] - regions["start"]).astype(int)
    kept = int(size[keep.astype(bool)].sum())
    assert int((sums["end"] - sums["start"]).sum()) == 12175
    first = " | ".join("%d %d %d" % tuple(r)[:3] for r in sums[:3])
    return "records 42 kept 42 changed 42 left 12175 | %s\nall: kept %d changed %d left %d kept letters %d selected %d of %d letters, flags %d\n" \
           "selection: records %d changed 0 left %d same 1 refused 2\n" % (first, keep.sum(), (size != np_lengths(ends)).sum(), size.sum(), kept, keep.sum(), kept,
                                                                            keep.sum(), keep.sum(), kept)


def np_lengths(ends):
    import numpy as np
    return np.diff(np.concatenate(([0], ends.astype(np.int64))))


def test_c_abi_under_sanitizers():
    """tests/trim_asan_main.cpp: a program of its own drives the edges of the four steps (window lengths, tile, lane and chunk
    edges, record ends, both routes) and the refusals through the C-ABI against a loop of its own, the sections in allocations of
    exactly their size at four alignments.  `make trim-asan` compiles it together with the CPU harness with
    -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an ordinary child process in the
    environment it is given: nothing is preloaded and nothing is taken out."""
    make("trim-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "trim_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
