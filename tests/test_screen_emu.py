"""Decoder.kmers / .screen, the same on Selection and ParsedText, kmers() and screen() on the CPU harness (libnafgpu_emu.so: the
same screen.hip / screen.cpp, one fibre per work-item): the set's figures and every table of a screen against a plain loop over
what the CPU oracle decodes (tests/screen_checks.py holds the checks, shared with tests/test_gpu_screen.py)."""
import os
import subprocess
import sys

import pytest

import screen_checks as sk
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
    sk.check_composition(emu, threads=False)


def test_refusals(emu):
    sk.check_refusals(emu)


def test_table_hooks():
    """NAFGPU_KMER_HASH_BITS and NAFGPU_KMER_SLOTS after nafgpu_test_hooks(1): in a process of its own, so that the hooks do not leak"""
    make("emu")
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import screen_checks as sk\nfrom nafcodec_amd import _ffi\nsk.check_hooks(sk.bind(_ffi.Library(%r)))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu.so"))
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    typedef unsigned long long ull;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    std::vector<Region> head;
    for (uint64_t r = 0; r < 8; r++) head.push_back(Region(r));
    Selection first = dec.select(head);
    KmerSet set = kmers(first);                             // k = 31, canonical
    first = dec.select(head);                               // a set outlives its source
    Screens s = dec.screen(set);
    ScreenOptions half, mates;
    half.min_percent = 50;
    mates.interleaved = true;
    std::printf("kmers %llu of %llu windows | windows %llu hits %llu matched %llu, at 50 %% %llu, mates %llu | unmatched letters %llu", ull(set.n_kmers()),
                ull(set.n_windows()), ull(s.n_windows()), ull(s.n_hits()), ull(s.n_matched()), ull(dec.screen(set, half).n_matched()),
                ull(dec.screen(set, mates).n_matched()), ull(s.bases_kept()));
    const std::vector<nafgpu_region> regions = s.regions();
    std::printf("\nread 13: %llu of %llu, %llu .. %llu", ull(s.hits()[13]), ull(s.windows()[13]), ull(regions[13].start), ull(regions[13].end));
    Selection clean = dec.select(s);                        // the reads that do not match, whole
    uint64_t keep = 0, match = 0;
    for (uint8_t v : s.keep()) keep += v;
    for (uint8_t v : s.match()) match += v;
    std::printf("\nselected %llu of %llu letters, flags %llu and %llu", ull(clean.n_records()), ull(clean.source().n_bases), ull(keep), ull(match));
    ScreenOptions bait;
    bait.keep_matched = true;
    KmerOptions forward;
    forward.k = 15;
    forward.canonical = false;
    KmerSet small = dec.kmers(forward);
    Screens same = screen(clean, small, bait);
    Screens again = screen(clean.source(), small, bait);
    std::printf("\nselection: records %llu kept %llu hits %llu of %llu same %d", ull(same.n_records()), ull(same.n_kept()), ull(same.n_hits()), ull(same.n_windows()),
                int(again.n_hits() == same.n_hits() && again.kept_regions().size() == same.n_kept()));
    int refused = 0;
    KmerOptions wide;
    wide.k = 32;
    try { dec.kmers(wide); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    ScreenOptions much;
    much.min_percent = 101;
    try { dec.screen(set, much); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    nafgpu_encode_source nothing{};
    try { kmers(nothing); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""

CPP_EXPECTED = "kmers 2009 of 2160 windows | windows 11135 hits 4114 matched 25, at 50 %% 15, mates 34 | unmatched letters 4911\n" \
               "read 13: 81 of 270, 190 .. 301\n" \
               "selected 17 of 4911 letters, flags 17 and 25\n" \
               "selection: records 17 kept 17 hits %d of %d same 1 refused 3\n"


def test_cpp_screen(tmp_path):
    """include/nafcodec.hpp: a set of a selection and of a decoder, screens of a decoder, of a selection and of a source, compiled
    and run against the CPU harness build on phix.naf.  The first lines are the issue's table (k = 31, canonical) and its read 13;
    the last one is what tests/screen_checks.py's loop gives for the unmatched reads against all 15-mers of the archive."""
    make("emu")
    from conftest import golden_bytes
    import select_checks as sc
    import trim_checks as tk
    recs = sc.oracle_records(golden_bytes("phix.naf"))
    letters, _, ends = tk.layout(recs)
    ref = sk.Ref(b"".join(r[2] for r in recs[:8]), ends[:8], 31)
    windows, hits, _, match, keep = sk.expected(letters, ends, ref)
    assert (int(match.sum()), int(keep.sum())) == (25, 17)
    clean = [r[2] for r, flag in zip(recs, keep) if flag]
    own = sk.expected(b"".join(clean), sk.ends_of(clean), sk.Ref(letters, ends, 15, False))
    assert (own[0] == own[1]).all()                          # every 15-mer of a read is one of the archive's
    src, exe = tmp_path / "screen.cpp", tmp_path / "screen"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "phix.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED % (int(own[1].sum()), int(own[0].sum())), out.stdout


def test_c_abi_under_sanitizers():
    """tests/screen_asan_main.cpp: a program of its own drives the set and the screen through the C-ABI against a loop of its own
    (every k, windows at tile and lane edges, record ends, non-letters, nearly full tables, the refusals), the sections in
    allocations of exactly their size at four alignments.  `make screen-asan` compiles it together with the CPU harness with
    -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an ordinary child process in the
    environment it is given: nothing is preloaded and nothing is taken out."""
    make("screen-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "screen_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
