"""Decoder.summarize, Selection.summarize, ParsedText.summarize and summarize() on the CPU harness (libnafgpu_emu.so: the
same summary.hip / summary.cpp, one fibre per work-item): class counts, quality sums and histograms against numpy over what
the CPU oracle decodes (tests/summary_checks.py holds the checks, shared with tests/test_gpu_summary.py)."""
import os
import subprocess
import sys

import pytest

import summary_checks as sk
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


def test_default_table():
    sk.check_default_table()


def test_fixtures(emu):
    sk.check_fixtures(emu)


def test_edges(emu):
    sk.check_edges(emu)


def test_long_record(emu):
    sk.check_long_record(emu)


def test_read_set(emu):
    sk.check_read_set(emu)


@pytest.mark.parametrize("route", sk.ROUTES)
def test_routes(route):
    """NAFGPU_SUM_ROUTE after nafgpu_test_hooks(1): checks 1-4 with every tile forced down one route, in a process of its
    own, so that the hook does not leak"""
    make("emu")
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import summary_checks as sk\nfrom nafcodec_amd import _ffi\nsk.check_route(sk.bind(_ffi.Library(%r)), %r)\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu.so"), route)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_refusals(emu):
    sk.check_refusals(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    Summary all = summarize(dec);
    const std::vector<uint64_t> counts = all.counts(), hist = all.letter_hist(), totals = all.totals();
    std::printf("records %llu quality %zu", static_cast<unsigned long long>(all.n_records()), all.quality_sum().size());
    for (size_t k = 0; k < counts.size(); k++) std::printf("%s%llu", k % 8 ? " " : " | ", static_cast<unsigned long long>(counts[k]));
    std::printf(" | totals");
    for (uint64_t v : totals) std::printf(" %llu", static_cast<unsigned long long>(v));
    std::printf(" | a %llu N %llu\n", static_cast<unsigned long long>(hist['a']), static_cast<unsigned long long>(hist['N']));
    Selection sel = dec.select({Region(1).slice(522, 534).reverse(), Region(0).slice(653, 680)});
    uint8_t upper[256] = {0};                               // a table of its own: column 0 upper case, column 1 G or C in either case
    for (int c = 'A'; c <= 'Z'; c++) upper[c] = 1;
    for (int c : {'G', 'C', 'g', 'c'}) upper[c] |= 2;
    Summary cut = summarize(sel, 0, upper);
    dec = DecoderBuilder().with_path(argv[1]);              // a summary outlives its source
    Summary same = summarize(sel.source(), 0, upper);
    std::printf("cut");
    for (uint64_t v : cut.counts()) std::printf(" %llu", static_cast<unsigned long long>(v));
    std::printf(" same %d", int(cut.counts() == same.counts() && cut.totals() == same.totals()));
    int refused = 0;
    nafgpu_encode_source none{};
    try { summarize(none, 0); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf(" refused %d\n", refused);
    return 0;
}
"""


def test_cpp_summary(tmp_path):
    """include/nafcodec.hpp: summarize of a decoder, of a selection and of a source, compiled and run against the CPU harness
    build.  masked.naf: two records, the expected numbers are written out below (the regions are those of test_cpp_select:
    ggtggaaatGTT and GCATcatcatcaagaagcaggacGAAT)."""
    make("emu")
    src, exe = tmp_path / "summary.cpp", tmp_path / "summary"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "masked.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED, out.stdout


CPP_EXPECTED = "records 2 quality 0 | 565 221 321 443 0 0 0 58 | 541 388 205 666 0 0 0 123 | totals 1106 609 526 1109 0 0 0 181 | a 54 N 0\n" \
               "cut 3 5 0 0 0 0 0 0 8 12 0 0 0 0 0 0 same 1 refused 1\n"


def test_c_abi_under_sanitizers():
    """tests/summary_asan_main.cpp: a program of its own drives the edges of the per-record pass, a table of its own, every
    route and the refusals of hand-made end tables (decreasing, beyond the section, the first record, the last record) through
    the C-ABI against expectations it computes itself.  `make summary-asan` compiles it together with the CPU harness with
    -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an ordinary child process in the
    environment it is given: nothing is preloaded and nothing is taken out."""
    make("summary-asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "summary_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
