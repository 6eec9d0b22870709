"""Decoder.select and Decoder.find on the CPU harness (libnafgpu_emu.so: the same select.hip / select.cpp, one fibre per
work-item): records and regions of a decoded archive against Python slicing of what the CPU oracle decodes
(tests/select_checks.py holds the checks, shared with tests/test_gpu_select.py)."""
import os
import subprocess
import sys

import pytest

import select_checks as sc
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return sc.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_phix(emu):
    sc.check_phix(emu)


def test_masked(emu):
    sc.check_masked(emu)


def test_protein(emu):
    sc.check_protein(emu)


def test_cp040672(emu):
    sc.check_cp040672(emu)


def test_long_record(emu):
    sc.check_long_record(emu)


def test_small_fixture(emu):
    sc.check_small_fixture(emu)


def test_edges_of_the_gather(emu):
    sc.check_edges(emu)


def test_names(emu):
    sc.check_names(emu)


def test_find_records(emu):
    sc.check_find(emu)


def test_find_records_colliding():
    """NAFGPU_SEL_HASH_BITS=2 after nafgpu_test_hooks(1): in a process of its own, so that the hook does not leak"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import select_checks as sc\nfrom nafcodec_amd import _ffi\nsc.check_find_colliding(sc.bind(_ffi.Library(%r)))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu.so"))
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_refusals(emu):
    sc.check_refusals(emu)


def test_composition(emu):
    sc.check_composition(emu)


CPP_PROGRAM = r"""
#include <cstdio>
#include "nafcodec.hpp"
int main(int argc, char **argv) {
    using namespace nafcodec;
    Decoder dec = DecoderBuilder().with_path(argv[1]);
    const std::vector<std::optional<uint64_t>> found = dec.find({"test2", "nobody", "test1"});
    std::vector<Region> regions;
    regions.push_back(Region(*found[0], 522, 534).reverse());
    regions.push_back(Region(*found[2]).slice(653, 680));
    Selection sel = dec.select(regions, true);
    dec = DecoderBuilder().with_path(argv[1]);      // the selection is a copy
    const std::string text = sel.to_text(0);
    const EncoderBuilder fields = EncoderBuilder(SequenceType::Dna).id(true).sequence(true).compression_level(1).mask(true);
    const std::string archive = encode_device(sel, fields, 0);
    Decoder back = DecoderBuilder().with_bytes(reinterpret_cast<const uint8_t *>(archive.data()), archive.size());
    std::string seen;
    while (auto rec = back.next()) seen += *rec->id + "=" + *rec->sequence + "|";
    int refused = 0;
    try { dec.select({Region(2)}); } catch (const Error &e) { refused += e.raw.status == NAFGPU_E_INVALID_ARG; }
    std::printf("%s%s found %d%d%d regions %llu letters %llu refused %d\n", text.c_str(), seen.c_str(), int(found[0].has_value()), int(found[1].has_value()),
                int(found[2].has_value()), static_cast<unsigned long long>(sel.n_regions()), static_cast<unsigned long long>(sel.source().n_bases), refused);
    return 0;
}
"""


def test_cpp_select(tmp_path):
    """include/nafcodec.hpp: find, select, Selection, encode_device of a selection, compiled and run against the CPU harness
    build.  Two regions of masked.naf by name, one on the reverse strand, both across a soft-masked stretch; the expected text
    is written out below."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    src, exe = tmp_path / "select.cpp", tmp_path / "select"
    src.write_text(CPP_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", EMU_DIR, "-l:libnafgpu_emu.so", "-Wl,-rpath," + EMU_DIR])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "masked.naf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout == CPP_EXPECTED, out.stdout


CPP_EXPECTED = ">test2:523-534/rc\nggtggaaatGTT\n>test1:654-680\nGCATcatcatcaagaagcaggacGAAT\n" \
               "test2:523-534/rc=ggtggaaatGTT|test1:654-680=GCATcatcatcaagaagcaggacGAAT| found 101 regions 2 letters 39 refused 1\n"


def test_c_abi_under_sanitizers():
    """tests/select_asan_main.cpp: a program of its own drives the edges of the gather and the id lookup through the C-ABI
    against expectations it computes itself.  `make select-asan` compiles it together with the CPU harness (the sources and
    flags of `make emu-asan`) with -fsanitize=address,undefined and the sanitizer runtimes linked statically, so it runs as an
    ordinary child process in the environment it is given: nothing is preloaded and nothing is taken out."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "select-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    out = subprocess.run([os.path.join(EMU_DIR, "select_asan")], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-2000:] + out.stderr[-4000:]
