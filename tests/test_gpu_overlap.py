"""Decoder.overlap, Selection.overlap, ParsedText.overlap, overlap() and Decoder.merge on an MI355X (run with -m gpu): the
checks of tests/test_overlap_emu.py through libnafgpu.so (tests/overlap_checks.py holds them; four pairs per workgroup here),
and positions past 2^32.

Bar: every table equals, as struct and integer arrays, a plain loop over all shifts of every pair, over what the CPU oracle
decodes or over the source's own bytes read back (integer work only, no tolerance).  No time is asserted."""
import os
import subprocess
import sys

import pytest

import overlap_checks as oc
from conftest import ROOT
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = oc.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_fixtures(lib):
    oc.check_fixtures(lib)


def test_edges(lib):
    oc.check_edges(lib)


def test_random(lib):
    oc.check_random(lib, 2 ** 22)


def test_composition(lib):
    oc.check_composition(lib)


def test_refusals(lib):
    oc.check_refusals(lib)


def test_past_4_gib(lib):
    """2^28 synthetic letters as pairs of reads, the first 2 000 pairs against the loop; their record list selected 17 times
    (4.56 G letters: absolute positions past 2^32): the tables of copy c are those of copy 0 with the record shifted; in a
    process of its own, under a time limit."""
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import overlap_checks as oc\nfrom nafcodec_amd import _ffi\noc.check_past_u32(oc.bind(_ffi.default()))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
