"""Decoder.kmers / .screen, the same on Selection and ParsedText, kmers() and screen() on an MI355X (run with -m gpu): the checks
of tests/test_screen_emu.py through libnafgpu.so (tests/screen_checks.py holds them), and positions and tile indices past 2^32.

Bar: the set's figures and every table of a screen equal, as struct and integer arrays, a plain loop over what the CPU oracle
decodes or over the source's own bytes read back (integer work only, no tolerance).  No time is asserted."""
import os
import subprocess
import sys

import pytest

import screen_checks as sk
from conftest import ROOT
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = sk.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_fixtures(lib):
    sk.check_fixtures(lib)


def test_edges(lib):
    sk.check_edges(lib)


def test_random(lib):
    sk.check_random(lib, 2 ** 22)


def test_composition(lib):
    sk.check_composition(lib)


def test_refusals(lib):
    sk.check_refusals(lib)


def run_alone(call, timeout):
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import screen_checks as sk\nfrom nafcodec_amd import _ffi\nsk.%s(sk.bind(_ffi.default()))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), call)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_table_hooks():
    """NAFGPU_KMER_HASH_BITS and NAFGPU_KMER_SLOTS after nafgpu_test_hooks(1): in a process of its own, so that the hooks do not leak"""
    run_alone("check_hooks", 300)


def test_past_4_gib():
    """2^28 synthetic letters against the yardstick, the set built from their first 2^20; their record list selected 17 times
    (4.56 G letters: absolute positions and tile indices past 2^32): the screens of copy c are those of copy 0 with the record
    shifted; in a process of its own, under a time limit."""
    run_alone("check_past_u32", 600)
