"""Decoder.select and Decoder.find on an MI355X (run with -m gpu): the checks of tests/test_select_emu.py through
libnafgpu.so (tests/select_checks.py holds them), and a selection whose output positions pass 2^32.

Bar: ids, comments, letters, qualities and the three end tables are, byte for byte, Python slices of what the CPU oracle
decodes; at size the 64-bit checksums (integer work only).  No time is asserted."""
import os
import subprocess
import sys

import pytest

import select_checks as sc
from conftest import ROOT
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = sc.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_phix(lib):
    sc.check_phix(lib)


def test_masked(lib):
    sc.check_masked(lib)


def test_protein(lib):
    sc.check_protein(lib)


def test_cp040672(lib):
    sc.check_cp040672(lib)


def test_long_record(lib):
    sc.check_long_record(lib)


def test_small_fixture(lib):
    sc.check_small_fixture(lib)


def test_edges_of_the_gather(lib):
    sc.check_edges(lib)


def test_names(lib):
    sc.check_names(lib)


def test_find_records(lib):
    sc.check_find(lib)


def run_alone(call, timeout):
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import select_checks as sc\nfrom nafcodec_amd import _ffi\nsc.%s(sc.bind(_ffi.default()))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), call)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_find_records_colliding(lib):
    """NAFGPU_SEL_HASH_BITS=2 after nafgpu_test_hooks(1): in a process of its own, so that the hook does not leak"""
    run_alone("check_find_colliding", 300)


def test_refusals(lib):
    sc.check_refusals(lib)


def test_composition(lib):
    sc.check_composition(lib)


def test_output_past_4_gib(lib):
    """2^28 synthetic letters, masked, every record whole, the list 17 times: 4.56 GB of output, positions past 2^32; in a
    process of its own, under a time limit."""
    run_alone("check_past_u32", 600)
