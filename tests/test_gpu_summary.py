"""Decoder.summarize, Selection.summarize, ParsedText.summarize and summarize() on an MI355X (run with -m gpu): the checks
of tests/test_summary_emu.py through libnafgpu.so (tests/summary_checks.py holds them), and positions and counters past 2^32.

Bar: every table equals, as uint64, numpy over what the CPU oracle decodes or over the source's own bytes read back (integer
work only, no tolerance).  No time is asserted."""
import os
import subprocess
import sys

import pytest

import summary_checks as sk
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


def test_long_record(lib):
    sk.check_long_record(lib)


def test_read_set(lib):
    sk.check_read_set(lib)


def run_alone(call, timeout, first=""):
    script = "%simport sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import summary_checks as sk\nfrom nafcodec_amd import _ffi\nsk.%s(sk.bind(_ffi.default()))\nprint('OK')\n" \
             % (first, ROOT, os.path.join(ROOT, "tests"), call)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("route", sk.ROUTES)
def test_routes(lib, route):
    """NAFGPU_SUM_ROUTE after nafgpu_test_hooks(1): checks 1-4 with every tile forced down one route, in a process of its
    own, so that the hook does not leak"""
    run_alone("check_route_" + route, 300)


def test_refusals(lib):
    sk.check_refusals(lib)


def test_past_4_gib(lib):
    """2^28 synthetic letters, masked, against numpy; the record list 17 times (4.56 G letters, histograms and totals past
    2^32); the same letters as one record (columns past 2^32 in one row); in a process of its own, under a time limit."""
    # (PyTorch, whose tensor holds the end table, is loaded before libnafgpu.so: it brings its own copy of the HIP runtime, and
    # loaded second that copy finds no device -- bench.py has the same order)
    run_alone("check_past_u32", 600, first="import torch\n")
