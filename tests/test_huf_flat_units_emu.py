"""k_huf_flat's work unit on the CPU harness (libnafgpu_emu.so: the same huf_flat.hip and zplan.cpp, one fibre per
work-item): round boundaries of a workgroup, many units in one class, a refusal in the middle of them
(tests/huf_flat_unit_checks.py holds the checks, shared with tests/test_gpu_huf_flat_units.py)."""
import os
import re
import subprocess

import pytest

import huf_flat_unit_checks as uk
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return _ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so"))


def test_geometry_is_the_kernels():
    """the round the checks are built around is the one huf_flat.hip is compiled with"""
    with open(os.path.join(CSRC, "huf_flat.hip")) as f:
        src = f.read()
    got = {name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
           for name in ("NAFGPU_FLAT_THREADS", "NAFGPU_FLAT_UNROLL_ASCII", "NAFGPU_FLAT_UNROLL_BYTES")}
    assert got == {"NAFGPU_FLAT_THREADS": uk.LANES, "NAFGPU_FLAT_UNROLL_ASCII": uk.IN_FLIGHT["ascii"],
                   "NAFGPU_FLAT_UNROLL_BYTES": uk.IN_FLIGHT["bytes"]}


def test_fast_stream_writer():
    uk.check_fast_writer()


def test_round_boundaries_ascii(emu):
    uk.check_rounds(emu, "ascii")


def test_round_boundaries_bytes(emu):
    uk.check_rounds(emu, "bytes")


def test_many_units(emu):
    uk.check_many(emu)


def test_refusal_in_the_middle(emu):
    uk.check_refusal_in_the_middle(emu)
