"""parse_text and encode_text on an MI355X (run with -m gpu): the checks of tests/test_text_parse_emu.py through libnafgpu.so
(tests/text_parse_checks.py holds them), text -> archive -> text on the device, and round trips at size in which the text
never leaves HBM between format_device and parse_text.

Bar: the records are the yardstick parser's, the archive is byte-identical to the host encoder's, the 64-bit checksums of
letters, record ends and qualities are those of the writer (integer work only).  No time is asserted."""
import os
import subprocess
import sys

import pytest

import text_parse_checks as tc
from conftest import ROOT
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = tc.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_fixture_texts_and_back(lib):
    for name in tc.FIXTURES:
        tc.check_fixture(lib, name, round_trip=True)


def test_hand_made_texts(lib):
    for case in tc.hand_made_cases():
        tc.check_hand_made(lib, *case)


def test_lines_longer_than_the_scan_span(lib):
    tc.check_lines_longer_than_the_scan_span(lib)


def test_crlf_and_lone_cr(lib):
    tc.check_crlf(lib)


def test_empty_text(lib):
    tc.check_empty(lib)


def test_unaligned_device_pointer(lib):
    tc.check_unaligned_pointer(lib)


def test_errors(lib):
    tc.check_errors(lib)


def test_host_path_unchanged(lib):
    tc.ec.check_host_path_unchanged(lib)


def test_synthetic_text_at_size(lib):
    """nafgpu_synth_write (256 Mbases, masked) -> decode_all_device -> format_device -> parse_text on d_text -> the writer's
    checksums; encode_device of the parse result, decoded again, gives them once more."""
    tc.check_synthetic_at_size(lib)


def test_fastq_text_at_size(lib):
    """2 000 040 FASTQ records from host text: encode_text, decode, format_device (= the input), parse_text, encode_device."""
    tc.check_fastq_at_size(lib)


def test_text_past_4_gib(lib):
    """2^32 + 200 000 003 letters as FASTA text in HBM, parsed where it lies; in a process of its own, under a time limit."""
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import text_parse_checks as tc\nfrom nafcodec_amd import _ffi\ntc.check_past_u32(tc.bind(_ffi.default()))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=900)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
