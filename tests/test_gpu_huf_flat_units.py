"""k_huf_flat's work unit on an MI355X (run with -m gpu): the checks of tests/test_huf_flat_units_emu.py through
libnafgpu.so (tests/huf_flat_unit_checks.py holds them).

Bar: every decoded byte equals the CPU oracle's, at every round boundary of a workgroup the format can reach, over more
than 520 units of two trees in one class, and with a class of another kind in between; a malformed stream in the middle is
refused as the oracle refuses it, with the kernel switched on and off.  No time is asserted."""
import pytest

import huf_flat_unit_checks as uk
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = _ffi.default()                   # raises if libnafgpu.so is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_round_boundaries_ascii(lib):
    uk.check_rounds(lib, "ascii")


def test_round_boundaries_bytes(lib):
    uk.check_rounds(lib, "bytes")


def test_many_units(lib):
    uk.check_many(lib)


def test_refusal_in_the_middle(lib):
    uk.check_refusal_in_the_middle(lib)
