"""k_huf_flat (Huffman streams of a flat tree, decoded as a gather) on an MI355X (run with -m gpu): the checks of
tests/test_huf_flat_emu.py through libnafgpu.so (tests/huf_flat_checks.py holds them).

Bar: every decoded byte equals the CPU oracle's; malformed streams are refused as the oracle refuses them; a synthetic
archive of 8 M bases hashes the same with the kernel switched on and off.  No time is asserted."""
import pytest

import huf_flat_checks as hk
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = _ffi.default()                   # raises if libnafgpu.so is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_code_lengths(lib):
    hk.check_lengths(lib)


def test_sizes(lib):
    hk.check_sizes(lib)


def test_tree_reuse_mixing_and_sequences(lib):
    hk.check_mixing(lib)


def test_destination_alignment(lib):
    hk.check_fronts(lib)


def test_switch_off(lib):
    hk.check_switch_off(lib)


def test_refusals(lib):
    hk.check_refusals(lib)


def test_synthetic_archive(lib):
    hk.check_synthetic(lib)
