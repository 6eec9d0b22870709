"""Decoder.group, Selection.group, ParsedText.group and group() on an MI355X (run with -m gpu): the checks of
tests/test_group_emu.py through libnafgpu.so (tests/group_checks.py holds them), and positions past 2^32.

Bar: every table equals, as uint64 / uint8 arrays, a Python dict over the canonicalised bytes of what the CPU oracle decodes
or of the source's own bytes read back (integer work only, no tolerance).  No time is asserted."""
import pytest

import group_checks as gc
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = gc.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_fixtures(lib):
    gc.check_fixtures(lib)


def test_edges(lib):
    gc.check_edges(lib)


def test_random(lib):
    gc.check_random(lib, 2 ** 22)


def test_collisions():
    """hashes cut to 0, 1 and 4 bits (NAFGPU_GRP_HASH_BITS behind nafgpu_test_hooks): the same tables, and the rounds are reached;
    in a process of its own, since the hook is process-wide"""
    gc.bind(_ffi.default())
    gc.run_in_process(_ffi.DEFAULT_PATH, "check_collisions", timeout=300)


def test_composition(lib):
    gc.check_composition(lib)


def test_refusals(lib):
    gc.check_refusals(lib)


def test_past_4_gib():
    """2^26 synthetic letters against the dict; their record list selected 65 times (4.36 G letters: positions past 2^32): every
    record of copy c has the representative of its twin in copy 0, every group is 65 times as large, n_groups is unchanged; in
    a process of its own, under a time limit."""
    gc.bind(_ffi.default())
    gc.run_in_process(_ffi.DEFAULT_PATH, "check_past_u32", timeout=600)
