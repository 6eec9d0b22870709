"""The checks of tests/test_gpu_beyond_u32.py on the CPU harness (libnafgpu_emu.so) with a boundary of 2^20 letters instead of
2^32: what is proven here is the test logic -- window cuts, run arithmetic, re-framing, expected words -- before it meets a
GPU.  A 32-bit truncation cannot show at this size; that question is the GPU run's (tests/beyond_u32_checks.py)."""
import os
import subprocess

import pytest

import beyond_u32_checks as bc
import cases
import zstd_ref
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")
B, EXTRA = 2**20, 300_003
needs_libzstd = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable (tests/naf_writer.py writes the comparison archives with it)")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return bc.ec.bind(_ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so")))


def test_the_helpers_on_the_real_numbers():
    """length words of a record of exactly 0xFFFFFFFF letters, the bytes of a unit longer than 2^32, the window cut, the merge
    of zero-length units, the hand-made variants at B = 2^32: computed for the real sizes, no archive needed"""
    bc.check_helpers()


def test_synthetic_masked_runs_stay_inside_records(emu):
    """the premise of reading the full-size masked archive with the default rule (40 Mbases, host code only)"""
    assert cases.check_synth_mask_premise(emu, 40_000_000, 0x4E4146) > 4000


@pytest.mark.parametrize("n_blk", [2, 4])
def test_both_ends_of_a_masked_archive(emu, n_blk):
    """A: cases.check_archive_ends(with_mask=True) on 3.3 Mbases, windows of 2 and 4 blocks; and without a mask, as before"""
    lower = cases.check_archive_ends(emu, 3_300_001, 5, n_blk, with_mask=True)
    assert min(lower) > 0
    if n_blk == 2:
        assert cases.check_archive_ends(emu, 3_300_001, 5, n_blk) == (0, 0)


@pytest.fixture(scope="module")
def synthetic(emu):
    s = bc.Synthetic(emu, B, EXTRA)
    yield s
    s.close()


def test_synthetic_archive_device_to_device(synthetic):
    """B1 at B = 2^20"""
    assert bc.check_device_to_device(synthetic) == 6


@pytest.mark.parametrize("name", ["long_unit", "edges", "first_lower_past_B"])
def test_hand_made_records_and_mask(emu, name):
    """B2 at B = 2^20"""
    bc.check_hand_made(emu, B, EXTRA, name)


@needs_libzstd
def test_hand_made_mask_over_a_section_with_matches(emu):
    """B2-lz at B = 2^20: a quarter of the fixture, once"""
    times = bc.check_lz_decode(emu, B, EXTRA, period_div=4)
    assert sorted(times) == [("edges", False), ("edges", True), ("long_unit", False), ("long_unit", True)]


@needs_libzstd
def test_text_section_of_three_slabs(emu, monkeypatch):
    """B3 with the slab lowered to 8 MiB: 16.3 M letters as text are three slabs"""
    monkeypatch.setenv("NAFGPU_ENC_SLAB_MIB", "8")
    s = bc.Synthetic(emu, 2**24, EXTRA)
    emu.c.nafgpu_test_hooks(1)
    try:
        bc.check_text_section(s, 3, slab=8 << 20)
    finally:
        emu.c.nafgpu_test_hooks(0)
        s.close()
