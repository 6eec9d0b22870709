"""The device encoder and the decoder's mask passes past 2^32 letters on an MI355X (run with -m gpu): the checks of
tests/test_beyond_u32_emu.py through libnafgpu.so with the boundary B = 2^32 (tests/beyond_u32_checks.py holds them), at
product defaults -- no hook, the real 512 MiB slab.

n = 2^32 + 200 000 003 letters (odd): 2.25 GB packed, five slabs, and fewer than 2^32 BYTES, so that the oracle's own zstd
decoder is not taken past 2^32 output bytes, where nobody has tested it; the one section of more than 2^32 bytes (B3) is read
back by the system libzstd, streaming.

Bar: equality of bytes, counts and 64-bit checksums against the CPU oracle, the system libzstd and the run / length-word
rules; byte identity with the host encoder where it is asked at size (B4).  No time is asserted.

Wall times on an MI355X host, one run (the oracle drains 4.5 Gbases in about 12 s on one core there, two at a time where they
are independent): the synthetic archive 15.6 s (synthesis, one drain, decode), device to device 15.5 s, the text section
5.6 s, hand-made records and mask 21.7 / 18.3 / 18.4 s, the section with matches 40.3 s (2.25 GB through libzstd at level 1,
four drains), the slab boundary 3.0 s: 139 s for the module, against 14.7 s for
test_both_ends_of_the_full_size_archive_against_the_oracle in the same session.  That is more than twice that test, so the
second device decode of the device-to-device test is left to the hand-made cases, which decode what they encoded anyway;
n stays.  k_mask_apply on the unit of 2^32 + 12 345 letters (one workgroup sweeps a whole run): 969 ms of mask and scan
passes, against 0.9 ms for the short units."""
import numpy as np
import pytest

import beyond_u32_checks as bc
import zstd_ref
from nafcodec_amd import _ffi

pytestmark = pytest.mark.gpu

B, EXTRA = 2**32, 200_000_003
needs_libzstd = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable (tests/naf_writer.py writes the comparison archives with it)")


@pytest.fixture(scope="module")
def lib():
    L = bc.ec.bind(_ffi.default())       # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


@pytest.fixture(scope="module")
def synthetic(lib):
    s = bc.Synthetic(lib, B, EXTRA)
    yield s
    s.close()


def test_the_helpers_on_the_real_numbers():
    bc.check_helpers()


def test_synthetic_archive_device_to_device(synthetic):
    """B1: synth (masked, IUPAC) -> decode_all_device -> encode_device(mask=True) -> the oracle and the device read the new
    archive as the old one; 17 147 literal-only blocks, none treeless at the head of a 64-block chunk; the Mask section is the
    original's units without the writer's zero-length fillers."""
    assert bc.check_device_to_device(synthetic, redecode=False) == 17147


@needs_libzstd
def test_text_section_beyond_4_gib(synthetic):
    """B3: the same letters as a text section of 4.5 GB: nine slabs, section offsets beyond 2^32; libzstd reads it back."""
    bc.check_text_section(synthetic, 9)


@pytest.mark.parametrize("name", ["long_unit", "edges", "first_lower_past_B"])
def test_hand_made_records_and_mask(lib, name):
    """B2: records [0xFFFFFFFF, 0, rest] (or one record of n) and hand-made units: one longer than 2^32; edges at B - 1, B,
    B + 1 and every offset modulo 16 around B and B +- 4096; the first lower-case letter at B + 5 ("letter 4294967301)")."""
    bc.check_hand_made(lib, B, EXTRA, name)


@needs_libzstd
def test_hand_made_mask_over_a_section_with_matches(lib):
    """B2-lz: the same masks through k_mask_apply (a section with LZ sequences), both readings of the record-end rule."""
    times = bc.check_lz_decode(lib, B, EXTRA)
    print("mask and scan passes, ms:", times)
    assert len(times) == 4


def test_the_slab_boundary_byte_for_byte(lib):
    """B4: 512 MiB + 2 * 128 KiB + 5 bytes at default settings: the device frame is the host encoder's frame."""
    rng = np.random.default_rng(512)
    data = bc.ec.letters(rng, b"ACGTN", (512 << 20) + 2 * bc.ec.BLOCK + 5)
    heads = lambda t: [i for i, k in enumerate(t) if i % 64 == 0 and k != "huf"]
    bc.ec.check_section(lib, "slab_boundary", data, lambda t: len(t) == 4099 and not heads(t[:4098]) and t[4096] == "huf" and t[-1] == "raw")
