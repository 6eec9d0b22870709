"""Encoder(mask=True) and encode_device(mask=True) on an MI355X (run with -m gpu): the checks of
tests/test_mask_encode_emu.py through libnafgpu.so (tests/mask_encode_checks.py holds them), and round trips at size that
never leave HBM between decode and encode.

Bar: the Mask section is the run rule's bytes, and the device archive is byte-identical to the host encoder's (integer work only)."""
import ctypes
import io

import numpy as np
import pytest

import mask_encode_checks as mc
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device
from oracle import oracle

pytestmark = pytest.mark.gpu

N_AT_SIZE = 256_000_000


@pytest.fixture(scope="module")
def lib():
    L = mc.ec.bind(_ffi.default())       # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_fixture_mask_sections_are_reproduced(lib):
    mc.check_rule_helpers()
    for name in mc.FIXTURES:
        mc.check_fixture(lib, name)


def test_hand_made_letters(lib):
    for case in mc.hand_made_cases():
        mc.check_hand_made(lib, *case)


def test_masked_runs_and_record_ends(lib):
    mc.check_record_ends(lib)


def test_unaligned_device_pointer(lib):
    mc.check_unaligned_pointer(lib)


def test_errors(lib):
    mc.check_errors(lib)


def test_synthetic_masked_archive_device_to_device(lib):
    """nafgpu_synth_write (256 Mbases, soft-masked runs inside records) -> decode_all_device -> encode_device(mask=True, level 1)
    -> decode_all_device: sequence (lower-cased text) and record table hash to the synthetic archive's own checksums; the
    oracle reads the first and the last record of the new archive as the first decode gave them."""
    arc = lib.synth(N_AT_SIZE, seed=12, with_mask=True, iupac_permille=5)
    try:
        dec = Decoder(io.BytesIO(ctypes.string_at(arc.bytes, arc.n)))
        res = dec.decode_all_device()
        assert (res.n_bases, res.n_records) == (arc.n_bases, arc.n_records)
        ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
        last_at = int(ends[-2]) if len(ends) > 1 else 0
        first = dec.copy_to_host(res.d_sequence, int(ends[0]))
        last = dec.copy_to_host(res.d_sequence + last_at, int(ends[-1]) - last_at)
        again = encode_device(res, sequence_type="dna", id=bool(res.n_ids), sequence=True, compression_level=1, device=0, mask=True)
        dec.close()
        assert mc.flags_of(again) & 0x04
        dec2 = Decoder(io.BytesIO(again))
        res2 = dec2.decode_all_device()
        assert (res2.n_bases, res2.n_records) == (arc.n_bases, arc.n_records)
        assert dec2.hash_device(res2.d_sequence, res2.n_bases) == arc.seq_hash
        assert dec2.hash_device(res2.d_record_end, 8 * res2.n_records) == arc.offsets_hash
        dec2.close()
        seen = None
        for k, r in enumerate(oracle.Decoder(again, raw=True)):
            if k == 0:
                assert r.sequence == first and any(97 <= c <= 122 for c in first + last)
            seen = r.sequence
        assert k + 1 == arc.n_records and seen == last
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))


def test_one_unit_at_size(lib):
    """256 Mbases without a lower-case letter: one unit, n // 255 bytes FF and one byte n % 255 -- the case a loop over a
    unit's length would serialise."""
    arc = lib.synth(N_AT_SIZE, seed=13, with_mask=False)
    try:
        dec = Decoder(io.BytesIO(ctypes.string_at(arc.bytes, arc.n)))
        res = dec.decode_all_device()
        n = res.n_bases
        assert n == N_AT_SIZE
        again = encode_device(res, sequence_type="dna", id=bool(res.n_ids), sequence=True, compression_level=1, device=0, mask=True)
        dec.close()
        orig, payload = mc.ec.sections(again)["mask"]
        assert orig == n // 255 + 1
        got = oracle.zstd_decode(payload, orig + 8)
        assert got == b"\xff" * (n // 255) + bytes([n % 255])
        dec2 = Decoder(io.BytesIO(again))
        res2 = dec2.decode_all_device()
        assert dec2.hash_device(res2.d_sequence, res2.n_bases) == arc.seq_hash
        assert dec2.hash_device(res2.d_record_end, 8 * res2.n_records) == arc.offsets_hash
        dec2.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))
