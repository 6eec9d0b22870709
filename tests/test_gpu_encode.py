"""The device encoder on an MI355X (run with -m gpu): the identity checks of tests/test_encode_emu.py through libnafgpu.so
(tests/encode_checks.py holds them), and round trips that never leave HBM between decode and encode.

Bar: byte-identical to the host encoder (integer / bit work only)."""
import ctypes
import io

import pytest

import encode_checks as ec
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = ec.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_section_bytes_equal_the_host_encoder(lib):
    for name, data, expect in ec.section_inputs():
        ec.check_section(lib, name, data, expect)


def test_archives_equal_the_host_encoder(lib):
    for case in ec.archive_cases():
        ec.check_archive(lib, *case)


def test_errors(lib):
    ec.check_errors(lib)


def test_host_path_writes_what_the_parent_commit_wrote(lib):
    ec.check_host_path_unchanged(lib)


def test_slab_loop(lib, monkeypatch):
    ec.check_slabs(lib, monkeypatch)


def test_synthetic_archive_device_to_device(lib):
    """nafgpu_synth_write (256 Mbases, a few IUPAC codes, no mask) -> decode_all_device -> nafgpu_encode_device level 1 ->
    nafgpu_open_bytes -> decode_all_device: sequence and record table hash to the synthetic archive's own checksums."""
    arc = lib.synth(256_000_000, seed=11, with_mask=False, iupac_permille=5)
    try:
        blob = ctypes.string_at(arc.bytes, arc.n)
        dec = Decoder(io.BytesIO(blob))
        res = dec.decode_all_device()
        assert (res.n_bases, res.n_records) == (arc.n_bases, arc.n_records)
        again = encode_device(res, sequence_type="dna", id=bool(res.n_ids), sequence=True, compression_level=1, device=0)
        dec.close()
        del blob
        dec2 = Decoder(io.BytesIO(again))
        res2 = dec2.decode_all_device()
        assert (res2.n_bases, res2.n_records) == (arc.n_bases, arc.n_records)
        assert dec2.hash_device(res2.d_sequence, res2.n_bases) == arc.seq_hash
        assert dec2.hash_device(res2.d_record_end, 8 * res2.n_records) == arc.offsets_hash
        dec2.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))


def test_fastq_device_to_device(lib):
    """phix with its qualities: decode (mask off: no Mask section is written) -> encode_device -> decode: the same buffers."""
    from conftest import golden_bytes
    dec = Decoder(io.BytesIO(golden_bytes("phix.naf")), mask=False)
    res = dec.decode_all_device()
    want = [dec.copy_to_host(p, n) for p, n in ((res.d_sequence, res.n_bases), (res.d_quality, res.n_quality), (res.d_record_end, 8 * res.n_records),
                                                (res.d_ids, res.n_ids_bytes), (res.d_comments, res.n_comments_bytes))]
    again = encode_device(res, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, compression_level=1, device=0)
    dec.close()
    dec2 = Decoder(io.BytesIO(again))
    res2 = dec2.decode_all_device()
    got = [dec2.copy_to_host(p, n) for p, n in ((res2.d_sequence, res2.n_bases), (res2.d_quality, res2.n_quality), (res2.d_record_end, 8 * res2.n_records),
                                                (res2.d_ids, res2.n_ids_bytes), (res2.d_comments, res2.n_comments_bytes))]
    assert got == want and res2.n_records == res.n_records
    dec2.close()
