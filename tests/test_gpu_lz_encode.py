"""Blocks with LZ sequences from the device encoder on an MI355X (run with -m gpu): the checks of tests/test_lz_encode_emu.py
through libnafgpu.so (tests/lz_encode_checks.py holds them) -- the sizes and hashes pinned there were taken on the CPU harness,
so the frames are the same bytes here -- and two round trips at size.

Bar: integer / bit work only; the frames are byte-identical to the harness's, and every reader gives the input back."""
import io

import pytest

import lz_encode_checks as lc
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = lc.bind(_ffi.default())          # raises if libnafgpu.so or an entry point is missing: nothing here skips
    name, hbm, cus = L.device_info(0)
    assert "gfx950" in name, name
    return L


def test_sections(lib):
    for name, data, check in lc.section_inputs():
        lc.check_section(lib, name, data, check)


def test_size_is_nearer_the_host_lz_frame_than_the_literal_only_frame(lib):
    for name, data in lc.size_inputs():
        lc.check_size(lib, name, data)


def test_nothing_to_find_gives_the_level_1_frame(lib):
    lc.check_no_repeat(lib)


def test_chunk_border(lib):
    lc.check_chunk_border(lib)


def test_slab_loop(lib, monkeypatch):
    lc.check_slabs(lib, monkeypatch)


def test_device_pointer_at_every_offset(lib):
    lc.check_device_pointer(lib)


def test_archives(lib):
    for case in lc.archive_cases():
        lc.check_archive(lib, *case)


def test_text_archives(lib):
    for name in sorted(lc.tc.FIXTURES):
        lc.check_text_archive(lib, name)


def test_refused_without_the_flag(lib):
    lc.check_refused_without_the_flag(lib)


def test_64_mib_of_ids_round_trip(lib):
    """64 MiB of SRR-like ids -> zstd_compress(lz=True) -> nafgpu_zstd_decompress, compared by hash64."""
    ids = lc.srr_ids(3_600_000)[:64 << 20]
    assert len(ids) == 64 << 20
    frame = lib.zstd_compress(ids, 0, True)
    assert len(frame) < len(ids) // 3
    back = lib.zstd_decompress(frame, len(ids), 0)
    assert len(back) == len(ids) and lc.hash64(lib, back) == lc.hash64(lib, ids)


def test_fastq_text_to_archive_to_device(lib):
    """200 000 generated FASTQ records -> format_device -> encode_text(device_lz=True, level 0) -> decode_all_device: the five
    buffers hash to those of the first decode."""
    import numpy as np
    rng = np.random.default_rng(2024)
    n, width = 200_000, 151
    seq = np.frombuffer(lc.ec.letters(rng, b"ACGT", n * width), dtype=np.uint8).reshape(n, width)
    qual = rng.choice(np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8), (n, width))
    lf = np.full((n, 1), 10, dtype=np.uint8)
    body = np.concatenate([seq, lf, np.full((n, 1), ord("+"), dtype=np.uint8), lf, qual, lf], axis=1)
    generated = b"".join(b"@SRR1770413.%d %d length=%d\n" % (i + 1, i + 1, width) + body[i].tobytes() for i in range(n))
    first = encode_text(generated, compression_level=1, device=0, _lib=lib)

    def buffers(dec, res):
        return [dec.hash_device(p, m) for p, m in ((res.d_sequence, res.n_bases), (res.d_quality, res.n_quality), (res.d_record_end, 8 * res.n_records),
                                                   (res.d_ids, res.n_ids_bytes), (res.d_comments, res.n_comments_bytes))]
    dec = Decoder(io.BytesIO(first), _lib=lib)
    res = dec.decode_all_device()
    want = buffers(dec, res)
    text = dec.to_text()                                    # format_device, copied to the host: encode_text takes host text
    assert text == generated
    dec.close()
    archive = encode_text(text, compression_level=0, device=0, device_lz=True, _lib=lib)
    assert len(archive) < len(first)
    dec2 = Decoder(io.BytesIO(archive), _lib=lib)
    res2 = dec2.decode_all_device()
    assert res2.n_records == n and buffers(dec2, res2) == want
    dec2.close()
