"""Shared by tests/test_encode_emu.py (CPU harness) and tests/test_gpu_encode.py (MI355X): the device encoder's bytes
against the host encoder's.  Not a test module; every function takes the library binding it is to check."""
import ctypes
import hashlib
import io

import numpy as np

import cases
import zstd_ref
from conftest import golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Encoder, Record, encode_device
from oracle import oracle

BLOCK = 128 << 10
# bound unconditionally: a library without the feature fails here, it does not skip
ENTRY_POINTS = ("nafgpu_zstd_compress", "nafgpu_encoder_set_device", "nafgpu_encode_device", "nafgpu_encode_free")


def bind(lib):
    for name in ENTRY_POINTS:
        getattr(lib.c, name)
    return lib


# ---------------------------------------------------------------- the container, as tests/naf_writer.py lays it out
def read_varint(blob, at):
    v = 0
    while True:
        b = blob[at]
        at += 1
        v = (v << 7) | (b & 0x7F)
        if not b & 0x80:
            return v, at


def sections(blob):
    """-> {name: (original_size, payload)} of an archive (header per naf_writer.write_naf)"""
    assert blob[:3] == b"\x01\xF9\xEC"
    if blob[3] == 1:
        flags, at = blob[4], 6
    else:
        flags, at = blob[5], 7
    _, at = read_varint(blob, at)                   # line length
    _, at = read_varint(blob, at)                   # number of sequences
    out = {}
    for name, bit in (("ids", 0x20), ("comments", 0x10), ("lengths", 0x08), ("mask", 0x04), ("sequence", 0x02), ("quality", 0x01)):
        if flags & bit:
            orig, at = read_varint(blob, at)
            comp, at = read_varint(blob, at)
            out[name] = (orig, blob[at:at + comp])
            at += comp
    assert at == len(blob)
    return out


def section_spans(blob):
    """-> {name: (original_size, first byte, end) of the payload} without copying a payload (`blob`: bytes or a memoryview
    over an archive of any size); "n_records" and "flags" beside them"""
    assert bytes(blob[:3]) == b"\x01\xF9\xEC"
    if blob[3] == 1:
        flags, at = blob[4], 6
    else:
        flags, at = blob[5], 7
    _, at = read_varint(blob, at)
    out = {"flags": flags}
    out["n_records"], at = read_varint(blob, at)
    for name, bit in (("ids", 0x20), ("comments", 0x10), ("lengths", 0x08), ("mask", 0x04), ("sequence", 0x02), ("quality", 0x01)):
        if flags & bit:
            orig, at = read_varint(blob, at)
            comp, at = read_varint(blob, at)
            out[name] = (orig, at, at + comp)
            at += comp
    assert at == len(blob)
    return out


def host_archive(lib, records, sequence_type, level, device=None, **fields):
    buf = io.BytesIO()
    with Encoder(buf, sequence_type, compression_level=level, device=device, _lib=lib, **fields) as enc:
        for r in records:
            enc.write(r if isinstance(r, Record) else Record(**r))
    return buf.getvalue()


def host_frame(lib, data):
    """the section payload the host encoder writes for `data`: a text archive with only the sequence, level 1"""
    blob = host_archive(lib, [Record(sequence=data)], "text", 1, sequence=True)
    orig, payload = sections(blob)["sequence"]
    assert orig == len(data)
    return payload


def block_types(frame):
    """block by block: 'raw', 'rle', 'huf' (Huffman with a new tree), 'treeless'; anything else fails"""
    assert bytes(frame[:2]) == b"\x00\x48"                 # (`frame`: bytes or a memoryview)
    at, out = 2, []
    while True:
        bh = frame[at] | (frame[at + 1] << 8) | (frame[at + 2] << 16)
        at += 3
        last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
        if kind == 0:
            out.append("raw")
            at += size
        elif kind == 1:
            out.append("rle")
            at += 1
        else:
            assert kind == 2
            lit = frame[at] & 3
            assert lit in (2, 3), "literals neither Huffman nor treeless"
            out.append("huf" if lit == 2 else "treeless")
            assert frame[at + size - 1] == 0            # no sequences
            at += size
        if last:
            assert at == len(frame)
            return out


def letters(rng, alphabet, n):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def golden_sequence_ascii(name):
    return "".join(r.sequence for r in oracle.Decoder(golden_bytes(name + ".naf"), mask=False)).encode()


def pack(ascii_bytes):
    import naf_writer as nw
    lut = np.zeros(256, dtype=np.uint8)
    for c, v in nw.CODE.items():
        lut[ord(c)] = v
    codes = lut[np.frombuffer(ascii_bytes, dtype=np.uint8)]
    if len(codes) & 1:
        codes = np.append(codes, np.uint8(0))
    return bytes(codes[0::2] | (codes[1::2] << 4))


def section_inputs(multi_chunk=True):
    """(name, data, expected block types or a predicate over them): every branch of plan_block, taken by the host path itself"""
    rng = np.random.default_rng(20240607)
    out = [
        ("empty", b"", ["raw"]),
        ("one_byte", b"A", ["raw"]),
        ("63_bytes", letters(rng, b"ACGT", 63), ["raw"]),
        ("64_bytes", letters(rng, b"ACGT", 64), ["huf"]),
        ("block_minus_1", letters(rng, b"ACGTN", BLOCK - 1), ["huf"]),
        ("block", letters(rng, b"ACGTN", BLOCK), ["huf"]),
        ("block_plus_1", letters(rng, b"ACGTN", BLOCK + 1), ["huf", "raw"]),
        ("one_value", b"G" * (3 * BLOCK + 5), ["rle", "rle", "rle", "raw"]),
        ("all_values_equally_often", bytes(rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 2 * BLOCK // 256))), ["raw", "raw"]),
        ("random_1_255", bytes(rng.integers(1, 256, 2 * BLOCK, dtype=np.uint8)), ["huf", "treeless"]),
        ("two_alphabets", letters(rng, b"AC", 2 * BLOCK) + letters(rng, b"ACGT", 2 * BLOCK), ["huf", "treeless", "huf", "treeless"]),
    ]
    skew = rng.geometric(0.03, 3 * BLOCK // 2)
    skewed = (255 - np.minimum(skew - 1, 199)).astype(np.uint8)            # 200 byte values, 0xFF the commonest
    assert len(set(skewed.tolist())) == 200 and skewed.max() == 0xFF
    out.append(("200_values_skewed", bytes(skewed), lambda t: t[0] == "huf" and set(t) <= {"huf", "treeless"}))
    ascii_ = golden_sequence_ascii("NZ_AAEN01000029")
    out.append(("genome_packed", pack(ascii_), lambda t: (t.count("huf"), t.count("treeless"), len(t)) == (15, 6, 21)))
    out.append(("genome_ascii", ascii_, lambda t: (t.count("huf"), t.count("treeless"), len(t)) == (19, 23, 42)))
    phix = oracle.Decoder(golden_bytes("phix.naf"))
    out.append(("phix_quality", phix.section(5)[0], lambda t: "huf" in t))
    out.append(("phix_ids", phix.section(0)[0], lambda t: "huf" in t))
    if multi_chunk:
        out.append(("64_blocks_plus_1", letters(rng, b"ACGT", 64 * BLOCK + 1), ["huf"] + ["treeless"] * 63 + ["raw"]))
        out.append(("129_blocks", letters(rng, b"ACGT", 129 * BLOCK),
                    lambda t: len(t) == 129 and [i for i, k in enumerate(t) if k == "huf"] == [0, 64, 128] and t.count("treeless") == 126))
    return out


def check_section(lib, name, data, expect):
    want = host_frame(lib, data)
    types_ = block_types(want)
    assert expect(types_) if callable(expect) else types_ == expect, (name, types_[:8], len(types_))
    got = lib.zstd_compress(data, 0)
    assert hashlib.sha256(got).digest() == hashlib.sha256(want).digest() and got == want, name
    assert zstd_ref.decompress_magicless(got, len(data) + 8) == data, name
    # a destination that is too small: refused, with the size that is needed
    if len(got) > 4:
        buf, produced, err = ctypes.create_string_buffer(4), ctypes.c_size_t(0), _ffi.Error()
        assert lib.c.nafgpu_zstd_compress(data, len(data), buf, 4, ctypes.byref(produced), 0, ctypes.byref(err)) == _ffi.E_INVALID_ARG
        assert produced.value == len(want)


# ---------------------------------------------------------------- archives
def archive_cases():
    """(name, archive bytes, sequence type, fields, oracle options).  phix has a few soft-masked letters too: like `masked`
    it is decoded with mask=False, the encoder writes no Mask section and refuses lower case."""
    dna = dict(id=True, comment=True, sequence=True)
    out = [("phix", golden_bytes("phix.naf"), "dna", dict(dna, quality=True), {"mask": False}),
           ("CP040672", golden_bytes("CP040672.naf"), "dna", dna, {}),
           ("NZ_AAEN01000029", golden_bytes("NZ_AAEN01000029.naf"), "dna", dna, {}),
           ("LuxC", golden_bytes("LuxC.naf"), "protein", dna, {}),
           ("masked", golden_bytes("masked.naf"), "dna", dna, {"mask": False})]
    rna = next(blob for name, blob, _ in cases.build_cases(scale=1) if name == "rna_l3")
    out.append(("rna_l3", rna, "rna", dna, {}))
    return out


def records_of(blob, **opts):
    return [Record(id=r.id, comment=r.comment, sequence=r.sequence, quality=r.quality, length=r.length) for r in oracle.Decoder(blob, **opts)]


def as_tuples(records):
    return [(r.id, r.comment, r.sequence, r.quality, r.length) for r in records]


def check_archive(lib, name, blob, sequence_type, fields, opts):
    recs = records_of(blob, **opts)
    for r in recs:                                   # only what the archive is to hold
        for f in ("id", "comment", "sequence", "quality"):
            if not fields.get(f):
                setattr(r, f, None)
    for level in (1, 2):
        want = host_archive(lib, recs, sequence_type, level, **fields)
        assert host_archive(lib, recs, sequence_type, level, device=0, **fields) == want, (name, level, "Encoder(device=0)")
        # the records in HBM: the host archive decoded in bulk (mask: none is written)
        dec = Decoder(io.BytesIO(want), _lib=lib)
        res = dec.decode_all_device()
        got = encode_device(res, sequence_type=sequence_type, compression_level=level, device=0, _lib=lib, **fields)
        assert got == want, (name, level, "encode_device")
        dec.close()
    assert as_tuples(oracle.Decoder(want)) == as_tuples(recs), name


def device_text(lib, data):
    """`data` in device memory: a text archive decoded in bulk -> (decoder to keep alive, result)"""
    dec = Decoder(io.BytesIO(host_archive(lib, [Record(sequence=data)], "text", 1, sequence=True)), _lib=lib)
    res = dec.decode_all_device()
    assert res.n_bases == len(data) and res.n_records == 1
    return dec, res


def call_encode_device(lib, src, sequence_type, level=1, **fields):
    """the C entry point itself -> (status, archive bytes or None)"""
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(("dna", "rna", "protein", "text").index(sequence_type), ctypes.byref(opts))
    opts.id, opts.comment, opts.sequence, opts.quality = (int(bool(fields.get(f))) for f in ("id", "comment", "sequence", "quality"))
    opts.compression_level = level
    p, n, err = ctypes.c_void_p(), ctypes.c_uint64(), _ffi.Error()
    rc = lib.c.nafgpu_encode_device(ctypes.byref(src), ctypes.byref(opts), 0, ctypes.byref(p), ctypes.byref(n), ctypes.byref(err))
    call_encode_device.message = err.message.decode("utf-8", "replace")
    if rc != _ffi.OK:
        assert not p.value and n.value == 0 and err.status == rc
        return rc, None
    try:
        return rc, ctypes.string_at(p, n.value)
    finally:
        lib.c.nafgpu_encode_free(p)


def check_errors(lib):
    rng = np.random.default_rng(5)
    good = letters(rng, b"ACGTN", 1 << 20)
    for bad_letter, stype in ((b"a", "dna"), (b"X", "dna"), (b"U", "dna"), (b"T", "rna")):
        at = (1 << 19) + 12345
        data = good[:at] + bad_letter + good[at + 1:]
        if stype == "rna":
            data = data.replace(b"T", b"U")[:at] + b"T" + data.replace(b"T", b"U")[at + 1:]
        dec, res = device_text(lib, data)
        src = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=1)
        rc, blob = call_encode_device(lib, src, stype, sequence=True)
        assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None), (bad_letter, stype, rc)
        assert "letter %d)" % at in call_encode_device.message, call_encode_device.message      # the first offender is named
        dec.close()
    dec, res = device_text(lib, good)                                       # the same letters without the offender: accepted
    src = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=1)
    rc, blob = call_encode_device(lib, src, "dna", sequence=True)
    assert rc == _ffi.OK and blob == host_archive(lib, [Record(sequence=good.decode())], "dna", 1, sequence=True)
    # quality shorter than the sequence; a record table that ends elsewhere; fields and options that disagree; level 0 and 3
    src_q = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_quality=res.d_sequence, n_quality=res.n_bases - 1,
                              d_record_end=res.d_record_end, n_records=1)
    assert call_encode_device(lib, src_q, "dna", sequence=True, quality=True)[0] == _ffi.E_INVALID_LENGTH
    src_short = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases - 2, d_record_end=res.d_record_end, n_records=1)
    assert call_encode_device(lib, src_short, "dna", sequence=True)[0] == _ffi.E_INVALID_LENGTH
    assert call_encode_device(lib, src, "dna", sequence=True, quality=True)[0] == _ffi.E_INVALID_ARG
    assert call_encode_device(lib, src, "dna", level=0, sequence=True)[0] == _ffi.E_INVALID_ARG
    assert call_encode_device(lib, src, "dna", level=3, sequence=True)[0] == _ffi.E_INVALID_ARG
    # ids that are not one string per record
    src_ids = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=1,
                                d_ids=res.d_sequence, n_ids_bytes=100)
    assert call_encode_device(lib, src_ids, "dna", id=True, sequence=True)[0] == _ffi.E_MISSING_FIELD
    dec.close()
    for level, want in ((0, _ffi.E_INVALID_ARG), (3, _ffi.E_INVALID_ARG), (1, _ffi.OK), (2, _ffi.OK)):
        opts, h, err = _ffi.EncoderOpts(), ctypes.c_void_p(), _ffi.Error()
        lib.c.nafgpu_encoder_opts_default(0, ctypes.byref(opts))
        opts.sequence, opts.compression_level = 1, level
        assert lib.c.nafgpu_encoder_new(ctypes.byref(opts), ctypes.byref(h), ctypes.byref(err)) == _ffi.OK
        assert lib.c.nafgpu_encoder_set_device(h, 0) == want, level
        lib.c.nafgpu_encoder_free(h)


# what the parent commit's host encoder wrote for forty times the two records of tests/test_encoder.py (every field, DNA)
PARENT_SHA256 = {0: "df4f568a79e34a746f530c239122bd35b338a44eed809fd3732515814ca9f562",
                 1: "94ad51c736c4e71c8fc8a572f7b529e16034469f61f445bfef3a301c07155a2c"}


def check_host_path_unchanged(lib):
    r1 = dict(id="r1", comment="record 1", sequence="NGCTCTTAAACCTGCTA", quality="#8CCCGGGGGGGGGGGG", length=17)
    r2 = dict(id="r2", comment="record 2", sequence="NTAATAAGCAATGACGGCAGC", quality="#8AACCFF<FFGGFGE@@@@@", length=21)
    for level, want in PARENT_SHA256.items():
        blob = host_archive(lib, [r1, r2] * 40, "dna", level, id=True, comment=True, sequence=True, quality=True)
        assert hashlib.sha256(blob).hexdigest() == want, level


def check_slabs(lib, monkeypatch):
    """2 slabs + 1 block with the slab lowered to 8 MiB: the slab loop gives the host frame"""
    rng = np.random.default_rng(77)
    data = letters(rng, b"ACGTN", 2 * (8 << 20) + BLOCK)
    want = host_frame(lib, data)
    monkeypatch.setenv("NAFGPU_ENC_SLAB_MIB", "8")
    lib.c.nafgpu_test_hooks(1)
    try:
        got = lib.zstd_compress(data, 0)
    finally:
        lib.c.nafgpu_test_hooks(0)
    assert got == want
    types_ = block_types(want)
    assert len(types_) == 129 and types_[0] == types_[64] == types_[128] == "huf"
