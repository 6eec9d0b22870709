"""Shared by tests/test_mask_encode_emu.py (CPU harness) and tests/test_gpu_mask_encode.py (MI355X): the Mask section both
encoders write with mask=True.  Not a test module; every function takes the library binding it is to check.

The yardstick is the format as the reference's decoder reads it (reader.rs:198-231, the CPU oracle here) and the reference's
own fixtures, which `ennaf` wrote: the Mask section written for a fixture's text must decode to the fixture's Mask bytes."""
import ctypes
import io
import os

import numpy as np

import encode_checks as ec
import naf_writer as nw
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Encoder, Record, encode_device
from oracle import oracle

# fixture: (letters, units of its Mask section, bytes of its Mask section)
# nafcodec_amd/csrc/encode.h (kEncMaskTile) and encode.hip (16 letters per lane): asserted against the source below
MASK_TILE, LANE_LETTERS = 4096, 16
FIXTURES = {"masked": (3350, 11, 20), "phix": (12436, 5, 53), "CP040672": (89094, 1, 350), "NZ_AAEN01000029": (5488676, 1, 21525)}
DNA = dict(id=True, comment=True, sequence=True)


def mask_bytes(text):
    """the run rule over the concatenated letters (bytes): the specification of the feature"""
    out, i, n, masked = bytearray(), 0, len(text), False
    while i < n:
        j = i
        while j < n and (97 <= text[j] <= 122) == masked:
            j += 1
        l = j - i
        out += b"\xff" * (l // 255) + bytes([l % 255])
        i, masked = j, not masked
    return bytes(out)


def mask_bytes_np(text):
    """the same rule without a Python loop per letter (checked against mask_bytes in check_rule_helpers)"""
    a = np.frombuffer(text, dtype=np.uint8)
    if not len(a):
        return b""
    m = (a >= 97) & (a <= 122)
    edges = np.flatnonzero(m != np.concatenate(([False], m[:-1])))
    lens = np.diff(np.concatenate(([0], edges, [len(a)])))
    out = bytearray()
    for l in lens.tolist():
        out += b"\xff" * (l // 255) + bytes([l % 255])
    return bytes(out)


def check_rule_helpers():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 1000):
        t = bytes(rng.choice(np.frombuffer(b"ACGTacgt-", dtype=np.uint8), n))
        assert mask_bytes_np(t) == mask_bytes(t)
        if n:                                               # tests/naf_writer.py has the rule too (it differs for no letters only)
            assert nw.mask_bytes(nw.runs_from_case(t.decode())) == mask_bytes(t)
    assert mask_bytes(b"A" * 255) == b"\xff\x00" and mask_bytes(b"a") == b"\x00\x01" and mask_bytes(b"") == b""


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "encode.h")) as f:
        assert "constexpr uint32_t kEncMaskTile = %d;" % MASK_TILE in f.read()
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "encode.hip")) as f:
        assert "static_assert(kEncMaskTile == kMaskThreads * %d" % LANE_LETTERS in f.read()


def flags_of(blob):
    return blob[4] if blob[3] == 1 else blob[5]


def mask_section(blob):
    return oracle.Decoder(blob).section(3)[0]


def text_of(records):
    return "".join(r.sequence or "" for r in records).encode()


def split(text, lengths):
    assert sum(lengths) == len(text)
    out, at = [], 0
    for i, l in enumerate(lengths):
        out.append(Record(id="r%d" % i, comment="c", sequence=text[at:at + l].decode(), length=l))
        at += l
    return out


def device_archive(lib, host_blob, sequence_type, level, fields):
    """encode_device over the records as decode_all_device() leaves them (lower-case runs included)"""
    dec = Decoder(io.BytesIO(host_blob), spec_mask=True, _lib=lib)
    try:
        res = dec.decode_all_device()
        return encode_device(res, sequence_type=sequence_type, compression_level=level, device=0, mask=True, _lib=lib, **fields)
    finally:
        dec.close()


def check_records(lib, name, records, sequence_type="dna", fields=DNA, host_levels=(0, 1, 3), want_mask=None):
    """host Encoder(mask=True) at host_levels; Encoder(device=0) and encode_device at 1 and 2: the container, the Mask
    section against the run rule (and `want_mask`), the oracle's reading, device == host.  -> the level-1 archive"""
    text = text_of(records)
    rule = mask_bytes_np(text)
    if want_mask is not None:
        assert rule == want_mask, name
    want = ec.as_tuples(records)
    archives = {}
    for level in sorted(set(host_levels) | {1, 2}):
        blob = ec.host_archive(lib, records, sequence_type, level, mask=True, **fields)
        archives[level] = blob
        assert flags_of(blob) & 0x04, name
        expected = [s for s, f in (("ids", "id"), ("comments", "comment"), ("lengths", None), ("mask", None), ("sequence", "sequence"),
                                   ("quality", "quality")) if f is None or fields.get(f)]
        assert list(ec.sections(blob)) == expected, (name, level)
        orig, _ = ec.sections(blob)["mask"]
        got = mask_section(blob) if rule else (oracle.Decoder(blob).section(3) or (b"",))[0]
        assert orig == len(rule) and got == rule, (name, level, len(got), len(rule))
        assert ec.as_tuples(oracle.Decoder(blob, spec_mask=True)) == want, (name, level, "spec_mask")
    for level in (1, 2):
        assert ec.host_archive(lib, records, sequence_type, level, mask=True, device=0, **fields) == archives[level], (name, level, "Encoder(device=0)")
        assert device_archive(lib, archives[level], sequence_type, level, fields) == archives[level], (name, level, "encode_device")
    return archives[1]


# ---------------------------------------------------------------- 1. pinned on the fixtures
def check_fixture(lib, name):
    letters, units, n_mask = FIXTURES[name]
    blob = golden_bytes(name + ".naf")
    fields = dict(DNA, quality=(name == "phix"))
    recs = ec.records_of(blob, spec_mask=True)
    fixture_mask = mask_section(blob)
    assert (len(text_of(recs)), sum(b != 0xFF for b in fixture_mask), len(fixture_mask)) == (letters, units, n_mask)
    new = check_records(lib, name, recs, "dna", fields, want_mask=fixture_mask)
    # the fixtures have no masked run that touches a record's end: the reference's default reading is the same text
    assert ec.as_tuples(oracle.Decoder(new)) == ec.as_tuples(recs) == ec.as_tuples(oracle.Decoder(blob)), name
    if name == "masked":
        with open(os.path.join(ROOT, "tests", "golden", "masked.fna"), "rb") as f:
            fasta = b"".join(l.strip() for l in f.read().splitlines() if not l.startswith(b">"))
        assert text_of(oracle.Decoder(new)) == fasta and any(97 <= c <= 122 for c in fasta)


# ---------------------------------------------------------------- 2. hand-made letters
def random_case(rng, n, alphabet=b"ACGTN", mean_run=40):
    """n letters whose case changes with probability 1 / mean_run at every letter"""
    up = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n)
    low = np.cumsum(rng.random(n) < 1.0 / mean_run) & 1
    return bytes(np.where((low == 1) & (up != ord("-")), up | 0x20, up).astype(np.uint8))


def units_text(rng, lengths, first_masked=False):
    """units of exactly these lengths, alternating case"""
    out, low = [], first_masked
    for l in lengths:
        t = ec.letters(rng, b"ACGT", l)
        out.append(t.lower() if low else t)
        low = not low
    return b"".join(out)


def hand_made_cases():
    """(name, sequence type, records); the lengths come from MASK_TILE and LANE_LETTERS, which check_hand_made asserts"""
    rng = np.random.default_rng(20240915)
    one = lambda t: split(t, [len(t)])
    out = [
        ("lower_at_0", "dna", one(b"acgtACGTTTacA")),
        ("lower_at_the_end", "dna", one(b"ACGTACGTTTacg")),
        ("all_lower", "dna", one(ec.letters(rng, b"acgtn", 1000))),
        ("all_upper", "dna", one(ec.letters(rng, b"ACGTN", 1000))),
        ("no_records", "dna", []),
        ("records_of_length_0", "dna", split(b"", [0, 0, 0])),
        ("units_254_255_256_510_65536", "dna", one(units_text(rng, [254, 255, 256, 510, 65536, 255, 254, 510, 3]))),
        ("units_masked_first", "dna", one(units_text(rng, [255, 254, 510, 256, 65536, 1], first_masked=True))),
        ("case_changes_at_every_letter", "dna", one(bytes(np.where(np.arange(100_000) & 1, ord("a"), ord("C")).astype(np.uint8)))),
        ("rna_with_u", "rna", one(b"ACGUacguuuNNnnACGU" * 50)),
        ("dash_inside_a_lower_case_run", "dna", one(b"ACGTac--gtACG-Tacgt-")),
    ]
    # edges at every offset modulo 16, on both sides of a lane's 16 letters and of the edge kernel's tile
    for base in (0, MASK_TILE - LANE_LETTERS, 2 * MASK_TILE - LANE_LETTERS):
        t = bytearray(ec.letters(rng, b"ACGT", 3 * MASK_TILE + 5))
        at = base
        for k in range(2 * LANE_LETTERS + 1):                 # lower-case runs of 1 + k % 3 letters starting at base + 17 k: every offset mod 16
            for j in range(1 + k % 3):
                t[at + j] |= 0x20
            at += LANE_LETTERS + 1
        starts = {(base + 17 * k) % 16 for k in range(2 * LANE_LETTERS + 1)}
        assert starts == set(range(16))
        out.append(("edges_mod_16_from_%d" % base, "dna", one(bytes(t))))
    for first, last in ((MASK_TILE - 1, MASK_TILE), (MASK_TILE, MASK_TILE + 1), (MASK_TILE - 1, MASK_TILE + 1), (0, MASK_TILE),
                        (MASK_TILE, 2 * MASK_TILE), (LANE_LETTERS - 1, LANE_LETTERS), (LANE_LETTERS, 2 * LANE_LETTERS)):
        t = bytearray(ec.letters(rng, b"ACGT", 2 * MASK_TILE + LANE_LETTERS + 3))
        for j in range(first, last):
            t[j] |= 0x20
        out.append(("run_%d_%d_across_the_tile_boundary" % (first, last), "dna", one(bytes(t))))
    for n in (MASK_TILE - 1, MASK_TILE, MASK_TILE + 1, LANE_LETTERS - 1, LANE_LETTERS, LANE_LETTERS + 1):
        out.append(("%d_letters_random_case" % n, "dna", one(random_case(rng, n, mean_run=5))))
    out.append(("many_records_random_case", "dna", split(random_case(rng, 60_000, b"ACGTN-RY"), [0, 1, 15, 16, 17, 4095, 4096, 4097, 0, 30_000, 17_663])))
    # the Mask section itself is larger than one 128 KiB zstd block
    big = random_case(rng, 300_000, mean_run=2)
    assert len(mask_bytes_np(big)) > (128 << 10)
    out.append(("mask_section_of_several_blocks", "dna", split(big, [100_000, 200_000])))
    return out


def check_hand_made(lib, name, sequence_type, records):
    kernel_constants()
    blob = check_records(lib, name, records, sequence_type, host_levels=(1,))
    if name == "mask_section_of_several_blocks":
        frame = ec.sections(blob)["mask"][1]
        assert len(ec.block_types(frame)) >= 2
    if name in ("no_records", "records_of_length_0"):       # an empty section, not one unit `00`
        assert ec.sections(blob)["mask"][0] == 0


def check_record_ends(lib):
    """A masked run that spans three records, and one that ends exactly on a record end.  The archive is exact under
    spec_mask=True; the reference's decoder leaves the tail of a masked unit that reaches a record's end in upper case
    (oracle/naf_oracle.c:460-471), and the default reading of the new archive is the oracle's default reading of an
    archive that tests/naf_writer.py writes for the same text."""
    rng = np.random.default_rng(3)
    text = units_text(rng, [30, 100, 40, 20, 60])         # masked: [30, 130) over records 0..2; [170, 190) ends with record 3
    records = split(text, [50, 40, 60, 40, 60])
    blob = check_records(lib, "record_ends", records, host_levels=(1,))
    ref = nw.write_naf([dict(id=r.id, comment=r.comment, sequence=r.sequence) for r in records],
                       mask_runs=nw.runs_from_case(text.decode()))
    assert mask_section(ref) == mask_section(blob)
    assert ec.as_tuples(oracle.Decoder(blob)) == ec.as_tuples(oracle.Decoder(ref))
    assert ec.as_tuples(oracle.Decoder(blob)) != ec.as_tuples(records)        # the quirk does bite here
    assert ec.as_tuples(oracle.Decoder(blob, spec_mask=True)) == ec.as_tuples(records)


def call_encode_device(lib, src, sequence_type, level=1, mask=1, **fields):
    """the C entry point itself, with opts->mask -> (status, archive bytes or None); the message in .message"""
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(("dna", "rna", "protein", "text").index(sequence_type), ctypes.byref(opts))
    opts.id, opts.comment, opts.sequence, opts.quality = (int(bool(fields.get(f))) for f in ("id", "comment", "sequence", "quality"))
    opts.compression_level, opts.mask = level, mask
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


def check_unaligned_pointer(lib):
    """the letters at addresses that are not multiples of 16: the 16-byte loads of the pack and edge kernels give way"""
    rng = np.random.default_rng(4)
    text = random_case(rng, 2 * MASK_TILE + 100, mean_run=7)
    dec, res = ec.device_text(lib, text)
    try:
        assert res.d_sequence % 16 == 0
        for shift in (1, 7, 13):
            body = text[shift:]
            want = ec.host_archive(lib, [Record(sequence=body.decode())], "dna", 1, sequence=True, mask=True)
            dec2 = Decoder(io.BytesIO(want), spec_mask=True, _lib=lib)       # for a record table in device memory: [len(body)]
            res2 = dec2.decode_all_device()
            src = _ffi.EncodeSource(d_sequence=res.d_sequence + shift, n_bases=len(body), d_record_end=res2.d_record_end, n_records=1)
            rc, got = call_encode_device(lib, src, "dna", sequence=True)
            dec2.close()
            assert rc == _ffi.OK and got == want, shift
    finally:
        dec.close()


# ---------------------------------------------------------------- 3. errors
def check_errors(lib):
    # mask needs a nucleotide sequence
    for stype, fields in (("protein", dict(sequence=True)), ("text", dict(sequence=True)), ("dna", dict(id=True)), ("rna", dict(quality=True))):
        try:
            Encoder(io.BytesIO(), stype, mask=True, _lib=lib, **fields)
        except ValueError:
            pass
        else:
            raise AssertionError("Encoder(mask=True) accepted %s %r" % (stype, fields))
        opts, h, err = _ffi.EncoderOpts(), ctypes.c_void_p(), _ffi.Error()
        lib.c.nafgpu_encoder_opts_default(("dna", "rna", "protein", "text").index(stype), ctypes.byref(opts))
        for f in fields:
            setattr(opts, f, 1)
        opts.mask = 1
        assert lib.c.nafgpu_encoder_new(ctypes.byref(opts), ctypes.byref(h), ctypes.byref(err)) == _ffi.E_INVALID_ARG and not h.value
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_from_flags(0, 0x3F, ctypes.byref(opts))       # flag 0x04 is ignored, as EncoderBuilder::from_flags does
    assert (opts.id, opts.comment, opts.sequence, opts.quality, opts.mask) == (1, 1, 1, 1, 0) and ctypes.sizeof(opts) == 16
    rng = np.random.default_rng(6)
    good = random_case(rng, 1 << 18)
    dec, res = ec.device_text(lib, good)
    src = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=1)
    for stype in ("protein", "text"):
        assert call_encode_device(lib, src, stype, sequence=True)[0] == _ffi.E_INVALID_ARG
    src_q = _ffi.EncodeSource(d_quality=res.d_sequence, n_quality=res.n_bases, d_record_end=res.d_record_end, n_records=1)
    assert call_encode_device(lib, src_q, "dna", quality=True)[0] == _ffi.E_INVALID_ARG
    for stype in ("protein", "text"):
        try:
            encode_device(res, sequence_type=stype, sequence=True, mask=True, device=0, _lib=lib)
        except ValueError:
            pass
        else:
            raise AssertionError("encode_device(mask=True) accepted " + stype)
    # the same letters are accepted, and refused without the option exactly as before
    rc, blob = call_encode_device(lib, src, "dna", sequence=True)
    assert rc == _ffi.OK and blob == ec.host_archive(lib, [Record(sequence=good.decode())], "dna", 1, sequence=True, mask=True)
    first_lower = next(i for i, c in enumerate(good) if 97 <= c <= 122)
    rc, blob = call_encode_device(lib, src, "dna", mask=0, sequence=True)
    assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None) and "letter %d)" % first_lower in call_encode_device.message
    dec.close()
    try:
        ec.host_archive(lib, [Record(sequence="ACgT")], "dna", 1, sequence=True)
    except ValueError:
        pass
    else:
        raise AssertionError("lower case accepted without mask=True")
    assert not flags_of(ec.host_archive(lib, [Record(sequence="ACGT")], "dna", 1, sequence=True)) & 0x04
    # a lower-case letter whose upper-case form the table refuses, inside a lower-case run
    for bad, stype in ((b"x", "dna"), (b"u", "dna"), (b"t", "rna")):
        at = (1 << 17) + 4321
        body = good.replace(b"T", b"U").replace(b"t", b"u") if stype == "rna" else good
        lower = body[:at - 3] + body[at - 3:at].lower() + bad + body[at + 1:at + 4].lower() + body[at + 4:]
        assert len(lower) == len(good)
        dec, res = ec.device_text(lib, lower)
        src = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=1)
        rc, blob = call_encode_device(lib, src, stype, sequence=True)
        assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None), (bad, stype, rc)
        assert "letter %d)" % at in call_encode_device.message, call_encode_device.message
        dec.close()
        try:
            ec.host_archive(lib, [Record(sequence=lower[at - 10:at + 10].decode())], stype, 1, sequence=True, mask=True)
        except ValueError:
            pass
        else:
            raise AssertionError("the host encoder accepted %r in %s" % (bad, stype))
    # a refused push between two accepted ones: as if it had never happened (the open unit included)
    a, b = Record(id="a", sequence="ACGTacg"), Record(id="b", sequence="tacgTTga")
    refused = [Record(id="x", sequence="ggggxGGG"), Record(id="y", sequence="GGGG", length=5), Record(sequence="acgt")]
    for level in (0, 1):
        want = ec.host_archive(lib, [a, b], "dna", level, id=True, sequence=True, mask=True)
        buf = io.BytesIO()
        with Encoder(buf, "dna", id=True, sequence=True, compression_level=level, mask=True, _lib=lib) as enc:
            enc.write(a)
            for r in refused:
                try:
                    enc.write(r)
                except ValueError:
                    pass
                else:
                    raise AssertionError("accepted %r" % r.sequence)
            enc.write(b)
        assert buf.getvalue() == want
        assert mask_section(want) == mask_bytes(b"ACGTacgtacgTTga")
