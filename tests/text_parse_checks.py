"""Shared by tests/test_text_parse_emu.py (CPU harness) and tests/test_gpu_text_parse.py (MI355X): parse_text and encode_text,
FASTA / FASTQ text -> records in device memory -> archive.  Not a test module; every function takes the library binding it
is to check.

The yardstick is `parse` below, a plain Python parser of the rules in include/nafgpu.h (nafgpu_parse_text), which reads from
the fixtures' texts the records the CPU oracle reads from the fixtures' archives; the archives are compared byte for byte
with what the host Encoder writes when those records are pushed one by one."""
import ctypes
import io
import os

import numpy as np

import encode_checks as ec
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Record, encode_device, encode_text, parse_text
from oracle import oracle

ENTRY_POINTS = ("nafgpu_parse_opts_default", "nafgpu_parse_text", "nafgpu_parse_copy_to_host", "nafgpu_parse_hash64", "nafgpu_parse_free",
                "nafgpu_encode_text")
TILE, LANE = 4096, 16        # nafcodec_amd/csrc/parse.h (kParseTile) and parse.hip (16 text bytes per lane): asserted below
# fixture: (text file, sequence type, mask, records, longest sequence line)
FIXTURES = {"LuxC": ("LuxC.faa", "protein", False, 12, 60), "masked": ("masked.fna", "dna", True, 2, 50),
            "phix": ("phix.fastq", "dna", True, 42, 301)}


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return ec.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "parse.h")) as f:
        assert "constexpr uint32_t kParseTile = %d;" % TILE in f.read()
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "parse.hip")) as f:
        assert "static_assert(kParseTile == kThreads * %d" % LANE in f.read()


# ---------------------------------------------------------------- the yardstick
class Refused(Exception):
    def __init__(self, kind, at):
        super().__init__("%s at %d" % (kind, at))
        self.kind, self.at = kind, at        # kind: "arg" (at: a byte offset) or "length" (at: a record index)


def parse(text, format=None):
    """-> (fastq, [(id, comment, sequence, quality or None)], longest sequence line); Refused where the rules refuse"""
    text = bytes(text)
    if not text:
        return format == "fastq", [], 0
    if text[:1] not in (b">", b"@") or (format == "fasta" and text[:1] != b">") or (format == "fastq" and text[:1] != b"@"):
        raise Refused("arg", 0)
    fastq = text[:1] == b"@"
    lines, at = [], 0                                   # (offset, bytes without the line end)
    for piece in text.split(b"\n"):
        lines.append((at, piece[:-1] if piece.endswith(b"\r") else piece))
        at += len(piece) + 1
    if text.endswith(b"\n"):
        lines.pop()
    bad, records, longest = [], [], 0

    def header(off, line):
        if b"\0" in line:
            bad.append(off + line.index(b"\0"))
        name, _, comment = line[1:].partition(b" ")
        return name, comment

    if not fastq:
        for off, line in lines:
            if line[:1] == b">":
                records.append(list(header(off, line)) + [b"", None])
            else:
                records[-1][2] += line
                longest = max(longest, len(line))
    else:
        for i, (off, line) in enumerate(lines):
            if i % 4 == 0:
                if line[:1] != b"@":
                    bad.append(off)
                records.append(list(header(off, line)) + [b"", b""])
            elif i % 4 == 1:
                records[-1][2] = line
                longest = max(longest, len(line))
            elif i % 4 == 2:
                if line[:1] != b"+":
                    bad.append(off)
            else:
                records[-1][3] = line
        if len(lines) % 4:
            bad.append(len(text))
    if bad:
        raise Refused("arg", min(bad))
    for k, r in enumerate(records):
        if fastq and len(r[2]) != len(r[3]):
            raise Refused("length", k)
    return fastq, [tuple(r) for r in records], longest


def as_records(tuples):
    return [Record(id=i.decode("latin-1"), comment=c.decode("latin-1"), sequence=s.decode("latin-1"),
                   quality=None if q is None else q.decode("latin-1"), length=len(s)) for i, c, s, q in tuples]


# ---------------------------------------------------------------- what the device made
def device_records(p):
    """the fields of a ParsedText, copied to the host -> [(id, comment, sequence, quality or None)]"""
    ends = np.frombuffer(p.copy_to_host(p.d_record_end, 8 * p.n_records), dtype=np.uint64).tolist()
    seq = p.copy_to_host(p.d_sequence, p.n_bases)
    qual = p.copy_to_host(p.d_quality, p.n_quality) if p.fastq else None
    ids = p.copy_to_host(p.d_ids, p.n_ids_bytes)
    com = p.copy_to_host(p.d_comments, p.n_comments_bytes)
    if not p.n_records:
        assert (p.n_bases, p.n_quality, p.n_ids_bytes, p.n_comments_bytes) == (0, 0, 0, 0)
        return []
    assert ids.endswith(b"\0") and com.endswith(b"\0") and ends[-1] == len(seq)
    ids, com = ids[:-1].split(b"\0"), com[:-1].split(b"\0")
    assert len(ids) == len(com) == p.n_records
    if p.fastq:
        assert len(qual) == len(seq)
    out, a = [], 0
    for k, b in enumerate(ends):
        out.append((ids[k], com[k], seq[a:b], qual[a:b] if p.fastq else None))
        a = b
    return out


def varint(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    return bytes(reversed(out))


def with_line_length(blob, line_length):
    """the archive with the header's line length (60, one byte) replaced: all that keep_line_length may change"""
    at = 6 if blob[3] == 1 else 7
    assert blob[at] == 60
    return blob[:at] + varint(line_length) + blob[at + 1:]


def header_line_length(blob):
    return ec.read_varint(blob, 6 if blob[3] == 1 else 7)[0]


def fields_for(fastq):
    return dict(id=True, comment=True, sequence=True, quality=bool(fastq))


def check_text(lib, name, text, sequence_type="dna", mask=None, levels=(1,), format=None):
    """parse_text against the yardstick, encode_text against the host Encoder -> the records"""
    mask = sequence_type in ("dna", "rna") if mask is None else mask
    fastq, want, longest = parse(text, format)
    with parse_text(text, format=format, device=0, _lib=lib) as p:
        assert (p.fastq, p.n_records, p.line_length, p.n_text) == (fastq, len(want), longest, len(text)), (name, p.n_records, p.line_length)
        got = device_records(p)
        assert got == want, (name, [k for k, (a, b) in enumerate(zip(got, want)) if a != b][:3])
        assert p.hash_device(p.d_sequence, p.n_bases) == lib.c.nafgpu_hash64_host(b"".join(r[2] for r in want), p.n_bases), name
        fields = fields_for(fastq)
        via_records = encode_device(p, sequence_type=sequence_type, compression_level=1, device=0, mask=mask, _lib=lib, **fields)
    records = as_records(want)
    for level in levels:
        host = ec.host_archive(lib, records, sequence_type, level, mask=mask, **fields)
        got = encode_text(text, sequence_type=sequence_type, mask=mask, compression_level=level, keep_line_length=False, format=format,
                          device=0, _lib=lib)
        assert got == host, (name, level, "encode_text")
        if level == 1:
            assert via_records == host, (name, "encode_device of the parse result")
        kept = encode_text(text, sequence_type=sequence_type, mask=mask, compression_level=level, format=format, device=0, _lib=lib)
        assert kept == with_line_length(host, longest) and header_line_length(kept) == longest, (name, level, "keep_line_length")
    return want


# ---------------------------------------------------------------- 1. the fixtures
def fixture_text(name):
    with open(os.path.join(ROOT, "tests", "golden", FIXTURES[name][0]), "rb") as f:
        return f.read()


def check_fixture(lib, name, round_trip=False):
    file_, stype, mask, n_rec, longest = FIXTURES[name]
    text = fixture_text(name)
    want = check_text(lib, name, text, stype, mask, levels=(1, 2))
    fastq = name == "phix"
    assert (len(want), parse(text)[2], parse(text)[0]) == (n_rec, longest, fastq)
    blob = golden_bytes(name + ".naf")
    assert header_line_length(blob) == longest                        # what `ennaf` wrote into the fixture's own header
    from_oracle = [((r.id or "").encode("latin-1"), (r.comment or "").encode("latin-1"), (r.sequence or "").encode("latin-1"),
                    r.quality.encode("latin-1") if fastq else None) for r in oracle.Decoder(blob)]
    assert from_oracle == want, name
    for level in (1, 2):
        got = encode_text(text, sequence_type=stype, mask=mask, compression_level=level, keep_line_length=False, device=0, _lib=lib)
        read = [((r.id or "").encode("latin-1"), (r.comment or "").encode("latin-1"), (r.sequence or "").encode("latin-1"),
                 r.quality.encode("latin-1") if fastq else None) for r in oracle.Decoder(got, spec_mask=True)]
        assert read == want, (name, level, "the oracle's reading of the new archive")
    if round_trip:                                                    # text -> archive -> text, on the device
        kept = encode_text(text, sequence_type=stype, mask=mask, device=0, _lib=lib)
        dec = Decoder(io.BytesIO(kept), spec_mask=True, _lib=lib)
        try:
            assert dec.to_text() == text + (b"" if text.endswith(b"\n") else b"\n"), name
        finally:
            dec.close()
        assert name != "masked" or not text.endswith(b"\n")           # the one final line feed the file lacks


# ---------------------------------------------------------------- 2. hand-made texts
def seq_lines(rng, n, width):
    s = ec.letters(rng, b"ACGT", n)
    return b"".join(s[i:i + width] + b"\n" for i in range(0, n, width))


def boundary_text(kind, at):
    """FASTA whose second header has its '>' (kind 0), its separator (1) or its line feed (2) at text offset `at`"""
    rng = np.random.default_rng(at * 3 + kind)
    pad = at - 8 - (0, 3, 6)[kind]
    text = b">r0 c0\n" + ec.letters(rng, b"ACGT", pad) + b"\n>r1 c1\nACGTTGCA\nAC\n"
    assert text[at:at + 1] == (b">", b" ", b"\n")[kind]
    return text


def random_fasta(rng, n_bytes):
    out, k = [], 0
    while sum(map(len, out)) < n_bytes:
        name = b"s%d" % k + b"x" * int(rng.integers(0, 9))
        comment = (b"", b" ", b" note", b" two words " + b"y" * int(rng.integers(0, 7)))[int(rng.integers(0, 4))]
        out.append(b">" + name + comment + b"\n" + seq_lines(rng, int(rng.integers(0, 200)), int(rng.integers(1, 38))))
        k += 1
    return b"".join(out)


def random_fastq(rng, n_bytes, eol=b"\n"):
    out, k = [], 0
    while sum(map(len, out)) < n_bytes:
        l = int(rng.integers(0, 320))
        comment = (b"", b" 1:N:0", b" ")[k % 3]
        qual = bytes(rng.integers(33, 75, l, dtype=np.uint8))
        out.append(b"@q%d" % k + comment + eol + ec.letters(rng, b"ACGTN", l) + eol + (b"+", b"+q%d" % k)[k % 2] + eol + qual + eol)
        k += 1
    return b"".join(out)


def positions(text, what):
    a = np.frombuffer(text, dtype=np.uint8)
    if what == "lf":
        return np.flatnonzero(a == 10)
    starts = np.concatenate(([0], np.flatnonzero(a[:-1] == 10) + 1))
    if what == "open":
        return starts[a[starts] == ord(">")]
    seps = []                                          # the first ' ' of every header line
    for s in starts[a[starts] == ord(">")].tolist():
        line = text[s:text.index(b"\n", s)]
        if b" " in line:
            seps.append(s + line.index(b" "))
    return np.array(seps)


def hand_made_cases(small=False):
    """(name, text, sequence type).  `small`: without the multi-tile random texts (the sanitizer leg)"""
    rng = np.random.default_rng(20241017)
    out = []
    for at in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, LANE - 1, LANE, LANE + 1):
        for kind in range(3):
            if at - 8 - (0, 3, 6)[kind] >= 0:
                out.append(("%s_at_%d" % (("open", "separator", "line_feed")[kind], at), boundary_text(kind, at), "dna"))
    if not small:
        text = random_fasta(rng, 5 * TILE)
        for what in ("lf", "open", "sep"):             # every offset mod 16
            assert set((positions(text, what) % LANE).tolist()) == set(range(LANE)), what
        out.append(("random_fasta_5_tiles", text, "dna"))
        out.append(("random_fastq_5_tiles", random_fastq(rng, 5 * TILE), "dna"))
        out.append(("random_fastq_crlf", random_fastq(rng, 2 * TILE, b"\r\n"), "dna"))
    out += [
        ("header_longer_than_a_tile", b">" + b"i" * (TILE + 904) + b" " + b"c d " * (TILE // 2) + b"\nACGT\n>b\nAC\n", "dna"),
        ("sequence_line_of_several_tiles", b">chr1 one line\n" + ec.letters(rng, b"ACGTN", 3 * TILE + 1234) + b"\n>b\nAC\n", "dna"),
        ("sequence_line_of_several_tiles_no_line_feed", b">chr1\n" + ec.letters(rng, b"ACGTacgt", 2 * TILE + 77), "dna"),
        ("one_record_no_line_feed", b">only one", "dna"),
        ("one_record_id_only_no_line_feed", b">only", "dna"),
        ("empty_sequences", b">a\n>b\n>c x\nACGT\n>d\n>e\n", "dna"),
        ("empty_sequence_last_no_line_feed", b">a\nAC\n>b", "dna"),
        ("empty_lines", b">a\n\nAC\n\n\nGT\n\n>b\n\n", "dna"),
        ("ids_and_comments", b">a\nAC\n>b \nAC\n>c d e  f \nAC\n> lone comment\nAC\n>\nGT\n>g\tnot a separator\nA\n", "dna"),
        ("greater_than_inside_a_line", b">a >b\nAC>GT\nG>\n", "text"),
        ("crlf_last_byte_cr", b">a b\r\nACGT\r\nAC\r", "dna"),
        ("lower_case_kept", b">a\nacgtNNacgt\nACGTnn\n", "dna"),
        ("protein", b">p1 some protein\nMKVLAAGIVGLCAqw\nMKK\n>p2\nmkv\n", "protein"),
        ("fastq_marks_in_quality", b"@r1 c\nACGT\n+r1 c\n@III\n@r2\nAC\n+\n+I\n@r3\n\n+\n\n", "dna"),
        ("fastq_no_final_line_feed", b"@r1\nACGT\n+\nIIII", "dna"),
        ("fastq_one_empty_record", b"@r1\n\n+\n\n", "dna"),
    ]
    return out


def check_hand_made(lib, name, text, sequence_type):
    kernel_constants()
    check_text(lib, name, text, sequence_type)


def check_lines_longer_than_the_scan_span(lib, parse_only=False):
    """a sequence line and a header of more than 2048 tiles each: the state passes through whole workgroups of the tile scan
    (`parse_only`: the records alone -- the CPU harness takes minutes for every pass over 17 MB)"""
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "parse.hip")) as f:
        assert "constexpr uint32_t kScanItems = 8, kScanSpan = kThreads * kScanItems;" in f.read()
    span = 256 * 8 * TILE
    rng = np.random.default_rng(12)
    text = b">chr1 a chromosome on one line\n" + ec.letters(rng, b"ACGTN", span + 3 * TILE + 17) + b"\n>r2 " + b"c " * (span // 2 + 999) + \
           b"\nACGT\nAC\n>r3\n" + ec.letters(rng, b"acgt", 77) + b"\n"
    if not parse_only:
        check_text(lib, "lines_longer_than_the_scan_span", text)
        return
    fastq, want, longest = parse(text)
    with parse_text(text, device=0, _lib=lib) as p:
        assert (p.fastq, p.n_records, p.line_length) == (fastq, len(want), longest) and device_records(p) == want


def check_crlf(lib):
    """CRLF throughout: the archive of the LF version, with and without the text's line length"""
    rng = np.random.default_rng(8)
    for text in (random_fasta(rng, TILE + 500), random_fastq(rng, TILE + 500)):
        crlf = text.replace(b"\n", b"\r\n")
        assert parse(crlf) == parse(text)
        for keep in (False, True):
            a, b = (encode_text(t, mask=True, keep_line_length=keep, device=0, _lib=lib) for t in (text, crlf))
            assert a == b
        check_text(lib, "crlf", crlf)
    # a lone CR is data: the parser keeps it, the nucleotide table refuses it, a text archive takes it
    lone = b">a\nAC\rGT\n\rA\n"
    assert parse(lone)[1] == [(b"a", b"", b"AC\rGT\rA", None)]
    check_text(lib, "lone_cr", lone, "text")
    rc, blob, message = call_encode_text(lib, lone)
    assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None) and "letter 2)" in message, message


def check_empty(lib):
    for format, fastq in ((None, False), ("fasta", False), ("fastq", True)):
        with parse_text(b"", format=format, device=0, _lib=lib) as p:
            assert (p.n_records, p.n_bases, p.fastq, p.line_length) == (0, 0, fastq, 0) and device_records(p) == []
        fields = fields_for(fastq)
        want = ec.host_archive(lib, [], "dna", 1, **fields)
        assert encode_text(b"", format=format, keep_line_length=False, device=0, _lib=lib) == want
        assert encode_text(b"", format=format, device=0, _lib=lib) == with_line_length(want, 0)


def check_unaligned_pointer(lib):
    """text in device memory at addresses that are not multiples of 16 (text_on_device): the 16-byte loads stay aligned"""
    rng = np.random.default_rng(9)
    for text in (random_fasta(rng, 2 * TILE + 100), random_fastq(rng, 2 * TILE + 100)):
        fastq, want, longest = parse(text)
        host = ec.host_archive(lib, as_records(want), "dna", 1, mask=True, **fields_for(fastq))
        for shift in (1, 7, 13, 15, 16):
            dec, res = ec.device_text(lib, b"#" * shift + text)
            try:
                assert res.d_sequence % 16 == 0
                with parse_text(res.d_sequence + shift, len(text), device=0, _lib=lib) as p:
                    assert (p.fastq, p.line_length) == (fastq, longest) and device_records(p) == want, shift
                    got = encode_device(p, sequence_type="dna", compression_level=1, device=0, mask=True, _lib=lib, **fields_for(fastq))
                assert got == host, shift
            finally:
                dec.close()


# ---------------------------------------------------------------- 3. errors
def call_encode_text(lib, text, sequence_type="dna", level=1, format=0, keep=0, quality=None, mask=1, **fields):
    """the C entry point itself -> (status, archive or None, message); nothing is produced with an error"""
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(("dna", "rna", "protein", "text").index(sequence_type), ctypes.byref(opts))
    opts.id, opts.comment, opts.sequence = (int(fields.get(f, True)) for f in ("id", "comment", "sequence"))
    opts.quality = int(text[:1] == b"@" if quality is None else quality)
    opts.compression_level, opts.mask = level, mask
    popts = _ffi.ParseOpts(format=format)
    p, n, err = ctypes.c_void_p(), ctypes.c_uint64(), _ffi.Error()
    rc = lib.c.nafgpu_encode_text(text, len(text), ctypes.byref(popts), ctypes.byref(opts), keep, 0, ctypes.byref(p), ctypes.byref(n),
                                  ctypes.byref(err))
    message = err.message.decode("utf-8", "replace")
    if rc != _ffi.OK:
        assert not p.value and n.value == 0 and err.status == rc
        return rc, None, message
    try:
        return rc, ctypes.string_at(p, n.value), message
    finally:
        lib.c.nafgpu_encode_free(p)


def call_parse_text(lib, text, format=0):
    """-> (status, message); with an error no handle and a zeroed result"""
    popts = _ffi.ParseOpts(format=format)
    h, res, err = ctypes.c_void_p(), _ffi.ParseResult(), _ffi.Error()
    rc = lib.c.nafgpu_parse_text(text, len(text), ctypes.byref(popts), 0, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_parse_free(h)
    return rc, err.message.decode("utf-8", "replace")


GOOD_FASTA, GOOD_FASTQ = b">a b\nACGT\nAC\n>c\nGG\n", b"@a b\nACGT\n+\nIIII\n@c\nGG\n+\nII\n"


def check_errors(lib):
    def good():                                          # the next valid call in the same process succeeds
        for text in (GOOD_FASTA, GOOD_FASTQ):
            check_text(lib, "after_an_error", text)

    def refused(text, status, needle, format=0):
        try:
            parse(text, (None, "fasta", "fastq")[format])
        except Refused as e:
            assert ("byte offset %d)" % e.at if e.kind == "arg" else "record %d " % e.at) == needle, (text[:40], e.kind, e.at, needle)
        else:
            raise AssertionError("the yardstick accepts %r" % text[:40])
        rc, message = call_parse_text(lib, text, format)
        assert rc == status and needle in message, (text[:40], rc, message)
        rc, blob, message = call_encode_text(lib, text, format=format)
        assert (rc, blob) == (status, None) and needle in message, (text[:40], rc, message)
        good()

    good()
    refused(b"ACGT\n>a\nAC\n", _ffi.E_INVALID_ARG, "byte offset 0)")                      # wrong first byte
    refused(b"\n>a\nAC\n", _ffi.E_INVALID_ARG, "byte offset 0)")
    refused(GOOD_FASTA, _ffi.E_INVALID_ARG, "byte offset 0)", format=2)                   # the stated format disagrees
    refused(GOOD_FASTQ, _ffi.E_INVALID_ARG, "byte offset 0)", format=1)
    for cut in (1, 2, 3):                                                                 # 4 k + 1 / 2 / 3 lines
        lines = GOOD_FASTQ.split(b"\n")[:4 + cut]
        for text in (b"\n".join(lines) + b"\n", b"\n".join(lines)):
            refused(text, _ffi.E_INVALID_ARG, "byte offset %d)" % len(text))
    big = random_fastq(np.random.default_rng(10), 3 * TILE)
    starts = [0] + [i + 1 for i in range(len(big) - 1) if big[i] == 10]
    for k_at, k_plus in ((20, 5), (5, 22)):                                             # two offenders: the lower offset is named
        t = bytearray(big)
        t[starts[4 * k_at]] = ord("a")
        t[starts[4 * k_plus + 2]] = ord("-")
        refused(bytes(t), _ffi.E_INVALID_ARG, "byte offset %d)" % min(starts[4 * k_at], starts[4 * k_plus + 2]))
    refused(b"@a\nAC\n\nII\n", _ffi.E_INVALID_ARG, "byte offset 6)")                      # an empty third line
    refused(GOOD_FASTQ + b"\n", _ffi.E_INVALID_ARG, "byte offset %d)" % len(GOOD_FASTQ))  # a stray empty line at the end
    short = b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n@c\nAC\n+\nI\n"
    refused(short, _ffi.E_INVALID_LENGTH, "record 1 ")                                    # a quality one byte short; the first is named
    refused(b"@a\nACGT\n+\nIII\n@b\nAC\n+\nIII\n", _ffi.E_INVALID_LENGTH, "record 0 ")    # the totals agree, the records do not
    refused(b">a b\0c\nAC\n>d\0\nAC\n", _ffi.E_INVALID_ARG, "byte offset 4)")             # NUL in a header
    refused(b"@a\nAC\n+\nII\n@b\0\nAC\n+\nII\n", _ffi.E_INVALID_ARG, "byte offset 13)")
    assert parse(b">a\nAC\0GT\n")[1][0][2] == b"AC\0GT"                                    # elsewhere it is data
    check_text(lib, "nul_in_a_sequence", b">a\nAC\0GT\n", "text")
    # the encode stage's refusals
    for text in (GOOD_FASTA, GOOD_FASTQ):
        for level in (0, 3):
            rc, blob, _ = call_encode_text(lib, text, level=level)
            assert (rc, blob) == (_ffi.E_INVALID_ARG, None), level
    rc, blob, message = call_encode_text(lib, GOOD_FASTA, quality=1)
    assert (rc, blob) == (_ffi.E_MISSING_FIELD, None) and "quality" in message
    rc, blob, _ = call_encode_text(lib, GOOD_FASTA, sequence_type="protein")               # mask needs nucleotides
    assert (rc, blob) == (_ffi.E_INVALID_ARG, None)
    rc, blob, message = call_encode_text(lib, b">a\nACGT\nACXT\n>b\nXX\n")
    assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None) and "letter 6)" in message, message
    rc, blob, message = call_encode_text(lib, b">a\nACgT\n", mask=0)                       # lower case without mask
    assert (rc, blob) == (_ffi.E_INVALID_SEQUENCE, None) and "letter 2)" in message, message
    good()
    # the Python mirror: ValueError, as for encode_device
    for bad in (dict(data=b"ACGT"), dict(data=GOOD_FASTA, quality=True), dict(data=GOOD_FASTA, compression_level=3),
                dict(data=b">a\nAXGT\n"), dict(data=GOOD_FASTA, format="fastq"), dict(data=GOOD_FASTA, sequence_type="protein", mask=True)):
        try:
            encode_text(bad.pop("data"), device=0, _lib=lib, **bad)
        except ValueError:
            pass
        else:
            raise AssertionError("encode_text accepted %r" % bad)
    try:
        parse_text(b"@a\nAC\n+\n", device=0, _lib=lib)
    except ValueError as e:
        assert "byte offset 8)" in str(e)
    else:
        raise AssertionError("parse_text accepted three lines")
    # fields the options do not name are dropped; quality=None follows the text
    want = ec.host_archive(lib, [Record(sequence="ACGTAC"), Record(sequence="GG")], "dna", 1, sequence=True)
    assert encode_text(GOOD_FASTA, id=False, comment=False, keep_line_length=False, device=0, _lib=lib) == want
    assert encode_text(GOOD_FASTQ, id=False, comment=False, quality=False, keep_line_length=False, device=0, _lib=lib) == \
        ec.host_archive(lib, [Record(sequence="ACGT"), Record(sequence="GG")], "dna", 1, sequence=True)
    assert ec.host_archive(lib, [Record(sequence="AC")], "dna", 1, sequence=True)[6] == 60    # every other caller's header says 60
    good()


# ---------------------------------------------------------------- 4. / 5. at size (MI355X only)
def text_round_trip_on_device(lib, dec, res, want_seq_hash, want_ends_hash, name, fields):
    """records in HBM (`dec`, `res`: a bulk decode) -> format_device -> parse_text on the text where it lies -> the hashes;
    encode_device of the parse result, decoded again -> the hashes once more.  -> (the text's size, the parse's ms)"""
    text = dec.format_device()
    want_qual_hash = dec.hash_device(res.d_quality, res.n_quality) if fields.get("quality") else None
    assert dec.hash_device(res.d_sequence, res.n_bases) == want_seq_hash and dec.hash_device(res.d_record_end, 8 * res.n_records) == want_ends_hash
    with parse_text(text.d_text, text.n_text, device=0, _lib=lib) as p:
        print("%s: %d bytes of text, %d records, parse %.3f ms" % (name, text.n_text, p.n_records, p.ms))
        assert (p.n_records, p.n_bases, p.n_text, p.fastq) == (res.n_records, res.n_bases, text.n_text, bool(fields.get("quality"))), name
        assert p.hash_device(p.d_sequence, p.n_bases) == want_seq_hash, name
        assert p.hash_device(p.d_record_end, 8 * p.n_records) == want_ends_hash, name
        if want_qual_hash is not None:
            assert p.n_quality == res.n_quality and p.hash_device(p.d_quality, p.n_quality) == want_qual_hash, name
        if dec.line_length:
            assert p.line_length == dec.line_length, (name, p.line_length)
        ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
        last_at = int(ends[-2]) if len(ends) > 1 else 0
        for at, n in ((0, int(ends[0])), (last_at, int(ends[-1]) - last_at)):     # the first and the last record's letters
            assert p.copy_to_host(p.d_sequence + at, n) == dec.copy_to_host(res.d_sequence + at, n), (name, at)
        again = encode_device(p, sequence_type="dna", compression_level=1, device=0, mask=True, _lib=lib, **fields)
        n_text, ms = text.n_text, p.ms
    dec2 = Decoder(io.BytesIO(again), _lib=lib)
    try:
        res2 = dec2.decode_all_device()
        assert (res2.n_bases, res2.n_records) == (res.n_bases, res.n_records)
        assert dec2.hash_device(res2.d_sequence, res2.n_bases) == want_seq_hash, name
        assert dec2.hash_device(res2.d_record_end, 8 * res2.n_records) == want_ends_hash, name
        if want_qual_hash is not None:
            assert dec2.hash_device(res2.d_quality, res2.n_quality) == want_qual_hash, name
    finally:
        dec2.close()
    return n_text, ms


def check_synthetic_at_size(lib, n_bases=256_000_000):
    arc = lib.synth(n_bases, seed=31, with_mask=True, iupac_permille=5)
    try:
        dec = Decoder(io.BytesIO(ctypes.string_at(arc.bytes, arc.n)), _lib=lib)
        try:
            res = dec.decode_all_device()
            assert (res.n_bases, res.n_records) == (arc.n_bases, arc.n_records)
            text_round_trip_on_device(lib, dec, res, arc.seq_hash, arc.offsets_hash, "synthetic, masked",
                                      dict(id=True, comment=True, sequence=True))
        finally:
            dec.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))


def check_fastq_at_size(lib, copies=47_620):
    """2 000 040 records: the fixture's 42, `copies` times (tools/fastq_probe.py's generator needs libzstd).  Host text ->
    encode_text -> decode: the letters and qualities are the yardstick's, the text formatted on the device is the input."""
    unit = fixture_text("phix")
    _, recs, longest = parse(unit)
    text = unit * copies
    seq, qual = b"".join(r[2] for r in recs) * copies, b"".join(r[3] for r in recs) * copies
    ends = np.cumsum(np.tile(np.array([len(r[2]) for r in recs], dtype=np.uint64), copies), dtype=np.uint64).tobytes()
    seq_hash, ends_hash = lib.c.nafgpu_hash64_host(seq, len(seq)), lib.c.nafgpu_hash64_host(ends, len(ends))
    archive = encode_text(text, mask=True, device=0, _lib=lib)
    assert header_line_length(archive) == longest
    dec = Decoder(io.BytesIO(archive), spec_mask=True, _lib=lib)
    try:
        res = dec.decode_all_device()
        assert res.n_records == len(recs) * copies
        assert dec.hash_device(res.d_quality, res.n_quality) == lib.c.nafgpu_hash64_host(qual, len(qual))
        formatted = dec.format_device()
        assert formatted.n_text == len(text) and dec.hash_device(formatted.d_text, formatted.n_text) == lib.c.nafgpu_hash64_host(text, len(text))
        text_round_trip_on_device(lib, dec, res, seq_hash, ends_hash, "fastq", dict(id=True, comment=True, sequence=True, quality=True))
    finally:
        dec.close()


def check_past_u32(lib, B=2**32, extra=200_000_003):
    """the archive of tests/test_gpu_beyond_u32.py: more than 2^32 bytes of text, of letters, and text offsets past 2^32"""
    import beyond_u32_checks as bc
    s = bc.Synthetic(lib, B, extra)
    try:
        n_text, _ = text_round_trip_on_device(lib, s.dec, s.res, s.seq_hash, s.offsets_hash, "past 2^32", dict(id=True, comment=True, sequence=True))
        assert n_text > B and s.res.n_bases > B
    finally:
        s.close()
