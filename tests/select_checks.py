"""Shared by tests/test_select_emu.py (CPU harness) and tests/test_gpu_select.py (MI355X): Decoder.select and Decoder.find,
records and regions of a decoded archive -> a new set of records in device memory.  Not a test module; every function takes
the library binding it is to check.

The yardstick is the records the CPU oracle decodes from the archive, sliced in Python; the reverse strand goes through the
256-entry table below and [::-1].  Ids, comments, letters, qualities and the three end tables are compared byte for byte."""
import ctypes
import io
import os
import struct

import numpy as np

import encode_checks as ec
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Record, encode_device, parse_text
from oracle import oracle

ENTRY_POINTS = ("nafgpu_select", "nafgpu_find_records", "nafgpu_selection_format", "nafgpu_selection_copy_to_host", "nafgpu_selection_hash64",
                "nafgpu_selection_free")
TILE, LANE = 4096, 16        # nafcodec_amd/csrc/select.h (kSelTile) and select.hip (16 output bytes per lane): asserted below
# A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H in both cases; S, W, N, '-' and every other byte map to themselves
COMPLEMENT = bytes.maketrans(b"ATCGRYKMBVDHatcgrykmbvdh", b"TAGCYRMKVBHDtagcyrmkvbhd")
COMPLEMENT_RNA = bytes.maketrans(b"AUCGRYKMBVDHaucgrykmbvdh", b"UAGCYRMKVBHDuagcyrmkvbhd")
assert len(COMPLEMENT) == 256 and COMPLEMENT[ord("N")] == ord("N") and COMPLEMENT[ord("U")] == ord("U") and COMPLEMENT_RNA[ord("T")] == ord("T")


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return ec.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "select.h")) as f:
        assert "constexpr uint32_t kSelTile = %d;" % TILE in f.read()
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "select.hip")) as f:
        text = f.read()
        assert "constexpr uint32_t kThreads = %d;" % (TILE // LANE) in text
        assert "static_assert(kSelTile == kThreads * %d" % LANE in text


# ---------------------------------------------------------------- the yardstick
def oracle_records(blob, **opts):
    """-> [(id, comment, sequence, quality or None)] as bytes, what the CPU oracle decodes"""
    return [(r.id or b"", r.comment or b"", r.sequence or b"", r.quality) for r in oracle.Decoder(blob, raw=True, **opts)]


def normal(region):
    """-> (record, start, end or None, '+' | '-')"""
    if not isinstance(region, tuple):
        return region, 0, None, "+"
    return region if len(region) == 4 else region + ("+",)


def cut(records, regions, name_regions=False, table=COMPLEMENT):
    out = []
    for region in regions:
        k, start, end, strand = normal(region)
        id_, com, seq, qual = records[k]
        end = len(seq) if end is None else end
        assert 0 <= start <= end <= len(seq), region
        s, q = seq[start:end], None if qual is None else qual[start:end]
        if strand == "-":
            s, q = s.translate(table)[::-1], None if q is None else q[::-1]
        if name_regions:
            id_ = id_ + b":%d-%d" % (start + 1, end) + (b"/rc" if strand == "-" else b"")
        out.append((id_, com, s, q))
    return out


def ends_of(sizes):
    return np.cumsum(np.array(sizes, dtype=np.uint64), dtype=np.uint64).tobytes() if sizes else b""


def compare(sel, want, fields=("id", "comment", "sequence", "quality"), what=""):
    """every buffer of a Selection against the expected records, byte for byte"""
    n = len(want)
    assert (sel.n_records, sel.n_regions) == (n, n), what
    assert sel.copy_to_host(sel.d_record_end, 8 * n) == ends_of([len(r[2]) for r in want]), (what, "record ends")
    seq = b"".join(r[2] for r in want)
    if "sequence" in fields:
        assert sel.n_bases == len(seq) and sel.d_sequence is not None
        got = sel.copy_to_host(sel.d_sequence, sel.n_bases)
        if got != seq:
            at = next(i for i, (a, b) in enumerate(zip(got, seq)) if a != b)
            raise AssertionError("%s: letter %d of %d differs: %r / %r" % (what, at, len(seq), got[at:at + 20], seq[at:at + 20]))
    else:
        assert (sel.d_sequence, sel.n_bases) == (None, 0), what
    if "quality" in fields:
        assert sel.n_quality == len(seq) and sel.fastq
        assert sel.copy_to_host(sel.d_quality, sel.n_quality) == b"".join(r[3] for r in want), (what, "qualities")
    else:
        assert (sel.d_quality, sel.n_quality, sel.fastq) == (None, 0, False), what
    for field, col, d_ptr, n_bytes, d_end in (("id", 0, sel.d_ids, sel.n_ids_bytes, sel.d_id_end),
                                              ("comment", 1, sel.d_comments, sel.n_comments_bytes, sel.d_comment_end)):
        if field in fields:
            blob = b"".join(r[col] + b"\0" for r in want)
            assert n_bytes == len(blob) and sel.copy_to_host(d_ptr, n_bytes) == blob, (what, field)
            assert sel.copy_to_host(d_end, 8 * n) == ends_of([len(r[col]) + 1 for r in want]), (what, field, "ends")
        else:
            assert (d_ptr, n_bytes, d_end) == (None, 0, None), (what, field)


def check_regions(dec, records, regions, name_regions=False, fields=("id", "comment", "sequence", "quality"), table=COMPLEMENT, what=""):
    want = cut(records, regions, name_regions, table)
    with dec.select(regions, name_regions=name_regions) as sel:
        compare(sel, want, fields, what)
    return want


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


# ---------------------------------------------------------------- 1. the fixtures
def check_phix(lib):
    blob = golden_bytes("phix.naf")
    recs = oracle_records(blob)
    assert len(recs) == 42 and all(r[3] is not None for r in recs) and any(r[2] != r[2].upper() for r in recs)
    n = len(recs)
    with open_decoder(lib, blob) as dec:
        check_regions(dec, recs, list(range(n)), what="whole")
        check_regions(dec, recs, [(k, 0, None, "-") for k in range(n)], what="reverse")
        check_regions(dec, recs, [(k, 3, len(recs[k][2]) - 5) for k in range(n)], what="inner")
        check_regions(dec, recs, [(k, 3, len(recs[k][2]) - 5, "-") for k in range(n)], name_regions=True, what="inner, reverse, named")
        check_regions(dec, recs, list(range(n))[::-1] * 2, what="reversed and doubled")


def check_masked(lib):
    blob = golden_bytes("masked.naf")
    recs = oracle_records(blob)
    assert any(c in r[2] for r in recs for c in b"acgt") and any(c in r[2] for r in recs for c in b"ACGT")
    with open_decoder(lib, blob) as dec:
        regions = [k for k in range(len(recs))] + [(k, 0, None, "-") for k in range(len(recs))] + \
                  [(k, 7, len(recs[k][2]) - 2, s) for k in range(len(recs)) for s in "+-"]
        want = check_regions(dec, recs, regions, fields=("id", "comment", "sequence"), what="masked")
        assert any(c in r[2] for r in want[len(recs):2 * len(recs)] for c in b"acgt")        # lower case survives the reverse strand


def check_protein(lib):
    blob = golden_bytes("LuxC.naf")
    recs = oracle_records(blob)
    with open_decoder(lib, blob) as dec:
        check_regions(dec, recs, [0, (3, 5, 40), (11, 0, None), (3, 0, 1), 3], name_regions=True, fields=("id", "comment", "sequence"), what="LuxC")
        refused(dec, [0, (1, 0, None, "-"), (2, 0, 5, "-")], "region 1:")
        check_regions(dec, recs, [5], fields=("id", "comment", "sequence"), what="LuxC after a refusal")


def check_cp040672(lib, name="CP040672"):
    """the fixture holds 100 coding sequences of 0.2 - 5 kbases: the first record's reverse strand from letter 1 on, five
    overlapping windows at odd offsets on both strands, every record whole and reversed"""
    blob = golden_bytes(name + ".naf")
    recs = oracle_records(blob)
    long_ = max(range(len(recs)), key=lambda k: len(recs[k][2]))
    n = len(recs[long_][2])
    assert len(recs) == 100 and n > TILE
    with open_decoder(lib, blob) as dec:
        regions = [(0, 1, None, "-")] + [(long_, 13 + 577 * i, 13 + 577 * i + n // 2 + 1, "+-"[i & 1]) for i in range(5)] + \
                  list(range(100)) + [(k, 0, None, "-") for k in range(100)]
        check_regions(dec, recs, regions, fields=("id", "comment", "sequence"), what=name)


def check_long_record(lib, n=5_500_003):
    """one record of 5.5 Mbases (written by the host Encoder: no fixture has one): regions more than a thousand tiles long on
    both strands"""
    rng = np.random.default_rng(77)
    blob = ec.host_archive(lib, [Record(id="chr", comment="one long record", sequence=ec.letters(rng, b"ACGTNacgtn", n).decode())], "dna", 1,
                           id=True, comment=True, sequence=True, mask=True)
    recs = oracle_records(blob)
    assert len(recs) == 1 and len(recs[0][2]) == n
    with open_decoder(lib, blob) as dec:
        regions = [(0, 1, None, "-")] + [(0, 13 + 777_777 * i, 13 + 777_777 * i + 1_000_003, "+-"[i & 1]) for i in range(5)]
        check_regions(dec, recs, regions, name_regions=True, fields=("id", "comment", "sequence"), what="long record")


def check_small_fixture(lib, name="NZ_AAEN01000029"):
    blob = golden_bytes(name + ".naf")
    recs = oracle_records(blob)
    with open_decoder(lib, blob) as dec:
        regions = [k for k in range(len(recs))] + [(k, len(recs[k][2]) // 3, None, "-") for k in range(len(recs))]
        check_regions(dec, recs, regions, fields=("id", "comment", "sequence"), what=name)


# ---------------------------------------------------------------- 2. the edges of the gather
EDGE_LENGTHS = (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1)


def edge_archive(lib):
    """64 records of lengths 0 .. 9 000, random IUPAC letters in both cases, written by the host Encoder -> (archive, records)"""
    rng = np.random.default_rng(20241019)
    lengths = [0, 9000, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1] + [int(v) for v in rng.integers(0, 9001, 64 - 11)] + [0, 33]
    assert len(lengths) == 64
    records = [Record(id="e%d" % k, comment="edge %d" % k if k % 3 else "", sequence=ec.letters(rng, b"ACGTRYSWKMBDHVN-acgtryswkmbdhvn", l).decode())
               for k, l in enumerate(lengths)]
    return ec.host_archive(lib, records, "dna", 1, id=True, comment=True, sequence=True, mask=True)


def edge_regions(records):
    """one region list with every case of the issue's check 2, on both strands"""
    lens = [len(r[2]) for r in records]
    big = lens.index(9000)
    regions, pos = [], 0

    def add(record, start, length, strand):
        nonlocal pos
        assert start + length <= lens[record]
        regions.append((record, start, start + length, strand))
        pos += length

    first, last = next(k for k, l in enumerate(lens) if l), max(k for k, l in enumerate(lens) if l)
    assert lens[0] == 0 and first == big and last == len(lens) - 1   # the section begins behind an empty record
    for strand in "+-":
        add(first, 0, 1, strand)                                      # the section's first letter
        add(last, lens[last] - 1, 1, strand)                          # ... and its last one
        for l in EDGE_LENGTHS:
            add(big, 101, l, strand)
        for l in EDGE_LENGTHS[1:]:                                    # whole records of these lengths
            add(lens.index(l), 0, l, strand)
        for r in range(LANE):                                         # the source at every residue mod 16
            add(big, 200 + r, 37, strand)
        add(big, 5, (-pos) % TILE or TILE, strand)                    # ends exactly on an output tile edge
        assert pos % TILE == 0
        add(big, 3, 100, strand)                                      # starts on one
        for i in range(600):                                          # more one-letter regions than a tile has lanes
            add(big, (i * 7) % 9000, 1, "+-"[(i + (strand == "-")) & 1] if i % 3 == 0 else strand)
            if i % 50 == 7:
                add(big, 10, 0, strand)
                add(0, 0, 0, "+")
        for i in range(300):                                          # a run of empty regions, then one letter
            add((i * 5) % len(lens), 0, 0, strand)
        add(big, 8999, 1, strand)
        add(first, 0, lens[first], strand)
        add(last, 0, lens[last], strand)
    assert pos > 4 * TILE
    return regions


def check_edges(lib):
    kernel_constants()
    blob = edge_archive(lib)
    recs = oracle_records(blob)
    fields = ("id", "comment", "sequence")
    with open_decoder(lib, blob) as dec:
        regions = edge_regions(recs)
        check_regions(dec, recs, regions, fields=fields, what="edges")
        check_regions(dec, recs, regions[::-1], fields=fields, name_regions=True, what="edges, reversed list")
        check_regions(dec, recs, [(k % 64, 0, 0, "+-"[k & 1]) for k in range(700)], fields=fields, what="every region empty")
        check_regions(dec, recs, [], fields=fields, what="no region")
        check_regions(dec, recs, list(range(64)), fields=fields, what="every record")
    return blob, recs


# ---------------------------------------------------------------- hand-made archives: raw blocks, no compressor needed
def raw_frame(data):
    """one magicless Zstandard frame of raw blocks"""
    out, at = bytearray(b"\x00\x48"), 0
    while True:
        piece = data[at:at + (128 << 10)]
        at += len(piece)
        last = at >= len(data)
        out += struct.pack("<I", int(last) | (len(piece) << 3))[:3] + piece
        if last:
            return bytes(out)


def varint(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    return bytes(reversed(out))


def length_words(lengths):
    out = bytearray()
    for n in lengths:
        while n >= 0xFFFFFFFF:
            out += struct.pack("<I", 0xFFFFFFFF)
            n -= 0xFFFFFFFF
        out += struct.pack("<I", n)
    return bytes(out)


def hand_archive(n_records, ids=None, comments=None, lengths=None, text=None):
    """a v2 text archive of raw-block sections: ids / comments (lists of bytes, possibly fewer than records), lengths, text"""
    flags, body = 0, b""
    for bit, data in ((0x20, None if ids is None else b"".join(i + b"\0" for i in ids)),
                      (0x10, None if comments is None else b"".join(c + b"\0" for c in comments)),
                      (0x08, None if lengths is None else length_words(lengths)), (0x02, text)):
        if data is not None:
            flags |= bit
            frame = raw_frame(data)
            body += varint(len(data)) + varint(len(frame)) + frame
    return b"\x01\xF9\xEC\x02\x03" + bytes([flags]) + b" " + varint(60) + varint(n_records) + body


# ---------------------------------------------------------------- 3. names
def check_names(lib):
    kernel_constants()
    # START / END of 1, 9, 10, 99, 100 on the edge archive's longest record, on both strands, whole records included
    blob = edge_archive(lib)
    recs = oracle_records(blob)
    big = [len(r[2]) for r in recs].index(9000)
    regions = [(big, a - 1, b, s) for a, b in ((1, 1), (1, 9), (9, 10), (10, 99), (99, 100), (100, 100), (1, 9000)) for s in "+-"] + [big, 0, 2]
    with open_decoder(lib, blob) as dec:
        want = check_regions(dec, recs, regions, name_regions=True, fields=("id", "comment", "sequence"), what="names")
        assert [w[0] for w in want[:4]] == [b"e1:1-1", b"e1:1-1/rc", b"e1:1-9", b"e1:1-9/rc"] and want[-3][0] == b"e1:1-9000" and want[-2][0] == b"e0:1-0"
        check_regions(dec, recs, regions, fields=("id", "comment", "sequence"), what="the same regions, not named")
    # a record of 10^10 + 7 letters exists only in the Length section: opened without the sequence, the strings alone
    huge = 10 ** 10 + 7
    blob = hand_archive(3, ids=[b"a", b"chrBig", b"c"], comments=[b"", b"a big one", b"x"], lengths=[5, huge, 12])
    recs = [(b"a", b"", b"", None), (b"chrBig", b"a big one", b"", None), (b"c", b"x", b"", None)]
    regions = [(1, 10 ** 10 - 1, None, "+"), (1, 10 ** 10, huge), (1, 0, None), (0, 4, 5), (2, 9, 10)]
    want_ids = [b"chrBig:10000000000-10000000007", b"chrBig:10000000001-10000000007", b"chrBig:1-10000000007", b"a:5-5", b"c:10-10"]
    with open_decoder(lib, blob, sequence=False) as dec:
        with dec.select(regions, name_regions=True) as sel:
            assert sel.copy_to_host(sel.d_ids, sel.n_ids_bytes) == b"".join(i + b"\0" for i in want_ids)
            assert sel.copy_to_host(sel.d_id_end, 8 * 5) == ends_of([len(i) + 1 for i in want_ids])
            assert sel.copy_to_host(sel.d_comments, sel.n_comments_bytes) == b"a big one\0a big one\0a big one\0\0x\0"
            assert sel.copy_to_host(sel.d_record_end, 8 * 5) == ends_of([8, 7, huge, 1, 1])
            assert (sel.d_sequence, sel.n_bases, sel.d_quality) == (None, 0, None)
            try:
                sel.format_device()
            except ValueError:
                pass
            else:
                raise AssertionError("text of a selection without letters")
        refused(dec, [(1, huge, huge + 1)], "region 0:")
    # fewer id / comment strings than records: the missing ones are empty
    text = b"AAAACCCCCGGGGGGTTTTTTT"
    blob = hand_archive(4, ids=[b"r0", b"r1"], comments=[b"only one"], lengths=[4, 5, 6, 7], text=text)
    recs = [(b"r0", b"only one", text[0:4], None), (b"r1", b"", text[4:9], None), (b"", b"", text[9:15], None), (b"", b"", text[15:22], None)]
    with open_decoder(lib, blob) as dec:
        assert dec.decode_all_device().n_ids == 2
        for named in (False, True):
            want = check_regions(dec, recs, [3, (2, 1, 4), 1, 0, (3, 0, 0)], name_regions=named, fields=("id", "comment", "sequence"), what="beyond the id count")
        assert [w[0] for w in want] == [b":1-7", b":2-4", b"r1:1-5", b"r0:1-4", b":1-0"]


# ---------------------------------------------------------------- 4. find_records
def call_find(lib, dec, blob, n_names):
    out, err = (ctypes.c_uint64 * max(n_names, 1))(), _ffi.Error()
    rc = lib.c.nafgpu_find_records(dec._h, blob, len(blob), n_names, out, ctypes.byref(err))
    return rc, list(out[:n_names]), err.message.decode("utf-8", "replace")


def check_find(lib):
    blob = golden_bytes("phix.naf")
    ids = [r[0] for r in oracle_records(blob)]
    assert len(set(ids)) == len(ids) == 42
    rng = np.random.default_rng(4)
    with open_decoder(lib, blob) as dec:
        order = [int(k) for k in rng.permutation(len(ids))]
        assert dec.find([ids[k] for k in order]) == order
        assert dec.find([ids[k].decode() for k in order[:5]]) == order[:5]
        probes = [b"no such read", b"", ids[7][:-1], ids[7] + b"x", ids[7], b"\xff" * 40, ids[0], ids[0]]
        assert dec.find(probes) == [None, None, None, None, 7, None, 0, 0]
        assert dec.find([]) == []
        with dec.select([ids[3].decode(), (ids[5], 2, 9, "-"), 3]) as sel:               # names in the place of indices
            compare(sel, cut(oracle_records(blob), [3, (5, 2, 9, "-"), 3]), what="select by name")
        try:
            dec.select([b"no such read"])
        except KeyError:
            pass
        else:
            raise AssertionError("a missing name was accepted")
        # the blob itself: a missing NUL, a NUL too many, a count that disagrees
        for bad, n in ((b"abc", 1), (b"abc\0def", 2), (b"abc\0", 2), (b"abc\0\0", 1), (b"", 1)):
            rc, _, message = call_find(lib, dec, bad, n)
            assert rc == _ffi.E_INVALID_ARG and "NUL" in message, (bad, rc, message)
        assert call_find(lib, dec, b"\0" + ids[2] + b"\0", 2)[:2] == (_ffi.OK, [_ffi.NOT_FOUND, 2])
    with open_decoder(lib, blob, id=False) as dec:                                       # the ids were not decoded
        rc, _, message = call_find(lib, dec, b"abc\0", 1)
        assert rc == _ffi.E_INVALID_ARG and "ids" in message
        try:
            dec.find(["abc"])
        except ValueError:
            pass
        else:
            raise AssertionError("find without ids")
    # duplicated ids (the empty id among them): the lowest index wins; more ids than a workgroup has lanes
    names = [b"dup", b"x1", b"dup", b"", b"x2", b"", b"dup"] + [b"n%d" % (k % 500) for k in range(1300)]
    blob = hand_archive(len(names), ids=names, lengths=[1] * len(names), text=b"A" * len(names))
    with open_decoder(lib, blob) as dec:
        want = {}
        for k, name in enumerate(names):
            want.setdefault(name, k)
        probes = sorted(want) + [b"n500", b"du", b"dupp"]
        assert dec.find(probes) == [want.get(p) for p in probes]
        assert want[b"dup"] == 0 and want[b""] == 3 and want[b"n499"] == 7 + 499


def check_find_colliding(lib):
    """the same lookups with the hash cut to 2 bits: every id in one of four probe chains (after nafgpu_test_hooks(1); the
    caller runs this in a process of its own)"""
    os.environ["NAFGPU_SEL_HASH_BITS"] = "2"
    lib.c.nafgpu_test_hooks(1)
    check_find(lib)


# ---------------------------------------------------------------- 5. refusals
def call_select(lib, dec, regions, name_regions=0):
    """the C entry point itself -> (status, message, io kind); with an error no handle and a zeroed result"""
    arr = (_ffi.Region * max(len(regions), 1))()
    for k, (record, start, end, rc) in enumerate(regions):
        arr[k].record, arr[k].start, arr[k].end, arr[k].reverse_complement = record, start, _ffi.REGION_END if end is None else end, rc
    opts = _ffi.SelectOpts(name_regions=name_regions)
    h, res, err = ctypes.c_void_p(), _ffi.SelectResult(), _ffi.Error()
    rc = lib.c.nafgpu_select(dec._h, arr, len(regions), ctypes.byref(opts), ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_selection_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def refused(dec, regions, needle):
    try:
        dec.select(regions)
    except ValueError as e:
        assert needle in str(e), (needle, str(e))
    else:
        raise AssertionError("accepted: %r" % (regions[:4],))


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    recs = oracle_records(blob)
    l5 = len(recs[5][2])
    with open_decoder(lib, blob) as dec:
        good = [(k, 0, None, 0) for k in range(42)]
        assert call_select(lib, dec, good)[0] == _ffi.OK
        for bad in ((42, 0, None, 0), (2 ** 40, 0, 0, 0), (5, l5 + 1, None, 0), (5, 7, 6, 0), (5, 0, l5 + 1, 0), (5, l5, l5 + 1, 1), (5, 2 ** 63, 2 ** 63 + 5, 0)):
            for at in (0, 17, 41):
                regions = good[:at] + [bad] + good[at + 1:]
                rc, message, _ = call_select(lib, dec, regions)
                assert rc == _ffi.E_INVALID_ARG and message.startswith("region %d:" % at), (bad, at, rc, message)
        assert call_select(lib, dec, [(5, l5, None, 1), (5, l5, l5, 0), (5, 0, l5, 1)])[0] == _ffi.OK      # the record's end is a valid (empty) slice
        # several offenders: the lowest index is named, wherever the others are
        many = good * 30
        for at in (1259, 700, 64, 3):
            many[at] = (at % 42, 10 ** 6, None, 0)
            rc, message, _ = call_select(lib, dec, many)
            assert rc == _ffi.E_INVALID_ARG and message.startswith("region %d:" % at), (at, message)
        check_regions(dec, recs, [4, (5, 1, 9, "-")], what="after the refusals")                           # and the decoder is as good as before
        for bad in ([(0, 1)], [(0, 1, 2, "x")], [(0, -1, 2)], [-1]):                                       # the Python mirror's own checks
            refused(dec, bad, "")
    with open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _ = call_select(lib, dec, [(0, 0, None, 0)])
        assert rc == _ffi.E_INVALID_ARG and "shard" in message
        refused(dec, [0], "shard")
    # without the sequence: ids, comments, qualities and record ends of the regions
    with open_decoder(lib, blob, sequence=False) as dec:
        check_regions(dec, recs, [2, (3, 4, 50, "-")], fields=("id", "comment", "quality"), what="sequence=False")
    with open_decoder(lib, blob, id=False, comment=False, quality=False, mask=False) as dec:
        check_regions(dec, oracle_records(blob, mask=False), [2, (3, 4, 50, "-")], fields=("sequence",), what="sequence alone")
    # no Length section
    with open_decoder(lib, hand_archive(1, ids=[b"a"], text=b"ACGT")) as dec:
        rc, message, _ = call_select(lib, dec, [(0, 0, None, 0)])
        assert rc == _ffi.E_INVALID_ARG and "Length" in message, message
    # lengths that promise more than the sequence holds: the records inside it are served, the one beyond is an EOF
    with open_decoder(lib, hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 4], text=b"ACGTACGTAC")) as dec:
        rc, message, kind = call_select(lib, dec, [(0, 0, None, 0), (1, 1, 3, 0), (2, 0, 1, 0), (1, 0, None, 0)])
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "region 2" in message, (rc, kind, message)
        try:
            dec.select([2])
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")
        with dec.select([1, (0, 1, None)]) as sel:
            assert sel.copy_to_host(sel.d_sequence, sel.n_bases) == b"ACGTCGT"


# ---------------------------------------------------------------- 6. composition
def fasta(records, line_length):
    out = []
    for id_, com, seq, qual in records:
        head = id_ + (b" " + com if com else b"")
        if qual is not None:
            out.append(b"@" + head + b"\n" + seq + b"\n+\n" + qual + b"\n")
        else:
            width = line_length or len(seq) or 1
            out.append(b">" + head + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width)))
    return b"".join(out)


def as_records(tuples):
    return [Record(id=i.decode("latin-1"), comment=c.decode("latin-1"), sequence=s.decode("latin-1"),
                   quality=None if q is None else q.decode("latin-1"), length=len(s)) for i, c, s, q in tuples]


def check_composition(lib):
    import text_parse_checks as tc
    for name, regions in (("phix", [3, (7, 5, 250, "-"), (7, 5, 250), 41, (0, 0, 0), 3]), ("masked", [(0, 3, None, "-"), 1, (1, 2, 30), (0, 0, 0)])):
        blob = golden_bytes(name + ".naf")
        recs = oracle_records(blob)
        fastq = recs[0][3] is not None
        want = cut(recs, regions, name_regions=True)
        dec = open_decoder(lib, blob)
        sel = dec.select(regions, name_regions=True)
        dec.close()                                                    # the selection is a copy: it outlives the decoder
        with sel:
            compare(sel, want, ("id", "comment", "sequence") + (("quality",) if fastq else ()), name)
            got = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, quality=fastq, mask=True, compression_level=1,
                                device=0, _lib=lib)
            host = ec.host_archive(lib, as_records(want), "dna", 1, id=True, comment=True, sequence=True, quality=fastq, mask=True)
            assert got == host, (name, "encode_device of a selection")
            assert oracle_records(got, spec_mask=True) == want, (name, "the oracle's reading of the new archive")
            for line_length in (60, 0, 7):
                assert sel.to_text(line_length) == fasta(want, line_length), (name, line_length)
            assert sel.to_text() == sel.to_text(60)
            text = sel.format_device()
            assert (text.n_records, bool(text.fastq)) == (len(want), fastq)
            assert sel.hash_device(text.d_text, text.n_text) == lib.c.nafgpu_hash64_host(fasta(want, 60), text.n_text)
            with parse_text(text.d_text, text.n_text, device=0, _lib=lib) as p:
                assert tc.device_records(p) == want, (name, "parse_text of the selection's text")
        try:
            sel.to_text()
        except RuntimeError:
            pass
        else:
            raise AssertionError("a closed selection was used")
    # an RNA archive: A <-> U, and T is no letter of it
    rna = [Record(id="r", comment="", sequence="ACGUNNRYKMacguBVDHSW-")]
    blob = ec.host_archive(lib, rna, "rna", 1, id=True, comment=True, sequence=True, mask=True)
    recs = oracle_records(blob)
    with open_decoder(lib, blob) as dec:
        want = check_regions(dec, recs, [(0, 0, None, "-"), 0], fields=("id", "comment", "sequence"), table=COMPLEMENT_RNA, what="rna")
        assert want[0][2] == b"-WSDHBVacguKMRYNNACGU" and want[0][2] == recs[0][2].translate(COMPLEMENT_RNA)[::-1]


# ---------------------------------------------------------------- 9. output positions past 2^32 (MI355X only)
def check_past_u32(lib, n_bases=2 ** 28, copies=17):
    arc = lib.synth(n_bases, seed=31, with_mask=True, iupac_permille=5)
    try:
        dec = open_decoder(lib, ctypes.string_at(arc.bytes, arc.n))
        try:
            res = dec.decode_all_device()
            assert (res.n_bases, res.n_records) == (n_bases, arc.n_records) and n_bases % 4096 == 0
            src_ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
            want_hash = sum(dec.hash_device(res.d_sequence, n_bases, first_chunk=k * (n_bases // 4096)) for k in range(copies)) % 2 ** 64
            with dec.select(list(range(res.n_records)) * copies) as sel:
                print("select past 2^32: %d regions, %d letters, %.3f ms" % (sel.n_regions, sel.n_bases, sel.ms))
                assert sel.n_bases == copies * n_bases > 2 ** 32 and sel.n_records == copies * res.n_records
                assert sel.hash_device(sel.d_sequence, sel.n_bases) == want_hash
                ends = np.frombuffer(sel.copy_to_host(sel.d_record_end, 8 * sel.n_records), dtype=np.uint64)
                want_ends = (np.tile(src_ends, copies) + np.repeat(np.arange(copies, dtype=np.uint64) * np.uint64(n_bases), res.n_records))
                assert int(ends[-1]) == copies * n_bases and np.array_equal(ends, want_ends)
        finally:
            dec.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))
