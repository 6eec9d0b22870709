"""Shared by tests/test_summary_emu.py (CPU harness) and tests/test_gpu_summary.py (MI355X): Decoder.summarize,
Selection.summarize, ParsedText.summarize and summarize(), records in device memory -> class counts and a quality sum per
record and a histogram per section.  Not a test module; every function takes the library binding it is to check.

The yardstick is numpy over what the CPU oracle decodes (or over a selection's own bytes read back): np.add.reduceat over
((table[letters] >> c) & 1) per column, np.bincount(letters, minlength=256), the same over the quality bytes.  Every table
is compared for equality as uint64: integer work, no tolerance."""
import ctypes
import io
import os

import numpy as np

import encode_checks as ec
import select_checks as sc
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi, summary as sm
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Record, encode_text, parse_text
from oracle import oracle

ENTRY_POINTS = ("nafgpu_summarize", "nafgpu_summarize_decoder", "nafgpu_summary_copy_to_host", "nafgpu_summary_free")
TILE, LANE, RUN = 4096, 16, 16       # nafcodec_amd/csrc/summary.h (kSumTile, kSumRun) and summary.hip (16 bytes per lane): asserted below
ROUTES = ("long", "short")           # NAFGPU_SUM_ROUTE
DEFAULT = np.frombuffer(sm.DEFAULT_CLASSES, dtype=np.uint8)
# a table whose columns overlap: 0 hydrophobic, 1 aromatic (all of them in 0 or 2 as well), 2 charged, 3 every upper-case
# letter, 4 '*', 5 M (also in 0), 6 nothing, 7 every byte
OVERLAP = np.zeros(256, dtype=np.uint8)
for _c, _letters in ((0, b"AVILMFWY"), (1, b"FWYH"), (2, b"DEKRH"), (3, bytes(range(65, 91))), (4, b"*"), (5, b"M"), (7, bytes(range(256)))):
    for _b in _letters:
        OVERLAP[_b] |= 1 << _c


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sc.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "summary.h")) as f:
        text = f.read()
        assert "constexpr uint32_t kSumTile = %d;" % TILE in text and "constexpr uint32_t kSumRun = %d;" % RUN in text
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "summary.hip")) as f:
        text = f.read()
        assert "constexpr uint32_t kThreads = %d;" % (TILE // LANE) in text
        assert "static_assert(kSumTile == kThreads * %d" % LANE in text


def check_default_table():
    """the table of include/nafgpu.h, written out: one of columns 0-6 for every byte, column 7 for a..z beside it"""
    t = sm.DEFAULT_CLASSES
    assert (sm.A, sm.C, sm.G, sm.T, sm.N, sm.IUPAC, sm.OTHER, sm.LOWER) == tuple(range(8)) and len(t) == 256
    for b in range(256):
        col = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3, "N": 4}.get(chr(b).upper(), 5 if chr(b).upper() in "RYKMSWBDHV" else 6)
        assert t[b] == (1 << col) | (128 if 97 <= b <= 122 else 0), b
    assert t[ord("-")] == 64 and t[ord("u")] == 8 | 128 and t[0] == 64


# ---------------------------------------------------------------- the yardstick
def per_record(values, ends):
    """np.add.reduceat of `values` over the records that `ends` (inclusive prefix sums) cut; empty records give 0"""
    ends = np.asarray(ends, dtype=np.int64)
    out = np.zeros(len(ends), dtype=np.uint64)
    if len(ends):
        starts = np.concatenate(([0], ends[:-1]))
        full = ends > starts
        if full.any():
            out[full] = np.add.reduceat(values[:ends[-1]].astype(np.uint64), starts[full])
    return out


def expected(letters, quals, ends, table=DEFAULT):
    """-> counts (n x 8) or None, quality sums or None, letter histogram or None, quality histogram or None; all uint64"""
    counts = qsum = lhist = qhist = None
    if letters is not None:
        l = np.frombuffer(letters, dtype=np.uint8)
        classes = np.asarray(table, dtype=np.uint8)[l]
        counts = np.stack([per_record((classes >> c) & 1, ends) for c in range(8)], axis=1) if len(ends) else None
        lhist = np.bincount(l, minlength=256).astype(np.uint64)
    if quals is not None:
        q = np.frombuffer(quals, dtype=np.uint8)
        qsum = per_record(q, ends) if len(ends) else None
        qhist = np.bincount(q, minlength=256).astype(np.uint64)
    return counts, qsum, lhist, qhist


def table_of(view, shape=None):
    if view is None:
        return None
    a = np.frombuffer(view, dtype=np.uint64)
    return a.reshape(shape) if shape else a


def compare(s, letters, quals, ends, table=DEFAULT, what=""):
    """every table of a Summary against numpy"""
    counts, qsum, lhist, qhist = expected(letters, quals, ends, table)
    n = len(ends)
    assert s.n_records == n and s.n_bases == (len(letters) if letters is not None else 0) and s.n_quality == (len(quals) if quals is not None else 0), what
    for name, got, want in (("counts", table_of(s.counts(), (-1, 8)), counts), ("quality_sum", table_of(s.quality_sum()), qsum),
                            ("letter_hist", table_of(s.letter_hist()), lhist), ("quality_hist", table_of(s.quality_hist()), qhist)):
        if want is None:
            assert got is None or got.size == 0, (what, name)
            continue
        assert got is not None and got.dtype == np.uint64 and got.shape == want.shape, (what, name, None if got is None else got.shape, want.shape)
        if not np.array_equal(got, want):
            at = np.argwhere(got != want)[0]
            raise AssertionError("%s: %s differs at %s: %s / %s (%d entries differ)" % (what, name, at, got[tuple(at)], want[tuple(at)], (got != want).sum()))
    covered = n and int(ends[-1]) == (len(letters) if letters is not None else len(quals))
    if counts is not None:
        want_totals = counts.sum(axis=0, dtype=np.uint64)
        assert np.array_equal(np.array(s.totals, dtype=np.uint64), want_totals), (what, "totals", s.totals, want_totals)
        if covered:
            assert all(int(want_totals[c]) == int(lhist[((np.asarray(table) >> c) & 1) == 1].sum()) for c in range(8)), (what, "totals / histogram")
        if table is DEFAULT:                                                    # columns 0-6 are a partition of the byte values
            lengths = np.diff(np.concatenate(([0], np.asarray(ends, dtype=np.uint64)))).astype(np.uint64)
            assert np.array_equal(table_of(s.counts(), (-1, 8))[:, :7].sum(axis=1, dtype=np.uint64), lengths), (what, "columns 0-6 / lengths")
    if qsum is not None:
        assert s.quality_total == int(qsum.sum(dtype=np.uint64)), (what, "quality_total")


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


def records_layout(recs, with_quality=True):
    """oracle records -> letters, qualities or None, ends"""
    letters = b"".join(r[2] for r in recs)
    quals = b"".join(r[3] for r in recs) if with_quality and recs and recs[0][3] is not None else None
    ends = np.cumsum([len(r[2]) for r in recs], dtype=np.uint64) if recs else np.zeros(0, dtype=np.uint64)
    return letters, quals, ends


def selection_layout(sel):
    """a Selection's (or ParsedText's) own bytes read back -> letters, qualities or None, ends"""
    letters = sel.copy_to_host(sel.d_sequence, sel.n_bases) if sel.d_sequence else None
    quals = sel.copy_to_host(sel.d_quality, sel.n_quality) if sel.d_quality else None
    ends = np.frombuffer(sel.copy_to_host(sel.d_record_end, 8 * sel.n_records), dtype=np.uint64)
    return letters, quals, ends


# ---------------------------------------------------------------- 1. the fixtures
def check_fixtures(lib):
    for name in ("phix", "masked", "LuxC", "CP040672", "NZ_AAEN01000029"):
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob)
        letters, quals, ends = records_layout(recs)
        with open_decoder(lib, blob) as dec:
            s = dec.summarize()
        with s:                                                                 # a summary outlives its source
            compare(s, letters, quals, ends, what=name)
            counts = table_of(s.counts(), (-1, 8))
            lower = np.array([sum(97 <= b <= 122 for b in r[2]) for r in recs], dtype=np.uint64)
            assert np.array_equal(counts[:, sm.LOWER], lower), name
            if name == "phix":
                assert quals is not None and lower.sum() > 0 and s.quality_total == sum(quals)
            if name == "masked":
                assert 0 < lower.sum() < len(letters)
            if name == "LuxC":                                                  # a protein under the nucleotide table: most of it is "other"
                assert counts[:, sm.OTHER].sum() > 0 and s.totals[sm.LOWER] == 0
        try:
            s.counts()
        except RuntimeError:
            pass
        else:
            raise AssertionError("a closed summary was used")
    blob = golden_bytes("LuxC.naf")
    letters, quals, ends = records_layout(sc.oracle_records(blob))
    with open_decoder(lib, blob) as dec, dec.summarize(classes=OVERLAP.tobytes()) as s:
        compare(s, letters, quals, ends, table=OVERLAP, what="LuxC, overlapping columns")
        assert s.totals[7] == len(letters) and s.totals[6] == 0 and 0 < s.totals[5] <= s.totals[0] and s.totals[1] > 0
    for bad in (b"", bytes(255), bytes(257)):
        try:
            sm.summarize(None, bad, _lib=lib)
        except ValueError:
            pass
        else:
            raise AssertionError("a table of %d bytes was accepted" % len(bad))


# ---------------------------------------------------------------- 2. the edges
def edge_selections(recs):
    """named region lists over the edge archive (select_checks.edge_archive): every case of the issue's check 2"""
    lens = [len(r[2]) for r in recs]
    big = lens.index(9000)
    out = {}
    regions, pos = [], 0

    def add(record, start, length):
        nonlocal pos
        assert start + length <= lens[record]
        regions.append((record, start, start + length))
        pos += length

    for l in sc.EDGE_LENGTHS:                                 # 0, 1, 15, 16, 17, tile - 1, tile, tile + 1
        add(big, 101, l)
    for r in range(LANE):                                     # records that start at every residue mod 16
        add(big, 200 + r, 16 + r + (1 if r % 3 == 0 else 0))
    add(big, 5, (-pos) % TILE or TILE)                        # ends exactly on a tile edge
    assert pos % TILE == 0
    add(big, 3, TILE)                                         # begins and ends on one
    add(big, 3, 100)                                          # begins on one
    for i in range(600):                                      # more one-letter records than a tile has lanes, empty ones among them
        add(big, (i * 7) % 9000, 1)
        if i % 50 == 7:
            add(big, 10, 0)
            add(0, 0, 0)
    for i in range(300):                                      # a run of empty records, then one letter
        add((i * 5) % len(lens), 0, 0)
    add(big, 8999, 1)
    for i in range(40):                                       # short ones, one record of a few tiles, short ones again
        add(big, 11 * i, 90 + i)
    add(big, 0, 9000)
    for i in range(40):
        add(big, 13 * i, 1 + 3 * i)
    add(big, 0, 9000)                                         # two long ones side by side, the run's last
    add(big, 1, 8999)
    for i in range(4):                                        # and into the next workgroup's run
        add(big, i, 9000 - i)
        add(0, 0, 0)
    assert pos > RUN * TILE                                   # more than one workgroup
    out["edges"] = regions
    out["edges, reversed list"] = regions[::-1]
    out["empty records in front"] = [(k % 64, 0, 0) for k in range(700)] + [(big, 7, 8)] + [(3, 0, 0)] * 5
    out["every record empty"] = [(k % 64, 0, 0) for k in range(700)]
    out["no record"] = []
    out["every record"] = list(range(64))
    out["one letter"] = [(big, 77, 78)]
    return out


def check_edges(lib):
    kernel_constants()
    blob = sc.edge_archive(lib)
    recs = sc.oracle_records(blob)
    assert recs[0][2] == b"" and any(not r[2] for r in recs[1:-1])             # empty records at the front and inside
    with open_decoder(lib, blob) as dec:
        letters, quals, ends = records_layout(recs)
        with dec.summarize() as s:
            compare(s, letters, quals, ends, what="the edge archive")
        for what, regions in edge_selections(recs).items():
            with dec.select(regions) as sel:
                got = selection_layout(sel)
                assert got[0] == b"".join(r[2] for r in sc.cut(recs, regions)), what
                with sel.summarize() as s:
                    compare(s, *got, what=what)
                if what == "edges":
                    with sm.summarize(sel, OVERLAP.tobytes(), _lib=lib) as s:
                        compare(s, *got, table=OVERLAP, what=what + ", another table")
    # qualities through the same edges: the reads of phix cut and repeated
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    with open_decoder(lib, blob) as dec:
        regions = [(k % 42, k % 7, len(recs[k % 42][2]) - k % 5) for k in range(300)] + [(1, 0, 0)] * 3 + [(k, 0, 1) for k in range(42)]
        with dec.select(regions) as sel, sel.summarize() as s:
            got = selection_layout(sel)
            assert got[1] is not None and len(got[0]) > 2 * TILE
            compare(s, *got, what="phix, cut and repeated")


# ---------------------------------------------------------------- 3. one long record
def check_long_record(lib, n=5_500_003):
    rng = np.random.default_rng(78)
    blob = ec.host_archive(lib, [Record(id="chr", comment="", sequence=ec.letters(rng, b"ACGTNacgtnRY-", n).decode())], "dna", 1,
                           id=True, comment=True, sequence=True, mask=True)
    recs = sc.oracle_records(blob)
    assert len(recs) == 1 and len(recs[0][2]) == n
    letters = recs[0][2]
    with open_decoder(lib, blob) as dec:
        with dec.summarize() as s:
            compare(s, letters, None, np.array([n], dtype=np.uint64), what="one long record")
            whole = table_of(s.counts(), (-1, 8)).copy()
        regions = [(0, at, min(at + 100, n)) for at in range(0, n, 100)]
        with dec.select(regions) as sel, sel.summarize() as s:
            ends = np.frombuffer(sel.copy_to_host(sel.d_record_end, 8 * sel.n_records), dtype=np.uint64)
            assert len(ends) == (n + 99) // 100 and int(ends[-1]) == n
            compare(s, letters, None, ends, what="the same letters in records of 100")
            assert np.array_equal(table_of(s.counts(), (-1, 8)).sum(axis=0, dtype=np.uint64), whole[0])


# ---------------------------------------------------------------- 4. a read set
def read_set(n_reads=3000, seed=5):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 301, n_reads)
    lengths[:3] = (0, 300, 0)
    out = []
    for k, l in enumerate(lengths):
        seq = ec.letters(rng, b"ACGTNacgt", int(l))
        qual = bytes(rng.integers(33, 127, int(l), dtype=np.uint8))
        out.append(b"@r%d\n" % k + seq + b"\n+\n" + qual + b"\n")
    text = b"".join(out)
    assert set(range(33, 127)) <= set(text)
    return text, [int(l) for l in lengths]


def check_read_set(lib):
    text, lengths = read_set()
    with parse_text(text, device=0, _lib=lib) as parsed:
        assert parsed.fastq and parsed.n_records == len(lengths)
        got = selection_layout(parsed)
        assert [int(e) for e in got[2]] == [int(v) for v in np.cumsum(lengths)]
        with parsed.summarize() as s:
            compare(s, *got, what="read set")
            mine = [bytes(v) for v in (s.counts(), s.quality_sum(), s.letter_hist(), s.quality_hist())] + [s.totals, s.quality_total]
    blob = encode_text(text, sequence_type="dna", mask=True, device=0, _lib=lib)
    with open_decoder(lib, blob, spec_mask=True) as dec, dec.summarize() as s:   # (spec_mask: every masked letter lower case, as in the text)
        compare(s, *got, what="read set, encoded and decoded")
        assert mine == [bytes(v) for v in (s.counts(), s.quality_sum(), s.letter_hist(), s.quality_hist())] + [s.totals, s.quality_total]


# ---------------------------------------------------------------- 5. every route
def check_route(lib, route):
    """checks 1-4 with NAFGPU_SUM_ROUTE forcing one route on every tile (after nafgpu_test_hooks(1); the caller runs this in a
    process of its own)"""
    assert route in ROUTES
    os.environ["NAFGPU_SUM_ROUTE"] = route
    lib.c.nafgpu_test_hooks(1)
    check_fixtures(lib)
    check_edges(lib)
    check_long_record(lib)
    check_read_set(lib)


def check_route_long(lib):
    check_route(lib, "long")


def check_route_short(lib):
    check_route(lib, "short")


# ---------------------------------------------------------------- 6. refusals
class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def call_summarize(lib, src_fields, device=0):
    src = _ffi.EncodeSource(**src_fields)
    h, res, err = ctypes.c_void_p(), _ffi.SummaryResult(), _ffi.Error()
    rc = lib.c.nafgpu_summarize(ctypes.byref(src), None, device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_summary_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_summarize_decoder(lib, dec):
    h, res, err = ctypes.c_void_p(), _ffi.SummaryResult(), _ffi.Error()
    rc = lib.c.nafgpu_summarize_decoder(dec._h, None, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_summary_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, quals, ends = records_layout(recs)
    with open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_quality=res.d_quality, n_quality=res.n_quality, d_record_end=res.d_record_end,
                    n_records=res.n_records)
        assert call_summarize(lib, good)[0] == _ffi.OK
        # both sections absent
        assert call_summarize(lib, dict(d_record_end=res.d_record_end, n_records=res.n_records))[0] == _ffi.E_INVALID_ARG
        assert call_summarize(lib, {})[0] == _ffi.E_INVALID_ARG
        # n_quality != n_bases
        rc, message = call_summarize(lib, dict(good, n_quality=res.n_quality - 1))
        assert rc == _ffi.E_INVALID_LENGTH and str(res.n_quality - 1) in message, (rc, message)
        # null arguments
        src, h, r, err = _ffi.EncodeSource(**good), ctypes.c_void_p(), _ffi.SummaryResult(), _ffi.Error()
        assert lib.c.nafgpu_summarize(None, None, 0, ctypes.byref(h), ctypes.byref(r), ctypes.byref(err)) == _ffi.E_INVALID_ARG
        assert lib.c.nafgpu_summarize(ctypes.byref(src), None, 0, None, ctypes.byref(r), ctypes.byref(err)) == _ffi.E_INVALID_ARG
        assert lib.c.nafgpu_summarize(ctypes.byref(src), None, 0, ctypes.byref(h), None, ctypes.byref(err)) == _ffi.E_INVALID_ARG
        for bad in (Source(), Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_quality=res.d_quality, n_quality=3)):
            try:
                sm.summarize(bad, _lib=lib)
            except ValueError:
                pass
            else:
                raise AssertionError("accepted")
        # one section alone, and without a record table: histograms only
        with sm.summarize(Source(d_quality=res.d_quality, n_quality=res.n_quality, d_record_end=res.d_record_end, n_records=res.n_records), _lib=lib) as s:
            compare(s, None, quals, ends, what="qualities alone")
        with sm.summarize(Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=0), _lib=lib) as s:
            compare(s, letters, None, ends[:0], what="no records")
            assert s.counts() is None and sum(s.totals[:7]) == len(letters)
        # letters behind the last record end count in the histograms only
        with sm.summarize(Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_quality=res.d_quality, n_quality=res.n_quality,
                                 d_record_end=res.d_record_end, n_records=res.n_records - 5), _lib=lib) as s:
            compare(s, letters, quals, ends[:-5], what="letters behind the last record")
            assert sum(s.totals[:7]) == int(ends[-6]) < len(letters)
        with dec.summarize() as s:                                              # and the decoder is as good as before
            compare(s, letters, quals, ends, what="after the refusals")
    # a decoder opened without sequence and quality
    with open_decoder(lib, blob, sequence=False, quality=False) as dec:
        rc, message, _ = call_summarize_decoder(lib, dec)
        assert rc == _ffi.E_INVALID_ARG and "sequence" in message, (rc, message)
        try:
            dec.summarize()
        except ValueError:
            pass
        else:
            raise AssertionError("a summary without letters and qualities")
    with open_decoder(lib, blob, sequence=False) as dec, dec.summarize() as s:
        compare(s, None, quals, ends, what="sequence=False")
    with open_decoder(lib, blob, quality=False) as dec, dec.summarize() as s:
        compare(s, letters, None, ends, what="quality=False")
    # a shard
    with open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _ = call_summarize_decoder(lib, dec)
        assert rc == _ffi.E_INVALID_ARG and "shard" in message, (rc, message)
    # no Length section: histograms only
    with open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"ACGTTTnn")) as dec, dec.summarize() as s:
        compare(s, b"ACGTTTnn", None, np.zeros(0, dtype=np.uint64), what="no Length section")
        assert s.totals == (1, 1, 1, 3, 2, 0, 0, 2)
    # lengths that promise more than the sequence holds: an archive that ends early
    with open_decoder(lib, sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 4], text=b"ACGTACGTAC")) as dec:
        rc, message, kind = call_summarize_decoder(lib, dec)
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 2" in message, (rc, kind, message)
        try:
            dec.summarize()
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")


# ---------------------------------------------------------------- 7. positions and counters past 2^32 (MI355X only)
def check_past_u32(lib, n_bases=2 ** 28, copies=17):
    import torch
    arc = lib.synth(n_bases, seed=31, with_mask=True, iupac_permille=5)
    try:
        dec = open_decoder(lib, ctypes.string_at(arc.bytes, arc.n))
        try:
            res = dec.decode_all_device()
            assert (res.n_bases, res.n_records) == (n_bases, arc.n_records)
            letters = dec.copy_to_host(res.d_sequence, n_bases)                 # the 256 MB, read back once
            ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
            with dec.summarize() as s:
                print("summarize: %d records, %d letters, %.3f ms" % (s.n_records, s.n_bases, s.ms))
                compare(s, letters, None, ends, what="2^28 letters")
                rows, hist, totals = table_of(s.counts(), (-1, 8)).copy(), table_of(s.letter_hist()).copy(), s.totals
                assert totals[sm.LOWER] > 0 and totals[sm.IUPAC] > 0
            del letters
            with dec.select(list(range(res.n_records)) * copies) as sel:
                assert sel.n_bases == copies * n_bases > 2 ** 32
                with sel.summarize() as s:
                    print("summarize past 2^32: %d records, %d letters, %.3f ms" % (s.n_records, s.n_bases, s.ms))
                    assert s.n_records == copies * res.n_records and s.n_bases == copies * n_bases
                    assert np.array_equal(table_of(s.counts(), (-1, 8)), np.tile(rows, (copies, 1)))          # rows of copy j = the original's
                    assert np.array_equal(table_of(s.letter_hist()), hist * np.uint64(copies))
                    assert s.totals == tuple(copies * t for t in totals), (s.totals, totals)
                    assert sum(s.totals[:7]) == copies * n_bases > 2 ** 32                                     # totals past 2^32
                # the same letters as ONE record: an 8-byte end table in device memory
                one = torch.tensor([copies * n_bases], dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                with sm.summarize(Source(d_sequence=sel.d_sequence, n_bases=sel.n_bases, d_record_end=one.data_ptr(), n_records=1), device=0, _lib=lib) as s:
                    print("summarize, one record of %d letters: %.3f ms" % (s.n_bases, s.ms))
                    row = tuple(int(v) for v in table_of(s.counts()))
                    assert row == s.totals == tuple(copies * t for t in totals), (row, s.totals, totals)
                # ... and under a table whose columns overlap, so that single columns of the one record pass 2^32 (a fourth
                # of the letters each is what the default table's columns hold): 0 A or C, 1 G or T, 2 upper case,
                # 3 lower case, 7 every byte
                wide = np.zeros(256, dtype=np.uint8)
                for c, members in ((0, b"ACac"), (1, b"GTgt"), (2, bytes(range(65, 91))), (3, bytes(range(97, 123))), (7, bytes(range(256)))):
                    for b in members:
                        wide[b] |= 1 << c
                want = tuple(copies * int(hist[((wide >> c) & 1) == 1].sum()) for c in range(8))
                with sm.summarize(Source(d_sequence=sel.d_sequence, n_bases=sel.n_bases, d_record_end=one.data_ptr(), n_records=1), wide.tobytes(),
                                  device=0, _lib=lib) as s:
                    row = tuple(int(v) for v in table_of(s.counts()))
                    assert row == s.totals == want, (row, s.totals, want)
                    assert row[7] == copies * n_bases > 2 ** 32 and row[0] + row[1] > 2 ** 32 and row[2] + row[3] > 2 ** 32
        finally:
            dec.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))
