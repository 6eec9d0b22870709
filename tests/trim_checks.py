"""Shared by tests/test_trim_emu.py (CPU harness) and tests/test_gpu_trim.py (MI355X): Decoder.trim, Selection.trim,
ParsedText.trim and trim(), records in device memory -> the window of every record that quality trimming keeps, as regions for
Decoder.select.  Not a test module; every function takes the library binding it is to check.

The yardstick is expected() below: the four steps of include/nafgpu.h at nafgpu_trim as a plain loop over what the CPU oracle
decodes (or over the source's own bytes read back).  Every table is compared for equality as struct and integer arrays:
integer work, no tolerance, no time asserted."""
import ctypes
import importlib
import io
import os

import numpy as np

import select_checks as sc
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device, encode_text, parse_text

tr = importlib.import_module("nafcodec_amd.trim")            # (the module: the package's attribute of that name is its trim())

ENTRY_POINTS = ("nafgpu_trim", "nafgpu_trim_decoder", "nafgpu_trims_copy_to_host", "nafgpu_trims_free")
TILE, LANE, HALO, SHORT, CHUNK = 4096, 16, 64, 1024, 256    # nafcodec_amd/csrc/trim.h: asserted below
REGION = np.dtype(tr.REGION)
assert REGION.itemsize == ctypes.sizeof(_ffi.Region) == 32
WINDOWS = (1, 2, 15, 16, 17, 63, 64)


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sc.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "trim.h")) as f:
        text = f.read()
    for name, value in (("kTrimTile", TILE), ("kTrimHalo", HALO), ("kTrimShort", SHORT), ("kTrimShortLanes", CHUNK // LANE), ("kTrimLongLanes", TILE // LANE)):
        assert "constexpr uint32_t %s = %d;" % (name, value) in text, name
    assert tr.MAX_WINDOW == 64 == max(WINDOWS) and HALO >= tr.MAX_WINDOW - 1


# ---------------------------------------------------------------- the yardstick
def options(cut_front=0, cut_tail=0, window=None, trim_n=False, min_length=0, interleaved=False, quality_base=33):
    return dict(cut_front=cut_front, cut_tail=cut_tail, window=window, trim_n=trim_n, min_length=min_length, interleaved=interleaved,
                quality_base=quality_base)


def window_loop(s, q, o):
    """one record, the rules as they are written: s letters or None, q quality bytes or None -> (a, b) before the canonical form"""
    L = len(s) if q is None else len(q)
    v = None if q is None else [int(x) - o["quality_base"] for x in q]
    a, b = 0, L
    if o["cut_front"]:
        total = best = 0
        for i in range(L):
            total += o["cut_front"] - v[i]
            if total < 0:
                break
            if total > best:
                best, a = total, i + 1
    if o["cut_tail"]:
        total = best = 0
        for i in range(L - 1, -1, -1):
            total += o["cut_tail"] - v[i]
            if total < 0:
                break
            if total > best:
                best, b = total, i
    if o["window"]:
        W, Q = o["window"]
        for i in range(a, b - W + 1):
            if sum(v[i:i + W]) < W * Q:
                b = i
                break
    if o["trim_n"]:
        while a < b and s[a] in b"Nn":
            a += 1
        while a < b and s[b - 1] in b"Nn":
            b -= 1
    return a, b


def window_numpy(s, q, o):
    """the same for a long record, with numpy's sums"""
    L = len(s) if q is None else len(q)
    v = None if q is None else np.frombuffer(q, dtype=np.uint8).astype(np.int64) - o["quality_base"]
    a, b = 0, L
    for tail, cutoff in ((False, o["cut_front"]), (True, o["cut_tail"])):
        if cutoff and L:
            sums = np.cumsum(cutoff - (v[::-1] if tail else v))
            below = np.flatnonzero(sums < 0)
            stop = int(below[0]) if len(below) else L
            if stop and sums[:stop].max() > 0:
                at = int(np.argmax(sums[:stop]))                                # (the first of equal maxima)
                a, b = (a, L - 1 - at) if tail else (at + 1, b)
    if o["window"] and b - a >= o["window"][0]:
        W, Q = o["window"]
        sums = np.concatenate(([0], np.cumsum(v[a:b])))
        bad = np.flatnonzero(sums[W:] - sums[:-W] < W * Q)
        if len(bad):
            b = a + int(bad[0])
    if o["trim_n"] and a < b:
        letters = np.frombuffer(s, dtype=np.uint8)[a:b]
        other = np.flatnonzero((letters != ord("N")) & (letters != ord("n")))
        a, b = (a + int(other[0]), a + int(other[-1]) + 1) if len(other) else (b, b)
    return a, b


def _self_check():
    rng = np.random.default_rng(5)
    for _ in range(300):
        L = int(rng.integers(0, 40))
        s = bytes(rng.choice(list(b"ACGTNn"), L).astype(np.uint8))
        q = bytes(rng.integers(30, 50, L).astype(np.uint8))
        o = options(int(rng.integers(0, 12)), int(rng.integers(0, 12)), (int(rng.integers(1, 6)), int(rng.integers(0, 12))) if rng.random() < .7 else None,
                    bool(rng.integers(0, 2)), quality_base=int(rng.integers(30, 40)))
        assert window_loop(s, q, o) == window_numpy(s, q, o), (s, q, o)


_self_check()


def expected(letters, quality, ends, **opts):
    """-> regions (REGION), keep (uint8): what the rules of include/nafgpu.h give; letters or quality may be None"""
    o = options(**opts)
    n = len(letters) if letters is not None else len(quality)
    ends = [int(e) for e in ends] if ends is not None and len(ends) else [n]
    regions, ok = np.zeros(len(ends), dtype=REGION), np.zeros(len(ends), dtype=bool)
    lo = 0
    for k, hi in enumerate(ends):
        s, q = None if letters is None else letters[lo:hi], None if quality is None else quality[lo:hi]
        a, b = (window_loop if hi - lo <= 400 else window_numpy)(s, q, o)
        if a >= b:
            a = b = 0
        regions[k] = (k, a, b, 0, 0)
        ok[k] = b - a >= o["min_length"]
        lo = hi
    if o["interleaved"]:
        ok[0::2] = ok[1::2] = ok[0::2] & ok[1::2]
    return regions, ok.astype(np.uint8)


def tables(trims):
    return (np.frombuffer(trims.regions(), dtype=REGION), np.frombuffer(trims.keep(), dtype=np.uint8), np.frombuffer(trims.kept_regions(), dtype=REGION))


def compare(trims, letters, quality, ends, what="", **opts):
    """every table and total of a Trims against expected(); -> regions, keep"""
    regions, keep = expected(letters, quality, ends, **opts)
    got_regions, got_keep, got_kept = tables(trims)
    n = len(letters) if letters is not None else len(quality)
    lengths = np.diff(np.concatenate(([0], np.asarray(ends, dtype=np.uint64).astype(np.int64)))) if ends is not None and len(ends) else np.array([n])
    assert trims.n_records == len(regions) == len(trims) and trims.n_bases == n, (what, trims.n_records, len(regions), trims.n_bases, n)
    for name, mine, want in (("regions", got_regions, regions), ("keep", got_keep, keep), ("kept_regions", got_kept, regions[keep.astype(bool)])):
        assert mine.shape == want.shape, (what, name, mine.shape, want.shape)
        if mine.tobytes() != want.tobytes():
            at = int(np.nonzero(mine != want)[0][0])
            raise AssertionError("%s: %s differs at %d of %d: %s / %s" % (what, name, at, len(want), mine[at], want[at]))
    size = (regions["end"] - regions["start"]).astype(np.int64)
    changed = int(((regions["start"] != 0) | (regions["end"].astype(np.int64) != lengths)).sum())
    assert (trims.n_kept, trims.n_changed, trims.bases_in_windows, trims.bases_kept) == (int(keep.sum()), changed, int(size.sum()), int(size[keep.astype(bool)].sum())), \
        (what, trims.n_kept, trims.n_changed, trims.bases_in_windows, trims.bases_kept, int(keep.sum()), changed, int(size.sum()))
    return regions, keep


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


def layout(recs):
    """oracle records -> letters, quality (None without), ends"""
    quality = None if any(r[3] is None for r in recs) else b"".join(r[3] for r in recs)
    return b"".join(r[2] for r in recs), quality, np.cumsum([len(r[2]) for r in recs], dtype=np.uint64)


def own_layout(source):
    """a Selection's (or ParsedText's) own bytes read back -> letters, quality, ends"""
    quality = source.copy_to_host(source.d_quality, source.n_quality) if source.d_quality else None
    return (source.copy_to_host(source.d_sequence, source.n_bases), quality,
            np.frombuffer(source.copy_to_host(source.d_record_end, 8 * source.n_records), dtype=np.uint64))


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


class DeviceBytes:
    """bytes in device memory, without any library but this one: they are the sequence of a one-record text archive, decoded by
    a decoder of its own (decode_all_device leaves the section's bytes where the kernels read them).  pad: bytes in front, so
    that `address` has that residue mod 16; the section ends with the data's last byte."""

    def __init__(self, lib, data, pad=0):
        data = bytes(pad) + bytes(data)
        self._dec = open_decoder(lib, sc.hand_archive(1, ids=[b"t"], text=data or b"\0"))
        res = self._dec.decode_all_device()
        assert res.d_sequence % 16 == 0 and (not data or self._dec.copy_to_host(res.d_sequence, len(data)) == data)
        self.address = res.d_sequence + pad

    def close(self):
        self._dec.close()


def device_case(lib, what, records, pad=0, n_records=None, with_letters=True, with_quality=True, behind=b"", **opts):
    """records [(letters, quality)] -> device buffers of this test's own -> trim() against expected(); -> regions, keep"""
    letters, quality = b"".join(r[0] for r in records) + behind, b"".join(r[1] for r in records) + behind
    ends = np.cumsum([len(r[0]) for r in records], dtype=np.uint64)
    assert len(letters) == len(quality) and len(letters) > 0
    bufs = [DeviceBytes(lib, letters, pad), DeviceBytes(lib, quality, pad), DeviceBytes(lib, ends.tobytes() or bytes(8))]
    try:
        src = Source(d_sequence=bufs[0].address if with_letters else None, n_bases=len(letters), d_quality=bufs[1].address if with_quality else None,
                     n_quality=len(quality), d_record_end=bufs[2].address, n_records=len(records) if n_records is None else n_records)
        with tr.trim(src, _lib=lib, **opts) as trims:
            use = ends if n_records is None else ends[:n_records]
            return compare(trims, letters if with_letters else None, quality if with_quality else None, use if src.n_records else None, what=what, **opts)
    finally:
        for b in bufs:
            b.close()


def fastq(records):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (k, s, q) for k, (s, q) in enumerate(records))


def text_case(lib, what, records, **opts):
    """records [(letters, quality)] as FASTQ through parse_text(...).trim() against expected() over the parsed bytes read back"""
    with parse_text(fastq(records), device=0, _lib=lib) as parsed:
        letters, quality, ends = own_layout(parsed)
        assert letters == b"".join(r[0] for r in records) and quality == b"".join(r[1] for r in records), what
        with parsed.trim(**opts) as trims:
            return compare(trims, letters, quality, ends, what=what, **opts)


# ---------------------------------------------------------------- 1. the fixtures
PHIX = (  # options, records changed, records with a front cut (None: not written out), letters left
    (dict(cut_front=20, cut_tail=20), 42, 41, 12175), (dict(cut_front=30, cut_tail=30), 42, None, 11632), (dict(window=(4, 20)), 41, None, 10688),
    (dict(window=(10, 30)), 42, None, 9805), (dict(window=(4, 30)), 42, None, 21))
PHIX_MORE = (dict(cut_front=20), dict(cut_tail=20), dict(trim_n=True), dict(min_length=150), dict(cut_tail=25, min_length=100, interleaved=True),
             dict(cut_front=20, cut_tail=20, window=(4, 20), trim_n=True, min_length=50), dict(cut_front=5, cut_tail=35, window=(64, 34), trim_n=True, min_length=1),
             dict(cut_front=20, cut_tail=20, window=(10, 30), trim_n=True, min_length=90, interleaved=True), dict(cut_tail=2, quality_base=64), dict())


def check_fixtures(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, quality, ends = layout(recs)
    assert len(recs) == 42 and len(letters) == 12436 and sum(r[2][:1] == b"N" for r in recs) == 40
    with open_decoder(lib, blob) as dec:
        for opts, changed, front, left in PHIX:
            with dec.trim(**opts) as trims:
                regions, keep = compare(trims, letters, quality, ends, what="phix %r" % (opts,), **opts)
                assert (trims.n_changed, trims.bases_in_windows, trims.n_kept) == (changed, left, 42), (opts, trims.n_changed, trims.bases_in_windows)
                assert front is None or int((regions["start"] > 0).sum()) == front
        seen = []
        for opts in PHIX_MORE:
            with dec.trim(**opts) as trims:
                compare(trims, letters, quality, ends, what="phix %r" % (opts,), **opts)
                seen.append((trims.n_changed, trims.n_kept))
        assert seen[2] == (41, 42) and seen[-1] == (0, 42) and 0 < seen[3][1] < 42 and 0 < seen[4][1] < seen[3][1] + 42 and seen[4][1] % 2 == 0, seen
        with dec.trim(trim_n=True) as trims:                                    # an answer written out: 41 reads lose their first letter, N in 40 and n in one
            regions, _, _ = tables(trims)
            assert int((regions["start"] == 1).sum()) == 41 and trims.bases_in_windows == 12436 - 41
    try:                                                                        # trims outlive their source; closed ones are refused
        trims.regions()
    except RuntimeError:
        pass
    else:
        raise AssertionError("closed trims were used")
    # the fixtures without qualities: trim_n and min_length alone; a quality step is refused
    for name in ("masked", "CP040672", "LuxC", "NZ_AAEN01000029"):
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob)
        letters, quality, ends = layout(recs)
        assert quality is None
        sizes = sorted(len(r[2]) for r in recs)
        with open_decoder(lib, blob) as dec:
            for opts in (dict(trim_n=True), dict(min_length=sizes[len(sizes) // 2]), dict(trim_n=True, min_length=sizes[len(sizes) // 2] + 1), dict()):
                with dec.trim(**opts) as trims:
                    compare(trims, letters, None, ends, what="%s %r" % (name, opts), **opts)
                    assert trims.n_kept == sum(l >= opts.get("min_length", 0) for l in sizes) or opts.get("trim_n"), (name, opts, trims.n_kept)
            for opts in (dict(cut_front=20), dict(cut_tail=20), dict(window=(4, 20))):
                try:
                    dec.trim(**opts)
                except ValueError as e:
                    assert "quality" in str(e), e
                else:
                    raise AssertionError("a quality step without qualities on %s" % name)


# ---------------------------------------------------------------- 2. the edges
BASE, LOW, HIGH = 34, b"!", b"~"     # with quality_base 34 and Q = 0: v = -1 and 92; a window fails when and only when all of it is low


def planted(n, starts, W):
    q = bytearray(HIGH * n)
    for at in starts:
        q[at:at + W] = LOW * W
    return bytes(q)


def cut_between(quality, starts, W, rng):
    """a section cut into records so that every planted window has a record of its own; -> [(letters, quality)]"""
    starts = sorted(starts)
    cuts = [0] + [int(rng.integers(a + W, b + 1)) for a, b in zip(starts[:-1], starts[1:])] + [len(quality)]
    return [(bytes(rng.choice(list(b"ACGT"), hi - lo).astype(np.uint8)), quality[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])], cuts


def check_edges(lib):
    kernel_constants()
    rng = np.random.default_rng(20250101)
    letters_of = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    # ---- step 2: the failing window at the section's first and last start, around every tile edge, at every residue of a lane
    for W in WINDOWS:
        n = TILE * (W + 1) + 200
        starts = [0, n - W] + [TILE * j - W + (j - 1) for j in range(1, W + 2)] + [112 + 81 * i for i in range(LANE + 1)]
        assert {s - TILE * (1 + i) for i, s in enumerate(starts[2:W + 3])} == set(range(-W, 1)) and {s % LANE for s in starts[W + 3:]} == set(range(LANE))
        quality = planted(n, starts, W)
        records, cuts = cut_between(quality, starts, W, rng)
        opts = dict(window=(W, 0), quality_base=BASE)
        regions, _ = device_case(lib, "planted windows, W = %d" % W, records, **opts)
        assert [int(e) for e in regions["end"]] == [s - c for s, c in zip(sorted(starts), cuts)], W    # every record is cut at its window
        if W in (2, 17, 64):
            text_case(lib, "planted windows as text, W = %d" % W, records[:W + 8], **opts)
        # one record: the lowest of them all; and the same bytes cut into random records
        device_case(lib, "one record, W = %d" % W, [(letters_of(n), quality)], pad=W % 16, **opts)
        pieces, at = [], 0
        while at < n:
            l = int(rng.integers(0, 3 * W + 40))
            pieces.append((letters_of(len(quality[at:at + l])), quality[at:at + l]))
            at += l
        device_case(lib, "random records, W = %d" % W, pieces, **opts)
        # record lengths 0, 1, W - 1, W, W + 1 and runs of empty records, all low: a record of W or more is cut at 0
        lengths = [0, 1, W - 1, W, W + 1, 0, 0, 0, W, 0] + [0] * 70 + [W, W - 1, 2 * W, 1]
        regions, _ = device_case(lib, "record lengths, W = %d" % W, [(letters_of(l), LOW * l) for l in lengths], **opts)
        assert [int(e) for e in regions["end"]] == [0 if l >= W else l for l in lengths]
        # a low run of W split by a record end: the window lies in neither record; one that ends exactly at the end does
        split = [(letters_of(30), HIGH * (31 - W if W < 31 else 0) + LOW * (W - 1 if W < 31 else 30)), (letters_of(20), LOW + HIGH * 19),
                 (letters_of(W + 5), HIGH * 5 + LOW * W)]
        regions, _ = device_case(lib, "a window across a record end, W = %d" % W, split, **opts)
        if 1 < W < 31:
            assert [tuple(r)[1:3] for r in regions] == [(0, 30), (0, 20), (0, 5)], regions
    # windows against [a, b) of step 1: the front cut takes five letters, a window over letters 1 .. 4 is not looked at; the tail
    # cut leaves b = 21 and the only failing window, at 20, reaches behind it
    front = LOW * 5 + HIGH * 20
    regions, _ = device_case(lib, "a window in front of a", [(letters_of(25), front)], cut_front=5, window=(4, 0), quality_base=BASE)
    assert tuple(regions[0])[1:3] == (5, 25)
    tail = HIGH * 20 + bytes([BASE + 30]) + LOW * 4
    regions, _ = device_case(lib, "a window that ends behind b", [(letters_of(25), tail)], cut_tail=5, window=(4, 7), quality_base=BASE)
    assert tuple(regions[0])[1:3] == (0, 21)
    regions, _ = device_case(lib, "the same window without the tail cut", [(letters_of(25), tail)], window=(4, 7), quality_base=BASE)
    assert tuple(regions[0])[1:3] == (0, 20)

    # ---- step 1
    q = lambda *values: bytes(33 + v for v in values)
    both = dict(cut_front=10, cut_tail=10)
    for what, values, want in (("a stop at the first letter", [30] * 12, (0, 12)), ("never stopping", [5] * 12, (0, 0)),
                               ("equal maxima: the shorter cut", [5, 15, 5, 15, 30, 30, 30, 15, 5, 15, 5], (1, 10)),
                               ("the maximum in the last letter before the stop", [5, 5, 0, 40, 40, 0, 5, 5], (3, 5)),
                               ("cuts that cross", [9, 9, 9, 11, 9, 9, 9], (0, 0)), ("one letter, low", [3], (0, 0)), ("one letter, high", [30], (0, 1))):
        regions, _ = device_case(lib, what, [(letters_of(len(values)), q(*values))], **both)
        assert tuple(regions[0])[1:3] == want, (what, regions)
        text_case(lib, what + ", as text", [(letters_of(len(values)), q(*values))] * 3, **both)
    regions, _ = device_case(lib, "values below the base", [(letters_of(6), bytes([60, 60, 126, 126, 60, 50]))], cut_front=1, cut_tail=1, quality_base=64)
    assert tuple(regions[0])[1:3] == (2, 4)
    # a stop and a maximum on either side of a chunk edge, on both routes (chunks of 256 and of 4 096 letters), from both ends
    for chunk, length in ((CHUNK, 3 * CHUNK + 77), (TILE, 3 * TILE + 77)):
        records = []
        for d in (-2, -1, 0, 1, 2):
            for stop in (1, 2, 17):
                values = np.full(length, 40, dtype=np.uint8)                    # the maximum at chunk + d - 1, the stop `stop` letters on
                values[:chunk + d] = 5
                values[chunk + d:chunk + d + stop - 1] = 12
                records.append((letters_of(length), q(*values)))
                records.append((letters_of(length), q(*values[::-1])))
        for pad in (0, 5):
            regions, _ = device_case(lib, "chunk edges of %d" % chunk, records, pad=pad, **both)
        assert tuple(regions[0])[1:3] == (chunk - 2, length) and tuple(regions[1])[1:3] == (0, length - chunk + 2), regions[:2]
    # three tiles of all-low qualities, one record: both ends walk the whole record; then with a high letter in the middle
    low = q(*([2] * (3 * TILE)))
    regions, _ = device_case(lib, "three tiles, all low", [(letters_of(3 * TILE), low)], **both)
    assert tuple(regions[0])[1:3] == (0, 0)
    middle = bytearray(low)
    middle[TILE + 7] = 33 + 90
    device_case(lib, "three tiles, low but for one letter", [(letters_of(3 * TILE), bytes(middle)), (letters_of(3), q(1, 2, 3))], pad=9, **both)
    # the whole range of bytes, random records, every step on
    for pad in range(16):
        n = 9000 + 13 * pad
        quality = bytes(rng.integers(0, 256, n).astype(np.uint8))
        pieces, at = [], 0
        while at < n:
            l = int(rng.choice([0, 1, 40, 300, 2000])) + int(rng.integers(0, 9))
            seq = bytearray(letters_of(len(quality[at:at + l])))
            seq[:int(rng.integers(0, 5))] = b"N" * min(4, len(seq))
            pieces.append((bytes(seq[:len(quality[at:at + l])]), quality[at:at + l]))
            at += l
        device_case(lib, "all byte values, the pointer at residue %d" % pad, pieces, pad=pad, behind=b"\x01" * (pad % 3), cut_front=100, cut_tail=140,
                    window=(1 + 4 * pad, 120), trim_n=True, min_length=pad, quality_base=33 + pad)

    # ---- step 3
    n_records = [(b"NNNNNNNN", HIGH * 8), (b"nNnACGTNACGnn", HIGH * 13), (b"ACNNNGT", HIGH * 7), (b"N", HIGH), (b"A", HIGH), (b"", b""),
                 (b"N" * CHUNK + b"A" + b"N" * CHUNK, HIGH * (2 * CHUNK + 1)), (b"N" * (CHUNK - 3) + b"AC" + b"n" * (2 * CHUNK - 5), HIGH * (3 * CHUNK - 6)),
                 (b"N" * TILE + b"ACG" + b"N" * (2 * TILE), HIGH * (3 * TILE + 3)), (b"N" * (2 * TILE + 9), HIGH * (2 * TILE + 9)),
                 (b"A" + b"N" * (TILE + CHUNK) + b"C", HIGH * (TILE + CHUNK + 2))]
    for pad in (0, 11):
        regions, _ = device_case(lib, "N ends", n_records, pad=pad, trim_n=True)
    assert [tuple(r)[1:3] for r in regions] == [(0, 0), (3, 11), (0, 7), (0, 0), (0, 1), (0, 0), (CHUNK, CHUNK + 1), (CHUNK - 3, CHUNK - 1),
                                                (TILE, TILE + 3), (0, 0), (0, TILE + CHUNK + 2)], regions
    device_case(lib, "N ends without qualities", n_records, with_quality=False, trim_n=True, min_length=2)
    text_case(lib, "N ends, as text", [r for r in n_records if r[0]], trim_n=True)

    # ---- step 4: min_length one below and at a window's length; mates with exactly one failing, in either position
    reads = [(letters_of(20), q(*([30] * 12 + [2] * 8))), (letters_of(20), q(*([30] * 20))), (letters_of(20), q(*([30] * 20))), (letters_of(20), q(*([30] * 12 + [2] * 8))),
             (letters_of(20), q(*([30] * 12 + [2] * 8))), (letters_of(20), q(*([30] * 11 + [2] * 9))), (letters_of(20), q(*([30] * 20))), (letters_of(20), q(*([30] * 20)))]
    for min_length, interleaved, want in ((11, False, [1] * 8), (12, False, [1, 1, 1, 1, 1, 0, 1, 1]), (13, False, [0, 1, 1, 0, 0, 0, 1, 1]), (12, True, [1, 1, 1, 1, 0, 0, 1, 1]), (13, True, [0] * 6 + [1, 1]),
                                          (0, True, [1] * 8), (21, False, [0] * 8)):
        _, keep = device_case(lib, "min_length %d" % min_length, reads, cut_tail=10, min_length=min_length, interleaved=interleaved)
        assert list(keep) == want, (min_length, interleaved, keep)
    _, keep = device_case(lib, "empty windows are kept without a length", [(letters_of(4), q(1, 1, 1, 1)), (b"", b"")], cut_tail=10)
    assert list(keep) == [1, 1]

    # ---- sources: letters behind the last end, no table, one section only
    device_case(lib, "letters behind the last end", reads, n_records=5, behind=LOW * 70, cut_front=10, cut_tail=10, window=(4, 20), trim_n=True)
    regions, _ = device_case(lib, "no records: the section is record 0", reads, n_records=0, cut_tail=10, window=(4, 20), trim_n=True)
    assert len(regions) == 1
    device_case(lib, "qualities only", reads, with_letters=False, cut_front=10, cut_tail=10, window=(4, 20), min_length=3)
    for opts in (dict(), dict(min_length=21)):                                  # all options off: every region is the whole record
        regions, _ = device_case(lib, "all options off", reads + [(b"", b"")], **opts)
        assert [tuple(r)[1:3] for r in regions] == [(0, 20)] * 8 + [(0, 0)]


# ---------------------------------------------------------------- 3. random
def random_reads(n, seed=11):
    """a FASTQ of about n letters: read lengths of 0 .. 300 and a few of 10^4; a part of the reads has a low tail, a low front, a
    dip in the middle, N at its ends, and a part has none of them"""
    rng = np.random.default_rng(seed)
    records, total = [], 0
    while total < n:
        l = 10_000 + int(rng.integers(0, 999)) if rng.random() < 0.002 else int(rng.integers(0, 301))
        s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), l)
        v = rng.integers(30, 41, l)
        if l > 20:
            if rng.random() < 0.5:
                v[l - int(rng.integers(1, 1 + l // 3)):] = rng.integers(2, 15)
            if rng.random() < 0.3:
                v[:int(rng.integers(1, 10))] = 2
            if rng.random() < 0.3:
                at = int(rng.integers(0, l - 12))
                v[at:at + 12] = rng.integers(2, 25)
            if rng.random() < 0.3:
                s[:int(rng.integers(1, 4))] = ord("N")
            if rng.random() < 0.3:
                s[l - int(rng.integers(1, 4)):] = ord("n")
            if rng.random() < 0.1:
                s[l // 2] = ord("N")
        records.append((s.astype(np.uint8).tobytes(), (v + 33).astype(np.uint8).tobytes()))
        total += l
    return records[:len(records) & ~1]


def check_random(lib, n):
    records = random_reads(n)
    with parse_text(fastq(records), device=0, _lib=lib) as parsed:
        letters, quality, ends = own_layout(parsed)
        assert letters == b"".join(r[0] for r in records) and len(ends) == len(records) and any(len(r[0]) > 9999 for r in records)
        lengths = np.array([len(r[0]) for r in records])
        shares = {}
        for name, opts in (("sums", dict(cut_front=20, cut_tail=20)), ("window", dict(window=(8, 25))), ("n", dict(trim_n=True)),
                           ("all", dict(cut_front=20, cut_tail=20, window=(8, 25), trim_n=True, min_length=60, interleaved=True))):
            with parsed.trim(**opts) as trims:
                regions, keep = compare(trims, letters, quality, ends, what="random, %d letters, %s" % (n, name), **opts)
                shares[name] = trims.n_changed
                print("trim %s: %d letters, %d records, %d changed, %d kept, %.3f ms" % (name, len(letters), len(records), trims.n_changed, trims.n_kept, trims.ms))
        for name, changed in shares.items():                                    # every step bites on a part of the reads and leaves a part alone
            assert 0.1 * len(records) < changed < 0.9 * len(records), (name, changed, len(records))
        assert 0.1 * len(records) < int(keep.sum()) < 0.9 * len(records)
        front, back = expected(letters, quality, ends, cut_front=20)[0], expected(letters, quality, ends, cut_tail=20)[0]
        assert 0 < int((front["start"] > 0).sum()) < len(records) and 0 < int((back["end"] < lengths).sum()) < len(records)


# ---------------------------------------------------------------- 4. composition
def check_composition(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, quality, ends = layout(recs)
    opts = dict(cut_front=20, cut_tail=20, window=(10, 30), trim_n=True, min_length=60)
    with open_decoder(lib, blob) as dec, dec.trim(**opts) as trims:
        regions, keep = compare(trims, letters, quality, ends, what="phix", **opts)
        mine = [bytes(t) for t in tables(trims)]
        assert 0 < trims.n_kept < 42
        # select(trims): every kept record cut to its window, letters and qualities, read back through the oracle
        with dec.select(trims) as sel:
            assert sel.n_records == trims.n_kept
            archive = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, mask=True, compression_level=1, device=0, _lib=lib)
        cleaned = sc.oracle_records(archive, spec_mask=True)
        kept = [r for r, k in zip(regions, keep) if k]
        assert len(cleaned) == len(kept)
        for out, r in zip(cleaned, kept):
            k, a, b = int(r["record"]), int(r["start"]), int(r["end"])
            assert out[0] == recs[k][0] and out[2] == recs[k][2][a:b] and out[3] == recs[k][3][a:b] and len(out[2]) >= 60, k
        # the buffer itself is what select takes, too
        with dec.select(trims.kept_regions()) as a, dec.select(trims) as b:
            assert own_layout(a)[0] == own_layout(b)[0]
        # Selection.trim and ParsedText.trim equal Decoder.trim on the same records
        with dec.select(list(range(42))) as sel, sel.trim(**opts) as again:
            assert mine == [bytes(t) for t in tables(again)] and (again.n_kept, again.n_changed, again.bases_kept) == (trims.n_kept, trims.n_changed, trims.bases_kept)
        with parse_text(dec.to_text(), device=0, _lib=lib) as parsed, parsed.trim(**opts) as again:
            assert mine == [bytes(t) for t in tables(again)] and again.bases_in_windows == trims.bases_in_windows
        res = dec.decode_all_device()
        with tr.trim(res, _lib=lib, **opts) as again:
            assert mine == [bytes(t) for t in tables(again)]
        # what select accepted before is read as before
        with dec.select([3, (7, 5, 250)]) as sel:
            assert own_layout(sel)[0] == recs[3][2] + recs[7][2][5:250]


# ---------------------------------------------------------------- 5. refusals
def call_trim(lib, src_fields, device=0, null_opts=False, **opts):
    src, o = _ffi.EncodeSource(**src_fields), _ffi.TrimOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.TrimResult(), _ffi.Error()
    rc = lib.c.nafgpu_trim(ctypes.byref(src), None if null_opts else ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_trims_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_trim_decoder(lib, dec, null_opts=False, **opts):
    o = _ffi.TrimOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.TrimResult(), _ffi.Error()
    rc = lib.c.nafgpu_trim_decoder(dec._h, None if null_opts else ctypes.byref(o), ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_trims_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    bad, length = _ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH
    with open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_quality=res.d_quality, n_quality=res.n_quality, d_record_end=res.d_record_end,
                    n_records=res.n_records)
        assert call_trim(lib, good, quality_base=33, cut_tail=20)[0] == _ffi.OK and call_trim(lib, good)[0] == _ffi.OK
        assert call_trim(lib, good, null_opts=True)[0] == bad
        assert call_trim(lib, dict(good, d_sequence=None, d_quality=None))[0] == bad
        for opts in (dict(cut_front=1), dict(cut_tail=1), dict(window=4)):
            rc, message = call_trim(lib, dict(good, d_quality=None), **opts)
            assert rc == bad and "quality" in message, (opts, rc, message)
        assert call_trim(lib, dict(good, d_quality=None), trim_n=1)[0] == _ffi.OK
        rc, message = call_trim(lib, dict(good, d_sequence=None), trim_n=1)
        assert rc == bad and "sequence" in message, (rc, message)
        assert call_trim(lib, dict(good, d_sequence=None), cut_tail=20)[0] == _ffi.OK
        rc, message = call_trim(lib, good, window=65)
        assert rc == bad and "window" in message and call_trim(lib, good, window=64, window_quality=20, quality_base=33)[0] == _ffi.OK, (rc, message)
        rc, message = call_trim(lib, dict(good, n_records=41), interleaved=1)
        assert rc == bad and "odd" in message and call_trim(lib, good, interleaved=1)[0] == _ffi.OK, (rc, message)
        assert call_trim(lib, dict(good, n_records=0), interleaved=1)[0] == bad                 # the section as one record: odd
        rc, message = call_trim(lib, dict(good, n_quality=res.n_quality - 1), cut_tail=20)
        assert rc == length and "quality bytes" in message, (rc, message)
        src, o, h, r, err = _ffi.EncodeSource(**good), _ffi.TrimOpts(), ctypes.c_void_p(), _ffi.TrimResult(), _ffi.Error()
        for args in ((None, ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), ctypes.byref(o), 0, None, ctypes.byref(r)),
                     (ctypes.byref(src), ctypes.byref(o), 0, ctypes.byref(h), None)):
            assert lib.c.nafgpu_trim(*args, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_trims_copy_to_host(None, None, 1, None) == bad
        lib.c.nafgpu_trims_free(None)
        assert call_trim_decoder(lib, dec, null_opts=True)[0] == bad and call_trim_decoder(lib, dec, window=65)[0] == bad
        assert call_trim_decoder(lib, dec, cut_tail=20, quality_base=33)[0] == _ffi.OK
        for call in (lambda: dec.trim(window=(65, 20)), lambda: dec.trim(window=(0, 20)), lambda: dec.trim(cut_front=256), lambda: dec.trim(min_length=-1),
                     lambda: tr.trim(Source(), _lib=lib), lambda: tr.trim(Source(d_sequence=res.d_sequence, n_bases=res.n_bases), cut_tail=3, _lib=lib)):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("accepted")
    check_end_tables(lib)
    # through a decoder: no qualities decoded; a shard; no Length section; an archive that ends early
    with open_decoder(lib, blob, quality=False) as dec:
        rc, message, _ = call_trim_decoder(lib, dec, cut_tail=20)
        assert rc == bad and "quality" in message, (rc, message)
        assert call_trim_decoder(lib, dec, trim_n=1)[0] == _ffi.OK
    with open_decoder(lib, blob, sequence=False) as dec:
        rc, message, _ = call_trim_decoder(lib, dec, trim_n=1)
        assert rc == bad and "sequence" in message, (rc, message)
        assert call_trim_decoder(lib, dec, cut_tail=20, quality_base=33)[0] == _ffi.OK
    with open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _ = call_trim_decoder(lib, dec, trim_n=1)
        assert rc == bad and "shard" in message, (rc, message)
    with open_decoder(lib, golden_bytes("LuxC.naf")) as dec:
        assert call_trim_decoder(lib, dec, window=4)[0] == bad and call_trim_decoder(lib, dec, min_length=5)[0] == _ffi.OK
    with open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"NNACGTTTnn")) as dec:
        rc, message, _ = call_trim_decoder(lib, dec, trim_n=1)
        assert rc == bad and "ength" in message, (rc, message)                  # the Length section is needed, as for select
    with open_decoder(lib, sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 4], text=b"NCGTACGTAC")) as dec:
        rc, message, kind = call_trim_decoder(lib, dec, trim_n=1)
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 2" in message, (rc, kind, message)
        try:
            dec.trim(trim_n=True)
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")
    with open_decoder(lib, sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 2], text=b"NCGTACGTAn")) as dec, dec.trim(trim_n=True) as trims:
        assert [tuple(r)[:3] for r in tables(trims)[0]] == [(0, 1, 4), (1, 0, 4), (2, 0, 1)]


def check_end_tables(lib):
    """hand-made end tables through nafgpu_trim: a selection's sections with a table of this test's own in device memory"""
    with open_decoder(lib, golden_bytes("phix.naf")) as dec, dec.select(list(range(42))) as sel:
        n = sel.n_bases
        good = np.arange(1, 201, dtype=np.uint64) * np.uint64(10)
        assert n > 2000
        for what, change, needle, status in (("decreasing", {100: 500}, "record 100 ", _ffi.E_INVALID_LENGTH),
                                             ("decreasing, three of them", {100: 500, 60: 300, 199: 1}, "record 60 ", _ffi.E_INVALID_LENGTH),
                                             ("the last record beyond the section", {199: n + 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("far beyond", {199: 2 ** 64 - 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("the first record bad", {0: 2 ** 40}, "record 0 ", _ffi.E_INVALID_LENGTH),
                                             ("the last record below the one in front", {199: 1989}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("a good table", {}, "", _ffi.OK)):
            table = good.copy()
            for k, v in change.items():
                table[k] = v
            d_table = DeviceBytes(lib, table.tobytes())
            try:
                rc, message = call_trim(lib, dict(d_sequence=sel.d_sequence, n_bases=n, d_quality=sel.d_quality, n_quality=n, d_record_end=d_table.address,
                                                  n_records=len(table)), quality_base=33, cut_front=20, cut_tail=20, window=4, window_quality=20, trim_n=1, min_length=3)
            finally:
                d_table.close()
            assert rc == status and needle in message, (what, rc, message)


# ---------------------------------------------------------------- 6. positions and tile indices past 2^32 (MI355X only)
def big_reads(n, seed=3):
    """n letters with qualities as FASTQ text: 2 000 short reads, then records of 2^16 .. 2^22 letters with low stretches"""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(0, 301, 2000)]
    while sum(lengths) < n:
        lengths.append(min(int(2 ** rng.uniform(16, 22)), n - sum(lengths)))
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
    v = rng.integers(30, 41, n, dtype=np.uint8)
    at = 0
    for k, l in enumerate(lengths):
        if l > 20 and k % 2:
            v[at + l - int(rng.integers(1, l // 2)):at + l] = 5
            v[at:at + int(rng.integers(1, 9))] = 2
        if l > 20 and k % 3 == 0:
            dip = at + int(rng.integers(0, l - 12))
            v[dip:dip + 12] = 11
            s[at:at + 2] = ord("N")
            s[at + l - 3:at + l] = ord("N")
        at += l
    s, v = s.tobytes(), (v + 33).tobytes()
    out, at = [], 0
    for k, l in enumerate(lengths):
        out.append(b"@r%d\n%s\n+\n%s\n" % (k, s[at:at + l], v[at:at + l]))
        at += l
    return b"".join(out), lengths


def check_past_u32(lib, n_bases=2 ** 28, copies=17):
    text, lengths = big_reads(n_bases)
    archive = encode_text(text, sequence_type="dna", id=False, comment=False, sequence=True, quality=True, compression_level=1, device=0, _lib=lib)
    del text
    opts = dict(cut_front=20, cut_tail=20, window=(8, 25), trim_n=True, min_length=100)
    with open_decoder(lib, archive) as dec:
        res = dec.decode_all_device()
        assert (res.n_bases, res.n_records) == (n_bases, len(lengths))
        letters, quality = dec.copy_to_host(res.d_sequence, n_bases), dec.copy_to_host(res.d_quality, n_bases)
        ends = np.cumsum(lengths, dtype=np.uint64)
        with dec.trim(**opts) as trims:
            print("trim: %d records, %d letters, %d changed, %d kept, %.3f ms" % (trims.n_records, trims.n_bases, trims.n_changed, trims.n_kept, trims.ms))
            regions, keep = compare(trims, letters, quality, ends, what="2^28 letters", **opts)
            assert 0 < trims.n_changed < len(lengths) and 0 < trims.n_kept < len(lengths)
            one = (trims.n_kept, trims.n_changed, trims.bases_in_windows, trims.bases_kept)
        del letters, quality
        with dec.select(list(range(res.n_records)) * copies) as sel:
            assert sel.n_bases == copies * n_bases > 2 ** 32
            with sel.trim(**opts) as trims:
                print("trim past 2^32: %d records, %d letters, %d kept, %.3f ms" % (trims.n_records, trims.n_bases, trims.n_kept, trims.ms))
                assert trims.n_records == copies * len(lengths) and trims.n_bases == copies * n_bases
                assert (trims.n_kept, trims.n_changed, trims.bases_in_windows, trims.bases_kept) == tuple(copies * v for v in one)
                all_regions, all_keep, all_kept = tables(trims)
                kept = regions[keep.astype(bool)]
                for c in range(copies):                                         # copy c: the trims of copy 0, the record shifted
                    want = regions.copy()
                    want["record"] += np.uint64(c * len(lengths))
                    assert all_regions[c * len(lengths):(c + 1) * len(lengths)].tobytes() == want.tobytes(), c
                    assert all_keep[c * len(lengths):(c + 1) * len(lengths)].tobytes() == keep.tobytes(), c
                    want = kept.copy()
                    want["record"] += np.uint64(c * len(lengths))
                    assert all_kept[c * len(kept):(c + 1) * len(kept)].tobytes() == want.tobytes(), c
