"""Shared by tests/test_overlap_emu.py (CPU harness) and tests/test_gpu_overlap.py (MI355X): Decoder.overlap, Selection.overlap,
ParsedText.overlap, overlap() and Decoder.merge: paired records in device memory -> where read 1 and the reverse complement of
read 2 overlap, the adapter cut as regions for Decoder.select, and the found pairs joined into a Selection.  Not a test module;
every function takes the library binding it is to check.

The yardstick is expected() below: the rules of include/nafgpu.h at nafgpu_overlap as a plain loop over all shifts of every pair
(counts_loop states it letter by letter; counts_numpy is the same count per shift taken off the matrix of all letter pairs, held
against the loop at import), and merged() for the joined records.  Every table is compared for equality as struct and integer
arrays: integer work, no tolerance, no time asserted."""
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

ov = importlib.import_module("nafcodec_amd.overlap")         # (the module: the package's attribute of that name is its overlap())

ENTRY_POINTS = ("nafgpu_overlap", "nafgpu_overlap_decoder", "nafgpu_merge_pairs", "nafgpu_overlaps_copy_to_host", "nafgpu_overlaps_free")
CAP, TILE, WAVES = 1024, 4096, 4                            # nafcodec_amd/csrc/overlap.h: asserted below
REGION, PAIR = np.dtype(ov.REGION), np.dtype(ov.PAIR)
assert REGION.itemsize == ctypes.sizeof(_ffi.Region) == 32 and PAIR.itemsize == ctypes.sizeof(_ffi.PairOverlap) == 32
DEFAULTS = dict(min_overlap=30, max_mismatches=5, max_mismatch_percent=20, quality_base=33)

CODE = np.full(256, 4, dtype=np.uint8)                       # A C G T/U in either case: 0 1 2 3; every other byte: no letter
for _c, _v in zip(b"ACGTU", (0, 1, 2, 3, 3)):
    CODE[_c] = CODE[_c | 0x20] = _v


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sc.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "overlap.h")) as f:
        text = f.read()
    assert "constexpr uint32_t kOvlWaves = %d; " % WAVES in text and "constexpr uint32_t kOvlTile = %d;" % TILE in text
    with open(os.path.join(ROOT, "include", "nafgpu.h")) as f:
        assert "#define NAFGPU_OVERLAP_MAX_LENGTH %d\n" % CAP in f.read()
    assert ov.MAX_LENGTH == CAP


# ---------------------------------------------------------------- the yardstick
def options(**opts):
    unknown = set(opts) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **opts)


def codes_of(r1, r2):
    """-> x, y: the codes of R1, and of R2 reversed and complemented (a non-letter stays 4)"""
    x = CODE[np.frombuffer(r1, dtype=np.uint8)]
    y = CODE[np.frombuffer(r2, dtype=np.uint8)][::-1].copy()
    y[y < 4] = 3 - y[y < 4]
    return x, y


def counts_loop(x, y):
    """the rules as they are written -> [(d, matches, mismatches)] for every shift"""
    n1, n2 = len(x), len(y)
    out = []
    for d in range(-(n2 - 1), n1):
        m = mm = 0
        for p in range(max(0, d), min(n1, d + n2)):
            a, b = x[p], y[p - d]
            if a < 4 and b < 4:
                if a == b:
                    m += 1
                else:
                    mm += 1
        out.append((d, m, mm))
    return out


_INDEX = {}


def counts_numpy(x, y):
    """the same counts for every shift at once: entry s = d + n2 - 1 sums the letter pairs (p, i) with p - i = d"""
    n1, n2 = len(x), len(y)
    if (n1, n2) not in _INDEX:
        if len(_INDEX) > 64:
            _INDEX.clear()
        _INDEX[n1, n2] = (np.arange(n1, dtype=np.int32)[:, None] - np.arange(n2, dtype=np.int32)[None, :] + (n2 - 1)).ravel()
    index = _INDEX[n1, n2]
    both = ((x < 4)[:, None] & (y < 4)[None, :]).ravel()
    same = (x[:, None] == y[None, :]).ravel()
    m = np.bincount(index[both & same], minlength=n1 + n2 - 1)
    mm = np.bincount(index[both & ~same], minlength=n1 + n2 - 1)
    return m.astype(np.int64), mm.astype(np.int64)


def best_shift(r1, r2, o):
    """one pair -> None (not found), "too_long", or (d, insert, matches, mismatches, compared)"""
    n1, n2 = len(r1), len(r2)
    if n1 > CAP or n2 > CAP:
        return "too_long"
    if not n1 or not n2:
        return None
    x, y = codes_of(r1, r2)
    m, mm = counts_numpy(x, y)
    ok = (m >= max(o["min_overlap"], 1)) & (mm <= o["max_mismatches"]) & (mm * 100 <= o["max_mismatch_percent"] * (m + mm))
    at = np.flatnonzero(ok)
    if not len(at):
        return None
    s = int(at[np.lexsort((at, -m[at], mm[at]))[0]])          # the fewest mismatches, then the most matches, then the lowest d
    d = s - (n2 - 1)
    return d, d + n2, int(m[s]), int(mm[s]), min(n1, d + n2) - max(0, d)


def _self_check():
    rng = np.random.default_rng(7)
    for _ in range(60):
        n1, n2 = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        r1, r2 = (bytes(rng.choice(list(b"ACGTacgtNU-"), n, p=[.2, .2, .2, .2, .02, .02, .02, .02, .04, .04, .04]).astype(np.uint8)) for n in (n1, n2))
        x, y = codes_of(r1, r2)
        loop = counts_loop(x, y)
        m, mm = counts_numpy(x, y)
        assert [d for d, _, _ in loop] == list(range(-(n2 - 1), n1)) and [v[1] for v in loop] == list(m) and [v[2] for v in loop] == list(mm), (r1, r2)
        o = options(min_overlap=int(rng.integers(0, 6)), max_mismatches=int(rng.integers(0, 4)), max_mismatch_percent=int(rng.integers(0, 50)))
        accepted = [(k, -a, d) for d, a, k in loop if a >= max(o["min_overlap"], 1) and k <= o["max_mismatches"] and k * 100 <= o["max_mismatch_percent"] * (a + k)]
        got = best_shift(r1, r2, o)
        assert (got is None) == (not accepted) and (got is None or (got[3], -got[2], got[0]) == min(accepted)), (r1, r2, o)


_self_check()


def expected(letters, ends, **opts):
    """-> pairs (PAIR), regions (REGION), unmerged (REGION), totals: what the rules of include/nafgpu.h give"""
    o = options(**opts)
    ends = [int(e) for e in ends]
    assert len(ends) % 2 == 0
    starts = [0] + ends[:-1]
    pairs, regions = np.zeros(len(ends) // 2, dtype=PAIR), np.zeros(len(ends), dtype=REGION)
    for j in range(len(pairs)):
        r1, r2 = letters[starts[2 * j]:ends[2 * j]], letters[starts[2 * j + 1]:ends[2 * j + 1]]
        got = best_shift(r1, r2, o)
        if got == "too_long":
            pairs[j]["too_long"] = 1
        elif got is not None:
            pairs[j] = got + (1, 0, 0)
        for m, read in enumerate((r1, r2)):
            regions[2 * j + m] = (2 * j + m, 0, min(len(read), got[1]) if pairs[j]["found"] else len(read), 0, 0)
    found = pairs["found"].astype(bool)
    unmerged = regions[np.repeat(~found, 2)]
    lengths = np.array(ends, dtype=np.int64) - np.array(starts, dtype=np.int64)
    totals = dict(n_records=len(ends), n_pairs=len(pairs), n_found=int(found.sum()), n_too_long=int(pairs["too_long"].sum()), n_unmerged=len(unmerged),
                  n_cut=int((regions["end"].astype(np.int64) < lengths).sum()), matches=int(pairs["matches"].sum()), mismatches=int(pairs["mismatches"].sum()),
                  bases_merged=int(pairs["insert"].sum()), bases_after_cut=int(regions["end"].sum()))
    return pairs, regions, unmerged, totals


def merged(records, pairs, quality_base=33, table=sc.COMPLEMENT):
    """records [(id, comment, letters, quality or None)], the pairs of expected() -> the records nafgpu_merge_pairs makes"""
    out = []
    for j, pr in enumerate(pairs):
        if not pr["found"]:
            continue
        (id_, com, r1, q1), (_, _, r2, q2) = records[2 * j], records[2 * j + 1]
        d, n1, n2 = int(pr["shift"]), len(r1), len(r2)
        s, q = bytearray(), bytearray()
        for p in range(int(pr["insert"])):
            at = n2 - 1 - (p - d)
            if p < d:
                c, v = r1[p], q1[p] if q1 else 0
            elif p >= n1:
                c, v = table[r2[at]], q2[at] if q2 else 0
            else:
                a, b, qa, qb = r1[p], table[r2[at]], q1[p] if q1 else 0, q2[at] if q2 else 0
                c = b if q1 and qb > qa else a
                v = max(qa, qb) if CODE[a] < 4 and CODE[a] == CODE[b] else min(255, quality_base + max(abs(qa - qb), 2))
            s.append(c)
            q.append(v)
        out.append((id_, com, bytes(s), bytes(q) if q1 else None))
    return out


def tables(overlaps):
    return (np.frombuffer(overlaps.pairs(), dtype=PAIR), np.frombuffer(overlaps.regions(), dtype=REGION), np.frombuffer(overlaps.unmerged_regions(), dtype=REGION))


def compare(overlaps, letters, ends, what="", **opts):
    """every table and total of an Overlaps against expected(); -> pairs, regions, unmerged, totals"""
    want = expected(letters, ends, **opts)
    assert overlaps.n_bases == len(letters) and len(overlaps) == len(want[0]), (what, overlaps.n_bases, len(letters))
    for name, mine, theirs in zip(("pairs", "regions", "unmerged_regions"), tables(overlaps), want):
        assert mine.shape == theirs.shape, (what, name, mine.shape, theirs.shape)
        if mine.tobytes() != theirs.tobytes():
            at = int(np.nonzero(mine != theirs)[0][0])
            raise AssertionError("%s: %s differs at %d of %d: %s / %s" % (what, name, at, len(theirs), mine[at], theirs[at]))
    got = {name: getattr(overlaps, name) for name in want[3]}
    assert got == want[3], (what, got, want[3])
    return want


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


def layout(recs):
    """oracle records -> letters, ends"""
    return b"".join(r[2] for r in recs), np.cumsum([len(r[2]) for r in recs], dtype=np.uint64)


def own_layout(source):
    """a Selection's (or ParsedText's, or a decode result's through `source.copy_to_host`) own bytes read back -> letters, quality, ends"""
    quality = source.copy_to_host(source.d_quality, source.n_quality) if source.d_quality else None
    return (source.copy_to_host(source.d_sequence, source.n_bases), quality,
            np.frombuffer(source.copy_to_host(source.d_record_end, 8 * source.n_records), dtype=np.uint64))


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


class DeviceBytes:
    """bytes in device memory, without any library but this one: they are the sequence of a one-record text archive, decoded by
    a decoder of its own.  pad: bytes in front, so that `address` has that residue mod 16."""

    def __init__(self, lib, data, pad=0):
        data = bytes(pad) + bytes(data)
        self._dec = open_decoder(lib, sc.hand_archive(1, ids=[b"t"], text=data or b"\0"))
        res = self._dec.decode_all_device()
        assert res.d_sequence % 16 == 0 and (not data or self._dec.copy_to_host(res.d_sequence, len(data)) == data)
        self.address = res.d_sequence + pad

    def close(self):
        self._dec.close()


def device_case(lib, what, reads, pad=0, behind=b"", **opts):
    """reads [letters] -> device buffers of this test's own -> overlap() against expected()"""
    letters = b"".join(reads)
    ends = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    bufs = [DeviceBytes(lib, letters + behind, pad), DeviceBytes(lib, ends.tobytes())]
    try:
        src = Source(d_sequence=bufs[0].address, n_bases=len(letters + behind), d_record_end=bufs[1].address, n_records=len(reads))
        with ov.overlap(src, _lib=lib, **opts) as overlaps:
            want = expected(letters, ends, **opts)
            assert overlaps.n_bases == len(letters + behind)
            for name, mine, theirs in zip(("pairs", "regions", "unmerged_regions"), tables(overlaps), want):
                assert mine.tobytes() == theirs.tobytes(), (what, name, mine[:4], theirs[:4])
            assert {name: getattr(overlaps, name) for name in want[3]} == want[3], what
            return want
    finally:
        for b in bufs:
            b.close()


def fastq(reads, quality=None):
    quality = quality or [b"I" * len(r) for r in reads]
    return b"".join(b"@r%d c%d\n%s\n+\n%s\n" % (k, k, s, q) for k, (s, q) in enumerate(zip(reads, quality)))


def text_case(lib, what, reads, **opts):
    """reads as FASTQ through parse_text(...).overlap() against expected() over the parsed bytes read back"""
    with parse_text(fastq(reads), device=0, _lib=lib) as parsed:
        letters, _, ends = own_layout(parsed)
        assert letters == b"".join(reads), what
        with parsed.overlap(**opts) as overlaps:
            return compare(overlaps, letters, ends, what=what, **opts)


def decoder_case(lib, what, reads, quality=None, fasta=False, **opts):
    """reads -> an archive -> Decoder.overlap and Decoder.merge against expected() and merged() over what the oracle decodes"""
    text = b"".join(b">r%d c%d\n%s\n" % (k, k, s) for k, s in enumerate(reads)) if fasta else fastq(reads, quality)
    archive = encode_text(text, sequence_type="dna", id=True, comment=True, sequence=True, quality=not fasta, mask=True, compression_level=1, device=0, _lib=lib)
    recs = sc.oracle_records(archive, spec_mask=True)
    letters, ends = layout(recs)
    assert [len(r[2]) for r in recs] == [len(r) for r in reads], what
    with open_decoder(lib, archive) as dec, dec.overlap(**opts) as overlaps:
        pairs, regions, unmerged, totals = compare(overlaps, letters, ends, what=what, **opts)
        want = merged(recs, pairs, options(**opts)["quality_base"])
        with dec.merge(overlaps) as sel:
            sc.compare(sel, want, fields=("id", "comment", "sequence") + (() if fasta else ("quality",)), what=what)
        return pairs, want


# ---------------------------------------------------------------- making pairs
def rc(seq):
    return seq.translate(sc.COMPLEMENT)[::-1]


def letters_of(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).astype(np.uint8))


def pair_of(rng, n1, n2, fragment, subs=0.0):
    """a fragment read from both ends, reads of n1 and n2 letters: what lies behind the fragment's end is adapter (random letters)"""
    F = len(fragment)
    r1 = bytearray(fragment[:n1] + letters_of(rng, max(0, n1 - F)))
    r2 = bytearray(rc(fragment)[:n2] + letters_of(rng, max(0, n2 - F)))
    for read in (r1, r2):
        for at in np.flatnonzero(rng.random(len(read)) < subs):
            read[at] = b"ACGT"[(b"ACGT".index(read[at]) + int(rng.integers(1, 4))) % 4]
    return bytes(r1), bytes(r2)


# ---------------------------------------------------------------- 1. the fixtures
PHIX_LIST = [0, 34, 1, 14, 2, 28, 3, 20, 5, 16, 6, 13, 8, 23, 9, 29, 15, 19, 21, 30, 4, 7]
PHIX_PAIRS = ((-6, 293, 0), (-184, 115, 0), (189, 111, 1), (88, 211, 2), (172, 129, 0), (190, 111, 0), (-25, 274, 0), (-71, 228, 0), (98, 199, 4), (34, 266, 1))
PHIX_TOTALS = ((dict(), 10, 1937, 8, 3495), (dict(max_mismatches=0), 6, 1150, 0, 1882), (dict(min_overlap=250), 3, 833, 1, 906),
               (dict(max_mismatch_percent=1), 9, 1738, 4, 3096))


def check_fixtures(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, ends = layout(recs)
    with open_decoder(lib, blob) as dec:
        with dec.overlap() as overlaps:                                         # as it lies: 21 pairs, one of them found
            pairs, regions, unmerged, totals = compare(overlaps, letters, ends, what="phix")
            assert (overlaps.n_pairs, overlaps.n_found, overlaps.n_unmerged) == (21, 1, 40) and list(np.flatnonzero(pairs["found"])) == [14]
            assert tuple(pairs[14])[:4] == (-251, int(pairs[14]["insert"]), 48, 0), pairs[14]
            with dec.merge(overlaps) as sel:
                sc.compare(sel, merged(recs, pairs), what="phix merged")
        with dec.select(PHIX_LIST) as picked:
            mine = [recs[k] for k in PHIX_LIST]
            own_letters, own_quality, own_ends = own_layout(picked)
            assert own_letters == b"".join(r[2] for r in mine)
            for opts, found, matches, mismatches, bases in PHIX_TOTALS:
                with picked.overlap(**opts) as overlaps:
                    pairs, regions, _, totals = compare(overlaps, own_letters, own_ends, what="phix list %r" % (opts,), **opts)
                    assert (overlaps.n_pairs, overlaps.n_found, overlaps.matches, overlaps.mismatches, overlaps.bases_merged) == (11, found, matches, mismatches, bases), \
                        (opts, overlaps.n_found, overlaps.matches, overlaps.mismatches, overlaps.bases_merged)
                    if not opts:
                        assert [(int(p["shift"]), int(p["matches"]), int(p["mismatches"])) for p in pairs[:10]] == list(PHIX_PAIRS) and not pairs[10]["found"]
                        kept = sum(int(regions[r]["end"]) for j in range(10) for r in (2 * j, 2 * j + 1))
                        assert (overlaps.n_cut, kept) == (8, 5448), (overlaps.n_cut, kept)
                    # swapping the mates of every pair keeps found, insert, matches and mismatches
                    swapped = [k for j in range(11) for k in (PHIX_LIST[2 * j + 1], PHIX_LIST[2 * j])]
                    with dec.select(swapped) as other, other.overlap(**opts) as again:
                        theirs = tables(again)[0]
                        for name in ("found", "insert", "matches", "mismatches"):
                            assert list(theirs[name]) == list(pairs[name]), (opts, name)
    try:                                                                        # overlaps outlive their source; closed ones are refused
        overlaps.pairs()
    except RuntimeError:
        pass
    else:
        raise AssertionError("closed overlaps were used")
    # the fixtures without qualities: FASTA, R1's letter wins
    for name in ("masked", "CP040672", "NZ_AAEN01000029"):
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob, spec_mask=True)
        recs = recs[:len(recs) & ~1]
        if not recs:
            continue
        letters, ends = layout(recs)
        with open_decoder(lib, blob) as dec, dec.select(list(range(len(recs)))) as even, even.overlap(min_overlap=4, max_mismatches=1000, max_mismatch_percent=80) as overlaps:
            compare(overlaps, letters, ends, what=name, min_overlap=4, max_mismatches=1000, max_mismatch_percent=80)
    with open_decoder(lib, golden_bytes("LuxC.naf")) as dec:                    # protein: refused by the decoder form
        try:
            dec.overlap()
        except ValueError as e:
            assert "nucleotide" in str(e), e
        else:
            raise AssertionError("a protein archive was analysed")


def check_fasta_merge(lib):
    """masked letters without qualities through Decoder.merge: R1's letter wins, case kept"""
    rng = np.random.default_rng(3)
    reads = []
    for F in (60, 100, 140, 171, 40):
        r1, r2 = pair_of(rng, 100, 90, letters_of(rng, F), subs=0.03)
        r1 = r1[:20] + r1[20:50].lower() + r1[50:]
        reads += [r1, r2[:10].lower() + r2[10:]]
    pairs, want = decoder_case(lib, "fasta pairs", reads, fasta=True, min_overlap=12)
    assert pairs["found"].sum() >= 4 and any(any(c in b"acgt" for c in r[2]) for r in want)


# ---------------------------------------------------------------- 2. the edges
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)


def check_edges(lib):
    kernel_constants()
    rng = np.random.default_rng(20250202)
    # ---- mates of every length of the list, equal and unequal both ways, cut from one fragment; every residue of the start mod 16
    reads = []
    for n1 in LENGTHS:
        for n2 in LENGTHS:
            F = max(1, int(rng.integers(max(n1, n2) // 2, n1 + n2 + 2)))
            reads += list(pair_of(rng, n1, n2, letters_of(rng, F)))
    want = device_case(lib, "lengths", reads, min_overlap=1, max_mismatches=3)
    assert want[3]["n_too_long"] == 2 * len(LENGTHS) - 1 and 40 < want[3]["n_found"] < len(reads) // 2 - 21, want[3]
    short = [r for r in reads if len(r) < 200]
    for pad in range(16):
        device_case(lib, "residue %d" % pad, short[2 * pad:2 * pad + 40], pad=pad, behind=b"ACGT" * (pad % 3), min_overlap=1 + pad)
    # letters behind the last end, runs of empty records, four pairs a workgroup with a too_long among them at every place
    some = list(pair_of(rng, 70, 80, letters_of(rng, 100)))
    long = [letters_of(rng, 1025), letters_of(rng, 30)]
    for k in range(WAVES + 1):
        want = device_case(lib, "too long at %d" % k, some * k + long + some * (2 * WAVES - k), behind=letters_of(rng, 99), min_overlap=10)
        assert list(want[0]["too_long"]) == [0] * k + [1] + [0] * (2 * WAVES - k) and want[3]["n_found"] == 2 * WAVES
    device_case(lib, "empty records", [b""] * 6 + some + [b"", b"ACGT", b"ACGT", b""] + [b""] * 20 + some, min_overlap=3)
    text_case(lib, "as text", short[:60], min_overlap=5)

    # ---- a planted overlap at EVERY shift of a 70 + 66 pair: y = x moved by d where they share letters, its complement elsewhere
    n1, n2 = 70, 66
    reads, where = [], []
    for d in range(-(n2 - 1), n1):
        x = letters_of(rng, n1)
        y = bytearray(letters_of(rng, n2))
        for p in range(max(0, d), min(n1, d + n2)):
            y[p - d] = x[p]
        reads += [x, rc(bytes(y))]
        where.append((d, min(n1, d + n2) - max(0, d)))
    pairs = text_case(lib, "a plant at every shift", reads, min_overlap=8, max_mismatches=0)[0]
    assert {d + n2 - 1 for d, _ in where} >= {63, 64, 65, n1 + n2 - 2}
    for (d, size), pr in zip(where, pairs):                                       # the loop finds the plant alone
        assert (bool(pr["found"]), int(pr["shift"]), int(pr["matches"])) == ((True, d, size) if size >= 8 else (False, 0, 0)), (d, size, pr)
    # the first and the last shift of the longest pair: one letter under one letter, every other letter pair a mismatch
    first = [b"A" + b"C" * (CAP - 1), rc(b"G" * (CAP - 1) + b"A")]
    last = [b"C" * (CAP - 1) + b"A", rc(b"A" + b"G" * (CAP - 1))]
    pairs = device_case(lib, "the outermost shifts", first + last, min_overlap=1, max_mismatches=0, max_mismatch_percent=0)[0]
    assert [(int(p["shift"]), int(p["insert"]), int(p["matches"]), int(p["compared"])) for p in pairs] == [(-(CAP - 1), 1, 1, 1), (CAP - 1, 2 * CAP - 1, 1, 1)]

    # ---- counting: one mismatch, one N, one lower-case letter and one U through every position of a 130-letter overlap
    frag = letters_of(rng, 130)
    reads = []
    for p in range(130):
        other = b"ACGT"[(b"ACGT".index(frag[p]) + 1) % 4:][:1]
        for change in (other, b"N", frag[p:p + 1].lower(), b"U" if frag[p] == ord("T") else b"u" if frag[p] == ord("A") else b"-"):
            r1 = frag[:p] + change + frag[p + 1:]
            reads += [r1, rc(frag)] if change != b"u" else [frag, rc(frag)[:129 - p] + b"u" + rc(frag)[130 - p:]]      # (an A in R1: the u goes to R2)
    pairs = text_case(lib, "one change at every position", reads, min_overlap=100)[0]
    assert all(p["found"] and p["shift"] == 0 and p["compared"] == 130 for p in pairs)
    want = [(129, 1), (129, 0), (130, 0)]
    for p in range(130):
        last = (130, 0) if frag[p] in b"TA" else (129, 0)
        assert [(int(v["matches"]), int(v["mismatches"])) for v in pairs[4 * p:4 * p + 4]] == want + [last], (p, pairs[4 * p:4 * p + 4])

    # ---- the three limits, at and one off: 45 matches and 5 mismatches in a 50-letter fragment read by mates of 50
    frag = letters_of(rng, 50)
    r1 = bytearray(frag)
    for at in (3, 11, 24, 37, 49):
        r1[at] = b"ACGT"[(b"ACGT".index(r1[at]) + 2) % 4]
    for opts, found in ((dict(min_overlap=45), True), (dict(min_overlap=46), False), (dict(min_overlap=40, max_mismatches=5), True),
                        (dict(min_overlap=40, max_mismatches=4), False), (dict(min_overlap=40, max_mismatch_percent=10), True),
                        (dict(min_overlap=40, max_mismatch_percent=9), False), (dict(min_overlap=0, max_mismatches=0, max_mismatch_percent=0), None)):
        pairs = device_case(lib, "limits %r" % (opts,), [bytes(r1), rc(frag)], **opts)[0]
        assert found is None or (bool(pairs[0]["found"]) == found and (not found or tuple(pairs[0])[:4] == (0, 50, 45, 5))), (opts, pairs)

    # ---- ties: poly-A and a period-2 repeat (the fewest mismatches, then the most matches, then the lowest d)
    pairs = text_case(lib, "ties", [b"A" * 50, b"T" * 40, b"A" * 40, b"T" * 50, b"AC" * 30, rc(b"AC" * 20), b"AC" * 30 + b"A", rc(b"CA" * 20)], min_overlap=10)[0]
    assert [(int(p["shift"]), int(p["matches"])) for p in pairs] == [(0, 40), (-10, 40), (0, 40), (1, 40)], pairs

    # ---- the merge: qualities above, equal and below on agreeing and on disagreeing letters, the floor of 2; d < 0, = 0, > 0; n1 != n2
    frag = letters_of(rng, 90)
    reads, quals = [], []
    for n1, n2, F in ((60, 60, 40), (60, 60, 60), (60, 60, 90), (70, 45, 80), (45, 70, 80), (60, 50, 30)):
        r1, r2 = pair_of(rng, n1, n2, frag[:F])
        r1 = bytearray(r1)
        for at in (2, 7, 12, 17):                                                 # four disagreeing letters inside every overlap
            r1[at] = b"ACGT"[(b"ACGT".index(r1[at]) + 1) % 4]
        r1[22:24] = b"Nn"
        q1 = bytes(40 + (i % 7) for i in range(n1))
        q2 = bytearray(40 + ((3 * i) % 7) for i in range(n2))
        y_at = lambda p: n2 - 1 - (p - (F - n2))                                  # where position p of R1 lies in R2
        for p, q in ((2, q1[2] + 9), (7, q1[7]), (12, q1[12] - 1), (17, q1[17] - 5)):
            if 0 <= y_at(p) < n2:
                q2[y_at(p)] = q
        reads += [bytes(r1), r2[:5] + r2[5:9].lower() + r2[9:]]
        quals += [q1, bytes(q2)]
    pairs, want = decoder_case(lib, "merge", reads, quals, min_overlap=15, max_mismatches=8)
    assert [int(p["shift"]) for p in pairs] == [-20, 0, 30, 35, 10, -20] and all(p["found"] for p in pairs), pairs
    assert want[1][3][2] == 33 + 9 and want[1][3][7] == 33 + 2 and want[1][3][12] == 33 + 2 and want[1][3][17] == 33 + 5      # (d = 0: positions are R1's)
    assert want[1][2][2:3] == rc(reads[3])[2:3] != reads[2][2:3] and want[1][2][7:8] == reads[2][7:8], "the higher quality wins, R1 on a tie"
    decoder_case(lib, "merge with another base", reads, quals, min_overlap=15, max_mismatches=8, quality_base=64)
    # a tile edge of the merged output inside an overlap: 40 pairs that overlap wholly, 150 letters each
    reads = []
    for _ in range(40):
        reads += list(pair_of(rng, 150, 150, letters_of(rng, 150), subs=0.01))
    quals = [bytes(rng.integers(35, 74, 150).astype(np.uint8)) for _ in reads]
    pairs, want = decoder_case(lib, "merge across a tile edge", reads, quals)
    assert all(pairs["found"]) and sum(len(r[2]) for r in want) == 6000 > TILE and TILE % 150
    check_fasta_merge(lib)


# ---------------------------------------------------------------- 3. random
def random_pairs(n_letters, seed=17, read=150):
    """pairs of `read` letters cut from a reference of 2^16 letters: fragments of 40 .. 520, 1 % substitutions, adapters of random letters"""
    rng = np.random.default_rng(seed)
    reference = letters_of(rng, 2 ** 16)
    reads = []
    for _ in range(n_letters // (2 * read)):
        F = int(rng.integers(40, 521))
        at = int(rng.integers(0, len(reference) - F))
        reads += list(pair_of(rng, read, read, reference[at:at + F], subs=0.01))
    return reads


def check_random(lib, n_letters):
    reads = random_pairs(n_letters)
    with parse_text(fastq(reads), device=0, _lib=lib) as parsed:
        letters, _, ends = own_layout(parsed)
        with parsed.overlap() as overlaps:
            pairs, _, _, totals = compare(overlaps, letters, ends, what="random, %d letters" % n_letters)
            print("overlap: %d letters, %d pairs, %d found, %.3f ms" % (len(letters), len(pairs), overlaps.n_found, overlaps.ms))
    share = totals["n_found"] / totals["n_pairs"]                                 # the loop's own share: a kernel that finds nothing cannot pass
    assert 0.25 <= share <= 0.75, share


# ---------------------------------------------------------------- 4. composition
def check_composition(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    with open_decoder(lib, blob) as dec, dec.select(PHIX_LIST) as picked:
        archive = encode_device(picked, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, mask=True, compression_level=1, device=0, _lib=lib)
    mine = sc.oracle_records(archive, spec_mask=True)
    assert [r[2] for r in mine] == [recs[k][2] for k in PHIX_LIST]
    letters, ends = layout(mine)
    with open_decoder(lib, archive) as dec, dec.overlap() as overlaps:
        pairs, regions, unmerged, totals = compare(overlaps, letters, ends, what="phix list")
        want = merged(mine, pairs)
        assert len(want) == 10 and sum(len(r[2]) for r in want) == 3495
        with dec.merge(overlaps) as sel:
            sc.compare(sel, want, what="phix list merged")
            text = b"".join(b"@%s%s\n%s\n+\n%s\n" % (r[0], b" " + r[1] if r[1] else b"", r[2], r[3]) for r in want)
            assert bytes(sel.to_text(0)) == text
            again = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, mask=True, compression_level=1, device=0, _lib=lib)
            with sel.summarize() as summary:                                    # an ordinary selection: the other jobs take it
                assert summary.n_records == 10 and summary.n_bases == 3495
        assert sc.oracle_records(again, spec_mask=True) == want
        # select(overlaps): every record cut where it reads into the adapter; select(unmerged_regions): the mates of pair 10, whole
        with dec.select(overlaps) as cut:
            sc.compare(cut, sc.cut(mine, [(int(r["record"]), int(r["start"]), int(r["end"])) for r in regions]), what="select(overlaps)")
            assert cut.n_bases == overlaps.bases_after_cut
        with dec.select(overlaps.unmerged_regions()) as rest:
            sc.compare(rest, mine[20:22], what="select(unmerged_regions)")
        # the source forms equal the decoder form
        tabs = [bytes(t) for t in tables(overlaps)]
        res = dec.decode_all_device()
        with ov.overlap(res, _lib=lib) as again:
            assert tabs == [bytes(t) for t in tables(again)]
        with parse_text(dec.to_text(), device=0, _lib=lib) as parsed, parsed.overlap() as again:
            assert tabs == [bytes(t) for t in tables(again)] and again.bases_merged == 3495
        with dec.select([3, (7, 5, 250)]) as sel:                                 # what select accepted before is read as before
            assert own_layout(sel)[0] == mine[3][2] + mine[7][2][5:250]


# ---------------------------------------------------------------- 5. refusals
def call_overlap(lib, src_fields, device=0, null_opts=False, **opts):
    src, o = _ffi.EncodeSource(**src_fields), _ffi.OverlapOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.OverlapResult(), _ffi.Error()
    rc = lib.c.nafgpu_overlap(ctypes.byref(src), None if null_opts else ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_overlaps_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_overlap_decoder(lib, dec, null_opts=False, **opts):
    o = _ffi.OverlapOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.OverlapResult(), _ffi.Error()
    rc = lib.c.nafgpu_overlap_decoder(dec._h, None if null_opts else ctypes.byref(o), ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_overlaps_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def call_merge(lib, dec, overlaps_handle, null_out=False):
    h, res, err = ctypes.c_void_p(), _ffi.SelectResult(), _ffi.Error()
    rc = lib.c.nafgpu_merge_pairs(dec._h, overlaps_handle, None if null_out else ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_selection_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    bad = _ffi.E_INVALID_ARG
    with open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        assert call_overlap(lib, good, min_overlap=30, max_mismatches=5, max_mismatch_percent=20)[0] == _ffi.OK and call_overlap(lib, good)[0] == _ffi.OK
        assert call_overlap(lib, good, null_opts=True)[0] == bad
        rc, message = call_overlap(lib, dict(good, d_sequence=None))
        assert rc == bad and "sequence" in message, (rc, message)
        for fields in (dict(good, d_record_end=None), dict(good, n_records=0)):
            rc, message = call_overlap(lib, fields)
            assert rc == bad and "record table" in message, (rc, message)
        rc, message = call_overlap(lib, dict(good, n_records=41))
        assert rc == bad and "odd" in message, (rc, message)
        rc, message = call_overlap(lib, good, max_mismatch_percent=101)
        assert rc == bad and "percent" in message and call_overlap(lib, good, max_mismatch_percent=100)[0] == _ffi.OK, (rc, message)
        src, o, h, r, err = _ffi.EncodeSource(**good), _ffi.OverlapOpts(), ctypes.c_void_p(), _ffi.OverlapResult(), _ffi.Error()
        for args in ((None, ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), ctypes.byref(o), 0, None, ctypes.byref(r)),
                     (ctypes.byref(src), ctypes.byref(o), 0, ctypes.byref(h), None)):
            assert lib.c.nafgpu_overlap(*args, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_overlaps_copy_to_host(None, None, 1, None) == bad
        lib.c.nafgpu_overlaps_free(None)
        assert call_overlap_decoder(lib, dec, null_opts=True)[0] == bad and call_overlap_decoder(lib, dec, max_mismatch_percent=101)[0] == bad
        assert call_overlap_decoder(lib, dec, min_overlap=30)[0] == _ffi.OK
        for call in (lambda: dec.overlap(max_mismatch_percent=101), lambda: dec.overlap(min_overlap=-1), lambda: dec.overlap(quality_base=256),
                     lambda: ov.overlap(Source(), _lib=lib), lambda: ov.overlap(Source(d_sequence=res.d_sequence, n_bases=res.n_bases), _lib=lib)):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("accepted")
        # ---- the merge: what select refuses, overlaps of another number of records, overlaps that do not fit these records
        with dec.overlap() as overlaps:
            assert call_merge(lib, dec, overlaps._h)[0] == _ffi.OK
            assert call_merge(lib, dec, None)[0] == bad and call_merge(lib, dec, overlaps._h, null_out=True)[0] == bad
            assert lib.c.nafgpu_merge_pairs(None, overlaps._h, ctypes.byref(h), ctypes.byref(_ffi.SelectResult()), ctypes.byref(err)) == bad
            with dec.select(list(range(40))) as fewer, fewer.overlap() as other:
                rc, message, _ = call_merge(lib, dec, other._h)
                assert rc == bad and "40 records" in message, (rc, message)
            for opts, needle in ((dict(shard_count=2), "shard"), (dict(sequence=False), "sequence")):
                with open_decoder(lib, blob, **opts) as odd:
                    rc, message, _ = call_merge(lib, odd, overlaps._h)
                    assert rc == bad and needle in message, (opts, rc, message)
            with open_decoder(lib, blob, quality=False, id=False) as plain, plain.merge(overlaps) as sel:       # fewer fields: fewer fields out
                assert sel.d_quality is None and sel.d_ids is None and sel.n_records == 1
    other = dna_archive(lib, [b"ACGTACG"] * 42)                                 # 42 records of other lengths: pair 14 of phix does not fit them
    with open_decoder(lib, blob) as dec, dec.overlap() as overlaps, open_decoder(lib, other) as small:
        rc, message, _ = call_merge(lib, small, overlaps._h)
        assert rc == bad and "pair 14 " in message, (rc, message)
        try:
            small.merge(overlaps)
        except ValueError:
            pass
        else:
            raise AssertionError("overlaps of other records were merged")
    check_end_tables(lib)
    # through a decoder: no sequence decoded; a shard; no Length section; an archive that ends early; a protein archive
    with open_decoder(lib, blob, sequence=False) as dec:
        rc, message, _ = call_overlap_decoder(lib, dec)
        assert rc == bad and "sequence" in message, (rc, message)
    with open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _ = call_overlap_decoder(lib, dec)
        assert rc == bad and "shard" in message, (rc, message)
    with open_decoder(lib, golden_bytes("LuxC.naf")) as dec:
        rc, message, _ = call_overlap_decoder(lib, dec)
        assert rc == bad and "nucleotide" in message, (rc, message)
        with dec.select(list(range(2))) as sel, sel.overlap(min_overlap=1) as overlaps:
            rc, message, _ = call_merge(lib, dec, overlaps._h)
            assert rc == bad and "nucleotide" in message, (rc, message)
    with open_decoder(lib, golden_bytes("phix.naf")) as dec, dec.select([0, 1, 2]) as sel:
        try:
            sel.overlap()
        except ValueError as e:
            assert "odd" in str(e)
        else:
            raise AssertionError("three records were paired")


def dna_archive(lib, reads):
    text = b"".join(b">r%d\n%s\n" % (k, s) for k, s in enumerate(reads))
    return encode_text(text, sequence_type="dna", id=True, comment=False, sequence=True, quality=False, mask=False, compression_level=1, device=0, _lib=lib)


def check_end_tables(lib):
    """hand-made end tables through nafgpu_overlap: a selection's letters with a table of this test's own in device memory"""
    with open_decoder(lib, golden_bytes("phix.naf")) as dec, dec.select(list(range(42))) as sel:
        n = sel.n_bases
        good = np.arange(1, 201, dtype=np.uint64) * np.uint64(10)
        assert n > 2000
        for what, change, needle, status in (("decreasing", {100: 500}, "record 100 ", _ffi.E_INVALID_LENGTH),
                                             ("decreasing, three of them", {100: 500, 60: 300, 199: 1}, "record 60 ", _ffi.E_INVALID_LENGTH),
                                             ("the last record beyond the section", {199: n + 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("far beyond", {199: 2 ** 64 - 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("the first record bad", {0: 2 ** 40}, "record 0 ", _ffi.E_INVALID_LENGTH),
                                             ("a good table", {}, "", _ffi.OK)):
            table = good.copy()
            for k, v in change.items():
                table[k] = v
            d_table = DeviceBytes(lib, table.tobytes())
            try:
                rc, message = call_overlap(lib, dict(d_sequence=sel.d_sequence, n_bases=n, d_record_end=d_table.address, n_records=len(table)), min_overlap=3)
            finally:
                d_table.close()
            assert rc == status and needle in message, (what, rc, message)
    # an archive whose records end beyond its letters, through the decoder form
    # (hand_archive writes text archives; as dna the section's size counts letters, two to a byte: ten)
    early = bytearray(sc.hand_archive(4, ids=[b"a", b"b", b"c", b"d"], lengths=[4, 4, 1, 30], text=bytes(range(10))))
    early[4] = 0
    with open_decoder(lib, bytes(early)) as dec:
        rc, message, kind = call_overlap_decoder(lib, dec)
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 3" in message, (rc, kind, message)
        try:
            dec.overlap()
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")
    with open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"NNACGTTTnn")) as dec:
        rc, message, _ = call_overlap_decoder(lib, dec)
        assert rc == _ffi.E_INVALID_ARG and "ength" in message, (rc, message)    # the Length section is needed, as for select


# ---------------------------------------------------------------- 6. positions past 2^32 (MI355X only)
def check_past_u32(lib, n_bases=2 ** 28, copies=17, read=128):
    """2^28 synthetic letters as pairs of 128-letter reads, their record list selected 17 times"""
    rng = np.random.default_rng(5)
    n_reads = n_bases // read
    reference = np.frombuffer(letters_of(rng, 2 ** 16), dtype=np.uint8)
    table = np.frombuffer(sc.COMPLEMENT, dtype=np.uint8)
    letters = np.empty((n_reads // 2, 2, read), dtype=np.uint8)
    i = np.arange(read, dtype=np.int32)[None, :]
    for lo in range(0, n_reads // 2, 2 ** 16):                                    # read 1 and read 2 of 2^16 fragments at a time
        n = min(2 ** 16, n_reads // 2 - lo)
        F = rng.integers(40, 400, n, dtype=np.int32)[:, None]
        at = rng.integers(0, 2 ** 16 - 400, n, dtype=np.int32)[:, None]
        adapter = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, 2, read))
        inside = i < F
        letters[lo:lo + n, 0] = np.where(inside, reference[at + np.minimum(i, F - 1)], adapter[:, 0])
        letters[lo:lo + n, 1] = np.where(inside, table[reference[at + np.maximum(F - 1 - i, 0)]], adapter[:, 1])
    letters = letters.tobytes()
    archive = sc.hand_archive(n_reads, ids=None, lengths=[read] * n_reads, text=letters)
    with open_decoder(lib, archive, id=False, comment=False) as dec:
        res = dec.decode_all_device()
        assert (res.n_bases, res.n_records) == (n_bases, n_reads)
        sample = 4000
        with ov.overlap(res, _lib=lib) as overlaps:
            print("overlap: %d pairs, %d letters, %d found, %.3f ms" % (overlaps.n_pairs, overlaps.n_bases, overlaps.n_found, overlaps.ms))
            pairs, regions, unmerged = (t.copy() for t in tables(overlaps))
            want = expected(letters[:sample * read], np.arange(1, sample + 1, dtype=np.uint64) * np.uint64(read))
            assert pairs[:sample // 2].tobytes() == want[0].tobytes() and regions[:sample].tobytes() == want[1].tobytes()
            assert 0.25 * len(pairs) < overlaps.n_found < 0.75 * len(pairs) and int(pairs["found"].sum()) == overlaps.n_found
            one = (overlaps.n_found, overlaps.n_unmerged, overlaps.n_cut, overlaps.matches, overlaps.mismatches, overlaps.bases_merged, overlaps.bases_after_cut)
        del letters
        with dec.select(list(range(n_reads)) * copies) as sel:
            assert sel.n_bases == copies * n_bases > 2 ** 32
            with sel.overlap() as overlaps:
                print("overlap past 2^32: %d pairs, %d letters, %d found, %.3f ms" % (overlaps.n_pairs, overlaps.n_bases, overlaps.n_found, overlaps.ms))
                assert overlaps.n_records == copies * n_reads and overlaps.n_bases == copies * n_bases
                assert (overlaps.n_found, overlaps.n_unmerged, overlaps.n_cut, overlaps.matches, overlaps.mismatches, overlaps.bases_merged,
                        overlaps.bases_after_cut) == tuple(copies * v for v in one)
                all_pairs, all_regions, all_unmerged = tables(overlaps)
                for c in range(copies):                                           # copy c: the tables of copy 0, the record shifted
                    assert all_pairs[c * len(pairs):(c + 1) * len(pairs)].tobytes() == pairs.tobytes(), c
                    for mine, theirs in ((all_regions, regions), (all_unmerged, unmerged)):
                        shifted = theirs.copy()
                        shifted["record"] += np.uint64(c * n_reads)
                        assert mine[c * len(theirs):(c + 1) * len(theirs)].tobytes() == shifted.tobytes(), c
