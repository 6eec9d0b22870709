"""Shared by tests/test_search_emu.py (CPU harness) and tests/test_gpu_search.py (MI355X): Decoder.search, Selection.search,
ParsedText.search and search(), records in device memory -> where a set of patterns occurs, as regions for Decoder.select.
Not a test module; every function takes the library binding it is to check.

The yardstick is expected() below: numpy over what the CPU oracle decodes (or over a selection's own bytes read back), the
rules of include/nafgpu.h restated.  The three tables are compared for equality as struct and uint64 arrays: integer work,
no tolerance."""
import ctypes
import importlib
import io
import os

import numpy as np

import encode_checks as ec
import select_checks as sc
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Record, encode_device, parse_text

sr = importlib.import_module("nafcodec_amd.search")          # (the module: the package's attribute of that name is its search())

ENTRY_POINTS = ("nafgpu_search", "nafgpu_search_decoder", "nafgpu_hits_copy_to_host", "nafgpu_hits_free")
TILE, LANE, HALO = 4096, 16, 64      # nafcodec_amd/csrc/search.h (kSearchTile, kSearchHalo) and search.hip (16 starts per lane): asserted below
REGION, INFO = np.dtype(sr.REGION), np.dtype(sr.INFO)
assert REGION.itemsize == ctypes.sizeof(_ffi.Region) == 32 and INFO.itemsize == ctypes.sizeof(_ffi.HitInfo) == 8
FIXTURES = ("phix", "masked", "LuxC", "CP040672", "NZ_AAEN01000029")


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sc.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "search.h")) as f:
        text = f.read()
        assert "constexpr uint32_t kSearchTile = %d;" % TILE in text and "constexpr uint32_t kSearchHalo = %d;" % HALO in text
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "search.hip")) as f:
        text = f.read()
        assert "constexpr uint32_t kThreads = %d;" % (TILE // LANE) in text
        assert "static_assert(kSearchTile == kThreads * %d" % LANE in text
    assert (sr.MAX_PATTERNS, sr.MAX_LENGTH, sr.MAX_MISMATCHES) == (16, 64, 3) and HALO >= sr.MAX_LENGTH - 1


# ---------------------------------------------------------------- the yardstick
SETS = np.zeros(256, dtype=np.uint8)             # a letter's set: A 1, C 2, G 4, T and U 8, the IUPAC codes their unions; else empty
for _letter, _set in zip("ACGTURYKMSWBDHVN", (1, 2, 4, 8, 8, 5, 10, 12, 3, 6, 9, 14, 13, 11, 7, 15)):
    SETS[ord(_letter)] = SETS[ord(_letter.lower())] = _set
REVERSE4 = np.array([int("{:04b}".format(c)[::-1], 2) for c in range(16)], dtype=np.uint8)   # the complement: the four bits reversed


def as_bytes(pattern):
    return pattern.encode() if isinstance(pattern, str) else bytes(pattern)


def mismatches(text, pattern, nucleotide=True, reverse=False):
    """-> for every window start of `text` (uint8 array) the number of positions that do not accept their letter"""
    m = len(pattern)
    p = np.frombuffer(pattern, dtype=np.uint8)
    out = np.zeros(max(len(text) - m + 1, 0), dtype=np.int16)
    if nucleotide:
        sets, text = (REVERSE4[SETS[p]][::-1] if reverse else SETS[p]), SETS[text]
    for j in range(m if len(out) else 0):
        t = text[j:j + len(out)]
        out += ((t == 0) | ((t & ~sets[j]) != 0)) if nucleotide else (t != p[j])
    return out


def expected(letters, ends, patterns, max_mismatches=0, both_strands=True, nucleotide=True, cache=None):
    """-> regions (REGION), info (INFO), record_hit_begin (uint64), pattern_hits: what the rules of include/nafgpu.h give.
    cache: a dict the caller keeps for ONE text: the mismatch counts of a pattern are computed once for every max_mismatches"""
    text = np.frombuffer(letters, dtype=np.uint8)
    ends = np.asarray(ends, dtype=np.uint64).astype(np.int64) if ends is not None and len(ends) else np.array([len(text)], dtype=np.int64)
    text = text[:int(ends[-1])]                                                 # letters behind the last record end are not searched
    begins = np.concatenate(([0], ends[:-1]))
    found = []
    for p, pattern in enumerate(as_bytes(q) for q in patterns):
        for strand in range(2 if both_strands else 1):
            key = (pattern, strand, nucleotide, len(text))
            miss = cache[key] if cache is not None and key in cache else mismatches(text, pattern, nucleotide, bool(strand))
            if cache is not None:
                cache[key] = miss
            start = np.nonzero(miss <= max_mismatches)[0]
            record = np.searchsorted(ends, start, side="right")                 # the first record that ends behind the start: empty ones are skipped
            inside = start + len(pattern) <= ends[record]                       # a window never crosses a record end
            start, record = start[inside], record[inside]
            found.append(np.stack([start, np.full_like(start, p), np.full_like(start, strand), miss[start], record,
                                   start - begins[record], np.full_like(start, len(pattern))], axis=1))
    found = np.concatenate(found)
    found = found[np.lexsort((found[:, 2], found[:, 1], found[:, 0]))]          # (absolute start, pattern, strand with + first)
    regions, info = np.zeros(len(found), dtype=REGION), np.zeros(len(found), dtype=INFO)
    regions["record"], regions["start"], regions["end"], regions["reverse_complement"] = found[:, 4], found[:, 5], found[:, 5] + found[:, 6], found[:, 2]
    info["pattern"], info["mismatches"] = found[:, 1], found[:, 3]
    begin = np.searchsorted(found[:, 4], np.arange(len(ends) + 1), side="left").astype(np.uint64)
    return regions, info, begin, tuple(int((found[:, 1] == p).sum()) for p in range(len(patterns)))


def tables(hits):
    return np.frombuffer(hits.regions(), dtype=REGION), np.frombuffer(hits.info(), dtype=INFO), np.frombuffer(hits.record_hit_begin(), dtype=np.uint64)


def compare(hits, letters, ends, patterns, what="", **rules):
    """every table of a Hits against expected(); -> the tables"""
    regions, info, begin, per_pattern = expected(letters, ends, patterns, **rules)
    got = tables(hits)
    assert hits.n_hits == len(regions) == len(hits), (what, "n_hits", hits.n_hits, len(regions))
    assert hits.n_records == len(begin) - 1 and hits.n_bases == len(letters), (what, hits.n_records, hits.n_bases)
    for name, mine, want in zip(("regions", "info", "record_hit_begin"), got, (regions, info, begin)):
        assert mine.shape == want.shape, (what, name, mine.shape, want.shape)
        if mine.tobytes() != want.tobytes():
            at = int(np.nonzero(mine != want)[0][0])
            raise AssertionError("%s: %s differs at %d of %d: %s / %s" % (what, name, at, len(want), mine[at], want[at]))
    assert hits.pattern_hits == per_pattern, (what, hits.pattern_hits, per_pattern)
    return got


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


def layout(recs):
    """oracle records -> letters, ends"""
    return b"".join(r[2] for r in recs), np.cumsum([len(r[2]) for r in recs], dtype=np.uint64)


def own_layout(source):
    """a Selection's (or ParsedText's) own bytes read back -> letters, ends"""
    return source.copy_to_host(source.d_sequence, source.n_bases), np.frombuffer(source.copy_to_host(source.d_record_end, 8 * source.n_records), dtype=np.uint64)


def reverse_complement(pattern):
    return as_bytes(pattern).translate(sc.COMPLEMENT)[::-1]


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


# ---------------------------------------------------------------- 1. the fixtures
PATTERN_SETS = (["AGATCGGAAGAGC", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"], ["GAATTC", "GGATCC", "RAATTY", "CCWGGNNNNNNNNNNNNNNN"],
                ["ACGTNNRY", "ttgaca", "TATAAT", "UUGACA", "GATC", "A" * 17, "TTGACANNNNNNNNNNNNNNNNNTATAAT"])


def specific(pattern, k):
    """a pattern is searched with k substitutions when 5 k + 4 of its letters are no N: chance windows stay few, so that the
    yardstick over a 5.5-Mbase fixture takes a second and not a minute (the densest outputs are check_edges' business)"""
    return sum(c not in b"Nn" for c in as_bytes(pattern)) >= 5 * k + 4


def check_fixtures(lib):
    for name in FIXTURES:
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob)
        letters, ends = layout(recs)
        nucleotide = name != "LuxC"
        cache = {}
        with open_decoder(lib, blob) as dec:
            if not nucleotide:                                                  # a protein: the bytes alphabet, taken from the archive
                # (a pattern takes part at k substitutions when it is longer than k: the rules refuse the others)
                sets = ([letters[40:52], letters[5:6], b"MK", letters[-9:], b"MKLV"], [letters[100:164], b"LL", letters[200:204]])
                for patterns in sets:
                    for k in range(4):
                        use = [q for q in patterns if len(q) > k]
                        assert len(use) >= 2 and min(map(len, use)) > k
                        with dec.search(use, max_mismatches=k) as hits:
                            compare(hits, letters, ends, use, what="%s %r k=%d" % (name, use, k), nucleotide=False, both_strands=False,
                                    max_mismatches=k, cache=cache)
                        assert hits.n_hits > 0
                continue
            # a window of the fixture's own with two letters changed: found from two substitutions on, with 2 recorded
            own = bytearray(c if c in b"ACGT" else ord("N") for c in letters[1000:1024].upper())
            for j in (3, 20):
                own[j] = ord("C") if own[j] == ord("A") else ord("A")
            small = [["N" * 20, "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"]] if len(letters) < 100_000 else []
            for patterns in list(PATTERN_SETS) + [[bytes(own)]] + small:
                for k in range(4):
                    use = [q for q in patterns if specific(q, k) or patterns in small]
                    if not use or (patterns in small and k):
                        continue
                    with dec.search(use, max_mismatches=k) as hits:
                        regions, info, _ = compare(hits, letters, ends, use, what="%s %r k=%d" % (name, use, k), max_mismatches=k, cache=cache)
                    if use == [bytes(own)]:
                        at = np.searchsorted(ends, 1000, side="right")
                        mine = (regions["record"] == at) & (regions["start"] == 1000 - (int(ends[at - 1]) if at else 0)) & (regions["reverse_complement"] == 0)
                        assert int(mine.sum()) == (1 if k >= 2 and int(ends[at]) >= 1024 else 0) and (not mine.any() or int(info["mismatches"][mine][0]) == 2), (name, k)
            with dec.search(["GATC", "GAATTC"], both_strands=False) as hits:
                compare(hits, letters, ends, ["GATC", "GAATTC"], what=name + ", one strand", both_strands=False, cache=cache)
            # every set at every k, N-rich and short patterns included, on the fixture's first 20 000 letters (a selection)
            head, total = [], 0
            for r, rec in enumerate(recs):
                if total >= 20_000:
                    break
                head.append((r, 0, min(len(rec[2]), 20_000 - total)))
                total += head[-1][2]
            with dec.select(head) as sel:
                own_letters, own_ends = own_layout(sel)
                assert own_letters == b"".join(recs[r][2][:e] for r, _, e in head) and len(own_letters) == min(20_000, len(letters))
                slice_cache = {}
                for patterns in PATTERN_SETS:
                    for k in range(4):
                        with sel.search(patterns, max_mismatches=k) as hits:
                            compare(hits, own_letters, own_ends, patterns, what="%s, the first letters, %r k=%d" % (name, patterns, k), max_mismatches=k,
                                    cache=slice_cache)
                        assert k < 2 or "GATC" not in patterns or hits.n_hits > 100   # (short patterns: chance windows in plenty)
        try:                                                                    # hits outlive their source; closed ones are refused
            hits.regions()
        except RuntimeError:
            pass
        else:
            raise AssertionError("closed hits were used")
    # two answers written out as numbers
    with open_decoder(lib, golden_bytes("phix.naf")) as dec:
        with dec.search(["AGATCGGAAGAGC"]) as hits:
            regions, info, begin = tables(hits)
            assert hits.n_hits == 1 and hits.pattern_hits == (1,)
            assert tuple(regions[0])[:4] == (14, 221, 234, 0) and tuple(info[0])[:2] == (0, 0), (regions, info)
            assert list(begin[14:16]) == [0, 1]
        with dec.search(["AGATCGGAAGAGC"], max_mismatches=3) as hits:
            regions, info, _ = tables(hits)
            assert hits.n_hits == 4 and int((info["mismatches"] == 0).sum()) == 1, (regions, info)
    with open_decoder(lib, golden_bytes("masked.naf")) as dec, dec.search(["GAATTC"]) as hits:
        regions, info, _ = tables(hits)
        assert [tuple(r)[:4] for r in regions] == [(0, 1295, 1301, 0), (0, 1295, 1301, 1)], regions
    recs = sc.oracle_records(golden_bytes("masked.naf"))
    lower = next(r[2][i:i + 12] for r in recs for i in range(len(r[2]) - 12) if r[2][i:i + 12].islower())
    with open_decoder(lib, golden_bytes("masked.naf")) as dec, dec.search([lower.upper()], both_strands=False) as hits:
        assert hits.n_hits >= 1                                                 # the soft mask does not hide a hit


# ---------------------------------------------------------------- 2. the edges
def archive_of(lib, records):
    """hand-built records (bytes) -> an archive written by the host Encoder, what the oracle reads from it"""
    blob = ec.host_archive(lib, [Record(id="r%d" % k, comment="", sequence=r.decode()) for k, r in enumerate(records)], "dna", 1,
                           id=True, comment=True, sequence=True, mask=True)
    recs = sc.oracle_records(blob)
    assert [r[2].upper() for r in recs] == [bytes(r).upper() for r in records]   # (which letters come back lower case is the reference's mask rule)
    return blob, recs


def split(rng, text, longest=3000, empties=True):
    """text cut into records of 0 .. longest letters"""
    out, at = [], 0
    while at < len(text):
        l = int(rng.integers(0, longest + 1)) if empties or at else int(rng.integers(1, longest + 1))
        out.append(bytes(text[at:at + l]))
        at += l
    return out


def case(lib, what, records, patterns, assert_hits=None, **rules):
    """records -> archive -> Decoder.search against expected() over what the oracle decodes; -> the tables"""
    blob, recs = archive_of(lib, records)
    letters, ends = layout(recs)
    kwargs = dict(max_mismatches=rules.get("max_mismatches", 0), both_strands=rules.get("both_strands", True))
    with open_decoder(lib, blob) as dec, dec.search(patterns, **kwargs) as hits:
        got = compare(hits, letters, ends, patterns, what=what, **rules)
        if assert_hits is not None:
            assert hits.n_hits == assert_hits, (what, hits.n_hits, assert_hits)
    return got


def substituted(rng, pattern, where):
    out = bytearray(pattern)
    for j in where:
        out[j] = rng.choice([c for c in b"ACGT" if c != out[j]])
    return bytes(out)


def check_edges(lib):
    kernel_constants()
    rng = np.random.default_rng(20241019)
    # pattern lengths; the section's first and last letter; every offset around a tile edge and around a lane edge
    for m in (1, 2, 15, 16, 17, 63, 64):
        pattern = ec.letters(rng, b"ACGT", m)
        text = bytearray(ec.letters(rng, b"ACGT", TILE * (m + 1) + 200))
        starts = [0, len(text) - m] + [TILE * j - m + (j - 1) for j in range(1, m + 2)] + [112 + 80 * i + i for i in range(LANE + 1)]
        for at in starts:
            text[at:at + m] = pattern
        assert {s - TILE * (1 + i) for i, s in enumerate(starts[2:m + 3])} == set(range(-m, 1)) and {s % LANE for s in starts[m + 3:]} == set(range(LANE))
        regions, _, _ = case(lib, "one record, m = %d" % m, [bytes(text)], [pattern], both_strands=False)
        assert set(starts) <= set(int(s) for s in regions["start"])
        case(lib, "records, m = %d" % m, split(rng, text), [pattern, "N" * m], max_mismatches=1 if m > 1 else 0)
    # windows and record ends: records of 0, 1, m - 1, m letters, runs of empty records, every start of every record (all-N)
    for m in (1, 5, 16, 64):
        lengths = [0, 1, m - 1, m, 0, 0, 0, m + 1, 0] + [0] * 300 + [m, m, 2 * m, 1, 0, 3 * m + 7, TILE - 3 * m, m, TILE + 1, 0, 0]
        records = [ec.letters(rng, b"ACGTacgtNRY", l) for l in lengths]
        regions, _, begin = case(lib, "record ends, m = %d" % m, records, ["N" * m], both_strands=False,
                                 assert_hits=sum(max(l - m + 1, 0) for l in lengths))
        assert [int(b - a) for a, b in zip(begin[:-1], begin[1:])] == [max(l - m + 1, 0) for l in lengths]
    # a window that ends exactly at a record end is a hit; one letter past it is none
    pattern = b"GATTACAGATTACA"
    regions, _, _ = case(lib, "at and past a record end", [b"CC" + pattern, b"CC" + pattern[:-1], pattern[-1:] + b"CCC", b"", pattern[:3], pattern[3:]],
                         [pattern], both_strands=False, assert_hits=1)
    assert tuple(regions[0])[:3] == (0, 2, 2 + len(pattern))
    # overlapping hits
    case(lib, "homopolymer", [b"A" * 100, b"a" * 3, b"T" * 5], ["AAAA"], assert_hits=97 + 2)
    # the densest output: sixteen patterns of all-N on both strands over two full tiles (32 hits per position)
    lengths = [1 + 4 * p for p in range(16)]
    regions, info, _ = case(lib, "sixteen all-N patterns", [ec.letters(rng, b"ACGT", 2 * TILE)], ["N" * l for l in lengths],
                            assert_hits=sum(2 * (2 * TILE - l + 1) for l in lengths))
    assert list(info["pattern"][:32]) == [p for p in range(16) for _ in range(2)] and list(regions["reverse_complement"][:32]) == [0, 1] * 16
    # exactly d substitutions, in the first and in the last pattern position: d <= k is a hit, d = k + 1 is none
    pattern = ec.letters(rng, b"ACGT", 24)
    text, planted = bytearray(ec.letters(rng, b"ACGT", 3 * TILE)), {}
    for d in range(5):
        for side, anchor in enumerate((0, len(pattern) - 1)):
            where = ([anchor] + [3 + 4 * i for i in range(d - 1)]) if d else []
            at = TILE - 300 + 60 * (2 * d + side) + (d + side)       # (around the first tile edge, at changing residues)
            text[at:at + len(pattern)] = substituted(rng, pattern, where)
            planted[at] = d
    for k in range(4):
        regions, info, _ = case(lib, "substitutions, k = %d" % k, [bytes(text)], [pattern], max_mismatches=k, both_strands=False)
        got = {int(r["start"]): int(i["mismatches"]) for r, i in zip(regions, info)}
        assert {at: d for at, d in planted.items() if d <= k}.items() <= got.items() and not any(at in got for at, d in planted.items() if d > k), (k, got)
    # IUPAC both ways
    text = b"AGRN-CTYacgtrynWSKMBDHV"
    for pattern, want in ((b"R", [0, 1, 2, 8, 10, 12]), (b"N", [i for i in range(len(text)) if i != 4]), (b"A", [0, 8]), (b"Y", [5, 6, 7, 9, 11, 13])):
        regions, _, _ = case(lib, "IUPAC %r" % pattern, [text], [pattern], both_strands=False)
        assert [int(s) for s in regions["start"]] == want, (pattern, regions["start"])
    case(lib, "IUPAC patterns", [text, text[::-1], ec.letters(rng, b"AGRN-CTY", 500)], ["RYN", "NRY", "ARN", "NN", "AG", "RR"], max_mismatches=1)
    # U against T, either case: ACGTTGCA lies at 0 and 8 and its reverse complement TGCAACGT at 4; TGCA, its own reverse
    # complement, at 4 and 12 on either strand
    case(lib, "U and T", [b"ACGTTGCAacgttgca"], ["ACGUUGCA", "acguugca", "UGCA"], assert_hits=3 + 3 + 4)
    # a pattern that lies there only as its reverse complement; duplicate patterns
    pattern = b"AAACCCGGTAC"
    regions, info, _ = case(lib, "reverse strand only", [b"TT" + reverse_complement(pattern) + b"TT"], [pattern], assert_hits=1)
    assert tuple(regions[0])[:4] == (0, 2, 2 + len(pattern), 1)
    regions, info, _ = case(lib, "duplicates", [b"TTGATTACATT"], ["GATTACA", "GATTACA"], both_strands=False, assert_hits=2)
    assert list(info["pattern"]) == [0, 1]
    # zero hits
    regions, _, begin = case(lib, "zero hits", [b"ACGT" * 50, b"", b"ACG"], ["GGGGGGGG"], assert_hits=0)
    assert list(begin) == [0, 0, 0, 0]
    # unaligned sources: a selection with odd starts; no record table, letters behind the last end, every residue of the pointer
    blob = sc.edge_archive(lib)
    recs = sc.oracle_records(blob)
    big = [len(r[2]) for r in recs].index(9000)
    patterns = ["ACG", "NNNNNNNNNNNNNNNNN", recs[big][2][250:270].replace(b"-", b"N")]
    with open_decoder(lib, blob) as dec:
        with dec.search(patterns, max_mismatches=1) as hits:
            compare(hits, *layout(recs), patterns, what="the edge archive", max_mismatches=1)
        with dec.select([(big, 200 + r, 200 + r + 37 + r) for r in range(LANE)] + [(big, 1, 8999), (big, 3, 3), (big, 7, 7 + TILE)]) as sel:
            letters, ends = own_layout(sel)
            with sel.search(patterns, max_mismatches=1) as hits:
                compare(hits, letters, ends, patterns, what="a selection with odd starts", max_mismatches=1)
            for r in range(LANE):
                src = Source(d_sequence=sel.d_sequence + r, n_bases=sel.n_bases - r - (r % 3))
                with sr.search(src, patterns, _lib=lib) as hits:
                    assert hits.n_records == 1
                    compare(hits, letters[r:len(letters) - r % 3], None, patterns, what="no record table, the pointer at residue %d" % r)
            src = Source(d_sequence=sel.d_sequence, n_bases=sel.n_bases, d_record_end=sel.d_record_end, n_records=sel.n_records - 2)
            with sr.search(src, patterns, _lib=lib) as hits:
                assert hits.n_bases == len(letters) > int(ends[-3])
                regions, _, _ = compare(hits, letters, ends[:-2], patterns, what="letters behind the last end")
            src.n_records = 0                                                   # the table is there, but of no record: the whole section is record 0
            with sr.search(src, patterns, _lib=lib) as hits:
                compare(hits, letters, None, patterns, what="n_records = 0")


# ---------------------------------------------------------------- 3. random
def random_case(n, seed=7):
    rng = np.random.default_rng(seed)
    text = np.frombuffer(ec.letters(rng, b"ACGT", n), dtype=np.uint8).copy()
    text[rng.random(n) < 0.01] = ord("N")
    text = text.tobytes()
    lengths = []
    while sum(lengths) < n:
        lengths.append(min(int(rng.integers(0, 3001)), n - sum(lengths)))
    patterns = []
    for i in range(8):
        m = int(rng.integers(8, 13))
        at = int(rng.integers(0, n - m))
        patterns.append(text[at:at + m].replace(b"N", b"A") if i % 2 == 0 else ec.letters(rng, b"ACGT", m))
    return text, lengths, patterns


def check_random(lib, n):
    text, lengths, patterns = random_case(n)
    fasta = b"".join(b">r%d\n" % k + text[e - l:e] + b"\n" for k, (l, e) in enumerate(zip(lengths, np.cumsum(lengths))))
    with parse_text(fasta, device=0, _lib=lib) as parsed:
        letters, ends = own_layout(parsed)
        assert letters == text and [int(e) for e in ends] == [int(e) for e in np.cumsum(lengths)]
        with parsed.search(patterns, max_mismatches=1) as hits:
            compare(hits, letters, ends, patterns, what="random, %d letters" % n, max_mismatches=1)
            assert hits.n_hits > 8 and all(c > 0 for c in hits.pattern_hits[::2])
            print("search: %d letters, %d records, %d hits, %.3f ms" % (n, len(lengths), hits.n_hits, hits.ms))


# ---------------------------------------------------------------- 4. composition
def check_composition(lib):
    # select(hits): every record of the selection matches its pattern as written within its recorded mismatch count
    for name, patterns, k in (("masked", ["GAATTC", "RAATTY", "ACGTNNRY", "ttgaca"], 1), ("phix", ["AGATCGGAAGAGC", "GATC"], 2)):
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob)
        with open_decoder(lib, blob) as dec, dec.search(patterns, max_mismatches=k) as hits:
            regions, info, begin = compare(hits, *layout(recs), patterns, what=name, max_mismatches=k)
            assert hits.n_hits > 4 and regions["reverse_complement"].any() and not regions["reverse_complement"].all()
            assert np.array_equal(begin, np.searchsorted(regions["record"], np.arange(len(recs) + 1)).astype(np.uint64))
            with dec.select(hits) as sel:
                letters, ends = own_layout(sel)
                assert sel.n_records == hits.n_hits
                want = sc.cut(recs, [(int(r["record"]), int(r["start"]), int(r["end"]), "-" if r["reverse_complement"] else "+") for r in regions])
                assert letters == b"".join(w[2] for w in want)
                for i, (e, row) in enumerate(zip(ends, info)):
                    pattern = as_bytes(patterns[row["pattern"]])
                    window = np.frombuffer(letters[int(e) - len(pattern):int(e)], dtype=np.uint8)
                    assert len(window) == len(pattern) and list(mismatches(window, pattern)) == [row["mismatches"]], (name, i, bytes(window), pattern, row)
            # the buffer forms of select: bytes, a numpy array, a memoryview give what the tuples give
            some = regions[:7]
            tuples = [(int(r["record"]), int(r["start"]), int(r["end"]), "-" if r["reverse_complement"] else "+") for r in some]
            with dec.select(tuples) as a, dec.select(some.tobytes()) as b, dec.select(some.copy()) as c, dec.select(memoryview(some.tobytes())) as d:
                assert own_layout(a)[0] == own_layout(b)[0] == own_layout(c)[0] == own_layout(d)[0] and a.n_records == b.n_records == c.n_records == 7
            with dec.select(b"") as none:
                assert none.n_records == 0
            # an array of integers is a list of records, as before: four indices select four records, not one region of 32 bytes
            for indices in (np.arange(4), np.array([1, 0, 1, 0], dtype=np.int64), np.flatnonzero(np.ones(len(recs), dtype=bool))[:5], np.arange(4, dtype=np.uint32)):
                k = [int(v) % len(recs) for v in indices]
                with dec.select(np.asarray(k, dtype=indices.dtype)) as by_array, dec.select(k) as by_list:
                    assert by_array.n_records == len(k) and own_layout(by_array)[0] == own_layout(by_list)[0] == b"".join(recs[v][2] for v in k)
            try:
                dec.select(some.tobytes()[:-1])
            except ValueError:
                pass
            else:
                raise AssertionError("a buffer of 31 bytes short of whole regions was accepted")
    # Selection.search and ParsedText.search equal Decoder.search on the same letters
    blob = golden_bytes("phix.naf")
    patterns = ["AGATCGGAAGAGC", "GATC", "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"]
    with open_decoder(lib, blob) as dec, dec.search(patterns, max_mismatches=2) as hits:
        mine = [bytes(t) for t in tables(hits)] + [hits.pattern_hits, hits.n_records, hits.n_bases]
        with dec.select(list(range(hits.n_records))) as sel, sel.search(patterns, max_mismatches=2) as again:
            assert mine == [bytes(t) for t in tables(again)] + [again.pattern_hits, again.n_records, again.n_bases]
        text = dec.to_text()
        with parse_text(text, device=0, _lib=lib) as parsed, parsed.search(patterns, max_mismatches=2) as again:
            assert mine == [bytes(t) for t in tables(again)] + [again.pattern_hits, again.n_records, again.n_bases]
    # the adapter-trim pipeline: reads cut at the adapter's first hit, encoded again, read back through the oracle
    recs = sc.oracle_records(blob)
    with open_decoder(lib, blob) as dec, dec.search(["AGATCGGAAGAGC"], max_mismatches=1) as hits:
        first = hits.record_hit_begin()
        start = np.frombuffer(hits.regions(), dtype=REGION)["start"]
        cut = [(k, 0, int(start[first[k]]) if first[k] < first[k + 1] else None) for k in range(hits.n_records)]
        assert sum(c[2] is not None for c in cut) >= 1 and cut[14] == (14, 0, 221)
        with dec.select(cut) as sel:
            archive = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, mask=True, compression_level=1,
                                    device=0, _lib=lib)
    trimmed = sc.oracle_records(archive, spec_mask=True)
    assert trimmed == sc.cut(recs, cut) and len(trimmed[14][2]) == 221 and b"AGATCGGAAGAGC" not in trimmed[14][2]


# ---------------------------------------------------------------- 5. refusals
def call_search(lib, src_fields, patterns, n_patterns=None, device=0, **opts):
    blob = patterns if isinstance(patterns, bytes) else b"".join(as_bytes(p) + b"\0" for p in patterns)
    n = n_patterns if n_patterns is not None else len(patterns)
    src, o = _ffi.EncodeSource(**src_fields), _ffi.SearchOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.SearchResult(), _ffi.Error()
    rc = lib.c.nafgpu_search(ctypes.byref(src), blob, len(blob), n, ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_hits_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_search_decoder(lib, dec, patterns, opts=None):
    blob = b"".join(as_bytes(p) + b"\0" for p in patterns)
    h, res, err = ctypes.c_void_p(), _ffi.SearchResult(), _ffi.Error()
    rc = lib.c.nafgpu_search_decoder(dec._h, blob, len(blob), len(patterns), ctypes.byref(opts) if opts else None, ctypes.byref(h), ctypes.byref(res),
                                     ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_hits_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind, res.n_hits


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, ends = layout(recs)
    with open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        bad = _ffi.E_INVALID_ARG
        assert call_search(lib, good, ["GATC"])[0] == _ffi.OK
        # the number of patterns and their framing
        assert call_search(lib, good, [])[0] == bad and call_search(lib, good, ["ACGT"] * 17)[0] == bad and call_search(lib, good, ["ACGT"] * 16)[0] == _ffi.OK
        for blob_, n in ((b"ACGT", 1), (b"ACGT\0GG", 2), (b"ACGT\0", 2), (b"ACGT\0GG\0", 1), (b"", 1)):
            rc, message = call_search(lib, good, blob_, n_patterns=n)
            assert rc == bad and "NUL-terminated" in message, (blob_, rc, message)
        # a pattern that is empty or too long; the lowest index is named
        for patterns, index in ((["ACGT", "", "GG", ""], 1), (["ACGT", "AC", "A" * 65, ""], 2), (["A" * 64, "A" * 65], 1), ([""], 0)):
            rc, message = call_search(lib, good, patterns)
            assert rc == bad and "pattern %d:" % index in message, (patterns, rc, message)
        assert call_search(lib, good, ["A" * 64])[0] == _ffi.OK
        # letters the nucleotide alphabet does not have (the bytes alphabet takes them)
        for patterns, index in ((["ACGT", "ACGX", "AC-T"], 1), (["ACG T"], 0), (["acgturykmswbdhvn", "ACGTURYKMSWBDHVN", "ACGE"], 2), (["AC*"], 0)):
            rc, message = call_search(lib, good, patterns)
            assert rc == bad and "pattern %d:" % index in message, (patterns, rc, message)
            assert call_search(lib, good, patterns, alphabet=1)[0] == _ffi.OK
        # mismatches
        assert call_search(lib, good, ["ACGTACGT"], max_mismatches=4)[0] == bad and call_search(lib, good, ["ACGTACGT"], max_mismatches=3)[0] == _ffi.OK
        for patterns, k, rc_want in ((["ACGTACGT", "AC"], 2, bad), (["ACGTACGT", "ACG"], 2, _ffi.OK), (["A"], 1, bad), (["ACG"], 3, bad)):
            rc, message = call_search(lib, good, patterns, max_mismatches=k)
            assert rc == rc_want and (rc == _ffi.OK or "max_mismatches" in message), (patterns, k, rc, message)
        # the alphabet and the strands
        assert call_search(lib, good, ["ACGT"], alphabet=1, both_strands=1)[0] == bad and call_search(lib, good, ["ACGT"], alphabet=2)[0] == bad
        # no letters, null arguments
        assert call_search(lib, dict(good, d_sequence=None), ["ACGT"])[0] == bad
        src, h, r, err = _ffi.EncodeSource(**good), ctypes.c_void_p(), _ffi.SearchResult(), _ffi.Error()
        for args in ((None, b"A\0", 2, 1, None, 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), b"A\0", 2, 1, None, 0, None, ctypes.byref(r)),
                     (ctypes.byref(src), b"A\0", 2, 1, None, 0, ctypes.byref(h), None), (ctypes.byref(src), None, 2, 1, None, 0, ctypes.byref(h), ctypes.byref(r))):
            assert lib.c.nafgpu_search(*args, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_hits_copy_to_host(None, None, 1, None) == bad
        lib.c.nafgpu_hits_free(None)
        # max_hits: one below the true count is refused and the message gives the count, the count itself is accepted
        with dec.search(["GATC"]) as hits:
            n_hits = hits.n_hits
            assert n_hits > 1
        rc, message = call_search(lib, good, ["GATC"], both_strands=1, max_hits=n_hits - 1)
        assert rc == bad and str(n_hits) in message, (rc, message)
        assert call_search(lib, good, ["GATC"], both_strands=1, max_hits=n_hits)[0] == _ffi.OK
        with dec.search(["GATC"], max_hits=n_hits) as hits:
            assert hits.n_hits == n_hits
        for call in (lambda: dec.search(["GATC"], max_hits=n_hits - 1), lambda: dec.search(["GAXC"]), lambda: dec.search([]), lambda: dec.search(["A\0C"]),
                     lambda: dec.search(["GATC"], alphabet="bytes", both_strands=True), lambda: dec.search(["GATC"], alphabet="protein"),
                     lambda: sr.search(Source(), ["GATC"], _lib=lib)):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("accepted")
    # hand-made end tables: decreasing and beyond the section; the lowest offender is named
    check_end_tables(lib)
    # through a decoder: no letters; a shard; a protein under the nucleotide alphabet; an archive that ends early
    with open_decoder(lib, blob, sequence=False) as dec:
        rc, message, _, _ = call_search_decoder(lib, dec, ["GATC"])
        assert rc == _ffi.E_INVALID_ARG and "sequence" in message, (rc, message)
    with open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _, _ = call_search_decoder(lib, dec, ["GATC"])
        assert rc == _ffi.E_INVALID_ARG and "shard" in message, (rc, message)
    with open_decoder(lib, golden_bytes("LuxC.naf")) as dec:
        rc, message, _, _ = call_search_decoder(lib, dec, ["ACGT"], _ffi.SearchOpts(alphabet=0))
        assert rc == _ffi.E_INVALID_ARG and "nucleotide" in message, (rc, message)
        assert call_search_decoder(lib, dec, ["MK*"])[0] == _ffi.OK               # opts NULL: bytes, by the archive
        try:
            dec.search(["MK"], alphabet="nucleotide")
        except ValueError:
            pass
        else:
            raise AssertionError("the nucleotide alphabet on a protein")
    with open_decoder(lib, golden_bytes("masked.naf")) as dec:                    # opts NULL on dna: nucleotide, one strand, no mismatches
        rc, _, _, n = call_search_decoder(lib, dec, ["gaattc"])
        assert (rc, n) == (_ffi.OK, 1)
    with open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"ACGTTTnnACGT")) as dec, dec.search(["ACGT"], alphabet="bytes") as hits:
        compare(hits, b"ACGTTTnnACGT", None, ["ACGT"], what="no Length section", nucleotide=False, both_strands=False)   # the section is record 0
    with open_decoder(lib, sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 4], text=b"ACGTACGTAC")) as dec:
        rc, message, kind, _ = call_search_decoder(lib, dec, ["ACGT"])
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 2" in message, (rc, kind, message)
        try:
            dec.search(["ACGT"])
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")


def check_end_tables(lib):
    """hand-made end tables through nafgpu_search: a selection's letters with a table of this test's own in device memory"""
    with open_decoder(lib, golden_bytes("masked.naf")) as dec, dec.select([0, 1]) as sel:
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
            with DeviceWords(lib, table) as d_table:
                rc, message = call_search(lib, dict(d_sequence=sel.d_sequence, n_bases=n, d_record_end=d_table.address, n_records=len(table)), ["GAATTC"],
                                          both_strands=1)
            assert rc == status and needle in message, (what, rc, message)


class DeviceWords:
    """64-bit words in device memory, without any library but this one: the words are the sequence of a one-record text archive,
    decoded by a decoder of its own (decode_all_device leaves the section's bytes where the kernels read them)"""

    def __init__(self, lib, words):
        data = np.asarray(words, dtype=np.uint64).tobytes()
        self._dec = open_decoder(lib, sc.hand_archive(1, ids=[b"t"], text=data))
        res = self._dec.decode_all_device()
        assert res.n_bases == len(data) and res.d_sequence % 8 == 0 and self._dec.copy_to_host(res.d_sequence, len(data)) == data
        self.address = res.d_sequence

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._dec.close()
        return False


# ---------------------------------------------------------------- 8. positions and tile indices past 2^32 (MI355X only)
def check_past_u32(lib, n_bases=2 ** 28, copies=17):
    arc = lib.synth(n_bases, seed=31, with_mask=True, iupac_permille=5)
    try:
        dec = open_decoder(lib, ctypes.string_at(arc.bytes, arc.n))
        try:
            res = dec.decode_all_device()
            assert (res.n_bases, res.n_records) == (n_bases, arc.n_records)
            letters = dec.copy_to_host(res.d_sequence, n_bases)                 # the 256 MB, read back once
            ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
            patterns = [letters[12345:12354].upper().replace(b"N", b"A")]
            with dec.search(patterns, both_strands=False) as hits:
                print("search: %d records, %d letters, %d hits, %.3f ms" % (hits.n_records, hits.n_bases, hits.n_hits, hits.ms))
                regions, info, begin = compare(hits, letters, ends, patterns, what="2^28 letters", both_strands=False)
                assert 500 < hits.n_hits < 50000, hits.n_hits
            del letters
            with dec.select(list(range(res.n_records)) * copies) as sel:
                assert sel.n_bases == copies * n_bases > 2 ** 32
                with sel.search(patterns, both_strands=False) as hits:
                    print("search past 2^32: %d records, %d letters, %d hits, %.3f ms" % (hits.n_records, hits.n_bases, hits.n_hits, hits.ms))
                    assert hits.n_records == copies * res.n_records and hits.n_bases == copies * n_bases and hits.n_hits == copies * len(regions)
                    assert hits.pattern_hits == (copies * len(regions),)
                    all_regions, all_info, all_begin = tables(hits)
                    for c in range(copies):                                     # copy c: the hits of copy 0, the record shifted
                        want = regions.copy()
                        want["record"] += np.uint64(c * res.n_records)
                        piece = slice(c * len(regions), (c + 1) * len(regions))
                        assert all_regions[piece].tobytes() == want.tobytes() and all_info[piece].tobytes() == info.tobytes(), c
                        rows = slice(c * res.n_records, (c + 1) * res.n_records)
                        assert np.array_equal(all_begin[rows], begin[:-1] + np.uint64(c * len(regions))), c
                    assert int(all_begin[-1]) == hits.n_hits
        finally:
            dec.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))
