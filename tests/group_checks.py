"""Shared by tests/test_group_emu.py (CPU harness) and tests/test_gpu_group.py (MI355X): Decoder.group, Selection.group,
ParsedText.group and group(), records in device memory -> the groups of records whose sequences are equal.  Not a test
module; every function takes the library binding it is to check.

The yardstick is expected() below: a Python dict over the canonicalised bytes of what the CPU oracle decodes (or of the
source's own bytes read back), the rules of include/nafgpu.h restated: the first index per key, the strand by comparing with
the representative, the groups by ascending first index.  Every table is compared as a uint64 / uint8 array for equality:
integer work, no tolerance."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np

import encode_checks as ec
import search_checks as sk
import select_checks as sc
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.encoder import Record, encode_device, parse_text

gr = importlib.import_module("nafcodec_amd.group")           # (the module: the package's attribute of that name is its group())

ENTRY_POINTS = ("nafgpu_group", "nafgpu_group_decoder", "nafgpu_groups_copy_to_host", "nafgpu_groups_free")
IUPAC = b"ACGTURYKMSWBDHVN"


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sk.bind(lib)


def kernel_constants():
    """-> T, R: the kernels' tile bytes and tiles per run, read from group.h"""
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "group.h")) as f:
        text = f.read()
    tile = int(re.search(r"constexpr uint32_t kGrpTile = (\d+);", text).group(1))
    run = int(re.search(r"constexpr uint32_t kGrpRun = (\d+);", text).group(1))
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "group.hip")) as f:
        assert "static_assert(kGrpTile == kThreads * 16" in f.read()
    return tile, run


# ---------------------------------------------------------------- the yardstick
CANON = bytearray(range(256))                    # an IUPAC letter is compared as its upper case, U as T: equal 4-bit codes, equal bytes
for _c in IUPAC:
    CANON[_c] = CANON[_c | 0x20] = ord("T") if _c == ord("U") else _c
CANON = bytes(CANON)
COMPLEMENT = bytes.maketrans(b"ATCGRYKMBVDH", b"TAGCYRMKVBHD")   # over canonical bytes: the code with its bits reversed, any other byte itself


def expected(records, nucleotide=True, both_strands=False):
    """records (bytes each) -> representative, group_of, strand (None on one strand), group_first, group_size"""
    first, representative, strand, canon = {}, [], [], []
    for k, seq in enumerate(records):
        c = seq.translate(CANON) if nucleotide else bytes(seq)
        canon.append(c)
        key = min(c, c.translate(COMPLEMENT)[::-1]) if both_strands else c
        at = first.setdefault(key, k)
        representative.append(at)
        strand.append(int(c != canon[at]))       # (not equal read forward: then equal as the reverse complement)
    representative = np.array(representative, dtype=np.uint64)
    group_first = np.unique(representative)
    group_of = np.searchsorted(group_first, representative).astype(np.uint64)
    group_size = np.bincount(group_of.astype(np.int64), minlength=len(group_first)).astype(np.uint64)
    return representative, group_of, (np.array(strand, dtype=np.uint8) if both_strands else None), group_first.astype(np.uint64), group_size


def tables(g):
    strand = g.strand()
    return (np.frombuffer(g.representative(), dtype=np.uint64), np.frombuffer(g.group_of(), dtype=np.uint64),
            None if strand is None else np.frombuffer(strand, dtype=np.uint8), np.frombuffer(g.group_first(), dtype=np.uint64),
            np.frombuffer(g.group_size(), dtype=np.uint64))


NAMES = ("representative", "group_of", "strand", "group_first", "group_size")


def compare(g, records, what="", nucleotide=True, both_strands=False, rounds=1):
    """every table of a Groups against expected(); -> the tables"""
    want = expected(records, nucleotide, both_strands)
    got = tables(g)
    assert g.n_records == len(records) and g.n_bases >= sum(map(len, records)), (what, g.n_records, g.n_bases)
    assert g.n_groups == len(want[3]) == len(g) and g.n_duplicates == len(records) - len(want[3]), (what, "n_groups", g.n_groups, len(want[3]))
    for name, mine, yours in zip(NAMES, got, want):
        assert (mine is None) == (yours is None), (what, name)
        if mine is None:
            continue
        assert mine.shape == yours.shape and mine.dtype == yours.dtype, (what, name, mine.shape, yours.shape)
        if mine.tobytes() != yours.tobytes():
            at = int(np.nonzero(mine != yours)[0][0])
            raise AssertionError("%s: %s differs at %d of %d: %s / %s" % (what, name, at, len(yours), mine[at], yours[at]))
    assert g.largest_group == (int(want[4].max()) if len(records) else 0), (what, g.largest_group)
    assert rounds is None or g.rounds == (rounds if len(records) else 0), (what, g.rounds)
    # what the rules promise about the tables themselves
    rep, of, _, first, size = got
    assert int(size.sum()) == len(records) and (np.diff(first.astype(np.int64)) > 0).all() and np.array_equal(of[first.astype(np.int64)], np.arange(len(first), dtype=np.uint64))
    return got


def records_of(source):
    letters, ends = sk.own_layout(source)
    return [letters[int(a):int(b)] for a, b in zip(np.concatenate(([0], ends[:-1])).astype(np.int64), ends.astype(np.int64))]


def text_archive(records):
    """records (any bytes) -> a text archive of raw blocks: no letter is touched"""
    return sc.hand_archive(len(records), ids=[b"r%d" % k for k in range(len(records))], lengths=[len(r) for r in records], text=b"".join(records))


def case(lib, what, records, both_strands=False, nucleotide=True, dna=None, rounds=1):
    """records -> a text archive -> group() over its plain device addresses against expected() over what the oracle decodes;
    records of IUPAC letters and '-' also -> a dna archive written by the host Encoder -> Decoder.group.  -> the tables"""
    blob = text_archive(records)
    recs = [r[2] for r in sc.oracle_records(blob)]
    assert recs == [bytes(r) for r in records]
    with sk.open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        src = sk.Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        assert res.n_records == len(records)
        with gr.group(src, both_strands=both_strands, alphabet="nucleotide" if nucleotide else "bytes", _lib=lib) as g:
            got = compare(g, recs, what=what, nucleotide=nucleotide, both_strands=both_strands, rounds=rounds)
        if not nucleotide and not both_strands:
            with dec.group() as g:                           # a text archive: bytes, by the archive
                compare(g, recs, what=what + ", Decoder.group", nucleotide=False, rounds=rounds)
    if dna is None:
        dna = nucleotide and sum(map(len, records)) < 100_000 and all(c in IUPAC.replace(b"U", b"") + IUPAC.lower().replace(b"u", b"") + b"-" for r in records for c in r)
    if dna:
        blob, recs = sk.archive_of(lib, records)
        with sk.open_decoder(lib, blob) as dec, dec.group(both_strands=both_strands) as g:
            again = compare(g, [r[2] for r in recs], what=what + ", a dna archive", both_strands=both_strands, rounds=rounds)
        assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(got, again)), what
    return got


def reverse_complement(seq):
    return bytes(seq).translate(CANON).translate(COMPLEMENT)[::-1]


# ---------------------------------------------------------------- 1. the fixtures
def check_fixtures(lib):
    blob = golden_bytes("phix.naf")
    recs = [r[2] for r in sc.oracle_records(blob)]
    with sk.open_decoder(lib, blob) as dec:
        with dec.group() as g:
            compare(g, recs, what="phix, forward")
        with dec.group(both_strands=True) as g:
            compare(g, recs, what="phix, both strands", both_strands=True)
    # masked.naf: nucleotide against bytes; a record and its soft-masked copy are one group by their codes and two by their bytes
    blob = golden_bytes("masked.naf")
    recs = [r[2] for r in sc.oracle_records(blob)]
    with sk.open_decoder(lib, blob) as dec:
        with dec.group() as g:
            compare(g, recs, what="masked")
        with dec.group(alphabet="bytes") as g:
            compare(g, recs, what="masked, as bytes", nucleotide=False)
        with dec.select(list(range(len(recs)))) as sel:
            archive = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, mask=True, compression_level=1, device=0, _lib=lib)
    masked = [r[2] for r in sc.oracle_records(archive, spec_mask=True)]
    assert masked == recs and any(r != r.upper() for r in masked)
    both = masked + [r.upper() for r in masked]
    fasta = b"".join(b">r%d\n%s\n" % (k, r) for k, r in enumerate(both))
    with parse_text(fasta, device=0, _lib=lib) as parsed:
        assert records_of(parsed) == both
        with parsed.group() as g:
            rep, _, _, _, _ = compare(g, both, what="masked and its upper case")
            assert g.n_groups == len(set(r.upper() for r in masked)) and list(rep[len(masked):]) == list(rep[:len(masked)])
        with parsed.group(alphabet="bytes") as g:
            compare(g, both, what="masked and its upper case, as bytes", nucleotide=False)
            assert g.n_groups == len(set(both)) > len(set(r.upper() for r in masked))
    # a protein, as bytes by the archive
    blob = golden_bytes("LuxC.naf")
    recs = [r[2] for r in sc.oracle_records(blob)]
    with sk.open_decoder(lib, blob) as dec, dec.group() as g:
        compare(g, recs, what="LuxC", nucleotide=False)
    # an RNA archive whose records equal a DNA one's with U for T
    rng = np.random.default_rng(5)
    dna = [ec.letters(rng, b"ACGTN", int(l)) for l in rng.integers(1, 400, 40)]
    dna = dna + [dna[int(i)] for i in rng.integers(0, 40, 25)]
    answers = []
    for kind, records in (("dna", dna), ("rna", [r.replace(b"T", b"U") for r in dna])):
        archive = ec.host_archive(lib, [Record(id="r%d" % k, comment="", sequence=r.decode()) for k, r in enumerate(records)], kind, 1, id=True,
                                  comment=True, sequence=True)
        recs = [r[2] for r in sc.oracle_records(archive)]
        assert [r.upper() for r in recs] == records
        with sk.open_decoder(lib, archive) as dec, dec.group(both_strands=True) as g:
            answers.append([t.tobytes() for t in compare(g, recs, what=kind, both_strands=True)])
            assert g.n_duplicates >= 25
    assert answers[0] == answers[1]
    case(lib, "U and T in one source", [b"ACGTTGCA", b"ACGUUGCA", b"acguugca", b"ACGATGCA", b"TGCAACGU"], both_strands=True)


# ---------------------------------------------------------------- 2. the edges
def edge_records(rng, T, R):
    """-> the records of check_edges' large case: every length the kernels take another path at, each twice, in mixed order"""
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, T - 1, T, T + 1, R * T - 1, R * T + 1, 3 * R * T + 5]
    originals = [ec.letters(rng, b"ACGT", l) for l in lengths]
    records = list(originals)
    for k in rng.permutation(len(originals)):
        records.append(originals[int(k)])
        records.append(ec.letters(rng, b"ACGT", int(rng.integers(0, 40))))
    return records, lengths


def changed(seq, at):
    out = bytearray(seq)
    out[at] = ord("C") if out[at] != ord("C") else ord("A")
    return bytes(out)


def check_edges(lib):
    T, R = kernel_constants()
    rng = np.random.default_rng(20241019)
    # the record lengths, each twice; then the same with every second copy reversed and complemented
    records, lengths = edge_records(rng, T, R)
    rep, _, _, _, size = case(lib, "lengths", records, dna=False)
    assert all(int(rep[k]) <= k for k in range(len(records))) and int((rep != np.arange(len(records))).sum()) >= len(lengths)
    case(lib, "lengths, as bytes", records, nucleotide=False)
    turned = [reverse_complement(r) if k >= len(lengths) and k % 2 == 0 else r for k, r in enumerate(records)]
    _, _, strand, _, _ = case(lib, "lengths, both strands", turned, both_strands=True, dna=False)
    assert 5 <= int(strand.sum()) <= len(lengths)
    # equal pairs whose starts differ by every residue mod 16, short and longer than a lane's 16 letters
    for l in (5, 77, 300):
        seq, recs, at, starts = ec.letters(rng, b"ACGT", l), [], 0, []
        for residue in range(16):
            pad = (residue - at) % 16 or 16
            if residue:
                recs.append(ec.letters(rng, b"ACGT", pad))
                at += pad
            starts.append(at)
            recs.append(seq if residue % 2 == 0 else seq.lower())
            at += l
        assert {s % 16 for s in starts} == set(range(16))
        rep, _, _, _, _ = case(lib, "every residue, %d letters" % l, recs)
        assert sum(int(v) == 0 for v in rep) == 16
        case(lib, "every residue, %d letters, both strands" % l, [reverse_complement(r) if k % 4 == 2 else r for k, r in enumerate(recs)], both_strands=True)
    # pairs that differ only in the first letter, only in the last, only at a tile edge, only in length (one a prefix of the other)
    base = ec.letters(rng, b"ACGT", 2 * T + 7)
    variants = [base, changed(base, 0), changed(base, len(base) - 1), base[:-1], base[:-8], base + b"A", base[1:]]
    recs = list(variants)
    for other in variants[1:3]:                              # every variant is there twice, so that a difference missed would merge groups
        recs.append(other)
    recs += [changed(base, edge) for edge in (T - 1, T, 2 * T - 1, 2 * T)]   # at a tile edge of the record, which starts the section
    for k in range(4):
        start = sum(map(len, recs))
        index = (-start) % T + (T - 1 if k % 2 == 0 else 0)  # the record's letter that lies last / first in a tile of the section
        recs.append(changed(base, index % len(base)))
    recs.append(base)
    rep, _, _, first, _ = case(lib, "one letter apart", recs, dna=False)
    assert int(rep[-1]) == 0 and len(first) == len(set(recs)) >= 12
    case(lib, "one letter apart, both strands", recs + [reverse_complement(r) for r in recs[:9]], both_strands=True, dna=False)
    for short in (b"ACGTACGTA", b"ACGTACGTACGTACGTA"):         # around the 8-letter words: one letter apart at every position, every prefix
        near = [short] + [changed(short, i) for i in range(len(short))] + [short[:i] for i in range(len(short))] + [short]
        rep, _, _, first, _ = case(lib, "words of %d letters" % len(short), near)
        assert len(first) == 2 * len(short) + 1 and int(rep[-1]) == 0
        case(lib, "words of %d letters, both strands" % len(short), near + [reverse_complement(r) for r in near], both_strands=True)
    # several empty records, the first and the last among them: one group
    recs = [b"", b"ACGT", b"", b"", b"ACGT", b"A", b""]
    rep, of, _, first, size = case(lib, "empty records", recs)
    assert list(rep) == [0, 1, 0, 0, 1, 5, 0] and list(first) == [0, 1, 5] and list(size) == [4, 2, 1]
    rep, _, _, _, _ = case(lib, "only empty records", [b""] * 5, both_strands=True)
    assert list(rep) == [0] * 5
    # every record equal; no two equal (many records in a tile, and more records than one round of the short route takes)
    rep, _, _, _, size = case(lib, "every record equal", [b"ACGTTGCATT"] * 700)
    assert list(size) == [700]
    recs = [b"%dN" % k for k in range(1500)]                 # (digits: no IUPAC letters, equal only as the same byte)
    case(lib, "no two equal", recs, dna=False)
    case(lib, "no two equal, nucleotides", [ec.letters(rng, b"ACGT", 24) for _ in range(600)], both_strands=True)
    # a duplicate in front of and behind a long record
    long = ec.letters(rng, b"ACGT", 3 * R * T + 5)
    rep, _, _, _, _ = case(lib, "around a long record", [b"GATTACA", long, b"gattaca", long[:-1], b"GATTACA"], dna=False)
    assert list(rep) == [0, 1, 0, 3, 0]
    # letters outside IUPAC, and '-': equal only as the same byte; IUPAC letters by their code
    recs = [b"AC-GT", b"ac-gu", b"AC.GT", b"ACXGT", b"acxgt", b"ACxGT", b"AC GT", b"ACNGT", b"AC-GT", b"ACRGT", b"acrgu", b"AC\0GT", b"AC\0GT", b"ACG", b"ACG\0"]
    rep, _, _, _, _ = case(lib, "letters outside the alphabet", recs)
    assert list(rep) == [0, 0, 2, 3, 4, 4, 6, 7, 0, 9, 9, 11, 11, 13, 14]
    rep, _, _, _, _ = case(lib, "letters outside the alphabet, as bytes", recs, nucleotide=False)
    assert list(rep) == [0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 11, 13, 14]
    # both strands: a record and its reverse complement; its own reverse complement; IUPAC (R against Y); odd length; forward and
    # reverse duplicates of one representative in one group with the right strands
    recs = [b"AAACCCGGT", b"ACCGGGTTT", b"GAATTC", b"gaauuc", b"ARG", b"CYT", b"ACGTA", b"TACGT", b"AAACCCGGT", b"accgggttt", b"ACCGGGTTA",
            b"A-C", b"G-T", b"AXC", b"GXT", b"CXA", b"N", b"n", b"A", b"T"]
    rep, of, strand, first, size = case(lib, "both strands", recs, both_strands=True)
    assert list(rep) == [0, 0, 2, 2, 4, 4, 6, 6, 0, 0, 10, 11, 11, 13, 13, 15, 16, 16, 18, 18], rep
    assert list(strand) == [0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1], strand
    rep, _, strand, _, _ = case(lib, "one strand", recs)
    assert strand is None and list(rep) == [0, 1, 2, 2, 4, 5, 6, 7, 0, 1, 10, 11, 12, 13, 14, 15, 16, 16, 18, 19]
    # the edge archive of the selection's tests (IUPAC letters in both cases, '-'), a selection of it with odd starts, and sources
    # whose letters reach behind the last record end
    blob = sc.edge_archive(lib)
    recs = [r[2] for r in sc.oracle_records(blob)]
    big = [len(r) for r in recs].index(9000)
    with sk.open_decoder(lib, blob) as dec:
        with dec.group(both_strands=True) as g:
            compare(g, recs, what="the edge archive", both_strands=True)
        regions = [(big, 200 + r, 237 + 2 * r) for r in range(16)] + [(big, 200 + r, 237 + 2 * r) for r in range(16)] + \
                  [(big, 1, 8999), (big, 3, 3), (big, 7, 7 + T), (big, 1, 8999, "-"), (big, 7, 7 + T, "-")]
        with dec.select(regions) as sel:
            own = records_of(sel)
            with sel.group(both_strands=True) as g:
                rep, _, strand, _, _ = compare(g, own, what="a selection with odd starts", both_strands=True)
                assert list(rep[16:32]) == list(range(16)) and list(strand[-2:]) == [1, 1]
            src = sk.Source(d_sequence=sel.d_sequence, n_bases=sel.n_bases, d_record_end=sel.d_record_end, n_records=sel.n_records - 3)
            with gr.group(src, _lib=lib) as g:
                assert g.n_bases == sel.n_bases
                compare(g, own[:-3], what="letters behind the last end")


# ---------------------------------------------------------------- 3. random
def random_records(n, seed=11):
    """n letters cut into records; some 30 % of them then replaced by copies or reverse complements of earlier records, a few by
    near-copies with one substitution"""
    rng = np.random.default_rng(seed)
    text = np.frombuffer(ec.letters(rng, b"ACGT", n), dtype=np.uint8).copy()
    text[rng.random(n) < 0.002] = ord("N")
    text = text.tobytes()
    records, at = [], 0
    while at < n:
        kind = rng.random()
        l = int(rng.integers(0, 12)) if kind < 0.05 else int(rng.integers(20, 301)) if kind < 0.97 else int(rng.integers(1000, 20001))
        records.append(text[at:at + l])
        at += l
    for k in range(1, len(records)):
        kind = rng.random()
        if kind < 0.30:
            earlier = records[int(rng.integers(0, k))]
            records[k] = earlier if kind < 0.12 else reverse_complement(earlier) if kind < 0.24 else earlier.lower() if kind < 0.27 or not earlier else \
                changed(earlier, int(rng.integers(0, len(earlier))))
    return records


def check_random(lib, n):
    records = random_records(n)
    fasta = b"".join(b">r%d\n%s\n" % (k, r) for k, r in enumerate(records))
    with parse_text(fasta, device=0, _lib=lib) as parsed:
        assert records_of(parsed) == records
        for both in (False, True):
            with parsed.group(both_strands=both) as g:
                compare(g, records, what="random, %d letters" % n, both_strands=both)
                assert g.n_duplicates > len(records) // (5 if both else 10) and g.n_groups > len(records) // 2
                print("group: %d letters, %d records, %d groups, both strands %d, %.3f ms" % (g.n_bases, len(records), g.n_groups, both, g.ms))
        with parsed.group(alphabet="bytes") as g:
            compare(g, records, what="random, as bytes", nucleotide=False)


# ---------------------------------------------------------------- 4. hashes that collide (a process of its own: the hook is read from the environment)
def collision_records():
    rng = np.random.default_rng(3)
    distinct = [ec.letters(rng, b"ACGT", 40) for _ in range(4)] + [ec.letters(rng, b"ACGT", 5000), b"", b"ACG", b"ACT"]
    records = []
    for k in rng.integers(0, len(distinct), 60):
        seq = distinct[int(k)]
        records.append(reverse_complement(seq) if rng.random() < 0.3 else seq.lower() if rng.random() < 0.3 else seq)
    records += [changed(distinct[4], 4999), changed(distinct[4], 0), distinct[4][:-1]]
    assert len(set(r.upper() for r in records)) >= 5
    return records


def check_collisions(lib):
    """the tables with the hash cut to 0, 1 and 4 bits are those without the hook; at 0 bits every length is one key, so the
    rounds are reached"""
    records = collision_records()
    plain = {both: [None if t is None else t.tobytes() for t in case(lib, "no hook", records, both_strands=both, dna=False)] for both in (False, True)}
    lib.c.nafgpu_test_hooks(1)
    try:
        for bits in (0, 1, 4):
            os.environ["NAFGPU_GRP_HASH_BITS"] = str(bits)
            for both in (False, True):
                blob = text_archive(records)
                with sk.open_decoder(lib, blob) as dec:
                    res = dec.decode_all_device()
                    src = sk.Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
                    with gr.group(src, both_strands=both, _lib=lib) as g:
                        got = compare(g, records, what="%d hash bits" % bits, both_strands=both, rounds=None)
                        assert [None if t is None else t.tobytes() for t in got] == plain[both], bits
                        assert g.rounds > 1 if bits == 0 else g.rounds >= 1, (bits, g.rounds)
                        print("group: %d hash bits, both strands %d: %d rounds" % (bits, both, g.rounds))
    finally:
        os.environ.pop("NAFGPU_GRP_HASH_BITS", None)
        lib.c.nafgpu_test_hooks(0)


def run_in_process(library_path, check, timeout):
    """a check of this module in a process of its own, against the library at `library_path`"""
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
             "import group_checks as gc\nfrom nafcodec_amd import _ffi\ngc.%s(gc.bind(_ffi.Library(%r)))\nprint('OK')\n" \
             % (ROOT, os.path.join(ROOT, "tests"), check, library_path)
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------- 5. composition
def check_composition(lib):
    # Selection.group and ParsedText.group equal Decoder.group on the same records; group() takes plain device addresses
    blob = golden_bytes("phix.naf")
    with sk.open_decoder(lib, blob) as dec, dec.group(both_strands=True) as g:
        mine = [t.tobytes() for t in tables(g)] + [g.n_records, g.n_groups, g.n_bases, g.largest_group]
        with dec.select(list(range(g.n_records))) as sel, sel.group(both_strands=True) as again:
            assert mine == [t.tobytes() for t in tables(again)] + [again.n_records, again.n_groups, again.n_bases, again.largest_group]
        with parse_text(dec.to_text(), device=0, _lib=lib) as parsed, parsed.group(both_strands=True) as again:
            assert mine == [t.tobytes() for t in tables(again)] + [again.n_records, again.n_groups, again.n_bases, again.largest_group]
        res = dec.decode_all_device()
        src = sk.Source(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        with gr.group(src, both_strands=True, _lib=lib) as again:
            assert mine == [t.tobytes() for t in tables(again)] + [again.n_records, again.n_groups, again.n_bases, again.largest_group]
    # dereplication: select(groups) -> encode_device -> the oracle reads exactly the first occurrences, ids and comments with them
    rng = np.random.default_rng(9)
    distinct = [ec.letters(rng, b"ACGTN", int(l)) for l in rng.integers(1, 600, 30)]
    records = [distinct[int(k)] for k in rng.integers(0, 30, 100)]
    blob, recs = sk.archive_of(lib, records)
    dec = sk.open_decoder(lib, blob)
    g = dec.group()
    rep = compare(g, [r[2] for r in recs], what="reads with duplicates")[0]
    with dec.select(g) as unique:
        assert unique.n_records == g.n_groups < len(records)
        archive = encode_device(unique, sequence_type="dna", id=True, comment=True, sequence=True, mask=True, compression_level=1, device=0, _lib=lib)
    firsts = sorted(set(int(v) for v in rep))
    assert sc.oracle_records(archive, spec_mask=True) == [recs[k] for k in firsts]
    assert len(set(r[2].upper() for r in sc.oracle_records(archive))) == len(firsts) == len(set(r.upper() for r in records))
    # the groups outlive a closed decoder; closed groups are refused
    dec.close()
    assert tables(g)[0].tobytes() == rep.tobytes() and list(g.group_first()) == firsts
    g.close()
    try:
        g.representative()
    except RuntimeError:
        pass
    else:
        raise AssertionError("closed groups were used")


# ---------------------------------------------------------------- 6. refusals
def call_group(lib, src_fields, device=0, **opts):
    src, o = _ffi.EncodeSource(**src_fields), _ffi.GroupOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.GroupResult(), _ffi.Error()
    rc = lib.c.nafgpu_group(ctypes.byref(src), ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_groups_free(h)
    return rc, err.message.decode("utf-8", "replace"), res.n_groups


def call_group_decoder(lib, dec, opts=None):
    h, res, err = ctypes.c_void_p(), _ffi.GroupResult(), _ffi.Error()
    rc = lib.c.nafgpu_group_decoder(dec._h, ctypes.byref(opts) if opts else None, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        lib.c.nafgpu_groups_free(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind, res.n_groups


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    bad = _ffi.E_INVALID_ARG
    with sk.open_decoder(lib, blob) as dec:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        rc, _, n_groups = call_group(lib, good)
        assert rc == _ffi.OK and 0 < n_groups <= res.n_records
        # no letters; records without their table; the alphabet and the strands
        assert call_group(lib, dict(good, d_sequence=None))[0] == bad
        assert call_group(lib, dict(good, d_record_end=None))[0] == bad
        assert call_group(lib, good, alphabet=2)[0] == bad and call_group(lib, good, alphabet=1, both_strands=1)[0] == bad
        assert call_group(lib, good, alphabet=1)[0] == _ffi.OK and call_group(lib, good, alphabet=0, both_strands=1)[0] == _ffi.OK
        # n_records == 0: all counts 0, with or without a table
        for fields in (dict(good, n_records=0), dict(good, n_records=0, d_record_end=None)):
            src, o, h, r, err = _ffi.EncodeSource(**fields), _ffi.GroupOpts(), ctypes.c_void_p(), _ffi.GroupResult(), _ffi.Error()
            assert lib.c.nafgpu_group(ctypes.byref(src), ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r), ctypes.byref(err)) == _ffi.OK
            assert (r.n_records, r.n_groups, r.largest_group, r.rounds) == (0, 0, 0, 0) and h.value
            lib.c.nafgpu_groups_free(h)
        with gr.group(sk.Source(d_sequence=res.d_sequence, n_bases=res.n_bases), _lib=lib) as g:
            assert (g.n_records, g.n_groups, len(g), g.n_duplicates) == (0, 0, 0, 0) and len(g.representative()) == 0 and len(g.group_first()) == 0
        # null arguments
        src, o, h, r, err = _ffi.EncodeSource(**good), _ffi.GroupOpts(), ctypes.c_void_p(), _ffi.GroupResult(), _ffi.Error()
        for args in ((None, ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), None, 0, ctypes.byref(h), ctypes.byref(r)),
                     (ctypes.byref(src), ctypes.byref(o), 0, None, ctypes.byref(r)), (ctypes.byref(src), ctypes.byref(o), 0, ctypes.byref(h), None)):
            assert lib.c.nafgpu_group(*args, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_group_decoder(None, None, ctypes.byref(h), ctypes.byref(r), ctypes.byref(err)) == bad
        assert lib.c.nafgpu_group_decoder(dec._h, None, None, ctypes.byref(r), ctypes.byref(err)) == bad
        assert lib.c.nafgpu_group_decoder(dec._h, None, ctypes.byref(h), None, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_groups_copy_to_host(None, None, 1, None) == bad
        lib.c.nafgpu_groups_free(None)
        for call in (lambda: dec.group(alphabet="bytes", both_strands=True), lambda: dec.group(alphabet="protein"),
                     lambda: gr.group(sk.Source(), _lib=lib), lambda: gr.group(sk.Source(d_sequence=res.d_sequence, n_bases=res.n_bases, n_records=3), _lib=lib)):
            try:
                call()
            except ValueError:
                pass
            else:
                raise AssertionError("accepted")
    # hand-made end tables: decreasing and beyond the section; the lowest offender is named
    with sk.open_decoder(lib, golden_bytes("masked.naf")) as dec, dec.select([0, 1]) as sel:
        n = sel.n_bases
        good = np.arange(1, 201, dtype=np.uint64) * np.uint64(10)
        assert n > 2000
        for what, change, needle, status in (("decreasing", {100: 500}, "record 100 ", _ffi.E_INVALID_LENGTH),
                                             ("decreasing, three of them", {100: 500, 60: 300, 199: 1}, "record 60 ", _ffi.E_INVALID_LENGTH),
                                             ("the last record beyond the section", {199: n + 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("far beyond", {199: 2 ** 64 - 1}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("the first record bad", {0: 2 ** 40}, "record 0 ", _ffi.E_INVALID_LENGTH),
                                             ("the last record below the one in front", {199: 1989}, "record 199 ", _ffi.E_INVALID_LENGTH),
                                             ("beyond in front of decreasing", {50: 2 ** 50, 51: 510}, "record 50 ", _ffi.E_INVALID_LENGTH),
                                             ("a good table", {}, "", _ffi.OK)):
            table = good.copy()
            for k, v in change.items():
                table[k] = v
            with sk.DeviceWords(lib, table) as d_table:
                for both in (0, 1):
                    rc, message, _ = call_group(lib, dict(d_sequence=sel.d_sequence, n_bases=n, d_record_end=d_table.address, n_records=len(table)), both_strands=both)
                    assert rc == status and needle in message, (what, rc, message)
    # through a decoder: no letters; a shard; no Length section; a protein under the nucleotide alphabet; an archive that ends early
    with sk.open_decoder(lib, blob, sequence=False) as dec:
        rc, message, _, _ = call_group_decoder(lib, dec)
        assert rc == bad and "sequence" in message, (rc, message)
    with sk.open_decoder(lib, blob, shard_count=2) as dec:
        rc, message, _, _ = call_group_decoder(lib, dec)
        assert rc == bad and "shard" in message, (rc, message)
    with sk.open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"ACGTTTnnACGT")) as dec:
        rc, message, _, _ = call_group_decoder(lib, dec)
        assert rc == bad and "Length" in message, (rc, message)
    with sk.open_decoder(lib, golden_bytes("LuxC.naf")) as dec:
        rc, message, _, _ = call_group_decoder(lib, dec, _ffi.GroupOpts(alphabet=0))
        assert rc == bad and "nucleotide" in message, (rc, message)
        assert call_group_decoder(lib, dec)[0] == _ffi.OK                         # opts NULL: bytes, by the archive
        try:
            dec.group(alphabet="nucleotide")
        except ValueError:
            pass
        else:
            raise AssertionError("the nucleotide alphabet on a protein")
    with sk.open_decoder(lib, golden_bytes("masked.naf")) as dec:                 # opts NULL on dna: nucleotide, one strand
        recs = [r[2] for r in sc.oracle_records(golden_bytes("masked.naf"))]
        rc, _, _, n_groups = call_group_decoder(lib, dec)
        assert (rc, n_groups) == (_ffi.OK, len(expected(recs)[3]))
    with sk.open_decoder(lib, sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 4], text=b"ACGTACGTAC")) as dec:
        rc, message, kind, _ = call_group_decoder(lib, dec)
        assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 2" in message, (rc, kind, message)
        try:
            dec.group()
        except EOFError:
            pass
        else:
            raise AssertionError("a record beyond the decoded letters")


# ---------------------------------------------------------------- 7. positions past 2^32 (MI355X only)
def check_past_u32(lib, n_bases=2 ** 26, copies=65):
    arc = lib.synth(n_bases, seed=31, with_mask=True, iupac_permille=5)
    try:
        dec = sk.open_decoder(lib, ctypes.string_at(arc.bytes, arc.n))
        try:
            res = dec.decode_all_device()
            assert (res.n_bases, res.n_records) == (n_bases, arc.n_records)
            letters = dec.copy_to_host(res.d_sequence, n_bases)
            ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64).astype(np.int64)
            records = [letters[int(a):int(b)] for a, b in zip(np.concatenate(([0], ends[:-1])), ends)]
            del letters
            with dec.group(both_strands=True) as g:
                print("group: %d records, %d letters, %d groups, %.3f ms" % (g.n_records, g.n_bases, g.n_groups, g.ms))
                rep, _, strand, first, size = compare(g, records, what="2^26 letters", both_strands=True)
            del records
            n = res.n_records
            with dec.select(list(range(n)) * copies) as sel:
                assert sel.n_bases == copies * n_bases > 2 ** 32
                with sel.group(both_strands=True) as g:
                    print("group past 2^32: %d records, %d letters, %d groups, %.3f ms" % (g.n_records, g.n_bases, g.n_groups, g.ms))
                    assert g.n_records == copies * n and g.n_bases == copies * n_bases and g.n_groups == len(first) and g.rounds == 1
                    all_rep, all_of, all_strand, all_first, all_size = tables(g)
                    for c in range(copies):                  # every record of copy c has the representative of its twin in copy 0
                        rows = slice(c * n, (c + 1) * n)
                        assert np.array_equal(all_rep[rows], rep) and np.array_equal(all_strand[rows], strand), c
                    assert np.array_equal(all_first, first) and np.array_equal(all_size, size * np.uint64(copies))
                    assert g.largest_group == copies * int(size.max())
        finally:
            dec.close()
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))
