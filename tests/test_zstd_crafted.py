"""Hand-built zstd frames (tests/zstd_craft.py) for encodings libzstd does not emit at the levels the other tests use
-- direct and FSE-described Huffman weights, every literals header size, trees of depth 1 and 9-11, every sequence
table mode at its smallest and largest accuracy logs, every LL / ML code, offset codes up to 27, the nbSeq forms,
repeat offsets at the start of a frame, single-segment frames -- and for malformed frames on which the product, its
checker and the reference's stream decoder must all refuse.  Every valid frame is first decoded by libzstd (one-shot
and streaming) to the writer's own expectation, so that the writer is checked independently of the project."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import zstd_craft as zc
import zstd_ref
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu", "_build")
CSRC = os.path.join(ROOT, "nafcodec_amd", "csrc")

pytestmark = pytest.mark.skipif(not zstd_ref.available(), reason="libzstd not loadable")

ALL_SEQ = {"ll": zc.Tbl("repeat"), "of": zc.Tbl("repeat"), "ml": zc.Tbl("repeat")}


def _rand(rng, n, alphabet=None):
    if alphabet is None:
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n))


def depth_tree(depth, first=0):
    """weights of the prefix code of lengths 1, 2, ..., depth - 1, depth, depth over symbols first, first + 1, ..."""
    depths = {first + k: k + 1 for k in range(depth - 1)}
    depths[first + depth - 1] = depths[first + depth] = depth
    return zc.weights_for_depths(depths)


def valid_frames():
    """(name, payload, expected, features) -- every frame meant to decode"""
    rng = np.random.default_rng(0x2B5)
    out = []

    def add(name, fr):
        p, exp, feat = fr.payload()
        out.append((name, p, exp, feat))
        COUNTS[name] = dict(fr.counts)

    # ---- literals formats
    for n, sf in ((1, 0), (31, 0), (5, 2), (32, 1), (4095, 1), (4096, 3), (70000, 3)):
        f = zc.Frame(window_log=17)
        f.compressed(_rand(rng, n), lit=zc.Lit("raw", sf=sf))
        add("lit_raw_n%d_sf%d" % (n, sf), f)
    for n in (1, 31, 32, 4095, 4096, 100000):
        f = zc.Frame(window_log=17)
        f.compressed(b"\x37" * n, lit=zc.Lit("rle"))
        add("lit_rle_n%d" % n, f)
    dna = b"\x11\x12\x14\x18\x21\x22\x24\x28\x41\x42\x44\x48\x81\x82\x84\x88"     # packed nucleotide pairs
    w16 = [0] * 0x89
    for k, b in enumerate(dna):
        w16[b] = 1 + (k % 3 == 0)                        # 5 of weight 2 -> 10 + 11 of weight 1 = 21: pad to 32
    w16[0x89 - 1] = 0
    tot = sum(1 << (w - 1) for w in w16 if w)
    w16 += [0] * (0x90 - len(w16))
    for s in range(0x8A, 0x90):
        if tot < 32:
            w16[s] = 1
            tot += 1
    while tot < 32:
        w16.append(1)
        tot += 1
    alpha = bytes(s for s, w in enumerate(w16) if w)
    for streams, n, form in ((1, 900, "fse"), (4, 900, "fse"), (4, 10000, "fse"), (4, 100000, "fse"), (1, 200, "fse")):
        f = zc.Frame(window_log=17)
        data = _rand(rng, n, alpha)
        f.compressed(data, lit=zc.Lit("huf", weights=w16, form=form, streams=streams))
        f.compressed(_rand(rng, n // 2 + 1, alpha), lit=zc.Lit("treeless", streams=streams))
        add("lit_huf_dna_%dstreams_n%d" % (streams, n), f)
    # direct weights, odd and even counts; 4 streams of a handful of symbols (some streams nearly empty)
    for n_syms in (5, 6, 2):
        wts = depth_tree(n_syms - 1, first=0x41)
        syms = bytes(s for s, w in enumerate(wts) if w)
        f = zc.Frame(window_log=17)
        f.compressed(_rand(rng, 3000, syms), lit=zc.Lit("huf", weights=wts, form="direct", streams=4))
        f.compressed(_rand(rng, 7, syms), lit=zc.Lit("treeless", streams=4))
        f.compressed(_rand(rng, 600, syms), lit=zc.Lit("treeless", streams=1))
        add("lit_huf_direct_%dsyms" % n_syms, f)
    # deep trees (9, 10, 11 bits) over DNA-like bytes, with bytes >= 0x80 (FSE-described weights), with and without rare symbols
    for depth in (9, 10, 11):
        for form, first in (("fse", 0x78), ("direct", 0x41)):      # (direct weights reach symbol 128 at most)
            wts = depth_tree(depth, first=first)
            syms = [s for s, w in enumerate(wts) if w]
            p = np.array([2.0 ** -(12 - wts[s]) for s in syms])
            data = bytes(rng.choice(syms, 60000, p=p / p.sum()).astype(np.uint8))
            f = zc.Frame(window_log=20)
            f.compressed(data, lit=zc.Lit("huf", weights=wts, form=form, streams=4))
            f.compressed(data[:30000], lit=zc.Lit("treeless", streams=4))
            add("lit_huf_depth%d_%s" % (depth, form), f)
    # ---- sequences: every table mode, the smallest and largest accuracy logs, all LL / ML codes, OF codes to 22
    hist = _rand(rng, 70000)
    ll_vals = list(range(16)) + [zc.LL_BASE[c] + ((1 << zc.LL_BITS[c]) - 1 if c < 33 else c) for c in range(16, 36)]
    ml_vals = [zc.ML_BASE[c] + ((1 << zc.ML_BITS[c]) - 1 if c < 50 else c) for c in range(53)]
    f = zc.Frame(window_log=17)
    f.raw(hist[:60000])
    groups, cur = [], []
    for ll in ll_vals:                                   # every LL code, packed into blocks of at most 120000 bytes
        if sum(cur) + ll + 4 * len(cur) > 120000:
            groups.append(cur)
            cur = []
        cur.append(ll)
    groups.append(cur)
    for lls in groups:
        seqs = [(ll, 4 + k % 3, 3 + 1000 + 17 * k) for k, ll in enumerate(lls)]
        f.compressed(_rand(rng, sum(lls)), seqs, lit=zc.Lit("raw"), tables=zc.auto_tables(seqs, {"ll": 9, "ml": 5, "of": 5}))
    add("seq_all_ll_codes_al9", f)
    f = zc.Frame(window_log=17)
    f.raw(hist[:65536])
    f.raw(hist[:65536])
    groups, cur = [], []
    for ml in ml_vals:                                   # every ML code, packed into blocks of at most 120000 bytes
        if sum(cur) + ml > 120000:
            groups.append(cur)
            cur = []
        cur.append(ml)
    groups.append(cur)
    for g, mls in enumerate(groups):
        seqs = [(1, ml, 3 + 60000 + k) for k, ml in enumerate(mls)]
        f.compressed(_rand(rng, len(seqs)), seqs, lit=zc.Lit("raw"),
                     tables=zc.auto_tables(seqs, {"ll": 5, "ml": 9 if g % 2 else 6, "of": 5}))
    seqs = [(1, 3, (1 << c) + c) for c in range(2, 12)]   # small offset codes
    f.compressed(_rand(rng, len(seqs)), seqs, lit=zc.Lit("raw"), tables=zc.auto_tables(seqs))
    add("seq_all_ml_codes", f)
    # predefined tables, RLE tables, repeat mode; repeat offsets 1/4/8 at the start of a frame, the ll == 0 shifts
    f = zc.Frame(window_log=17)
    lits = _rand(rng, 400)
    seqs = [(10, 5, 1), (0, 4, 1), (3, 6, 2), (0, 3, 2), (4, 5, 3), (0, 3, 3), (7, 9, 3 + 9), (0, 3, 3)]
    f.compressed(lits, seqs, lit=zc.Lit("raw"))
    seqs2 = [(5, 7, 2), (6, 4, 3 + 20), (0, 8, 1), (9, 3, 1)]
    f.compressed(lits[:100], seqs2, lit=zc.Lit("raw"), tables=ALL_SEQ)
    seqs3 = [(3, 4, 3 + 100)] * 5
    f.compressed(lits[:50], seqs3, lit=zc.Lit("raw"),
                 tables={"ll": zc.Tbl("rle", code=3), "ml": zc.Tbl("rle", code=1), "of": zc.Tbl("rle", code=6)})
    f.compressed(lits[:50], seqs3, lit=zc.Lit("raw"), tables=ALL_SEQ)
    add("seq_predefined_rle_repeat_initial_reps", f)
    # FSE tables at accuracy log 5 (all three) and at their maxima (9 / 8 / 9), offsets of codes 10..22
    f = zc.Frame(window_log=23)
    big = _rand(rng, 120000)
    for _ in range(40):
        f.raw(big)
    for al in ({"ll": 5, "ml": 5, "of": 5}, {"ll": 9, "ml": 9, "of": 8}):
        seqs = [(1 + (k % 5), 3 + k % 20, 3 + (1 << (10 + k % 13)) + k) for k in range(200)]
        f.compressed(_rand(rng, sum(s[0] for s in seqs)), seqs, lit=zc.Lit("raw"), tables=zc.auto_tables(seqs, al))
    add("seq_fse_al_min_max_of22", f)
    # nbSeq headers 127 / 128 / 0x7EFF / 0x7F00 (the last two: 1-byte literal blocks of thousands of tiny matches)
    for nseq in (127, 128, 0x7EFF, 0x7F00):
        f = zc.Frame(window_log=17)
        f.raw(_rand(rng, 64))
        seqs = [(0 if k % 2 else 1, 3, 3 + 17 + (k % 7)) for k in range(nseq)]
        # (ll == 0 with Offset_Value > 3: a fresh offset, no shift)
        lits = _rand(rng, sum(s[0] for s in seqs))
        f.compressed(lits, seqs, lit=zc.Lit("raw"), tables=zc.auto_tables(seqs))
        add("seq_nseq_%d" % nseq, f)
    # a block of <= 64 sequences with Huffman literals (segment-wise literals) next to one of many (literal buffer)
    f = zc.Frame(window_log=17)
    w = depth_tree(5, first=0x41)
    syms = bytes(s for s, x in enumerate(w) if x)
    f.raw(_rand(rng, 5000, syms))
    lits = _rand(rng, 3000, syms)
    seqs = [(40, 20 + k, 3 + 4000 + k) for k in range(64)]
    f.compressed(lits, seqs, lit=zc.Lit("huf", weights=w, form="direct", streams=4), tables=zc.auto_tables(seqs))
    seqs = [(4, 5 + k % 9, 3 + 100 + k % 50) for k in range(700)]
    f.compressed(_rand(rng, 2800, syms), seqs, lit=zc.Lit("treeless", streams=4), tables=zc.auto_tables(seqs))
    add("seq_segmented_and_literal_buffer", f)
    # ---- frames: single segment with 1/2/4/8-byte FCS, window descriptors with mantissas, checksums, empty frames
    for nb, n in ((1, 200), (2, 300), (4, 70000), (8, 5000)):
        f = zc.Frame(single_segment=nb == 1 or nb == 2, window_log=17, fcs_bytes=nb, checksum=nb == 4)
        data = _rand(rng, n)
        f.raw(data[:n // 2])
        f.compressed(data[n // 2:], [(3, 8, 3 + 5)] if n > 20 else (), lit=zc.Lit("raw"))
        add("frame_fcs%d" % nb, f)
    f = zc.Frame(window_desc=(3 << 3) | 5, checksum=True)
    f.rle(0x41, 9000)
    f.raw(_rand(rng, 9000))
    add("frame_window_mantissa", f)
    f = zc.Frame(window_log=10)
    add("frame_empty_last_block", f)
    f = zc.Frame(single_segment=True)
    add("frame_single_segment_empty", f)
    # matches exactly Window_Size back, blocks as large as the window allows
    for wd in (0, (1 << 3) | 3, 7 << 3):
        f = zc.Frame(window_desc=wd)
        win = f.window_size()
        bmax = min(win, 1 << 17)
        data = _rand(rng, 3 * win)
        for k in range(0, len(data), bmax):
            f.raw(data[k:k + bmax])
        seqs = [(1, 300, 3 + win), (0, 200, 1), (5, win - 600 if win < 100000 else 900, 3 + win - 1)]
        f.compressed(_rand(rng, 6), seqs, lit=zc.Lit("raw"))
        add("window_edge_wd%d" % wd, f)
    return out


def malformed_frames():
    """(name, payload, stream_verdict_defined) -- frames everyone must refuse"""
    rng = np.random.default_rng(0xBAD)
    out = []

    def add(name, fr, defined=True, mutate=None):
        p = fr.payload()[0]
        if mutate:
            p = mutate(p)
        out.append((name, p, defined))

    f = zc.Frame(window_log=17, fcs=100, fcs_bytes=4)
    f.raw(bytes(99))
    add("fcs_100_decodes_99", f)
    f = zc.Frame(window_log=17, fcs=500, fcs_bytes=2)
    f.raw(_rand(rng, 200))
    f.compressed(b"ab", [(2, 10, 3 + 50)])
    add("fcs_500_with_sequences_decodes_212", f)
    for off in (1500, 1990, 1025):
        f = zc.Frame(window_desc=0)
        f.raw(_rand(rng, 1000))
        f.raw(_rand(rng, 1000))
        f.compressed(b"ab", [(2, 10, off + 3)])
        # libzstd's streaming answer for offsets beyond the window depends on its buffer (it may return other bytes)
        add("window_1k_offset_%d" % off, f, defined=False)
    f = zc.Frame(window_desc=0)
    f.raw(_rand(rng, 1000))
    f.raw(_rand(rng, 1000))
    f.compressed(b"abc", [(2, 10, 3 + 1000), (0, 4, 1), (1, 5, 3 + 1030)])
    add("window_1k_offset_1030_later_sequence", f, defined=False)
    for wd, nm in ((18 << 3, "2p28"), (31 << 3, "2p41"), ((17 << 3) | 1, "2p27_plus")):
        f = zc.Frame(window_desc=wd)
        f.raw(b"hello")
        add("window_" + nm, f)
    # (with a Frame_Content_Size the output buffer can hold, libzstd's stream decoder takes its single-pass path, which
    # neither applies windowLogMax nor keeps to the window: its verdict then depends on the caller's buffer)
    f = zc.Frame(window_desc=18 << 3, fcs_bytes=4)
    f.raw(b"hello")
    add("window_2p28_with_fcs", f, defined=False)
    f = zc.Frame(window_desc=0, fcs_bytes=4)
    f.raw(_rand(rng, 1000))
    f.raw(_rand(rng, 1000))
    f.compressed(b"ab", [(2, 10, 3 + 1500)])
    add("window_1k_offset_1500_with_fcs", f, defined=False)
    f = zc.Frame(single_segment=True, fcs_bytes=4)
    f.raw(b"x")
    add("single_segment_fcs_2p28", f, mutate=lambda p: p[:1] + (1 << 28).to_bytes(4, "little") + p[5:])
    f = zc.Frame(window_desc=0)
    f.raw(bytes(2000))
    add("window_1k_raw_block_2000", f)
    f = zc.Frame(window_desc=0)
    f.rle(7, 2000)
    add("window_1k_rle_block_2000", f)
    f = zc.Frame(window_desc=0)
    f.compressed(_rand(rng, 1100))
    add("window_1k_compressed_block_1100", f)
    f = zc.Frame(single_segment=True, fcs_bytes=1)
    f.raw(bytes(10))
    add("single_segment_block_beyond_fcs", f, mutate=lambda p: p[:1] + bytes([5]) + p[2:])
    f = zc.Frame(window_log=17, dict_id=7)
    f.raw(b"needs a dictionary")
    add("dictionary_id", f)
    f = zc.Frame(window_log=17, checksum=True)
    f.raw(_rand(rng, 300))
    add("checksum_wrong", f, mutate=lambda p: p[:-1] + bytes([p[-1] ^ 1]))
    return out


VALID = None
COUNTS = {}


def corpus():
    global VALID
    if VALID is None:
        VALID = valid_frames()
    return VALID


REQUIRED = (
    {"block_raw", "block_rle", "block_compressed", "block_empty_last", "window_descriptor", "single_segment", "checksum",
     "fcs_1", "fcs_2", "fcs_4", "fcs_8",
     "lit_raw_hdr1", "lit_raw_hdr2", "lit_raw_hdr3", "lit_rle_hdr1", "lit_rle_hdr2", "lit_rle_hdr3",
     "lit_huf_1stream_hdr3", "lit_huf_4stream_hdr3", "lit_huf_4stream_hdr4", "lit_huf_4stream_hdr5",
     "lit_treeless_1stream_hdr3", "lit_treeless_4stream_hdr3", "lit_treeless_4stream_hdr4",
     "huf_weights_direct", "huf_weights_fse", "huf_direct_odd", "huf_direct_even",
     "huf_depth_1", "huf_depth_9", "huf_depth_10", "huf_depth_11",
     "nseq_0", "nseq_1b", "nseq_2b", "nseq_3b", "seq_few", "seq_many",
     "rep_1_ll0", "rep_1_llx", "rep_2_ll0", "rep_2_llx", "rep_3_ll0", "rep_3_llx",
     "seq_ll_al5", "seq_ll_al9", "seq_ml_al5", "seq_ml_al9", "seq_of_al5", "seq_of_al8"}
    | {"seq_%s_%s" % (k, m) for k in ("ll", "ml", "of") for m in ("predefined", "rle", "fse", "repeat")}
    | {"ll_code_%d" % c for c in range(36)} | {"ml_code_%d" % c for c in range(53)} | {"of_code_%d" % c for c in range(28)}
)


def test_coverage_gate():
    """The corpus and the two far-offset frames cover every feature in REQUIRED (removing a builder makes this fail)."""
    have = set().union(*(feat for _, _, _, feat in corpus()))
    have |= far_offset_frame()[2] | long_offset_frame()[2]
    assert REQUIRED - have == set()


def test_writer_checked_by_libzstd():
    """Every valid frame decodes to the writer's expectation in libzstd, one-shot and streaming."""
    bad = []
    for name, p, exp, _ in corpus():
        if zstd_ref.decompress(zc.MAGIC + p, len(exp) + 64) != exp:
            bad.append(name + ": one-shot")
        got, err = zstd_ref.decompress_stream(zc.MAGIC + p)
        if err or got != exp:
            bad.append("%s: streaming %s" % (name, err))
    assert not bad


def test_oracle_statistics():
    """The oracle's own counters (ZoStats) agree frame by frame with what the writer built: literal sections of each kind,
    sequence table modes per table, sequences."""
    from oracle import oracle
    modes = ("predefined", "rle", "fse", "repeat")
    bad = []
    for name, p, exp, feat in corpus():
        out, st = oracle.zstd_decode(p, len(exp), stats=True)
        c = COUNTS[name]
        want = {k: c.get(k, 0) for k in ("lit_raw", "lit_rle", "lit_huf", "lit_treeless")}
        got = {k: getattr(st, k) for k in want}
        want["modes"] = [c.get("mode_%s_%s" % (t, m), 0) for t in ("ll", "of", "ml") for m in modes]
        got["modes"] = list(st.seq_mode_count)
        want["sequences"], got["sequences"] = c.get("sequences", 0), st.sequences
        if out != exp or got != want:
            bad.append("%s: oracle %s, writer %s" % (name, got, want))
    assert not bad


def test_malformed_refused_by_reference_where_defined():
    bad = []
    for name, p, defined in malformed_frames():
        if defined:
            got, err = zstd_ref.decompress_stream(zc.MAGIC + p)
            if err is None:
                bad.append(name)
    assert not bad


def oracle_verdict(p, capacity):
    """the oracle's zstd stage on one payload -> (bytes or None, error kind or None)"""
    from oracle import oracle
    try:
        return oracle.zstd_decode(p, capacity), None
    except oracle.OracleError as e:                        # (zo_decode_section: -1 cut short, -2 corrupt, -4 needs a dictionary)
        return None, {-1: "io:eof", -2: "io:invalid", -4: "io:invalid"}.get(e.kind, "oracle:%d" % e.kind)


def product_verdict(lib, p, capacity):
    """nafgpu_zstd_decompress on one payload -> (bytes or None, error kind or None)"""
    from nafcodec_amd import _ffi
    try:
        return lib.zstd_decompress(p, capacity), None
    except _ffi.NafError as e:
        if e.status == _ffi.E_IO and e.io_kind in (_ffi.IO_UNEXPECTED_EOF, _ffi.IO_INVALID_DATA):
            return None, "io:eof" if e.io_kind == _ffi.IO_UNEXPECTED_EOF else "io:invalid"
        return None, "other:%d/%d" % (e.status, e.io_kind)


def test_malformed_refused_by_oracle():
    """refused as corrupt (not for want of room, not by some other exception)"""
    bad = ["%s: %s" % (name, v[1]) for name, p, _ in malformed_frames() for v in [oracle_verdict(p, 1 << 16)] if v[1] != "io:invalid"]
    assert not bad


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from nafcodec_amd import _ffi
    return _ffi.Library(os.path.join(EMU_DIR, "libnafgpu_emu.so"))


def check_frames(lib, valid=True, malformed=True):
    """-> names of the frames on which the product disagrees: with the expectation (valid) or by decoding (malformed)"""
    bad = []
    if valid:
        for name, p, exp, _ in corpus():
            got = product_verdict(lib, p, len(exp))
            if got != (exp, None):
                bad.append("%s: %s" % (name, got[1] or "other bytes"))
            if oracle_verdict(p, len(exp)) != (exp, None):
                bad.append(name + " (oracle)")
    if malformed:
        for name, p, _ in malformed_frames():            # refused, and for the same reason as the oracle gives
            got, want = product_verdict(lib, p, 1 << 16), oracle_verdict(p, 1 << 16)
            if got[1] is None or got != want:
                bad.append("%s: product %s, oracle %s" % (name, got[1] or "ok", want[1] or "ok"))
    return bad


def ascii_frame():
    """a frame of letters (valid text): Huffman literals, FSE and repeat-mode tables, repeat offsets"""
    rng = np.random.default_rng(0xA5C)
    w = depth_tree(7, first=0x41)
    syms = bytes(s for s, x in enumerate(w) if x)
    f = zc.Frame(window_log=17)
    f.compressed(_rand(rng, 3000, syms), lit=zc.Lit("huf", weights=w, form="direct", streams=4))
    seqs = [(3 + k % 5, 4 + k % 11, 3 + 200 + k % 90 if k % 4 else 1 + k % 3) for k in range(300)]
    f.compressed(_rand(rng, 2500, syms), seqs, lit=zc.Lit("treeless", streams=4), tables=zc.auto_tables(seqs))
    f.compressed(_rand(rng, 400, syms), seqs[:40], lit=zc.Lit("treeless", streams=1), tables=ALL_SEQ)
    p, exp, _ = f.payload()
    return p, exp


def naf_cases():
    """(name, archive, options, valid): the frames as the Sequence section of DNA archives (several records; one with a
    Mask section), as text where they decode to letters, letters as the Sequence and the Quality section of reads, and
    the malformed frames inside DNA archives"""
    out = []
    for name, p, exp, _ in corpus():
        n = 2 * len(exp)
        lens = [n // 3, 0, n - n // 3] if n > 2 else [n]
        out.append(("dna:" + name, cases.naf_with_payload(p, len(exp), "dna", lens=lens), {}, True))
    for name, p, _ in malformed_frames():
        out.append(("dna:" + name, cases.naf_with_payload(p, 2000, "dna"), {}, False))
    name, p, exp, _ = next(c for c in corpus() if c[0] == "seq_segmented_and_literal_buffer")
    n = 2 * len(exp)
    runs = [37, 1200, 5, 5, 3000, 1, 0, 777]
    runs.append(n - sum(runs))
    out.append(("dna_masked:" + name, cases.naf_with_payload(p, len(exp), "dna", lens=[n // 2, n - n // 2], mask_runs=runs), {}, True))
    p, exp = ascii_frame()
    n = len(exp)
    lens = [151] * (n // 151) + [n % 151]
    out.append(("text:letters", cases.naf_with_payload(p, n, "text", lens=lens), {}, True))
    out.append(("reads:letters", cases.naf_with_payload(p, n, "text", lens=lens, quality=(p, n)), {}, True))
    return out


def check_naf(lib):
    bad = []
    for name, blob, opts, valid in naf_cases():
        got, want = cases.run_product(blob, opts, lib), cases.run_oracle(blob, opts)
        if got != want or (want[1] is None) != valid:
            bad.append("%s: product %s, oracle %s" % (name, got[1], want[1]))
    return bad


def test_emu_frames(emu):
    assert check_frames(emu) == []


def test_emu_naf_level(emu):
    assert check_naf(emu) == []


@pytest.mark.parametrize("var,values", [("NAFGPU_HUF_SPLIT", ("2", "16")), ("NAFGPU_K2_LDS", ("0", "1", "2")),
                                        ("NAFGPU_LZ_MODE", ("dense", "sparse")), ("NAFGPU_PJ_STRIPS", ("0", "1"))])
def test_emu_kernel_variants(emu, monkeypatch, var, values):
    emu.c.nafgpu_test_hooks(1)
    try:
        for v in values:
            monkeypatch.setenv(var, v)
            if var == "NAFGPU_PJ_STRIPS":
                monkeypatch.setenv("NAFGPU_LZ_MODE", "dense")
            assert check_frames(emu, malformed=(v == values[0])) == [], (var, v)
    finally:
        emu.c.nafgpu_test_hooks(0)


def window_edge_archive():
    """a DNA archive whose frame has a 1 KiB window, blocks of 1 KiB and matches exactly the window back, in 40 blocks"""
    rng = np.random.default_rng(5)
    f = zc.Frame(window_desc=0)
    for k in range(20):
        f.raw(_rand(rng, 1024))
        f.compressed(_rand(rng, 8), [(4, 500, 3 + 1024), (4, 300, 1), (0, 200, 3 + 1024)])
    p, exp, _ = f.payload()
    return cases.naf_with_payload(p, len(exp), "dna", lens=[len(exp), len(exp)]), exp


def test_emu_window_edge_tiles(emu, monkeypatch):
    """matches exactly Window_Size back across tile edges (NAFGPU_TILE_KIB) -- the tile halo is sized by the window"""
    blob, exp = window_edge_archive()
    want = cases.run_oracle(blob, {})
    assert want[1] is None
    emu.c.nafgpu_test_hooks(1)
    try:
        for kib in ("4", "9"):
            monkeypatch.setenv("NAFGPU_TILE_KIB", kib)
            assert cases.run_product(blob, {}, emu) == want, kib
    finally:
        emu.c.nafgpu_test_hooks(0)


def check_window_edge_shards(lib):
    from nafcodec_amd.decoder import Decoder
    from nafcodec_amd.sharding import decode_sharded_local
    blob, exp = window_edge_archive()
    want = "".join(r[2] for r in cases.run_oracle(blob, {})[0]).encode()
    for world in (2, 3):
        decs = [Decoder(io.BytesIO(blob), shard_rank=r, shard_count=world, shard_protocol=True, _lib=lib) for r in range(world)]
        res = decode_sharded_local(decs)
        got = b"".join(d.copy_to_host(x.d_sequence, x.n_bases) for d, x in zip(decs, res))
        assert got == want, world
        for d in decs:
            d.close()


def test_emu_window_edge_shards(emu):
    """... and across shard edges: the shard protocol on the same archive at worlds 2 and 3"""
    check_window_edge_shards(emu)


def long_offset_frame():
    """window 2^27, about 129 MiB of output: a raw block of random bytes, RLE blocks, then sequences with OF codes 26 / 27,
    ML codes 51 / 52 and LL codes 34 / 35 at FSE accuracy logs 9 / 8 / 9.  The longest reads of the sequence bitstream a
    frame within the 2^27 window limit allows: 27 + 16 + 15 extra bits and 26 bits of state updates per sequence (the
    89-bit bound of SeqWindow needs OF code 31, whose offsets no accepted window holds)"""
    rng = np.random.default_rng(27)
    f = zc.Frame(window_log=27)
    far = _rand(rng, 1 << 17)
    f.raw(far)
    for k in range(1023):
        f.rle(k & 255, 1 << 17)
    base = len(f.out)                                        # 2^27
    # (LL code 35 and ML code 52 cannot share a sequence -- 65536 + 65539 bytes exceed a block --: each goes with the
    # largest code the other leaves room for, and OF code 27 or 26)
    s1 = [(65536 + 1000, 32771 + 1000, 3 + (1 << 27)), (7, 4, 3 + (1 << 26) + 12345)]
    f.compressed(_rand(rng, 65536 + 1007), s1, lit=zc.Lit("raw"), tables=zc.auto_tables(s1, {"ll": 9, "ml": 9, "of": 8}))
    s2 = [(32768 + 1000, 65539 + 1000, (1 << 27) + 2), (5, 100, 3 + (1 << 26) + 99)]
    f.compressed(_rand(rng, 32768 + 1005), s2, lit=zc.Lit("raw"), tables=zc.auto_tables(s2, {"ll": 9, "ml": 9, "of": 8}))
    assert len(f.out) > base
    return f.payload()


def far_offset_frame():
    """window 2^25, a little over 32 MiB of output: random raw blocks, RLE filler, then offsets of codes 23, 24 and 25, the
    last exactly Window_Size back"""
    rng = np.random.default_rng(25)
    f = zc.Frame(window_log=25)
    for k in range(256):                                     # 2^25 bytes: random where the far matches land, RLE elsewhere
        if k in (0, 1, 128, 192):
            f.raw(_rand(rng, 1 << 17))
        else:
            f.rle((7 * k) & 255, 1 << 17)
    seqs = [(5, 300, 3 + (1 << 25)), (3, 200, 3 + (1 << 24) + 4321), (2, 100, 3 + (1 << 23) + 99), (4, 50, 3 + (1 << 25) - 17)]
    f.compressed(_rand(rng, 20), seqs, lit=zc.Lit("raw"), tables=zc.auto_tables(seqs, {"ll": 5, "ml": 5, "of": 5}))
    return f.payload()


@pytest.mark.parametrize("build", [far_offset_frame, long_offset_frame])
def test_far_offsets_libzstd(build):
    p, exp, feat = build()
    assert {"of_code_%d" % c for c in ((23, 24, 25) if build is far_offset_frame else (26, 27))} <= feat
    got, err = zstd_ref.decompress_stream(zc.MAGIC + p, chunk=1 << 20)
    assert err is None and got == exp
    assert zstd_ref.decompress(zc.MAGIC + p, len(exp)) == exp


@pytest.mark.parametrize("build", [far_offset_frame, long_offset_frame])
def test_emu_far_offsets(emu, build):
    p, exp, _ = build()
    assert oracle_verdict(p, len(exp)) == (exp, None)
    assert product_verdict(emu, p, len(exp)) == (exp, None)


# ---------------------------------------------------------------------------------------------------- address sanitizer


def test_malformed_under_address_sanitizer():
    """the malformed frames (and the valid ones) through the AddressSanitizer build of the CPU harness"""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.exists(asan):
        pytest.skip("libasan not available")
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    script = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_zstd_crafted as t
from nafcodec_amd import _ffi
lib = _ffi.Library(%r)
bad = t.check_frames(lib, valid=sys.argv[1] == "1", malformed=sys.argv[1] == "0")
print("BAD", bad)
sys.exit(1 if bad else 0)
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libnafgpu_emu_asan.so"))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1")
    procs = [subprocess.Popen([sys.executable, "-c", script, k], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in ("0", "1")]
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, out[-2000:] + err[-4000:]


# ---------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_gpu_frames():
    from nafcodec_amd import _ffi
    assert check_frames(_ffi.default()) == []


@pytest.mark.gpu
def test_gpu_naf_level():
    from nafcodec_amd import _ffi
    assert check_naf(_ffi.default()) == []


@pytest.mark.gpu
def test_gpu_kernel_variants(monkeypatch):
    from nafcodec_amd import _ffi
    lib = _ffi.default()
    lib.c.nafgpu_test_hooks(1)
    try:
        for var, values in (("NAFGPU_HUF_SPLIT", ("2", "16")), ("NAFGPU_K2_LDS", ("0", "1", "2")),
                            ("NAFGPU_LZ_MODE", ("dense", "sparse")), ("NAFGPU_PJ_STRIPS", ("0", "1"))):
            for v in values:
                monkeypatch.setenv(var, v)
                if var == "NAFGPU_PJ_STRIPS":
                    monkeypatch.setenv("NAFGPU_LZ_MODE", "dense")
                assert check_frames(lib, malformed=False) == [], (var, v)
            monkeypatch.delenv(var)
            monkeypatch.delenv("NAFGPU_LZ_MODE", raising=False)
        blob, exp = window_edge_archive()
        want = cases.run_oracle(blob, {})
        for kib in ("4", "9"):
            monkeypatch.setenv("NAFGPU_TILE_KIB", kib)
            assert cases.run_product(blob, {}, lib) == want, kib
    finally:
        lib.c.nafgpu_test_hooks(0)


@pytest.mark.gpu
def test_gpu_far_offsets_32mib():
    """offset codes 23 / 24 / 25, one exactly Window_Size (2^25) back"""
    from nafcodec_amd import _ffi
    p, exp, _ = far_offset_frame()
    assert oracle_verdict(p, len(exp)) == (exp, None)
    assert product_verdict(_ffi.default(), p, len(exp)) == (exp, None)


@pytest.mark.gpu
def test_gpu_window_edge_shards():
    """matches exactly Window_Size back across shard edges: the shard protocol at worlds 2 and 3 on the device"""
    from nafcodec_amd import _ffi
    check_window_edge_shards(_ffi.default())


@pytest.mark.gpu
def test_gpu_long_offsets_129mib():
    """offset codes 26 / 27 reaching 2^27 back with ML codes 51 / 52 and LL codes 34 / 35 (see long_offset_frame)"""
    from nafcodec_amd import _ffi
    from oracle import oracle
    p, exp, _ = long_offset_frame()
    assert oracle.zstd_decode(p, len(exp)) == exp
    got = _ffi.default().zstd_decompress(p, len(exp))
    assert len(got) == len(exp) and got == exp
