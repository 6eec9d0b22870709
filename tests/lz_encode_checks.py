"""Shared by tests/test_lz_encode_emu.py (CPU harness) and tests/test_gpu_lz_encode.py (MI355X): the device encoder's
blocks with LZ sequences (nafgpu_zstd_compress_lz, opts.device_lz).  Not a test module; every function takes the library
binding it is to check.

The frame is the device matcher's own, so nothing is compared with the host's level-0 bytes.  What is checked instead:
three readers (system libzstd, the CPU oracle, this library's decoder) give the input back; two calls give the same bytes;
size and hash64 of each frame are pinned below (taken on the CPU harness; the MI355X must give the same numbers); and the
frame is read back here, down to every sequence's (literal run, match length, distance), to prove that the input took the
branch it was made for."""
import ctypes
import io

import numpy as np

import encode_checks as ec
import text_parse_checks as tc
import zstd_ref
from conftest import golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import Encoder, Record, encode_device, encode_text
from oracle import oracle

BLOCK = 128 << 10
TILE, SUB, CAP, MIN_MATCH = 1024, 64, 256, 6      # encode.hip / encode.h: asserted in kernel_constants()
ENTRY_POINTS = ("nafgpu_zstd_compress_lz",)


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return tc.bind(lib)


def kernel_constants():
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "encode.hip")) as f:
        text = f.read()
    assert "kLzTile = %d, " % TILE in text and "kLzSubs = %d, " % (TILE // SUB) in text
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "encode.h")) as f:
        text = f.read()
    assert "kLzMatchCap = %d;" % CAP in text and "kLzMinMatch = %d;" % MIN_MATCH in text


# ---------------------------------------------------------------- reading a frame back (RFC 8878 3.1.1)
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def fse_table(norm, al):
    """the decoding table of a normalised distribution -> [(symbol, bits, base)] per state"""
    size = 1 << al
    sym, high, nxt = [0] * size, size - 1, []
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt.append(1)
        else:
            nxt.append(c)
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    out = []
    for i in range(size):
        d = nxt[sym[i]]
        nxt[sym[i]] += 1
        nb = al - (d.bit_length() - 1)
        out.append((sym[i], nb, (d << nb) - size))
    return out


T_LL, T_ML, T_OF = fse_table(LL_NORM, 6), fse_table(ML_NORM, 6), fse_table(OF_NORM, 5)


def read_sequences(stream, n):
    """the backward bitstream of n sequences coded with the three predefined tables -> [(ll, ml, distance)]"""
    v = int.from_bytes(stream, "little")
    assert stream[-1] != 0
    pos = v.bit_length() - 1                              # below the end mark

    def read(bits):
        nonlocal pos
        pos -= bits
        assert pos >= 0
        return (v >> pos) & ((1 << bits) - 1)

    s_ll, s_of, s_ml = read(6), read(5), read(6)
    out = []
    for i in range(n):
        lc, oc, mc = T_LL[s_ll][0], T_OF[s_of][0], T_ML[s_ml][0]
        ofv = (1 << oc) + read(oc)
        ml = ML_BASE[mc] + read(ML_BITS[mc])
        ll = LL_BASE[lc] + read(LL_BITS[lc])
        assert ofv > 3, "a repeat-offset code"              # every offset is a new offset
        out.append((ll, ml, ofv - 3))
        if i + 1 < n:
            s_ll = T_LL[s_ll][2] + read(T_LL[s_ll][1])
            s_ml = T_ML[s_ml][2] + read(T_ML[s_ml][1])
            s_of = T_OF[s_of][2] + read(T_OF[s_of][1])
    assert pos == 0
    return out


def read_frame(frame, n):
    """-> one dict per block: kind 'raw' / 'rle' / 'huf' / 'treeless' (no sequences) or 'seq'; for 'seq': lits ('raw', 'rle',
    'huf', 'treeless'), n_lit, seqs [(ll, ml, distance)]; n: bytes the block holds"""
    assert bytes(frame[:2]) == (b"\x00\x50" if n >= 64 else b"\x00\x48")
    at, out = 2, []
    while True:
        bh = frame[at] | (frame[at + 1] << 8) | (frame[at + 2] << 16)
        at += 3
        last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
        if kind == 0:
            out.append(dict(kind="raw", n=size))
            at += size
        elif kind == 1:
            out.append(dict(kind="rle", n=size))
            at += 1
        else:
            assert kind == 2 and size <= BLOCK
            end, b0 = at + size, frame[at]
            lit, fmt = b0 & 3, (b0 >> 2) & 3
            if lit < 2:                                       # raw / RLE literals
                if fmt in (0, 2):
                    n_lit, at = b0 >> 3, at + 1
                elif fmt == 1:
                    n_lit, at = (b0 >> 4) | (frame[at + 1] << 4), at + 2
                else:
                    n_lit, at = (b0 >> 4) | (frame[at + 1] << 4) | (frame[at + 2] << 12), at + 3
                at += n_lit if lit == 0 else 1
            else:
                assert fmt != 0, "one-stream literals"
                nbytes, bits = {1: (3, 10), 2: (4, 14), 3: (5, 18)}[fmt]
                v = int.from_bytes(frame[at:at + nbytes], "little")
                n_lit, comp = (v >> 4) & ((1 << bits) - 1), v >> (4 + bits)
                at += nbytes + comp
            lits = ("raw", "rle", "huf", "treeless")[lit]
            n_seq = frame[at]
            at += 1
            if n_seq >= 128:
                assert n_seq < 255, "three-byte sequence count"
                n_seq = ((n_seq - 128) << 8) | frame[at]
                at += 1
            if n_seq == 0:
                assert at == end and lit >= 2
                out.append(dict(kind=lits, n=n_lit))
            else:
                assert frame[at] == 0, "Symbol_Compression_Modes"
                seqs = read_sequences(bytes(frame[at + 1:end]), n_seq)
                assert all(ml >= MIN_MATCH for _, ml, _ in seqs)
                held = n_lit + sum(ml for _, ml, _ in seqs)
                assert sum(ll for ll, _, _ in seqs) <= n_lit
                pos = 0
                for ll, ml, dist in seqs:                     # no match reaches in front of its block
                    pos += ll
                    assert dist <= pos, (pos, dist)
                    pos += ml
                out.append(dict(kind="seq", lits=lits, n_lit=n_lit, seqs=seqs, n=held))
            at = end
        if last:
            assert at == len(frame) and sum(b["n"] for b in out) == n
            return out


# ---------------------------------------------------------------- inputs
def no_repeat(n, seed=1):
    """n bytes in which no 6-byte string occurs twice: a walk through a permutation of the 24-bit values (a full-period
    congruential generator), three bytes per step -- a 6-byte window holds at least one whole step, which occurs once; windows
    of different alignment could still agree, so the property itself is checked."""
    steps = (n + 2) // 3
    x = np.empty(steps, dtype=np.uint64)
    v = (seed * 7919) & 0xFFFFFF
    mul, add = 0x0A3D71, 0x3C6EF5                            # mul % 4 == 1, add odd: period 2^24
    for i in range(steps):
        x[i] = v
        v = (v * mul + add) & 0xFFFFFF
    out = np.empty((steps, 3), dtype=np.uint8)
    for k in range(3):
        out[:, k] = (x >> np.uint64(8 * k)) & np.uint64(0xFF)
    data = out.reshape(-1)[:n]
    if n >= 6:
        keys = np.zeros(n - 5, dtype=np.uint64)
        for k in range(6):
            keys |= data[k:n - 5 + k].astype(np.uint64) << np.uint64(8 * k)
        assert len(np.unique(keys)) == n - 5
    return bytes(data)


_FILL = {}


def fill(n, seed=1):
    """the first n bytes of one no-repeat text per seed"""
    if seed not in _FILL:
        _FILL[seed] = no_repeat(2 * BLOCK + 4096, seed)
    assert n <= len(_FILL[seed])
    return _FILL[seed][:n]


_DB = []


def de_bruijn_text(k=8, n=6, letters=b"ACGTNRYK"):
    """a de Bruijn sequence B(k, n) as text: every string of n letters occurs once (Lyndon words, in order)"""
    if not _DB:
        seq, w = bytearray(), [0]                           # (iterative form of the usual recursion: Duval's algorithm)
        while w:
            if n % len(w) == 0:
                seq += bytes(letters[c] for c in w)
            w = [w[j % len(w)] for j in range(n)]
            while w and w[-1] == k - 1:
                w.pop()
            if w:
                w[-1] += 1
        _DB.append(bytes(seq))
    return _DB[0]


def run_copy(head, run, copy_from=None, copy_len=0, tail=40, byte=b"z"):
    """`head` unique bytes, a run of `run` times one byte, then `copy_len` bytes of the head again (from `copy_from`), then
    `tail` unique bytes.  The run touches one slot of the matcher's table only, so the head is still found behind it.
    Expected: (head + 1, run - 1, 1) if run - 1 >= 6, then (0 or what the run left, copy_len, head - copy_from + run)."""
    u = fill(head + tail + 8)
    assert byte[0] not in (u[head - 1], u[head])             # the run is `run` bytes, no more
    data = u[:head] + byte * run
    if copy_len:
        data += u[copy_from:copy_from + copy_len]
        assert u[copy_from + copy_len] != u[head]             # the match ends where the copy ends
    return data + u[head:head + tail]


def expect_run_copy(head, run, copy_from=None, copy_len=0, tail=40):
    seqs, pend = [], head + run
    if run - 1 >= MIN_MATCH:
        seqs.append((head + 1, run - 1, 1))
        pend = 0
    if copy_len >= MIN_MATCH:
        seqs.append((pend, copy_len, head - copy_from + run))
        pend = 0
    else:
        pend += copy_len
    return seqs, pend + tail


def period(p, n, seed=2):
    u = fill(p, seed)
    return (u * (n // p + 1))[:n]


def srr_ids(n_reads):
    return b"".join(b"SRR1770413.%d\0" % i for i in range(1, n_reads + 1))


def illumina_ids(n_reads):
    return b"".join(b"A00123:45:HXXXXDSXX:1:%d:%d:%d\0" % (1101 + i // 5000, 1000 + (i * 7919) % 30000, 1000 + (i * 104729) % 36000)
                    for i in range(n_reads))


def one_seq_block(seqs, tail_lits=None, lits=None):
    def check(blocks):
        assert len(blocks) == 1 and blocks[0]["kind"] == "seq", blocks[0]["kind"]
        b = blocks[0]
        assert b["seqs"] == seqs, b["seqs"][:4]
        if tail_lits is not None:
            assert b["n_lit"] - sum(ll for ll, _, _ in b["seqs"]) == tail_lits
        if lits is not None:
            assert b["lits"] == lits, b["lits"]
        return True
    return check


def section_inputs(multi_chunk=True):
    """(name, data, check over read_frame's blocks)"""
    out = []

    def add(name, data, check):
        out.append((name, data, check))

    def add_run_copy(name, *args, lits=None, **kw):
        seqs, tail = expect_run_copy(*args, **kw)
        add(name, run_copy(*args, **kw), one_seq_block(seqs, tail, lits))

    kinds = lambda *want: (lambda blocks: [b["kind"] for b in blocks] == list(want))
    # ---- sizes
    add("empty", b"", kinds("raw"))
    add("63_bytes", b"ab" * 31 + b"a", kinds("raw"))                                   # under 64 bytes: raw_frame, no matching
    add("64_bytes", b"ab" * 32, one_seq_block([(2, 62, 2)], 0, "raw"))
    add("65_bytes", b"ab" * 32 + b"a", one_seq_block([(2, 63, 2)], 0))
    ids = srr_ids(7000)                                                                # 103 893 bytes
    assert len(ids) < BLOCK - 1
    pad = lambda n: ids + fill(n - len(ids), 3)
    add("block_minus_1", pad(BLOCK - 1), lambda b: [x["kind"] for x in b] == ["seq"] and b[0]["lits"] == "huf")
    add("block", pad(BLOCK), lambda b: [x["kind"] for x in b] == ["seq"])
    add("block_plus_1", pad(BLOCK + 1), lambda b: [x["kind"] for x in b] == ["seq", "raw"] and b[1]["n"] == 1)
    # ---- periods; up to the sub-tile every position finds its source, so the frame is one sequence
    add("period_1", period(1, 3000), kinds("rle"))                                     # (1, 2999, 1) is dearer than an RLE block
    for p in (2, 3, 5, 7, 40):
        add("period_%d" % p, period(p, 3000), one_seq_block([(p, 3000 - p, p)], 0, "raw"))
    for p in (TILE - 1, TILE, TILE + 1, 4095, 70000):                                  # across tiles: the source may have left the table,
        n = 100000 if p == 70000 else 3 * p + 1000                                      # but every source is the text one period back

        def check(blocks, p=p, n=n):
            b = blocks[0]
            return len(blocks) == 1 and b["kind"] == "seq" and all(d == p for _, _, d in b["seqs"]) and b["n_lit"] < p + 600 and \
                sum(ml for _, ml, _ in b["seqs"]) > n - p - 600
        add("period_%d" % p, period(p, n), check)
    add("one_value_block", b"G" * BLOCK, kinds("rle"))                                 # (1, 131071, 1) loses against an RLE block
    add("one_value_3_blocks", b"G" * (3 * BLOCK + 5), kinds("rle", "rle", "rle", "raw"))
    # a source that ends exactly at a tile border (and the copy just behind it); a copy of 30 bytes of which 20 lie in front
    # of a block border: the match is cut there, and the 10 behind the border find no source (theirs ends at the border)
    u = fill(BLOCK + 200, 4)
    add("source_ends_at_tile_border", u[:TILE] + u[TILE - 30:TILE] + u[TILE:TILE + 50], one_seq_block([(TILE, 30, 30)], 50))
    add("copy_across_block_border", u[:BLOCK - 20] + u[BLOCK - 50:BLOCK - 20] + u[BLOCK:BLOCK + 40] + u[BLOCK + 60:BLOCK + 100],
        lambda b: [x["kind"] for x in b] == ["seq", "raw"] and b[0]["seqs"] == [(BLOCK - 20, 20, 30)] and b[0]["n"] == BLOCK)
    # a match that would run across the block end: cut there; the next block begins with literals
    z = fill(BLOCK - 100, 5) + b"q" * 300 + fill(200, 6)

    def cut(blocks):
        a, b = blocks
        assert a["kind"] == "seq" and a["seqs"] == [(BLOCK - 100 + 1, 99, 1)] and a["n"] == BLOCK
        assert b["kind"] == "seq" and b["seqs"] == [(1, 199, 1)] and b["n_lit"] == 201
        return True
    add("match_cut_at_block_end", z, cut)
    # ---- match lengths: 5 is not taken, 6 is; both sides of every ML code border (run - 1 is the length)
    # (a copy of 20 bytes of the head behind the run keeps the block worth its sequences)
    for ml in (5, 6, 34, 35, 36, 37, 66, 67, 130, 131, CAP - 1, CAP, CAP + 1, 258, 259, 514, 515, 65538, 65539):
        add_run_copy("ml_%d" % ml, 30, ml + 1, 5, 20)
    # ---- literal runs: both sides of every LL code border (head + 1 is the run)
    for ll in (15, 16, 17, 18, 23, 24, 63, 64, 65535, 65536):
        add_run_copy("ll_%d" % ll, ll - 1, 20)
    # ---- distances: both sides of distance + 3 = 2^k; small ones as periods, the others behind a run
    for k in range(3, 17):
        for dist in ((1 << k) - 4, (1 << k) - 3):
            if dist < 60:
                add("dist_%d" % dist, period(dist, dist + 100, 7), one_seq_block([(dist, 100, dist)], 0))
            else:
                add_run_copy("dist_%d" % dist, 50, dist - 30, 20, 20)
    # ---- sequence counts: 127 and 128 (the one- and the two-byte count).  The three-byte form needs 32 512 sequences, and a
    # block of 128 KiB holds at most 21 845 matches of 6 bytes: it cannot occur.
    for count in (127, 128):
        # per sub-tile: 50 new bytes, 10 of them again (12 back: the lane finds the source in its own sub-tile), one byte that
        # ends the match, 3 new bytes
        u = fill(SUB * count, 8)
        data = b"".join(u[SUB * i:SUB * i + 50] + u[SUB * i + 38:SUB * i + 48] + bytes([u[SUB * i + 48] ^ 0xFF]) + u[SUB * i + 61:SUB * i + 64]
                        for i in range(count))
        assert len(data) == SUB * count
        add("%d_sequences" % count, data, one_seq_block([(50, 10, 12)] + [(54, 10, 12)] * (count - 1), 4))
    # ---- block endings and literal formats
    add("ends_in_a_match", fill(100, 9) + fill(100, 9)[60:100], one_seq_block([(100, 40, 40)], 0, "raw"))
    # literals of 255 / 256 bytes (raw, then Huffman), 1 023 / 1 024 and 16 383 / 16 384 (the three size formats): a text of
    # eight letters without a repeated 6-byte string; 40 of them replaced by 40 byte values that occur nowhere else, and those
    # again 52 bytes on, inside one sub-tile (the lane finds the nearest equal four bytes there: the source); a mark in front
    # and one behind, so that the match is those 40 bytes; 10 more letters.
    # 255 literals are raw literals, and dearer than the whole block Huffman-coded: no sequences there.
    # Literals that are all one byte value (RLE literals) cannot come out of this parse: 256 of them would have to stand in
    # runs shorter than 7 between matches whose sources are made of the same byte, and such a source is itself a run.
    L = de_bruijn_text()
    for n_lit in (255, 256, 1023, 1024, 16383, 16384):
        m = n_lit - 11
        assert m % SUB >= 52
        mark = bytes(range(200, 240))
        data = L[:m - 52] + mark + L[m - 12:m - 1] + b"#" + mark + b"%" + L[m + 100:m + 110]
        add("literals_%d" % n_lit, data, kinds("huf") if n_lit < 256 else one_seq_block([(m, 40, 52)], 11, "huf"))
    return out


# ---------------------------------------------------------------- checks
def hash64(lib, data):
    return lib.c.nafgpu_hash64_host(data, len(data))


def compress_lz(lib, data):
    return lib.zstd_compress(data, 0, True)


def three_readers(lib, frame, data, name):
    assert zstd_ref.decompress_magicless(frame, len(data) + 8) == data, (name, "libzstd")
    assert oracle.zstd_decode(frame, len(data) + 8) == data, (name, "oracle")
    assert lib.zstd_decompress(frame, len(data), 0) == data, (name, "decoder")


def check_section(lib, name, data, check):
    got = compress_lz(lib, data)
    print("%s: %d -> %d bytes, hash64 %#018x" % (name, len(data), len(got), hash64(lib, got)))
    three_readers(lib, got, data, name)
    assert compress_lz(lib, data) == got, (name, "two calls")
    assert check(read_frame(got, len(data))) is True, name
    assert (len(got), hash64(lib, got)) == PINNED[name], (name, len(got), hex(hash64(lib, got)))
    if len(got) > 4:                                        # a destination that is too small: refused, with the size that is needed
        buf, produced, err = ctypes.create_string_buffer(4), ctypes.c_size_t(0), _ffi.Error()
        assert lib.c.nafgpu_zstd_compress_lz(data, len(data), buf, 4, ctypes.byref(produced), 0, ctypes.byref(err)) == _ffi.E_INVALID_ARG
        assert produced.value == len(got)


def host_frames(lib, data):
    """-> (h0, h1): the host encoder's level-0 and level-1 frame of `data`"""
    out = []
    for level in (0, 1):
        blob = ec.host_archive(lib, [Record(sequence=data)], "text", level, sequence=True)
        out.append(ec.sections(blob)["sequence"][1])
    return out


def size_inputs():
    phix = oracle.Decoder(golden_bytes("phix.naf"))
    return [("srr_ids", srr_ids(200000)), ("illumina_ids", illumina_ids(200000)), ("phix_ids", phix.section(0)[0]),
            ("phix_quality", phix.section(5)[0])]


def check_size(lib, name, data):
    """closer to the host's LZ frame than to its literal-only frame: len(device) <= (h0 + h1) / 2"""
    h0, h1 = host_frames(lib, data)
    got = compress_lz(lib, data)
    print("%s: %d bytes; device %d, h0 %d, h1 %d, device / h0 %.3f" % (name, len(data), len(got), len(h0), len(h1), len(got) / len(h0)))
    three_readers(lib, got, data, name)
    assert 2 * len(got) <= len(h0) + len(h1), (name, len(got), len(h0), len(h1))
    assert (len(got), hash64(lib, got)) == PINNED[name], (name, len(got), hex(hash64(lib, got)))


def check_no_repeat(lib):
    """nothing to find: exactly the level-1 frame, except for the window byte"""
    for n in (64, 5000, BLOCK + 77, 2 * BLOCK + 4096):
        data = no_repeat(n, seed=12)
        got, want = compress_lz(lib, data), host_frames(lib, data)[1]
        assert want[:2] == b"\x00\x48" and got == b"\x00\x50" + want[2:], n
    # letters: Huffman blocks
    data = de_bruijn_text()[:2 * BLOCK]
    got, want = compress_lz(lib, data), host_frames(lib, data)[1]
    assert set(ec.block_types(want)) <= {"huf", "treeless"} and got == b"\x00\x50" + want[2:]


def chunk_text(n):
    ids = illumina_ids(n // 30)
    assert len(ids) >= n
    return ids[:n]


def check_chunk_border(lib):
    """64 blocks + 1 byte: the second chunk is one raw block of one byte; no block refers in front of itself (read_frame
    checks every distance) and no block of a chunk's start has treeless literals"""
    data = chunk_text(64 * BLOCK + 1)
    got = compress_lz(lib, data)
    three_readers(lib, got, data, "64_blocks_plus_1")
    blocks = read_frame(got, len(data))
    assert len(blocks) == 65 and all(b["kind"] == "seq" for b in blocks[:64]) and blocks[64] == dict(kind="raw", n=1)
    assert blocks[0]["lits"] == "huf" and "treeless" in [b["lits"] for b in blocks[1:64]]
    assert (len(got), hash64(lib, got)) == PINNED["64_blocks_plus_1"], (len(got), hex(hash64(lib, got)))


def check_slabs(lib, monkeypatch):
    """129 blocks: one slab, and three with the slab lowered to 8 MiB: the same bytes; chunks begin with a fresh tree"""
    data = chunk_text(129 * BLOCK)
    one = compress_lz(lib, data)
    monkeypatch.setenv("NAFGPU_ENC_SLAB_MIB", "8")
    lib.c.nafgpu_test_hooks(1)
    try:
        got = compress_lz(lib, data)
    finally:
        lib.c.nafgpu_test_hooks(0)
    assert got == one
    three_readers(lib, got, data, "129_blocks")
    blocks = read_frame(got, len(data))
    assert len(blocks) == 129 and all(b["kind"] == "seq" for b in blocks)
    assert [b["lits"] for b in (blocks[0], blocks[64], blocks[128])] == ["huf"] * 3
    assert (len(got), hash64(lib, got)) == PINNED["129_blocks"], (len(got), hex(hash64(lib, got)))


def ids_section(lib, src, n_records):
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(3, ctypes.byref(opts))
    opts.id, opts.compression_level, opts.device_lz = 1, 0, 1
    p, n, err = ctypes.c_void_p(), ctypes.c_uint64(), _ffi.Error()
    rc = lib.c.nafgpu_encode_device(ctypes.byref(src), ctypes.byref(opts), 0, ctypes.byref(p), ctypes.byref(n), ctypes.byref(err))
    assert rc == _ffi.OK, err.message
    try:
        blob = ctypes.string_at(p, n.value)
    finally:
        lib.c.nafgpu_encode_free(p)
    # (the Length section is written whatever the flags say, so ec.sections does not read an archive of ids alone)
    assert blob[:4] == b"\x01\xF9\xEC\x02" and blob[5] == 0x20
    _, at = ec.read_varint(blob, 7)
    count, at = ec.read_varint(blob, at)
    orig, at = ec.read_varint(blob, at)
    comp, at = ec.read_varint(blob, at)
    assert (count, orig) == (n_records, src.n_ids_bytes)
    return blob[at:at + comp]


def check_device_pointer(lib):
    """a source in device memory at every offset modulo 16: the bytes nafgpu_zstd_compress_lz gives for the same text in host memory"""
    data = srr_ids(12000)                                   # more than one block
    dec, res = ec.device_text(lib, data)
    try:
        for off in range(16):
            part = data[off:]
            src = _ffi.EncodeSource(d_ids=res.d_sequence + off, n_ids_bytes=len(part), d_record_end=res.d_record_end, n_records=part.count(b"\0"))
            assert ids_section(lib, src, part.count(b"\0")) == compress_lz(lib, part), off
    finally:
        dec.close()


# ---------------------------------------------------------------- archives
def generated_records(ids):
    return [Record(id=i.decode(), comment="%d length=151" % k, sequence="ACGTTGCAAC", length=10) for k, i in enumerate(ids.split(b"\0")[:-1])]


def archive_cases():
    dna = dict(id=True, comment=True, sequence=True)
    out = [(name, ec.records_of(blob, **opts), stype, fields) for name, blob, stype, fields, opts in ec.archive_cases()]
    for name, ids in (("srr", srr_ids(3000)), ("illumina", illumina_ids(3000)), ("counted", b"".join(b"read_%d/1\0" % (7 * i) for i in range(3000)))):
        out.append((name, generated_records(ids), "dna", dna))
    return out


def check_archive(lib, name, recs, sequence_type, fields):
    for r in recs:                                   # only what the archive is to hold
        for f in ("id", "comment", "sequence", "quality"):
            if not fields.get(f):
                setattr(r, f, None)
    for level in (0, 3):
        blob = device_lz_archive(lib, recs, sequence_type, level, **fields)
        assert ec.as_tuples(oracle.Decoder(blob)) == ec.as_tuples(recs), (name, level, "oracle")
        dec = Decoder(io.BytesIO(blob), _lib=lib)
        assert ec.as_tuples(list(dec)) == ec.as_tuples(recs), (name, level, "Decoder")
        dec.close()
        # the records in HBM: the archive decoded in bulk
        dec = Decoder(io.BytesIO(blob), _lib=lib)
        res = dec.decode_all_device()
        assert encode_device(res, sequence_type=sequence_type, compression_level=level, device=0, device_lz=True, _lib=lib, **fields) == blob, \
            (name, level, "encode_device")
        dec.close()
        for payload in ec.sections(blob).values():
            assert payload[1][:2] in (b"\x00\x50", b"\x00\x48")
    for level in (1, 2):                             # the flag changes nothing there
        assert device_lz_archive(lib, recs, sequence_type, level, **fields) == ec.host_archive(lib, recs, sequence_type, level, device=0, **fields)
    # without a device call the host encoder ignores the flag
    assert device_lz_archive(lib, recs, sequence_type, 0, device=None, **fields) == ec.host_archive(lib, recs, sequence_type, 0, **fields)


def device_lz_archive(lib, records, sequence_type, level, device=0, **fields):
    buf = io.BytesIO()
    with Encoder(buf, sequence_type, compression_level=level, device=device, device_lz=True, _lib=lib, **fields) as enc:
        for r in records:
            enc.write(r)
    return buf.getvalue()


def check_text_archive(lib, name):
    """the fixture's text through encode_text(device_lz=True): the archive Encoder(device=0, device_lz=True) writes for its records"""
    file_, stype, mask, n_rec, longest = tc.FIXTURES[name]
    text = tc.fixture_text(name)
    fastq, want, _ = tc.parse(text)
    fields = tc.fields_for(fastq)
    for level in (0, 3):
        got = encode_text(text, sequence_type=stype, mask=mask, compression_level=level, keep_line_length=False, device=0, device_lz=True, _lib=lib)
        assert got == device_lz_archive(lib, tc.as_records(want), stype, level, mask=mask, **fields), (name, level)
        read = [((r.id or "").encode("latin-1"), (r.comment or "").encode("latin-1"), (r.sequence or "").encode("latin-1"),
                 r.quality.encode("latin-1") if fastq else None) for r in oracle.Decoder(got, spec_mask=True)]
        assert read == want, (name, level, "oracle")
        kept = encode_text(text, sequence_type=stype, mask=mask, compression_level=level, device=0, device_lz=True, _lib=lib)
        assert kept == tc.with_line_length(got, longest), (name, level, "keep_line_length")
        dec = Decoder(io.BytesIO(kept), spec_mask=True, _lib=lib)      # text -> archive -> text
        try:
            assert dec.to_text() == text + (b"" if text.endswith(b"\n") else b"\n"), (name, level, "Decoder")
        finally:
            dec.close()


def check_refused_without_the_flag(lib):
    """device_lz = 0: levels 0 and 3 are refused by the three device calls, as before"""
    import pytest
    for level in (0, 3):
        with pytest.raises(ValueError):
            Encoder(io.BytesIO(), "dna", sequence=True, compression_level=level, device=0, _lib=lib)
        with pytest.raises(ValueError):
            encode_text(b">a\nACGT\n", compression_level=level, device=0, _lib=lib)
        dec, res = ec.device_text(lib, b"ACGT" * 100)
        try:
            with pytest.raises(ValueError):
                encode_device(res, sequence_type="text", sequence=True, compression_level=level, device=0, _lib=lib)
            encode_device(res, sequence_type="text", sequence=True, compression_level=level, device=0, device_lz=True, _lib=lib)
        finally:
            dec.close()
        Encoder(io.BytesIO(), "dna", sequence=True, compression_level=level, device=0, device_lz=True, _lib=lib).close()
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(0, ctypes.byref(opts))
    assert opts.device_lz == 0 and ctypes.sizeof(opts) == 16
    lib.c.nafgpu_encoder_opts_from_flags(0, 0x3F, ctypes.byref(opts))
    assert opts.device_lz == 0


# name: (bytes of the frame, its hash64), taken on the CPU harness
PINNED = {
    "empty": (5, 0x7010a21b7fc17617),
    "63_bytes": (68, 0x37307ebf47a1e6fb),
    "64_bytes": (13, 0x75270c862861f73d),
    "65_bytes": (13, 0xaee9ea3102ac859f),
    "block_minus_1": (49540, 0xb789f24b8d362794),
    "block": (49541, 0xb41b4bc4ebfc22c9),
    "block_plus_1": (49545, 0x52e0b816b4804c96),
    "period_1": (6, 0x33cd623a888a5fd8),
    "period_2": (14, 0xa4dca6350a2d80e7),
    "period_3": (15, 0x133076f4920ff004),
    "period_5": (17, 0x56ee40d6ecec9603),
    "period_7": (19, 0x2778c58e3c593665),
    "period_40": (54, 0xb243245fae5706c4),
    "period_1023": (1040, 0xb778d9524f14305b),
    "period_1024": (1040, 0x3d77868465d6a84f),
    "period_1025": (1041, 0x2b6ad13bb31448d3),
    "period_4095": (4111, 0x8a3646b150c9b778),
    "period_70000": (70037, 0xf981bf444dddc1f4),
    "one_value_block": (6, 0x0a9b4a1cc3ccf73c),
    "one_value_3_blocks": (22, 0x7c47bd4698d0346c),
    "source_ends_at_tile_border": (1088, 0x48c5ff25b2bf3831),
    "copy_across_block_border": (131160, 0x11270259b82ed82c),
    "match_cut_at_block_end": (131201, 0xaecd2e8120d6f72d),
    "ml_5": (89, 0xc0b7a1dfb33e13fa),
    "ml_6": (86, 0x3961476cd1a6efcb),
    "ml_34": (86, 0xe9ec47066542896f),
    "ml_35": (86, 0x3277c9e2fef4826b),
    "ml_36": (86, 0xe222a8cdc1703ea4),
    "ml_37": (86, 0xbe8fc9b191d07705),
    "ml_66": (86, 0x972b6a52b0e289a2),
    "ml_67": (86, 0x1a459081778abcf1),
    "ml_130": (87, 0x8c12d8b887e651fe),
    "ml_131": (87, 0x4bb643434d9f111e),
    "ml_255": (87, 0x2ba3a7ad58f6877e),
    "ml_256": (87, 0xd1653e8901efd765),
    "ml_257": (87, 0xfdde249350345afd),
    "ml_258": (87, 0x4498083be4da9be9),
    "ml_259": (87, 0xbb1a811b7935caa5),
    "ml_514": (87, 0xa88ef533a0bf470e),
    "ml_515": (87, 0x24ee612a59cafbcb),
    "ml_65538": (89, 0xe8e26115396cbe64),
    "ml_65539": (89, 0xa0a12178197ca625),
    "ll_15": (67, 0x6ad32d927e22f6be),
    "ll_16": (68, 0xd92541f76d8832b9),
    "ll_17": (69, 0xf4e9500754ecd640),
    "ll_18": (70, 0xf2ed7b2b0a0f193f),
    "ll_23": (75, 0x6ff6a2f4432b179f),
    "ll_24": (76, 0x81131000dd9758ad),
    "ll_63": (115, 0xf639fa2f30be5292),
    "ll_64": (117, 0x83468bd23579fa91),
    "ll_65535": (65590, 0x9337f95f6190a61c),
    "ll_65536": (65591, 0x7564e44dea5e23de),
    "dist_4": (16, 0xde5100ad4d22e05f),
    "dist_5": (17, 0x16c70b3005e6a04a),
    "dist_12": (24, 0x9b9da36e9e49f8f2),
    "dist_13": (25, 0x3e8e9b6864795a5f),
    "dist_28": (40, 0x56d2471b8dea11f0),
    "dist_29": (41, 0x677b317ae9c4592e),
    "dist_60": (106, 0xa19e137d571bb02e),
    "dist_61": (106, 0xbb85225e8c3a7aed),
    "dist_124": (107, 0xa6bd23c1c12d18f7),
    "dist_125": (107, 0x38e9b85f50f44544),
    "dist_252": (107, 0xb73abbca1367632c),
    "dist_253": (107, 0x7ecb5114880f1b71),
    "dist_508": (107, 0x1541bcd42e40d5ab),
    "dist_509": (108, 0xd73d84b9c8828edf),
    "dist_1020": (108, 0x3b5389e2f869d87b),
    "dist_1021": (108, 0x4a41e3e26a27ad52),
    "dist_2044": (108, 0xf85e244fffc977d5),
    "dist_2045": (108, 0xa0d1f41144bd7677),
    "dist_4092": (108, 0xc84b1926d207e345),
    "dist_4093": (108, 0xff4afc63d1408607),
    "dist_8188": (108, 0x012b50aa9b37f1f6),
    "dist_8189": (109, 0x59513f6af9002d81),
    "dist_16380": (109, 0xa588736a49779629),
    "dist_16381": (109, 0xaba196b569ce2bc9),
    "dist_32764": (109, 0x2defa1db333ae2f2),
    "dist_32765": (109, 0xa55d59e397d12b11),
    "dist_65532": (109, 0xf16415bd22fcce1b),
    "dist_65533": (109, 0x5188ea3de768c083),
    "127_sequences": (7218, 0x756f8a5e0fd9d218),
    "128_sequences": (7276, 0xbdc500cbca5e56ef),
    "ends_in_a_match": (113, 0x83e416a00b24545a),
    "literals_255": (187, 0x508a769b615e5f4f),
    "literals_256": (155, 0xaf4496f6b804cb2d),
    "literals_1023": (388, 0xc83f6c0ed1b6492e),
    "literals_1024": (390, 0xd8f7ac6d8b5e77d1),
    "literals_16383": (5763, 0xe09949b82256e5a7),
    "literals_16384": (5765, 0x60e85faf81a6e6e0),
    "srr_ids": (795970, 0xbbf33bdf93378a12),
    "illumina_ids": (1412219, 0x95f60103dad50b84),
    "phix_ids": (189, 0x2c7499edffb7feb8),
    "phix_quality": (2841, 0x5968d91653321edf),
    "64_blocks_plus_1": (1540491, 0x09f337d29922a513),
    "129_blocks": (3105125, 0xcfe05fce1717dcf5),
}
