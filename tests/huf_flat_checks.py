"""Checks of k_huf_flat (nafcodec_amd/csrc/huf_flat.hip: Huffman streams whose tree has 2^L symbols, all codes L bits),
shared by tests/test_huf_flat_emu.py (CPU harness) and tests/test_gpu_huf_flat.py (MI355X).

Every frame is hand-built with tests/zstd_craft.py (`weights_for_depths` with 2^L symbols at depth L) and every result is
compared with what the CPU oracle decodes (and with the writer's own model of the frame).  Integer work: no tolerance.

Sections of a few streams are otherwise cut into parts (zplan.cpp: g_split_target), and streams in parts stay on
k_huf_decode: the checks run after nafgpu_test_hooks(1) with NAFGPU_HUF_SPLIT=0, so that the small frames here reach the
kernel they are about (`hooks`).  NAFGPU_HUF_FLAT=0 sends the same frames through k_huf_decode."""
import contextlib
import os

import numpy as np

import cases
import naf_writer as nw
import zstd_craft as zc
import zstd_ref

SIZES_ONE = (1, 2, 7, 63, 64, 65)                 # literal counts of a single stream (Size_Format 0: below 1 024)
SIZES_FOUR = (4095, 4096, 4097, 128 << 10)        # ... of four streams; the last: one full block
FRONTS = (0, 1, 3, 15, 17, 63)                    # bytes of a raw block in front: the first piece starts at every kind of offset


@contextlib.contextmanager
def hooks(lib, **env):
    """NAFGPU_* switches for the calls inside (test hooks on, the variables set; both undone afterwards)"""
    env = dict({"NAFGPU_HUF_SPLIT": "0"}, **env)
    old = {k: os.environ.get(k) for k in env}
    lib.c.nafgpu_test_hooks(1)
    os.environ.update(env)
    try:
        yield
    finally:
        lib.c.nafgpu_test_hooks(0)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def flat_weights(syms):
    """the flat tree over `syms` (2^L byte values): every code L bits"""
    L = len(syms).bit_length() - 1
    assert len(syms) == 1 << L and 1 <= L <= 8
    return zc.weights_for_depths({s: L for s in syms})


def pick_syms(rng, L, lo=0, hi=256):
    return sorted(int(s) for s in rng.choice(np.arange(lo, hi), 1 << L, replace=False))


def describe_all_ones(weights, form):
    """Huffman_Tree_Description of 256 symbols of weight 1 (L = 8), which zstd_craft.huf_describe cannot write: with one
    weight value its FSE table reads no bits in any state.  Here weight 0 gets the "less than one" probability, so that one
    state of weight 1 reads a bit and the stream can end."""
    listed = weights[:255]
    assert len(weights) == 256 and set(weights) == {1}
    al, norm = 6, [-1, 63]
    enc = zc.FseEncoder(norm, al)
    n = len(listed)
    states, ups = [None] * n, [None] * n
    for i in range(n - 1, -1, -1):
        if i + 2 < n:
            states[i], v, nb = enc.step(1, states[i + 2])
            ups[i] = (v, nb)
        else:
            states[i] = [u for u, nb, _ in enc.by_sym[1] if i == n - 1 or nb > 0][0]
    bw = zc.BackwardBits()
    bw.put(states[0], al)
    bw.put(states[1], al)
    for i in range(n - 2):
        bw.put(*ups[i])
    body = zc.fse_describe(norm, al) + bw.bytes()
    assert len(body) < 128
    return bytes([len(body)]) + body


@contextlib.contextmanager
def patched(name, fn):
    old = getattr(zc, name)
    setattr(zc, name, fn)
    try:
        yield
    finally:
        setattr(zc, name, old)


def add_flat(frame, data, syms, streams, seqs=(), tables=None):
    """one compressed block whose literals `data` are coded with the flat tree over `syms`"""
    w = flat_weights(syms)
    lit = zc.Lit("huf", weights=w, form="direct" if max(syms) <= 128 else "fse", streams=streams)
    if len(syms) == 256:
        with patched("huf_describe", describe_all_ones):
            frame.compressed(data, seqs, lit=lit, tables=tables)
    else:
        frame.compressed(data, seqs, lit=lit, tables=tables)


def rand_of(rng, syms, n):
    return bytes(np.asarray(syms, dtype=np.uint8)[rng.integers(0, len(syms), n)])


def skew_weights(first=0x41):
    """a tree that is not flat: depths 1, 2, 3, 3"""
    return zc.weights_for_depths({first: 1, first + 1: 2, first + 2: 3, first + 3: 3})


def oracle_bytes(p, cap):
    from oracle import oracle
    return oracle.zstd_decode(p, cap)


def decode_ok(lib, frame, what):
    """the frame through nafgpu_zstd_decompress: the writer's model, the oracle and the product agree"""
    p, exp, _ = frame.payload()
    assert oracle_bytes(p, len(exp)) == exp, what + " (oracle)"
    got = lib.zstd_decompress(p, len(exp))
    assert got == exp, what
    return p, exp


# ---------------------------------------------------------------------------------------------- frames


def length_frames():
    """(name, Frame) for L = 1 .. 8 with one stream and with four"""
    rng = np.random.default_rng(0xF1A7)
    out = []
    for L in range(1, 9):
        syms = pick_syms(rng, L)
        for streams, n in ((1, 777), (4, 4097)):
            f = zc.Frame(window_log=17)
            add_flat(f, rand_of(rng, syms, n), syms, streams)
            out.append(("L%d_%dstream" % (L, streams), f))
    return out


def size_frames():
    """literal counts around a piece and a tile, one full block; L = 1 and 3 put the end mark at every bit of the last byte"""
    rng = np.random.default_rng(0x512E)
    out = []
    for L in (1, 3, 4, 8):
        syms = pick_syms(rng, L)
        for n in SIZES_ONE + tuple(range(8, 17)) + SIZES_FOUR:
            streams = 1 if n < 1024 else 4
            if L == 8 and n == 128 << 10:
                n = 120_000                                       # (8-bit codes save nothing: a full block would exceed the block maximum)
            f = zc.Frame(window_log=18)
            add_flat(f, rand_of(rng, syms, n), syms, streams)
            out.append(("L%d_n%d" % (L, n), f))
    return out


def mixing_frames():
    rng = np.random.default_rng(0x3A1)
    out = []
    syms = pick_syms(rng, 4)
    f = zc.Frame(window_log=17)                                   # a treeless block repeating a flat tree
    add_flat(f, rand_of(rng, syms, 3001), syms, 4)
    f.compressed(rand_of(rng, syms, 2999), lit=zc.Lit("treeless", streams=4))
    f.compressed(rand_of(rng, syms, 333), lit=zc.Lit("treeless", streams=1))
    out.append(("treeless_repeat", f))
    f = zc.Frame(window_log=17)                                   # a flat block, then one that is not: two classes
    add_flat(f, rand_of(rng, syms, 2001), syms, 4)
    f.compressed(rand_of(rng, range(0x41, 0x45), 1500), lit=zc.Lit("huf", weights=skew_weights(), streams=4))
    add_flat(f, rand_of(rng, syms, 500), syms, 1)
    out.append(("flat_then_skewed", f))
    f = zc.Frame(window_log=17)                                   # two flat trees (of two lengths) in one task
    other = pick_syms(rng, 6)
    add_flat(f, rand_of(rng, syms, 1999), syms, 4)
    add_flat(f, rand_of(rng, other, 2500), other, 4)
    add_flat(f, rand_of(rng, syms, 100), syms, 1)
    out.append(("two_flat_trees", f))
    return out


def seq_list(n):
    return [(3 + k % 5, 4 + k % 11, 3 + 200 + k % 90 if k % 4 else 1 + k % 3) for k in range(n)]


def lz_frames():
    """flat literals in blocks with sequences: many (literal buffer, stays flat) and a few (SEG: stays on k_huf_decode)"""
    rng = np.random.default_rng(0x175)
    syms = pick_syms(rng, 4)
    out = []
    for name, n_seq in (("literal_buffer", 300), ("few_sequences", 40)):
        seqs = seq_list(n_seq)
        f = zc.Frame(window_log=17)
        add_flat(f, rand_of(rng, syms, 3000), syms, 4)            # (something to match against)
        add_flat(f, rand_of(rng, syms, 2500), syms, 4, seqs, zc.auto_tables(seqs))
        add_flat(f, rand_of(rng, syms, 900), syms, 1 if n_seq == 40 else 4, seqs[:n_seq // 2], zc.auto_tables(seqs[:n_seq // 2]))
        out.append((name, f))
    return out


def broken_streams():
    """(name, payload): a flat stream one byte too long, one byte too short, and with a zero last byte"""
    rng = np.random.default_rng(0xBAD)
    syms = pick_syms(rng, 4)
    out = []
    for name, mend in (("one_byte_too_long", lambda s: b"\x00" + s), ("one_byte_too_short", lambda s: s[1:]),
                       ("zero_last_byte", lambda s: s + b"\x00")):
        for streams, n in ((1, 500), (4, 4097)):
            plain = zc.huf_stream
            calls = []

            def stream(data, codes):
                calls.append(1)
                s = plain(data, codes)
                return mend(s) if len(calls) == streams else s    # (the last stream of the block)
            f = zc.Frame(window_log=17)
            with patched("huf_stream", stream):
                add_flat(f, rand_of(rng, syms, n), syms, streams)
            out.append(("%s_%d" % (name, streams), f.payload()[0]))
    return out


# ---------------------------------------------------------------------------------------------- archives


def archive(payload, n, kind, lens, quality=None):
    """A NAF archive around a ready-made Sequence payload.  kind dna / rna: `n` bases (4-bit pairs, an odd count leaves
    the last byte's high half unused); text: n characters.  quality: (payload, decoded length)."""
    words = nw.length_words(lens)
    head = bytes([1, 0xF9, 0xEC, 2, {"dna": 0, "rna": 1, "text": 3}[kind]])
    flags = 0x0A | (0x01 if quality is not None else 0)
    secs = [(len(words), zstd_ref.compress_magicless(words, 1, True)), (n, payload)]
    if quality is not None:
        secs.append((quality[1], quality[0]))
    blob = bytearray(head) + bytes([flags, 0x20]) + nw.varint(60) + nw.varint(len(lens))
    for orig, data in secs:
        blob += nw.varint(orig) + nw.varint(len(data)) + data
    return bytes(blob)


def front_archives():
    """(name, archive): a raw block of FRONTS bytes in front of flat blocks, as the Sequence section of a DNA archive (an odd
    base count) and of an RNA one, and as the Sequence and Quality sections of reads (plain bytes)"""
    rng = np.random.default_rng(0xA11)
    out = []
    for front in FRONTS:
        syms = pick_syms(rng, 4)
        f = zc.Frame(window_log=17)
        if front:
            f.raw(bytes(rng.integers(0, 256, front, dtype=np.uint8)))
        add_flat(f, rand_of(rng, syms, 2777), syms, 4)
        add_flat(f, rand_of(rng, syms, 301), syms, 1)
        p, exp, _ = f.payload()
        n = 2 * len(exp) - 1
        out.append(("dna_front%d" % front, archive(p, n, "dna", [n // 3, 0, n - n // 3])))
        out.append(("rna_front%d" % front, archive(p, n, "rna", [n])))
        letters = pick_syms(rng, 4, 0x41, 0x5B)
        f = zc.Frame(window_log=17)
        if front:
            f.raw(rand_of(rng, letters, front))
        add_flat(f, rand_of(rng, letters, 2777), letters, 4)
        add_flat(f, rand_of(rng, letters, 301), letters, 1)
        p, exp, _ = f.payload()
        n = len(exp)
        lens = [151] * (n // 151) + [n % 151]
        out.append(("reads_front%d" % front, archive(p, n, "text", lens, quality=(p, n))))
    return out


# ---------------------------------------------------------------------------------------------- the checks


def check_lengths(lib):
    with hooks(lib):
        for name, f in length_frames():
            decode_ok(lib, f, name)


def check_sizes(lib):
    with hooks(lib):
        for name, f in size_frames():
            decode_ok(lib, f, name)


def check_mixing(lib):
    with hooks(lib):
        for name, f in mixing_frames() + lz_frames():
            decode_ok(lib, f, name)


def check_fronts(lib):
    with hooks(lib):
        for name, blob in front_archives():
            got, want = cases.run_product(blob, {}, lib), cases.run_oracle(blob, {})
            assert want[1] is None and want[0], name + " (oracle)"
            assert got == want, name
    rna = cases.run_oracle(front_archives()[1][1], {})[0]
    assert "U" in rna[0][2] and "T" not in rna[0][2]


def check_switch_off(lib):
    """NAFGPU_HUF_FLAT=0: the same frames through k_huf_decode, the same bytes"""
    with hooks(lib, NAFGPU_HUF_FLAT="0"):
        for name, f in length_frames()[::3] + mixing_frames() + lz_frames():
            decode_ok(lib, f, name + " (switch off)")


def check_refusals(lib):
    from oracle import oracle
    from nafcodec_amd import _ffi
    for flat in ("1", "0"):
        with hooks(lib, NAFGPU_HUF_FLAT=flat):
            for name, p in broken_streams():
                try:
                    oracle.zstd_decode(p, 1 << 16)
                    raise AssertionError(name + ": the oracle decodes it")
                except oracle.OracleError as e:
                    assert e.kind == -2, (name, e.kind)
                try:
                    lib.zstd_decompress(p, 1 << 16)
                    raise AssertionError(name + ": decoded")
                except _ffi.NafError as e:
                    assert e.status == _ffi.E_IO and e.io_kind == _ffi.IO_INVALID_DATA, (name, flat, e.status, e.io_kind)


def check_synthetic(lib, n_bases=8_000_000):
    """a synthetic archive (every block's tree is the complete 4-bit tree) with the switch on and off: the same hash64 of
    the bases -- the writer's own -- and of the record table"""
    import ctypes
    import io
    from nafcodec_amd.decoder import Decoder
    arc = lib.synth(n_bases, seed=11, with_mask=True)
    try:
        blob = ctypes.string_at(arc.bytes, arc.n)
        seen = []
        for flat in ("1", "0"):
            with hooks(lib, NAFGPU_HUF_FLAT=flat, NAFGPU_HUF_SPLIT=""):
                dec = Decoder(io.BytesIO(blob), _lib=lib)
                res = dec.decode_all_device()
                assert res.n_bases == arc.n_bases and res.n_records == arc.n_records
                seen.append((dec.hash_device(res.d_sequence, res.n_bases), dec.hash_device(res.d_record_end, 8 * res.n_records)))
        assert seen[0] == seen[1] and seen[0][0] == arc.seq_hash, seen
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))


def write_plan_inputs(folder):
    """files for tests/huf_flat_asan_main.cpp: NAME.zst (payload) and NAME.bin (what it decodes to); -> its arguments"""
    args = []
    for name, f in length_frames() + mixing_frames() + lz_frames() + size_frames()[::5]:
        p, exp, _ = f.payload()
        with open(os.path.join(folder, name + ".zst"), "wb") as fh:
            fh.write(p)
        with open(os.path.join(folder, name + ".bin"), "wb") as fh:
            fh.write(exp)
        kind = {"flat_then_skewed": "mixed", "few_sequences": "mixed"}.get(name, "flat")
        args.append("%s:%s" % (kind, os.path.join(folder, name)))
    for name, p in broken_streams():
        with open(os.path.join(folder, name + ".zst"), "wb") as fh:
            fh.write(p)
        args.append("refuse:%s" % os.path.join(folder, name))
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for fname in ("phix.naf", "masked.naf", "CP040672.naf", "NZ_AAEN01000029.naf", "LuxC.naf"):
        args.append("fixture:%s" % os.path.join(golden, fname))
    return args
