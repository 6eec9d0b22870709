"""Checks of k_huf_flat's work unit (nafcodec_amd/csrc/huf_flat.hip), shared by tests/test_huf_flat_units_emu.py (CPU
harness) and tests/test_gpu_huf_flat_units.py (MI355X): the shapes at which the rounds of a workgroup, the order of the
units in a class and a refusal among many units can go wrong.  tests/huf_flat_checks.py has the helpers and the basic cases.

A workgroup of LANES lanes decodes one stream in rounds of R = LANES x IN_FLIGHT aligned 16-byte pieces of the destination
(`geometry`; tests/test_huf_flat_units_emu.py holds the constants against the source).  Every frame is hand-built with
tests/zstd_craft.py, decoded by the CPU oracle first (a mistake of the writer shows as one) and then by the product, whose
bytes must equal the oracle's.  Integer work: no tolerance.  All of it runs under `hooks` (NAFGPU_HUF_SPLIT=0), so that the
small frames reach the kernel.

What the format leaves out.  A stream holds at most 32 768 literals (a four-stream literal section of a block of
Block_Maximum_Size; one stream alone holds fewer than 1 024; with 8-bit codes the compressed block must fit that size too,
which leaves 32 000), that is 4 096 pieces of ASCII and 2 048 of bytes.  Of the
whole-piece counts 1, R - 1, R, R + 1, 2R - 1, 2R, 2R + 1 those above that are not streams zstd can hold:
`round_cases` lists every combination, `infeasible` says which of them the format rules out, and the check asserts that
nothing else is left out."""
import numpy as np

import cases
import huf_flat_checks as hk
import zstd_craft as zc

LANES = 256                                        # huf_flat.hip: kFlatThreads
IN_FLIGHT = {"ascii": 8, "bytes": 4}               # huf_flat.hip: kFlatUnrollAscii, kFlatUnrollBytes


def stream_max(L):
    """literals of one stream at most (see above); a block of 8-bit codes saves nothing, and its tree and headers must fit
    Block_Maximum_Size beside the literals"""
    return 32768 if L < 8 else 32000

LENGTHS = (1, 3, 4, 5, 8)
MISALIGN = {"ascii": (0, 2, 14), "bytes": (0, 1, 15)}


def geometry(mode):
    """-> (output bytes per literal, literals per piece, pieces per round)"""
    out_b = 2 if mode == "ascii" else 1
    return out_b, 16 // out_b, LANES * IN_FLIGHT[mode]


_PLAIN_STREAM = zc.huf_stream


def fast_huf_stream(data, codes):
    """zstd_craft.huf_stream for codes of one length, without its quadratic big-integer shifts: literal j of n lies at bits
    [(n - 1 - j) L, (n - j) L), the end mark above them (check_fast_writer holds it against the plain one)"""
    L = codes[data[0]][1] if data else 0
    if not data or any(codes[b][1] != L for b in set(data)):
        return _PLAIN_STREAM(data, codes)
    table = np.zeros(256, dtype=np.uint32)
    for b in set(data):
        table[b] = codes[b][0]
    vals = table[np.frombuffer(bytes(data), dtype=np.uint8)][::-1]
    bits = ((vals[:, None] >> np.arange(L, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)
    bits = np.concatenate([bits, np.ones(1, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def fast_writer():
    return hk.patched("huf_stream", fast_huf_stream)


def check_fast_writer():
    rng = np.random.default_rng(0xFA57)
    for L in range(1, 9):
        syms = hk.pick_syms(rng, L)
        codes, _ = zc.huf_codes(hk.flat_weights(syms))
        for n in (1, 2, 7, 8, 9, 333):
            data = hk.rand_of(rng, syms, n)
            with fast_writer():
                fast = zc.huf_stream(data, codes)
            assert fast == _PLAIN_STREAM(data, codes), (L, n)


# ---------------------------------------------------------------------------------------------- round boundaries


def whole_pieces(mode, h, n):
    """the kernel's count of whole pieces of a stream of n literals whose first output byte lies h bytes into a piece"""
    out_b, _, _ = geometry(mode)
    end = h + n * out_b
    return (end >> 4) - (1 if h else 0)


def stream_literals(mode, L, h, count):
    """literals of a stream with `count` whole pieces behind a misalignment of h, and a last piece in part where the
    format has room for one; None: no stream of the format has that many"""
    out_b, per_piece, _ = geometry(mode)
    base = ((count + (1 if h else 0)) * 16 - h) // out_b
    for tail in (3, 0):
        if base + tail <= stream_max(L):
            assert whole_pieces(mode, h, base + tail) == count
            return base + tail
    return None


def round_cases():
    """(mode, L, count, h, raw blocks in front) for every mode, L and count; h and the number of raw blocks (which moves
    the stream's first source byte by three bytes each: the four offsets modulo 4) rotate, so that over the counts and
    lengths of a mode every h meets every source offset"""
    out = []
    for mode in ("ascii", "bytes"):
        _, _, R = geometry(mode)
        k = 0
        for L in LENGTHS:
            for count in (1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1):
                out.append((mode, L, count, MISALIGN[mode][k % 3], 1 + k % 4))
                k += 1
    return out


def infeasible(case):
    mode, L, count, h, blocks = case
    return stream_literals(mode, L, h, count) is None


def round_frame(rng, case):
    """-> (Frame, literals per stream): `blocks` raw blocks whose bytes set the misalignment h of stream 0, then one block
    of four streams of equal length, stream 0 with `count` whole pieces (the three behind it start at other offsets)"""
    mode, L, count, h, blocks = case
    out_b, _, _ = geometry(mode)
    n0 = stream_literals(mode, L, h, count)
    front = {("ascii", 0): 8, ("ascii", 2): 9, ("ascii", 14): 7, ("bytes", 0): 16, ("bytes", 1): 17, ("bytes", 15): 15}[mode, h]
    assert (front * out_b) % 16 == h and front >= blocks
    syms = hk.pick_syms(rng, L)
    f = zc.Frame(window_log=18)
    sizes = [1] * (blocks - 1) + [front - (blocks - 1)]
    for size in sizes:
        f.raw(hk.rand_of(rng, syms, size))
    hk.add_flat(f, hk.rand_of(rng, syms, 4 * n0), syms, 4)
    return f, n0


def check_rounds(lib, mode):
    rng = np.random.default_rng(0x20D5)
    todo = [c for c in round_cases() if c[0] == mode]
    left_out = [c for c in todo if infeasible(c)]
    out_b, per_piece, R = geometry(mode)
    for _, L, count, h, _ in left_out:             # only what no stream of the format can hold: the whole pieces and the
        assert count * per_piece + ((16 - h) % 16) // out_b > stream_max(L), (mode, L, count, h)      # literals of a first piece in part
    assert len(left_out) < len(todo) and any(c[2] >= R + 1 for c in todo if not infeasible(c)), "no case beyond one round"
    offsets = set()
    with hk.hooks(lib), fast_writer():
        for case in todo:
            if infeasible(case):
                continue
            f, n0 = round_frame(rng, case)
            name = "%s L%d count %d h %d raw blocks %d" % case
            if mode == "bytes":
                hk.decode_ok(lib, f, name)
            else:
                p, exp, _ = f.payload()
                assert hk.oracle_bytes(p, len(exp)) == exp, name + " (oracle)"
                n = 2 * len(exp) - 1
                blob = hk.archive(p, n, "dna", [n // 3, 0, n - n // 3])
                got, want = cases.run_product(blob, {}, lib), cases.run_oracle(blob, {})
                assert want[1] is None and want[0], name + " (oracle)"
                assert got == want, name
            offsets.add((case[3], case[4] % 4))
    assert len(offsets) == 12, "a misalignment that did not meet every source offset: %s" % sorted(offsets)


# ---------------------------------------------------------------------------------------------- many units

N_BLOCKS = 132                                     # x 4 streams: more than 520 units, more than two tasks of 64 streams
PER_BLOCK = 1200                                   # literals of a block: about 300 per stream


def many_frame(rng, lo, hi, skewed_every=0, mend=None, mend_at=None):
    """N_BLOCKS blocks of four streams, a tree of 3-bit codes (table inline) and one of 6-bit codes (table from the pool)
    alternating; skewed_every: every such block has a tree that is not flat instead (its streams go to k_huf_decode, the
    indices of the flat units then differ from the stream indices); mend / mend_at: the mend_at-th stream written is
    passed through mend (a refusal in the middle)"""
    small, large = hk.pick_syms(rng, 3, lo, hi), hk.pick_syms(rng, 6, lo, hi)
    plain = zc.huf_stream
    calls = []

    def stream(data, codes):
        calls.append(1)
        s = plain(data, codes)
        return mend(s) if mend is not None and len(calls) == mend_at else s
    f = zc.Frame(window_log=18)
    with hk.patched("huf_stream", stream):
        for b in range(N_BLOCKS):
            if skewed_every and b % skewed_every == skewed_every - 1:
                f.compressed(hk.rand_of(rng, range(0x41, 0x45), PER_BLOCK), lit=zc.Lit("huf", weights=hk.skew_weights(), streams=4))
            else:
                syms = large if b & 1 else small
                hk.add_flat(f, hk.rand_of(rng, syms, PER_BLOCK + b % 7), syms, 4)
    return f


def check_many(lib):
    with hk.hooks(lib):
        for skewed_every in (0, 5):
            tag = "many units" + (", a skewed tree every fifth block" if skewed_every else "")
            rng = np.random.default_rng(0x3A9 + skewed_every)
            f = many_frame(rng, 0, 256, skewed_every)
            p, exp = hk.decode_ok(lib, f, tag)
            n = 2 * len(exp) - 1                                               # the Sequence section of a DNA archive
            blob = hk.archive(p, n, "dna", [n // 3, 0, n - n // 3])
            got, want = cases.run_product(blob, {}, lib), cases.run_oracle(blob, {})
            assert want[1] is None and want[0], tag + " (dna, oracle)"
            assert got == want, tag + " (dna)"
            f = many_frame(rng, 0x21, 0x7F, skewed_every)                       # Sequence and Quality of a text archive
            p, exp, _ = f.payload()
            assert hk.oracle_bytes(p, len(exp)) == exp, tag + " (text, oracle)"
            n = len(exp)
            lens = [151] * (n // 151) + [n % 151]
            blob = hk.archive(p, n, "text", lens, quality=(p, n))
            got, want = cases.run_product(blob, {}, lib), cases.run_oracle(blob, {})
            assert want[1] is None and want[0], tag + " (text, oracle)"
            assert got == want, tag + " (text)"


def check_refusal_in_the_middle(lib):
    """one stream in the middle of many one byte too long, one byte too short, or with a zero last byte: refused with the
    same status and io_kind with the switch on and off, as the oracle refuses it"""
    from oracle import oracle
    from nafcodec_amd import _ffi
    payloads = []
    for name, mend in (("one_byte_too_long", lambda s: b"\x00" + s), ("one_byte_too_short", lambda s: s[1:]),
                       ("zero_last_byte", lambda s: s + b"\x00")):
        for skewed_every in (0, 5):
            rng = np.random.default_rng(0xBAD5)
            f = many_frame(rng, 0, 256, skewed_every, mend, 4 * (N_BLOCKS // 2) + 2)
            payloads.append(("%s skewed_every %d" % (name, skewed_every), f.payload()[0]))
    for name, p in payloads:
        try:
            oracle.zstd_decode(p, 1 << 18)
            raise AssertionError(name + ": the oracle decodes it")
        except oracle.OracleError as e:
            assert e.kind == -2, (name, e.kind)
    seen = {}
    for flat in ("1", "0"):
        with hk.hooks(lib, NAFGPU_HUF_FLAT=flat):
            for name, p in payloads:
                try:
                    lib.zstd_decompress(p, 1 << 18)
                    raise AssertionError(name + ": decoded")
                except _ffi.NafError as e:
                    assert e.status == _ffi.E_IO and e.io_kind == _ffi.IO_INVALID_DATA, (name, flat, e.status, e.io_kind)
                    seen[(name, flat)] = (e.status, e.io_kind)
    for name, _ in payloads:
        assert seen[(name, "1")] == seen[(name, "0")], name
