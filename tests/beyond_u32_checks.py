"""Shared by tests/test_beyond_u32_emu.py (CPU harness, a small boundary) and tests/test_gpu_beyond_u32.py (MI355X, the
boundary 2^32): the device encoder, and the decoder's mask passes, at letter positions on both sides of a boundary `B`.
Not a test module; every function takes the library binding it is to check, `B`, and sizes derived from it.

With B = 2^32 the questions are the 32-bit ones: a position `16 * g + k`, a tile's first letter, a unit's or a record's
length, a section offset that no longer fits a 32-bit word.  With a small B the same code proves the checks themselves (run
arithmetic, re-framing, expected words) where no GPU is needed; a truncation cannot show there.

The yardsticks are not the product: the CPU oracle (oracle/naf_oracle.c with its own zstd decoder), the reference-shaped
pipeline over the system libzstd (oracle/ref_shape.c), the run rule and the length-word rule computed with numpy."""
import ctypes
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cases
import encode_checks as ec
import mask_encode_checks as mc
import naf_writer as nw
import zstd_ref
from conftest import golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device
from oracle import oracle

U64 = np.uint64
SEED = 0x4E4146
_pool = ThreadPoolExecutor(4)


def drain_later(blob, **opts):
    """the oracle's drain of a whole archive on another host core (half a minute for 4.5 Gbases; the library holds no state
    between decoders, and ctypes gives up the interpreter lock for the call) -> a future"""
    oracle.lib()
    return _pool.submit(lambda: oracle.Decoder(blob, **opts).drain())


# ---------------------------------------------------------------- helpers (unit-tested by check_helpers)
def canonical_units(lengths):
    """unit lengths as a writer may have them (zero-length fillers, e.g. the synthetic writer's put_run(0)) -> the units the
    letters' case gives: zero-length units merged away, an unmasked unit of length 0 in front when the text starts masked"""
    lengths = np.asarray(lengths, dtype=U64)
    flag = (np.arange(len(lengths)) & 1).astype(np.uint8)
    keep = lengths > 0
    lengths, flag = lengths[keep], flag[keep]
    if not len(lengths):
        return lengths
    first = np.flatnonzero(np.concatenate(([True], flag[1:] != flag[:-1])))
    merged = np.add.reduceat(lengths, first)
    if flag[0]:
        merged = np.concatenate((np.zeros(1, dtype=U64), merged))
    return merged


def units_of(intervals, n):
    """lower-case intervals [(first, length)], in order, apart from each other and inside [0, n) -> canonical unit lengths"""
    runs, at = [], 0
    for first, length in intervals:
        assert length > 0 and (first > at or (first == 0 and at == 0)), (first, length, at)
        runs += [first - at, length]
        at = first + length
    assert at <= n
    if at < n:
        runs.append(n - at)
    return runs


def hand_made_variants(B, n):
    """(name, record lengths, unit lengths, first lower-case letter).  The runs are canonical (no zero-length unit but a
    leading one), so an encoder that derives the units from the letters' case must write exactly these bytes.
      long_unit            one masked unit longer than B, over the end of the record of B - 1 letters
      edges                short units with edges at B - 1, B, B + 1 and at every offset modulo 16 around B and B +- 4096
                           (mask_encode_checks.hand_made_cases' "edges_mod_16", shifted), in ONE record of n > B letters
      first_lower_past_B   no lower-case letter in front of B + 5 (the first offender of an encoder without mask=True needs
                           the high word of its position), then units of 254, 255, 256, 510, 65536 letters"""
    T, LL = mc.MASK_TILE, mc.LANE_LETTERS
    three = [B - 1, 0, n - (B - 1)]
    out = [("long_unit", three, [1000, B + 12_345, 777, 300, n - (B + 14_422)], 1000)]
    iv = []
    for base in (B - T - LL, B - LL, B + T - LL):
        for k in range(2 * LL + 1):
            iv.append((base + (LL + 1) * k, 1 + k % 3))
        assert {(base + (LL + 1) * k) % 16 for k in range(2 * LL + 1)} == set(range(16))
    iv.append((B - 1, 1))                                        # edges at B - 1 and at B; the run at B + 1 is one of the above
    iv.sort()
    assert (B + 1, 2) in iv
    out.append(("edges", [n], units_of(iv, n), iv[0][0]))
    iv = [(B + 5 + (LL + 1) * k, 1 + k % 3) for k in range(2 * LL + 1)]
    at = B + 2 * T
    for l in (254, 255, 256, 510, 65536):
        iv.append((at, l))
        at += l + 255
    assert at + 4096 < n
    out.append(("first_lower_past_B", three, units_of(iv, n), B + 5))
    for name, lens, runs, first in out:
        assert sum(lens) == sum(runs) == n and all(r > 0 for r in runs[1:]) and runs[0] == first, name
    return out


def check_helpers():
    """the expected bytes are computed by these at every B: proven here on the real numbers"""
    F = 0xFFFFFFFF
    w = lambda *v: b"".join(x.to_bytes(4, "little") for x in v)
    assert nw.length_words([F, 0, 200_000_004]) == w(F, 0, 0, 200_000_004)         # exactly 2^32 - 1: FFFFFFFF 00000000
    assert nw.length_words([2**32 + 200_000_003]) == w(F, 200_000_004)
    assert nw.length_words([F - 1, 2 * F + 1]) == w(F - 1, F, F, 1)
    rng = np.random.default_rng(2)
    for _ in range(20):
        runs = [int(x) for x in rng.choice([0, 1, 254, 255, 256, 509, 510, 511, 70_000], int(rng.integers(1, 12)))]
        assert cases.mask_section_bytes(runs) == nw.mask_bytes(runs), runs
        ends = cases.mask_unit_ends(nw.mask_bytes(runs))
        assert ends.tolist() == np.cumsum(runs).tolist()
        text = b"".join((b"a" if k & 1 else b"C") * r for k, r in enumerate(runs))
        canon = canonical_units(runs)
        assert cases.mask_section_bytes(canon) == mc.mask_bytes(text), runs
        if sum(runs) > 3:                                         # the window cut: any window reads as the text's own slice
            a, b = sorted(int(x) for x in rng.choice(sum(runs) + 1, 2, replace=False))
            cut = cases.cut_units(ends, a, b)
            assert cases.mask_section_bytes(canonical_units(cut)) == mc.mask_bytes(text[a:b]), (runs, a, b)
    big = cases.mask_section_bytes([1000, 2**32 + 12_345, 7])
    assert len(big) == 3 + 1 + (2**32 + 12_345) // 255 + 1 + 1 and big[4:4 + 16_843_057] == b"\xff" * 16_843_057
    assert big[-2:] == bytes([(2**32 + 12_345) % 255, 7])
    assert cases.raw_frame(b"") == b"\x00\x48\x01\x00\x00"
    for n in (1, 131072, 131073, 300_000):
        data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert oracle.zstd_decode(cases.raw_frame(data), n + 8) == data
    for B in (2**20, 2**32):
        for name, lens, runs, first in hand_made_variants(B, B + 300_003):
            low = np.cumsum(runs)[0::2]                           # where the masked units begin
            assert int(low[0]) == first
            if name == "edges":
                edges = set(np.cumsum(runs).tolist())
                assert {B - 1, B, B + 1} <= edges
            if name == "first_lower_past_B" and B == 2**32:
                assert first == 4294967301


def rehead(frame, n, lens, runs=None):
    """a v1 DNA archive around a ready-made Sequence frame of n letters: record lengths `lens`, Mask units `runs`; the small
    sections in raw blocks, so that nothing here goes through a compressor"""
    words = nw.length_words(lens)
    head = bytearray([1, 0xF9, 0xEC, 1, 0x0A | (0x04 if runs is not None else 0), 0x20]) + nw.varint(60) + nw.varint(len(lens))
    for data in (words,) + ((cases.mask_section_bytes(runs),) if runs is not None else ()):
        fr = cases.raw_frame(data)
        head += nw.varint(len(data)) + nw.varint(len(fr)) + fr
    head += nw.varint(n) + nw.varint(len(frame))
    return bytes(head) + bytes(frame)


def synth_blob(lib, n, with_mask, seed=SEED):
    """-> (archive bytes, the writer's seq_hash, offsets_hash, n_records)"""
    arc = lib.synth(n, seed=seed, with_mask=with_mask, iupac_permille=3)
    try:
        assert arc.n_bases == n
        return ctypes.string_at(arc.bytes, arc.n), arc.seq_hash, arc.offsets_hash, arc.n_records
    finally:
        lib.c.nafgpu_synth_free(ctypes.byref(arc))


def section_bytes(blob, spans, name):
    orig, a, b = spans[name]
    got = oracle.zstd_decode(bytes(memoryview(blob)[a:b]), orig + 8)
    assert len(got) == orig, name
    return got


def same(a, b, what):
    for f in ("n_records", "n_bases", "seq_hash", "ends_hash"):
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def device_equals(dec, res, want, what):
    assert (res.n_bases, res.n_records) == (want.n_bases, want.n_records), what
    assert dec.hash_device(res.d_sequence, res.n_bases) == want.seq_hash, (what, "sequence")
    assert dec.hash_device(res.d_record_end, 8 * res.n_records) == want.ends_hash, (what, "record ends")


# ---------------------------------------------------------------- B1, B3: a synthetic archive, device to device
class Synthetic:
    """B + extra letters written by nafgpu_synth_write with a Mask section, decoded in bulk: what B1 and B3 start from"""

    def __init__(self, lib, B, extra):
        self.lib, self.B, self.n = lib, B, B + extra
        assert extra & 1 and self.n & 1                                     # an odd number of letters: a pad nibble
        self.blob, self.seq_hash, self.offsets_hash, self.n_records = synth_blob(lib, self.n, True)
        self.want = oracle.Decoder(self.blob).drain()
        assert (self.want.n_bases, self.want.n_records, self.want.seq_hash, self.want.ends_hash) == \
            (self.n, self.n_records, self.seq_hash, self.offsets_hash)
        self.dec = Decoder(io.BytesIO(self.blob), _lib=lib)
        self.res = self.dec.decode_all_device()
        device_equals(self.dec, self.res, self.want, "the synthetic archive")

    def close(self):
        self.dec.close()


def check_device_to_device(s, redecode=True):
    """B1: decode_all_device -> encode_device(mask=True) -> the oracle's reading of the new archive is its reading of the
    old one (and the writer's checksums), so is the device's (`redecode`; check_hand_made always decodes what it encoded,
    so at full size the second decode is left to it); the Sequence frame's blocks; the Mask section's bytes."""
    lib, res = s.lib, s.res
    again = encode_device(res, sequence_type="dna", sequence=True, id=bool(res.n_ids), compression_level=1, mask=True, device=0, _lib=lib)
    read_again = drain_later(again)
    if redecode:
        dec2 = Decoder(io.BytesIO(again), _lib=lib)
        try:
            device_equals(dec2, dec2.decode_all_device(), s.want, "the re-encoded archive on the device")
        finally:
            dec2.close()
    spans = ec.section_spans(again)
    assert spans["flags"] & 0x04 and spans["n_records"] == s.n_records
    # structure: ceil(packed / 128 Ki) literal-only blocks, and a 64-block chunk (hence a slab) starts without a table to reuse
    orig, a, b = spans["sequence"]
    types_ = ec.block_types(memoryview(again)[a:b])
    packed = (s.n + 1) // 2
    assert orig == s.n and len(types_) == (packed + ec.BLOCK - 1) // ec.BLOCK
    assert not [i for i in range(0, len(types_), 64) if types_[i] == "treeless"] and "treeless" in types_
    # the Mask section: the original's units, zero-length fillers merged away
    units = np.diff(np.concatenate((np.zeros(1, dtype=U64), cases.mask_unit_ends(section_bytes(s.blob, ec.section_spans(s.blob), "mask")))))
    want_mask = cases.mask_section_bytes(canonical_units(units))
    got_mask = section_bytes(again, spans, "mask")
    assert len(got_mask) == len(want_mask) and got_mask == want_mask
    same(read_again.result(), s.want, "the oracle on the re-encoded archive")
    return len(types_)


def check_text_section(s, min_slabs, slab=512 << 20):
    """B3: the same letters in HBM as a TEXT section (one byte per letter: more than `min_slabs` - 1 slabs, at B = 2^32 a
    section offset beyond 2^32), read back by the reference-shaped pipeline over the system libzstd (streaming)."""
    assert s.n > (min_slabs - 1) * slab
    again = encode_device(s.res, sequence_type="text", sequence=True, compression_level=1, device=0, _lib=s.lib)
    spans = ec.section_spans(again)
    assert spans["sequence"][0] == s.n and not spans["flags"] & 0x04
    got = oracle.ref_shape_drain(again)
    same(got, s.want, "libzstd on the text archive")


# ---------------------------------------------------------------- B2: a hand-made record table and mask
def check_hand_made(lib, B, extra, name, frame_of=None):
    """B2: the synthetic letters (no mask of the writer's) under a hand-made record table and Mask section.  First the
    DECODE against the oracle (spec_mask=True: units cross record ends on purpose), then encode_device(mask=True): Length
    words, Mask bytes, the oracle's reading of the new archive, and the refusal without mask=True, which names the first
    lower-case letter."""
    n = B + extra
    _, lens, runs, first_lower = next(v for v in hand_made_variants(B, n) if v[0] == name)
    blob, plain_hash, _, _ = synth_blob(lib, n, False)
    spans = ec.section_spans(blob)
    assert spans["sequence"][0] == n
    blob = rehead(memoryview(blob)[spans["sequence"][1]:spans["sequence"][2]], n, lens, runs)
    read = drain_later(blob, spec_mask=True)
    dec = Decoder(io.BytesIO(blob), spec_mask=True, _lib=lib)
    try:
        res = dec.decode_all_device()
        got = (res.n_bases, res.n_records, dec.hash_device(res.d_sequence, res.n_bases), dec.hash_device(res.d_record_end, 8 * res.n_records))
        again = encode_device(res, sequence_type="dna", sequence=True, compression_level=1, mask=True, device=0, _lib=lib)
        read_again = drain_later(again, spec_mask=True)
        src = _ffi.EncodeSource(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        rc, refused = mc.call_encode_device(lib, src, "dna", mask=0, sequence=True)
        message = mc.call_encode_device.message
    finally:
        dec.close()
    # the decode first: the device against the oracle, the oracle's record ends against the hand-made table
    want = read.result()
    assert (want.n_bases, want.n_records) == (n, len(lens)) and want.seq_hash != plain_hash
    ends = np.cumsum(lens, dtype=U64).tobytes()
    assert want.ends_hash == lib.c.nafgpu_hash64_host(ends, len(ends))
    assert got == (want.n_bases, want.n_records, want.seq_hash, want.ends_hash), (name, "decode", got)
    check_reencoded(again, want, lens, runs, name, read_again.result())
    dec = Decoder(io.BytesIO(again), spec_mask=True, _lib=lib)
    try:
        device_equals(dec, dec.decode_all_device(), want, name + ": the re-encoded archive on the device")
    finally:
        dec.close()
    assert (rc, refused) == (_ffi.E_INVALID_SEQUENCE, None), (name, rc)
    assert "letter %d)" % first_lower in message, (name, first_lower, message)


def check_reencoded(again, want, lens, runs, name, read_again=None):
    """what B2 asks of the archive encode_device wrote (a function of its own, so that it can be handed a wrong archive);
    `read_again`: the oracle's drain of it with spec_mask=True, where the caller has it already"""
    spans = ec.section_spans(again)
    assert spans["n_records"] == len(lens) and spans["flags"] & 0x04, name
    assert section_bytes(again, spans, "lengths") == nw.length_words(lens), (name, "Length words")
    want_mask = cases.mask_section_bytes(runs)
    got_mask = section_bytes(again, spans, "mask")
    assert len(got_mask) == len(want_mask) and got_mask == want_mask, (name, "Mask bytes", len(got_mask), len(want_mask))
    same(read_again or oracle.Decoder(again, spec_mask=True).drain(), want, name + ": the oracle on the re-encoded archive")


# ---------------------------------------------------------------- B2-lz: the same masks over a section with matches
def lz_archive_parts(n, period_div=1):
    """-> (zstd payload, letters): the packed NZ_AAEN01000029 fixture (its first 1 / period_div) tiled until it passes n
    letters, system libzstd level 1, streaming -- the statistics of a real genome: a few far matches per block"""
    code = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate(nw.NUC.encode()):
        code[c] = i
    fixture = "".join(r.sequence.upper() for r in oracle.Decoder(golden_bytes("NZ_AAEN01000029.naf"))).encode()
    nib = code[np.frombuffer(fixture, dtype=np.uint8)]
    one = (nib[0:len(nib) & ~1:2] | (nib[1::2] << 4)).astype(np.uint8)
    one = one[:len(one) // period_div]
    copies = -(-n // (2 * len(one)))
    payload = zstd_ref.compress_magicless(np.tile(one, copies).tobytes(), 1, True)
    return payload, 2 * len(one) * copies


def check_lz_decode(lib, B, extra, names=("long_unit", "edges"), period_div=1):
    """B2-lz (decode only): a Sequence section WITH matches takes the mask through the separate pass (k_mask_apply), not
    through the bit map inside the Huffman kernel.  Both readings: with records [B - 1, 0, rest] the unit longer than B
    crosses a record end beyond B, which is the record-end rule's search and clamp in the default reading.
    -> {(variant, spec_mask): milliseconds of the decode's mask and scan passes}"""
    payload, n = lz_archive_parts(B + extra, period_div)
    assert n >= B + extra
    if n <= 1 << 26:                                             # (the same construction at any size: shown where it is cheap)
        assert oracle.zstd_decode(payload, n // 2 + 8, stats=True)[1].sequences > 0
    times = {}
    for name, lens, runs, _ in hand_made_variants(B, n):
        if name not in names:
            continue
        blob = rehead(payload, n, lens, runs)
        readings = {}
        reads = {spec: drain_later(blob, spec_mask=spec) for spec in (True, False)}
        for spec in (True, False):
            want = reads[spec].result()
            assert (want.n_bases, want.n_records) == (n, len(lens))
            readings[spec] = want.seq_hash
            dec = Decoder(io.BytesIO(blob), spec_mask=spec, _lib=lib)
            try:
                res = dec.decode_all_device()
                device_equals(dec, res, want, "%s, spec_mask=%s" % (name, spec))
                times[(name, spec)] = round(res.ms_other + res.ms_seq_lz, 1)
            finally:
                dec.close()
        # the readings differ exactly where a masked unit reaches a record's end
        touching = cases.masked_runs_touching_record_ends(np.cumsum(runs, dtype=U64), np.cumsum(lens, dtype=U64))[0]
        assert (readings[True] != readings[False]) == (touching > 0), (name, touching)
    return times
