"""Shared by tests/test_screen_emu.py (CPU harness) and tests/test_gpu_screen.py (MI355X): Decoder.kmers / .screen, the same on
Selection and ParsedText, kmers() and screen(): the k-mers of a reference as a set in device memory, and records screened
against it.  Not a test module; every function takes the library binding it is to check.

The yardstick is expected() below: the rules of include/nafgpu.h at nafgpu_kmers_build as a plain Python loop over what the
CPU oracle decodes (or over the source's own bytes read back), with a Python set for the k-mers.  Above LOOP_MAX letters the
same windows come from numpy (section_windows_numpy), which is held against the loop at import and in check_random.  Every
table is compared for equality as struct and integer arrays: integer work, no tolerance, no time asserted."""
import ctypes
import importlib
import io
import os
import threading

import numpy as np

import select_checks as sc
import trim_checks as tk
from conftest import ROOT, golden_bytes
from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device, encode_text, parse_text

scr = importlib.import_module("nafcodec_amd.screen")         # (the module: the package's attribute of that name is its screen())

ENTRY_POINTS = ("nafgpu_kmers_build", "nafgpu_kmers_build_decoder", "nafgpu_kmers_free", "nafgpu_screen", "nafgpu_screen_decoder",
                "nafgpu_screens_copy_to_host", "nafgpu_screens_free")
TILE, LANE, HALO = 4096, 16, 32                              # nafcodec_amd/csrc/screen.h: asserted below
REGION = np.dtype(scr.REGION)
assert REGION.itemsize == ctypes.sizeof(_ffi.Region) == 32
KS = (1, 2, 15, 16, 17, 30, 31)
LOOP_MAX = 300_000                                           # sections up to this many letters go through the plain loop

CODE = [4] * 256                                             # A C G T/U in either case: 0 1 2 3; every other byte: no letter
for _letters, _code in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"TtUu", 3)):
    for _b in _letters:
        CODE[_b] = _code
CODES = np.array(CODE, dtype=np.uint8)
COMPLEMENT = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")


def revcomp(s):
    return bytes(s).translate(COMPLEMENT)[::-1]


def bind(lib):
    for name in ENTRY_POINTS:        # bound unconditionally: a library without the feature fails here, it does not skip
        getattr(lib.c, name)
    return sc.bind(lib)


def kernel_constants():
    with open(os.path.join(ROOT, "nafcodec_amd", "csrc", "screen.h")) as f:
        text = f.read()
    for name, value in (("kScreenTile", TILE), ("kScreenHalo", HALO), ("kScreenMaxK", 31)):
        assert "constexpr uint32_t %s = %d;" % (name, value) in text, name
    assert scr.MAX_K == 31 == max(KS) and HALO >= scr.MAX_K - 1


# ---------------------------------------------------------------- the yardstick
def record_windows(s, k, canonical):
    """one record, rolled: -> [(start, key)] of its windows, ascending"""
    out, f, r, run, mask, top = [], 0, 0, 0, (1 << 2 * k) - 1, 2 * (k - 1)
    for j, b in enumerate(s):
        c = CODE[b]
        if c == 4:
            f = r = run = 0
            continue
        f, r, run = ((f << 2) | c) & mask, (r >> 2) | ((3 - c) << top), run + 1
        if run >= k:
            out.append((j - k + 1, min(f, r) if canonical else f))
    return out


def record_windows_plain(s, k, canonical):
    """the same as the rules are written, a slice per window"""
    out = []
    for i in range(len(s) - k + 1):
        codes = [CODE[b] for b in s[i:i + k]]
        if 4 in codes:
            continue
        f = r = 0
        for c in codes:
            f = f * 4 + c
        for c in reversed(codes):
            r = r * 4 + (3 - c)
        out.append((i, min(f, r) if canonical else f))
    return out


def table_of(letters, ends):
    return [int(e) for e in ends] if ends is not None and len(ends) else [len(letters)]


def section_windows_loop(letters, ends, k, canonical):
    """-> (rec, start, key) int arrays of every window of the section, ascending"""
    rows, lo = [], 0
    for rec, hi in enumerate(table_of(letters, ends)):
        rows.extend((rec, s, key) for s, key in record_windows(letters[lo:hi], k, canonical))
        lo = hi
    a = np.array(rows, dtype=np.uint64).reshape(-1, 3)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2]


def _join(x, a, y, b, m):
    """windows of a letters and of b letters -> the m windows of a + b letters: (forward, reverse complement, holds a non-letter)"""
    return ((x[0][:m] << np.uint64(2 * b)) | y[0][a:a + m], x[1][:m] | (y[1][a:a + m] << np.uint64(2 * a)), x[2][:m] | y[2][a:a + m])


def section_windows_numpy(letters, ends, k, canonical, chunk=1 << 22):
    """the same from numpy, in chunks of starts; the keys of k letters are joined from those of 1, 2, 4, .. letters"""
    codes = CODES[np.frombuffer(letters, dtype=np.uint8)]
    table = np.array(table_of(letters, ends), dtype=np.int64)
    limit = min(int(table[-1]), len(codes))
    for lo in range(0, max(limit - k + 1, 0), chunk):
        hi = min(lo + chunk, limit - k + 1)
        c = codes[lo:hi + k - 1]
        power, w, acc, acc_w = ((c & 3).astype(np.uint64), (3 - (c & 3)).astype(np.uint64), c > 3), 1, None, 0
        while w <= k:
            if k & w:
                acc, acc_w = (power, w) if acc is None else (_join(acc, acc_w, power, w, len(c) - acc_w - w + 1), acc_w + w)
            if 2 * w <= k:
                power = _join(power, w, power, w, len(c) - 2 * w + 1)
            w *= 2
        f, r, bad = acc
        m = hi - lo
        marks = np.zeros(m + 1, dtype=np.int64)              # the record of every start: the ends in (lo, hi] step it up
        inside = table[(table > lo) & (table <= hi)]
        np.add.at(marks, inside - lo, 1)
        rec = int(np.searchsorted(table, lo, side="right")) + np.cumsum(marks[:m])
        starts = np.arange(lo, hi, dtype=np.int64)
        ok = ~bad & (rec < len(table))
        ok[ok] = starts[ok] + k <= table[rec[ok]]
        rec, starts = rec[ok], starts[ok]
        begin = np.where(rec > 0, table[np.maximum(rec - 1, 0)], 0)
        yield rec, starts - begin, (np.minimum(f, r) if canonical else f)[ok]


def section_windows(letters, ends, k, canonical):
    if len(letters) <= LOOP_MAX:
        yield section_windows_loop(letters, ends, k, canonical)
    else:
        yield from section_windows_numpy(letters, ends, k, canonical)


class Ref:
    """what the rules give for a set: k, canonical, n_windows, the distinct keys"""

    def __init__(self, letters, ends, k, canonical=True):
        self.k, self.canonical, self.n_windows = k, bool(canonical), 0
        self.n_records, self.n_bases = len(table_of(letters, ends)), len(letters)
        parts = []
        for _, _, keys in section_windows(letters, ends, k, canonical):
            self.n_windows += len(keys)
            parts.append(np.unique(keys))
        self.keys = np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint64)
        self.n_kmers = len(self.keys)
        self.lut = None
        if k <= 13 and len(letters) > LOOP_MAX:              # a table of all 4^k keys: a gather instead of a search
            self.lut = np.zeros(4 ** k, dtype=bool)
            self.lut[self.keys.astype(np.int64)] = True

    def holds(self, keys):
        if self.lut is not None:
            return self.lut[keys.astype(np.int64)]
        if not len(self.keys):
            return np.zeros(len(keys), dtype=bool)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return self.keys[at] == keys


def options(min_hits=1, min_percent=0, interleaved=False, keep_matched=False):
    return dict(min_hits=min_hits, min_percent=min_percent, interleaved=interleaved, keep_matched=keep_matched)


def expected(letters, ends, ref, **opts):
    """-> windows, hits (uint64), regions (REGION), match, keep (uint8): what the rules of include/nafgpu.h give"""
    o = options(**opts)
    n = len(table_of(letters, ends))
    windows, hits = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    first, last = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for rec, start, keys in section_windows(letters, ends, ref.k, ref.canonical):
        windows += np.bincount(rec, minlength=n)
        hit = ref.holds(keys)
        rec, start = rec[hit], start[hit]
        hits += np.bincount(rec, minlength=n)
        if len(rec):
            which, at = np.unique(rec, return_index=True)                       # (ascending: the first of a record is its lowest start)
            new = first[which] < 0
            first[which[new]] = start[at[new]]
            which, at = np.unique(rec[::-1], return_index=True)
            last[which] = start[::-1][at] + ref.k
    regions = np.zeros(n, dtype=REGION)
    regions["record"], regions["start"], regions["end"] = np.arange(n), np.where(hits > 0, first, 0), np.where(hits > 0, last, 0)
    match = (hits >= max(o["min_hits"], 1)) & (hits * 100 >= o["min_percent"] * windows)
    if o["interleaved"]:
        match[0::2] = match[1::2] = match[0::2] | match[1::2]
    keep = match == bool(o["keep_matched"])
    return windows.astype(np.uint64), hits.astype(np.uint64), regions, match.astype(np.uint8), keep.astype(np.uint8)


def _self_check():
    rng = np.random.default_rng(7)
    for _ in range(120):
        k, canonical = int(rng.integers(1, 32)), bool(rng.integers(0, 2))
        s = bytes(rng.choice(list(b"ACGTacgtUuNR-\x00\xc1"), int(rng.integers(0, 90)), p=[.2, .2, .2, .2] + [.2 / 11] * 11).astype(np.uint8))
        assert record_windows(s, k, canonical) == record_windows_plain(s, k, canonical), (s, k, canonical)
        ends = np.sort(rng.integers(0, len(s) + 1, int(rng.integers(0, 6)))).astype(np.uint64)
        loop = section_windows_loop(s, ends, k, canonical)
        fast = list(section_windows_numpy(s, ends, k, canonical, chunk=int(rng.integers(1, 40))))
        fast = [np.concatenate([f[i] for f in fast]) if fast else np.zeros(0) for i in range(3)]
        assert all(len(a) == len(b) and (a.astype(np.uint64) == b.astype(np.uint64)).all() for a, b in zip(loop, fast)), (s, ends, k, canonical)


_self_check()


def tables(screens):
    return (np.frombuffer(screens.windows(), dtype=np.uint64), np.frombuffer(screens.hits(), dtype=np.uint64), np.frombuffer(screens.regions(), dtype=REGION),
            np.frombuffer(screens.match(), dtype=np.uint8), np.frombuffer(screens.keep(), dtype=np.uint8), np.frombuffer(screens.kept_regions(), dtype=REGION))


def compare_set(kset, ref, what=""):
    got = (kset.k, kset.canonical, kset.n_windows, kset.n_kmers, len(kset), kset.n_bases, kset.n_records)
    want = (ref.k, ref.canonical, ref.n_windows, ref.n_kmers, ref.n_kmers, ref.n_bases, ref.n_records)
    assert got == want, (what, got, want)
    assert kset.slots & (kset.slots - 1) == 0 and (kset.slots >= 2 * ref.n_windows or os.environ.get("NAFGPU_KMER_SLOTS")), (what, kset.slots)


def compare(screens, letters, ends, ref, what="", **opts):
    """every table and total of a Screens against expected(); -> windows, hits, regions, match, keep"""
    want = expected(letters, ends, ref, **opts)
    windows, hits, regions, match, keep = want
    table = np.array(table_of(letters, ends), dtype=np.int64)
    lengths = np.diff(np.concatenate(([0], table)))
    whole = np.zeros(len(table), dtype=REGION)
    whole["record"], whole["end"] = np.arange(len(table)), lengths
    got = tables(screens)
    assert screens.n_records == len(table) == len(screens) and screens.n_bases == len(letters), (what, screens.n_records, len(table), screens.n_bases)
    for name, mine, theirs in zip(("windows", "hits", "regions", "match", "keep", "kept_regions"), got, want + (whole[keep.astype(bool)],)):
        assert mine.shape == theirs.shape, (what, name, mine.shape, theirs.shape)
        if mine.tobytes() != theirs.tobytes():
            at = int(np.nonzero(mine != theirs)[0][0])
            raise AssertionError("%s: %s differs at %d of %d: %s / %s" % (what, name, at, len(theirs), mine[at], theirs[at]))
    totals = (screens.n_matched, screens.n_kept, screens.n_windows, screens.n_hits, screens.bases_kept)
    assert totals == (int(match.sum()), int(keep.sum()), int(windows.sum()), int(hits.sum()), int(lengths[keep.astype(bool)].sum())), (what, totals)
    return want


def open_decoder(lib, blob, **opts):
    return Decoder(io.BytesIO(blob), _lib=lib, **opts)


class DeviceSource:
    """letters and an end table in device buffers of the test's own (tk.DeviceBytes); pad: the residue of the letters' address mod
    16; n_records: how many of the ends the source announces; ends None: no table"""

    def __init__(self, lib, letters, ends=None, pad=0, n_records=None):
        self._bufs = [tk.DeviceBytes(lib, letters, pad)]
        self.d_sequence, self.n_bases, self.d_record_end, self.n_records = self._bufs[0].address, len(letters), None, 0
        if ends is not None:
            self._bufs.append(tk.DeviceBytes(lib, np.asarray(ends, dtype=np.uint64).tobytes() or bytes(8)))
            self.d_record_end, self.n_records = self._bufs[1].address, len(ends) if n_records is None else n_records

    def close(self):
        for b in self._bufs:
            b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def ends_of(records):
    return np.cumsum([len(r) for r in records], dtype=np.uint64)


def case(lib, what, ref_records, records, k, canonical=True, pad=0, behind=b"", tables_given=True, n_ref=None, n_query=None, text=False, **opts):
    """reference and query records -> device buffers of this test's own -> kmers() and screen() against the yardstick;
    -> (the set's Ref, windows, hits, regions, match, keep).  behind: letters behind the last end of both; n_ref / n_query: how many
    records the sources announce; tables_given False: no end tables; text: the query goes through parse_text"""
    ref_letters, letters = b"".join(ref_records) + behind, b"".join(records) + behind
    ref_ends, ends = ends_of(ref_records)[:n_ref], ends_of(records)[:n_query]
    with DeviceSource(lib, ref_letters or b"N", ends_of(ref_records) if tables_given else None, pad, n_ref) as d_ref:
        if not ref_letters:
            d_ref.n_bases = 0
        if not d_ref.n_records:
            ref_ends = None
        ref = Ref(ref_letters, ref_ends, k, canonical)
        with scr.kmers(d_ref, k, canonical, _lib=lib) as kset:
            compare_set(kset, ref, what)
            if text:
                with parse_text(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(records)), device=0, _lib=lib) as parsed:
                    own, _, own_ends = tk.own_layout(parsed)
                    assert own == b"".join(records), what
                    with parsed.screen(kset, **opts) as screens:
                        return (ref,) + compare(screens, own, own_ends, ref, what=what, **opts)
            with DeviceSource(lib, letters, ends_of(records) if tables_given else None, (pad * 7 + 3) % 16 if pad else 0, n_query) as d_query:
                if not d_query.n_records:
                    ends = None
                with scr.screen(d_query, kset, _lib=lib, **opts) as screens:
                    return (ref,) + compare(screens, letters, ends, ref, what=what, **opts)


# ---------------------------------------------------------------- 1. the fixtures
PHIX = (  # k, canonical: n_kmers, the set's windows, windows of all reads, n_hits, matched, at min_percent=50, interleaved, letters in unmatched reads
    ((31, True), (2009, 2160, 11135, 4114, 25, 15, 34, 4911)), ((31, False), (2009, 2160, 11135, 3016, 15, 12, 20, 7921)),
    ((15, True), (2105, 2288, 11807, 4650, 27, 15, 36, 4309)), ((4, True), (134, 2376, 12269, 12259, 42, 42, 42, 0)))


def check_fixtures(lib):
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, _, ends = tk.layout(recs)
    assert len(recs) == 42 and len(letters) == 12436
    ref_letters, ref_ends = b"".join(r[2] for r in recs[:8]), ends[:8]
    with open_decoder(lib, blob) as dec:
        for (k, canonical), figures in PHIX:
            ref = Ref(ref_letters, ref_ends, k, canonical)
            with dec.select(list(range(8))) as first:
                kset = first.kmers(k, canonical)
                compare_set(kset, ref, "phix set k = %d" % k)
            # (the set outlives the selection it was built from)
            seen = [ref.n_kmers, ref.n_windows]
            with dec.screen(kset) as s:
                windows, hits, regions, match, keep = compare(s, letters, ends, ref, what="phix k = %d" % k)
                seen += [s.n_windows, s.n_hits, s.n_matched]
                assert (hits[:8] == windows[:8]).all() and s.bases_kept == figures[7], (k, s.bases_kept)
                if (k, canonical) == (31, True):
                    assert (int(hits[13]), int(windows[13]), tuple(regions[13])[1:3]) == (81, 270, (190, 301)), (hits[13], windows[13], regions[13])
            with dec.screen(kset, min_percent=50) as s:
                compare(s, letters, ends, ref, what="phix k = %d, min_percent" % k, min_percent=50)
                seen.append(s.n_matched)
            with dec.screen(kset, interleaved=True) as s:
                compare(s, letters, ends, ref, what="phix k = %d, interleaved" % k, interleaved=True)
                seen.append(s.n_matched)
            assert tuple(seen) == figures[:7], ((k, canonical), seen, figures)
            with dec.screen(kset, keep_matched=True, min_hits=5) as s:
                compare(s, letters, ends, ref, what="phix k = %d, baiting" % k, keep_matched=True, min_hits=5)
            kset.close()
        # a set of another sequence: masked.naf has 3 290 31-mers and none of them is in a read
        with open_decoder(lib, golden_bytes("masked.naf")) as other, other.kmers(31) as kset:
            assert kset.n_kmers == 3290
            with dec.screen(kset) as s:
                assert (s.n_hits, s.n_matched, s.n_kept, s.n_windows) == (0, 0, 42, 11135)
    try:                                                                        # closed screens and sets are refused
        s.hits()
    except RuntimeError:
        pass
    else:
        raise AssertionError("closed screens were used")
    # the genome fixtures against their own set: every window hits
    for name in ("masked", "CP040672", "NZ_AAEN01000029"):
        blob = golden_bytes(name + ".naf")
        recs = sc.oracle_records(blob)
        letters, _, ends = tk.layout(recs)
        for k, canonical in ((31, True), (12, False)):
            ref = Ref(letters, ends, k, canonical)
            with open_decoder(lib, blob) as dec, dec.kmers(k, canonical) as kset, dec.screen(kset, keep_matched=True) as s:
                compare_set(kset, ref, name)
                windows, hits, _, _, _ = compare(s, letters, ends, ref, what=name, keep_matched=True)
                assert (hits == windows).all() and s.n_hits == s.n_windows == ref.n_windows, name
    # the protein fixture is refused through the decoder
    with open_decoder(lib, golden_bytes("LuxC.naf")) as dec:
        for call in (lambda: dec.kmers(5), lambda: dec.screen(kset)):
            try:
                call()
            except ValueError as e:
                assert "nucleotide" in str(e) or "closed" in str(e), e
            except RuntimeError:
                pass                                                            # (the closed set of above)
            else:
                raise AssertionError("k-mers of a protein archive")
        with open_decoder(lib, golden_bytes("masked.naf")) as other, other.kmers(31) as live:
            try:
                dec.screen(live)
            except ValueError as e:
                assert "nucleotide" in str(e), e
            else:
                raise AssertionError("a protein archive was screened")


# ---------------------------------------------------------------- 2. the edges
def check_edges(lib):
    kernel_constants()
    rng = np.random.default_rng(20250202)
    letters_of = lambda n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    R = letters_of(600)

    def random_records(section, most):
        pieces, at = [], 0
        while at < len(section):
            l = int(rng.integers(0, most))
            pieces.append(section[at:at + l])
            at += l
        return pieces

    for k in KS:
        # ---- every k on both kinds of key: reads cut from either strand of the reference, with a substitution, and random ones
        reads = [R[a:a + l] for a, l in ((0, 100), (37, k), (90, k + 1), (200, 150), (580, 20))] + [revcomp(R[300:420]), letters_of(90), R[450:500] + b"N" + R[501:560]]
        for canonical in (True, False):
            ref, windows, hits, _, _, _ = case(lib, "k = %d, canonical %d" % (k, canonical), [R[:250], R[250:251], R[251:]], reads, k, canonical, pad=k % 16)
            assert hits[0] == windows[0] == 100 - k + 1 and hits[1] == 1 and (k < 15 or hits[6] == 0) and (k < 15 or (hits[5] == windows[5]) == canonical)

        # ---- a planted window (its reverse complement at every other place) at the section's first and last start, around
        # every tile edge, at every residue of a lane
        P = letters_of(k)
        n = TILE * (k + 1) + 200
        starts = sorted([0, n - k] + [TILE * j - k + (j - 1) for j in range(1, k + 2)] + [112 + 81 * i for i in range(LANE + 1)])
        assert {s - TILE * (1 + i) for i, s in enumerate(starts[LANE + 2:-1])} == set(range(-k, 1)) and {s % LANE for s in starts[1:LANE + 2]} == set(range(LANE))
        section = bytearray(letters_of(n))
        for i, s in enumerate(starts):
            section[s:s + k] = revcomp(P) if i & 1 else P
        section = bytes(section)
        cuts = [0] + [int(rng.integers(a + k, b + 1)) for a, b in zip(starts[:-1], starts[1:])] + [n]
        own = [section[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        ref, windows, hits, regions, _, _ = case(lib, "planted windows, k = %d" % k, [P], own, k)
        if k >= 15:                                                             # (a random background holds no copy of 15 letters or more)
            assert (hits == 1).all() and [(int(r["start"]), int(r["end"])) for r in regions] == [(s - c, s - c + k) for s, c in zip(starts, cuts)], k
        if k in (2, 17, 31):
            case(lib, "planted windows as text, k = %d" % k, [P], [r for r in own[:k + 8] if r], k, text=True)
        _, _, hits, regions, _, _ = case(lib, "one record, k = %d" % k, [P], [section], k, pad=(k % 15) + 1)
        assert k < 15 or (int(hits[0]), tuple(regions[0])[1:3]) == (len(starts), (0, n))
        case(lib, "random records, k = %d" % k, [P, revcomp(P)], random_records(section, 3 * k + 40), k, canonical=False)
        case(lib, "no end tables, k = %d" % k, [P], [section], k, tables_given=False)

        # ---- record lengths 0, 1, k - 1, k, k + 1 and runs of empty records, all cut from the reference
        lengths = [0, 1, k - 1, k, k + 1, 0, 0, 0, k, 0] + [0] * 70 + [k, k - 1, 2 * k, 1]
        _, windows, hits, _, _, _ = case(lib, "record lengths, k = %d" % k, [R], [R[3 * i:3 * i + l] for i, l in enumerate(lengths)], k)
        assert [int(w) for w in windows] == [max(l - k + 1, 0) for l in lengths] and (hits == windows).all()

        # ---- a k-mer of the reference split by a record end in the query, and one split in the reference: neither counts
        if k > 1:
            _, windows, hits, _, _, _ = case(lib, "a window across a record end, k = %d" % k, [P], [P[:k // 2], P[k // 2:], P], k)
            assert [int(w) for w in windows] == [0, 0, 1] and int(hits[2]) == 1
            ref, _, hits, _, _, _ = case(lib, "a window across an end of the reference, k = %d" % k, [P[:k // 2], P[k // 2:]], [P, P + P], k)
            assert ref.n_kmers == 0 and not hits.any()

        # ---- one N moved through every position of a record of 2 k letters: exactly the windows over it vanish
        clean = R[100:100 + 2 * k]
        _, windows, hits, _, _, _ = case(lib, "an N at every position, k = %d" % k, [clean], [clean[:p] + b"N" + clean[p + 1:] for p in range(2 * k)], k)
        assert [int(w) for w in windows] == [k + 1 - (min(p, k) - max(p - k + 1, 0) + 1) for p in range(2 * k)] and (hits == windows).all(), k

    # ---- letter classes: case and T/U play no part; every other byte is no letter
    upper = R[:200].replace(b"T", b"U")
    _, windows, hits, _, _, _ = case(lib, "lower case and U", [R[:200]], [R[:200].lower(), upper, upper.lower(), R[:200]], 21)
    assert (hits == 180).all() and (windows == 180).all()
    others = b"NRYKMSWBDHVnrykmswbdhv-*.Xx" + bytes([0, 1, 64, 91, 96, 123, 127, 128, 0xC1, 0xE1, 255])
    _, windows, _, _, _, _ = case(lib, "no letters", [R[:100]], [R[:10] + bytes([b]) + R[11:21] for b in others], 10)
    assert (windows == 2).all()
    everything = bytes(rng.permutation(np.tile(np.arange(256, dtype=np.uint8), 40)))
    case(lib, "all byte values", [everything[:3000]], random_records(everything, 700), 2, canonical=False)
    case(lib, "all byte values, k = 1", [b"a"], random_records(everything, 700), 1)
    # ---- pointers at every residue mod 16, letters behind the last end
    for pad in range(1, 16):
        n = 9000 + 13 * pad
        section = bytearray(letters_of(n))
        for at in rng.integers(0, n, 40):
            section[at] = ord("N")
        case(lib, "the pointers at residue %d" % pad, random_records(R + bytes(section[:300]), 150), random_records(bytes(section) + R[100:400], 400), 15 + pad,
             pad=pad, behind=R[:40 + pad], min_hits=2)

    # ---- the ends of the key range: keys 0 and 4^31 - 1, with an empty slot that is neither
    for letter, want in ((b"A", [1, 0, 0, 0]), (b"T", [0, 1, 0, 0])):
        ref, _, hits, _, _, _ = case(lib, "poly-%s" % letter.decode(), [letter * 40], [b"A" * 31, b"T" * 31, b"C" * 31, b"A" * 30 + b"C"], 31, canonical=False)
        assert ref.n_kmers == 1 and int(ref.keys[0]) == (0 if letter == b"A" else 4 ** 31 - 1) and [int(h) for h in hits] == want
    ref, _, hits, _, _, _ = case(lib, "poly-A over three tiles", [b"A" * (3 * TILE)], [b"T" * 50, b"A" * 29 + b"CA"], 31)
    assert (ref.n_kmers, ref.n_windows) == (1, 3 * TILE - 30) and [int(h) for h in hits] == [20, 0]

    # ---- strands: the reverse complement of the reference as the query; palindromic keys at even k
    for k in (16, 31):
        _, windows, hits, _, _, _ = case(lib, "the other strand, canonical", [R], [revcomp(R), R], k)
        assert (hits == windows).all()
        _, windows, hits, _, _, _ = case(lib, "the other strand, forward keys", [R], [revcomp(R), R], k, canonical=False)
        assert int(hits[0]) < 3 and hits[1] == windows[1]
    half = letters_of(8)
    palindrome = half + revcomp(half)
    ref, _, hits, _, _, _ = case(lib, "a palindrome", [palindrome, b"ACGT" * 8], [palindrome, revcomp(palindrome), b"ACGT" * 5, half + half], 16)
    assert ref.n_kmers == 4 and [int(h) for h in hits] == [1, 1, 5, 0]           # (the palindrome; ACGT x 4 and its shifts: CGTA is TACG reversed, GTAC its own)

    # ---- spans and thresholds
    long = R[:40] + letters_of(3 * TILE) + R[100:140]
    _, windows, hits, regions, _, _ = case(lib, "a record over three tiles", [R], [R[300:330], long, R[:29]], 30, pad=5)
    assert [int(h) for h in hits] == [1, 22, 0] and tuple(regions[1])[1:3] == (0, len(long)) and int(windows[2]) == 0
    other = bytes([b"ACGT"[(b"ACGT".index(R[130]) + 1) % 4]])                    # (so that the eleventh window does not hit by chance)
    reads = [R[:60], letters_of(60), letters_of(60), R[100:130] + other + letters_of(29), letters_of(60), letters_of(60), R[200:260], R[300:360], b"ACGTN" * 12, R[400:460]]
    want = {(10, 0): [1, 0, 0, 1, 0, 0, 1, 1, 0, 1], (11, 0): [1, 0, 0, 0, 0, 0, 1, 1, 0, 1], (0, 25): [1, 0, 0, 1, 0, 0, 1, 1, 0, 1], (0, 26): [1, 0, 0, 0, 0, 0, 1, 1, 0, 1],
            (0, 100): [1, 0, 0, 0, 0, 0, 1, 1, 0, 1], (0, 0): [1, 0, 0, 1, 0, 0, 1, 1, 0, 1]}
    for (min_hits, min_percent), flags in want.items():                         # read 3: 10 hits of 40 windows, 25 %
        for keep_matched in (False, True):
            _, windows, hits, _, match, keep = case(lib, "thresholds %d, %d %%" % (min_hits, min_percent), [R], reads, 21, min_hits=min_hits, min_percent=min_percent,
                                                    keep_matched=keep_matched)
            assert (int(hits[3]), int(windows[3]), int(windows[8])) == (10, 40, 0) and list(match) == flags and list(keep) == [f == keep_matched for f in flags], \
                (min_hits, min_percent, keep_matched, hits, windows, match, keep)
    _, _, _, _, match, keep = case(lib, "mates", [R], reads, 21, interleaved=True)
    assert list(match) == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1] and list(keep) == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    _, _, _, _, match, _ = case(lib, "mates, a threshold", [R], reads, 21, interleaved=True, min_hits=11, keep_matched=True)
    assert list(match) == [1, 1, 0, 0, 0, 0, 1, 1, 1, 1]

    # ---- boundary inputs
    ref, _, _, _, _, keep = case(lib, "an empty set", [R[:10], R[10:20], b""], reads, 11)
    assert ref.n_kmers == 0 and keep.all()
    ref, windows, _, _, _, _ = case(lib, "no records announced: the section is record 0", [R[:50], R[50:90]], reads[:3], 12, n_ref=0, n_query=0)
    assert ref.n_windows == 90 - 11 and len(windows) == 1
    ref, windows, hits, _, _, _ = case(lib, "letters behind the last end", [R[:50], R[50:90]], [R[:40], R[60:130]], 12, n_ref=1, n_query=1, behind=R[200:260])
    assert ref.n_windows == 39 and len(windows) == 1 and int(hits[0]) == int(windows[0]) == 29


def check_hooks(lib):
    """NAFGPU_KMER_HASH_BITS at 0, 3 and 8 and a table that NAFGPU_KMER_SLOTS makes nearly full (after nafgpu_test_hooks(1); the
    caller runs this in a process of its own, so that the hooks do not leak): the same answers"""
    rng = np.random.default_rng(9)
    R = bytes(rng.choice(list(b"ACGT"), 2000).astype(np.uint8))
    reads = [R[a:a + 100] for a in range(0, 400, 37)] + [bytes(rng.choice(list(b"ACGT"), 100).astype(np.uint8)) for _ in range(8)] + [revcomp(R[50:200])]
    lib.c.nafgpu_test_hooks(1)
    try:
        for bits in ("0", "3", "8", None):
            for slots, n_ref in (("128", 133), ("128", 141), ("4096", 2000), (None, 2000)):   # 119 and 127 keys in 128 slots: nearly full
                for name, value in (("NAFGPU_KMER_HASH_BITS", bits), ("NAFGPU_KMER_SLOTS", slots)):
                    os.environ.pop(name, None)
                    if value is not None:
                        os.environ[name] = value
                ref, _, hits, _, _, _ = case(lib, "hash bits %s, slots %s" % (bits, slots), [R[:n_ref]], reads, 15, min_hits=3)
                assert ref.n_kmers == n_ref - 14 and int(hits[0]) == min(86, n_ref - 14)
        os.environ["NAFGPU_KMER_SLOTS"] = "64"                                  # fewer slots than keys: refused, and the probing ends
        try:
            case(lib, "too few slots", [R[:200]], reads, 15)
        except ValueError as e:
            assert "slots" in str(e), e
        else:
            raise AssertionError("186 keys in 64 slots")
    finally:
        os.environ.pop("NAFGPU_KMER_HASH_BITS", None)
        os.environ.pop("NAFGPU_KMER_SLOTS", None)
        lib.c.nafgpu_test_hooks(0)


# ---------------------------------------------------------------- 3. random
def random_reads(n, seed=13):
    """-> a reference of 2^16 random letters, reads of about n letters in all: lengths 0 .. 300 and a few of 10^4, N sprinkled in;
    half of them cut from the reference, either strand, with a substitution about every 40 letters, half of them random"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    reference = rng.choice(alphabet, 2 ** 16)
    records, total = [], 0
    while total < n:
        l = 10_000 + int(rng.integers(0, 999)) if rng.random() < 0.002 else int(rng.integers(0, 301))
        if rng.random() < 0.5:
            at = int(rng.integers(0, len(reference) - l))
            s = reference[at:at + l].copy()
            change = np.flatnonzero(rng.random(l) < 1 / 40)
            s[change] = rng.choice(alphabet, len(change))
            if rng.random() < 0.5:
                s = np.frombuffer(revcomp(s.tobytes()), dtype=np.uint8).copy()
        else:
            s = rng.choice(alphabet, l)
        s[rng.random(l) < 0.002] = ord("N")
        records.append(s.tobytes())
        total += l
    return reference.tobytes(), records[:len(records) & ~1]


def check_random(lib, n):
    reference, records = random_reads(n)
    text = b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(records))
    with parse_text(b">ref\n%s\n" % reference, device=0, _lib=lib) as d_ref, parse_text(text, device=0, _lib=lib) as parsed:
        letters, _, ends = tk.own_layout(parsed)
        assert letters == b"".join(records) and len(ends) == len(records) and any(len(r) > 9999 for r in records)
        for k in (15, 31):
            ref = Ref(reference, None, k)
            share = int(expected(letters, ends, ref)[3].sum())
            assert 0.25 * len(records) <= share <= 0.75 * len(records), (k, share, len(records))     # on the yardstick's answer
            if n <= LOOP_MAX:                                                   # the two forms of the yardstick agree on this input
                assert all((a == b).all() for a, b in zip(section_windows_loop(letters, ends, k, True), next(section_windows_numpy(letters, ends, k, True))))
            with d_ref.kmers(k) as kset:
                compare_set(kset, ref, "random reference")
                for opts in (dict(), dict(min_hits=3, min_percent=20, interleaved=True), dict(keep_matched=True, min_percent=60)):
                    with parsed.screen(kset, **opts) as s:
                        compare(s, letters, ends, ref, what="random, %d letters, k = %d, %r" % (n, k, opts), **opts)
                        print("screen k = %d %r: %d letters, %d records, %d matched, %d kept, set %.3f ms, screen %.3f ms"
                              % (k, opts, len(letters), len(records), s.n_matched, s.n_kept, kset.ms, s.ms))


# ---------------------------------------------------------------- 4. composition
def check_composition(lib, threads=True):
    """threads False: the two screens of one set run one after the other (the CPU harness is one device that runs one kernel at a
    time and is not re-entrant)"""
    blob = golden_bytes("phix.naf")
    recs = sc.oracle_records(blob)
    letters, _, ends = tk.layout(recs)
    with open_decoder(lib, blob) as source, source.select(list(range(8))) as first:
        kset = first.kmers(31)
    # (a set outlives its selection and its closed decoder)
    ref = Ref(b"".join(r[2] for r in recs[:8]), ends[:8], 31)
    opts = dict(interleaved=True, min_hits=2)
    with kset, open_decoder(lib, blob) as dec, dec.screen(kset, **opts) as screens:
        _, _, _, _, keep = compare(screens, letters, ends, ref, what="phix", **opts)
        mine = [bytes(t) for t in tables(screens)]
        assert 0 < screens.n_kept < 42
        # select(screens): exactly the kept records, whole, read back through the oracle
        with dec.select(screens) as sel:
            assert sel.n_records == screens.n_kept
            archive = encode_device(sel, sequence_type="dna", id=True, comment=True, sequence=True, quality=True, mask=True, compression_level=1, device=0, _lib=lib)
        cleaned = sc.oracle_records(archive, spec_mask=True)
        assert [tuple(r) for r in cleaned] == [tuple(r) for r, flag in zip(recs, keep) if flag]
        with dec.select(screens.kept_regions()) as a, dec.select(screens) as b:
            assert tk.own_layout(a)[0] == tk.own_layout(b)[0]
        # Selection.screen, ParsedText.screen and screen(decode_all_device()) equal Decoder.screen on the same records
        with dec.select(list(range(42))) as sel, sel.screen(kset, **opts) as again:
            assert mine == [bytes(t) for t in tables(again)] and (again.n_kept, again.n_hits, again.bases_kept) == (screens.n_kept, screens.n_hits, screens.bases_kept)
        with parse_text(dec.to_text(), device=0, _lib=lib) as parsed, parsed.screen(kset, **opts) as again:
            assert mine == [bytes(t) for t in tables(again)] and again.n_windows == screens.n_windows
        with scr.screen(dec.decode_all_device(), kset, _lib=lib, **opts) as again:
            assert mine == [bytes(t) for t in tables(again)]
        with parse_text(b"".join(b">%d\n%s\n" % (i, r[2]) for i, r in enumerate(recs[:8])), device=0, _lib=lib) as parsed, parsed.kmers(31) as same:
            compare_set(same, ref, "ParsedText.kmers")
        # two screens of one set from two threads agree
        seen = [None, None]

        def work(i):
            with dec.select(list(range(42))) as sel, sel.screen(kset, **opts) as s:
                seen[i] = [bytes(t) for t in tables(s)]
        workers = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in workers:
            t.start() if threads else t.run()
        for t in workers:
            t.join() if threads else None
        assert seen[0] == seen[1] == mine
        # what select accepted before is read as before
        with dec.select([3, (7, 5, 250)]) as sel:
            assert tk.own_layout(sel)[0] == recs[3][2] + recs[7][2][5:250]
    try:
        dec.screen(kset)
    except (RuntimeError, ValueError):
        pass
    else:
        raise AssertionError("a closed set was used")


# ---------------------------------------------------------------- 5. refusals
def call_build(lib, src_fields, device=0, null_opts=False, **opts):
    src, o = _ffi.EncodeSource(**src_fields), _ffi.KmerOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.KmersResult(), _ffi.Error()
    rc = lib.c.nafgpu_kmers_build(ctypes.byref(src), None if null_opts else ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_kmers_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_screen(lib, src_fields, kset, device=0, null_opts=False, **opts):
    src, o = _ffi.EncodeSource(**src_fields), _ffi.ScreenOpts(**opts)
    h, res, err = ctypes.c_void_p(), _ffi.ScreenResult(), _ffi.Error()
    rc = lib.c.nafgpu_screen(ctypes.byref(src), kset._h if kset else None, None if null_opts else ctypes.byref(o), device, ctypes.byref(h), ctypes.byref(res),
                             ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
    else:
        lib.c.nafgpu_screens_free(h)
    return rc, err.message.decode("utf-8", "replace")


def call_decoder(lib, dec, kset=None, null_opts=False, **opts):
    """nafgpu_kmers_build_decoder without a set, nafgpu_screen_decoder with one"""
    h, err = ctypes.c_void_p(), _ffi.Error()
    if kset is None:
        o, res = _ffi.KmerOpts(**opts), _ffi.KmersResult()
        rc = lib.c.nafgpu_kmers_build_decoder(dec._h, None if null_opts else ctypes.byref(o), ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    else:
        o, res = _ffi.ScreenOpts(**opts), _ffi.ScreenResult()
        rc = lib.c.nafgpu_screen_decoder(dec._h, kset._h, None if null_opts else ctypes.byref(o), ctypes.byref(h), ctypes.byref(res), ctypes.byref(err))
    if rc != _ffi.OK:
        assert not h.value and bytes(res) == bytes(ctypes.sizeof(res)) and err.status == rc
        last = _ffi.Error()
        lib.c.nafgpu_last_error(dec._h, ctypes.byref(last))
        assert last.status == rc and last.message == err.message
    else:
        (lib.c.nafgpu_kmers_free if kset is None else lib.c.nafgpu_screens_free)(h)
    return rc, err.message.decode("utf-8", "replace"), err.io_kind


def refused(call, error=ValueError):
    try:
        call()
    except error:
        return True
    raise AssertionError("accepted")


def check_refusals(lib):
    blob = golden_bytes("phix.naf")
    bad, length = _ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH
    with open_decoder(lib, blob) as dec, dec.kmers(21) as kset:
        res = dec.decode_all_device()
        good = dict(d_sequence=res.d_sequence, n_bases=res.n_bases, d_record_end=res.d_record_end, n_records=res.n_records)
        # ---- the set
        assert call_build(lib, good, k=1)[0] == call_build(lib, good, k=31, canonical=1)[0] == _ffi.OK
        for k in (0, 32, 255):
            rc, message = call_build(lib, good, k=k)
            assert rc == bad and "k %d" % k in message, (k, rc, message)
        assert call_build(lib, good, null_opts=True)[0] == bad and call_build(lib, dict(good, d_sequence=None), k=5)[0] == bad
        src, o, h, r, err = _ffi.EncodeSource(**good), _ffi.KmerOpts(k=5), ctypes.c_void_p(), _ffi.KmersResult(), _ffi.Error()
        for args in ((None, ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), ctypes.byref(o), 0, None, ctypes.byref(r)),
                     (ctypes.byref(src), ctypes.byref(o), 0, ctypes.byref(h), None), (ctypes.byref(src), ctypes.byref(o), -2, ctypes.byref(h), ctypes.byref(r))):
            assert lib.c.nafgpu_kmers_build(*args, ctypes.byref(err)) == bad
        lib.c.nafgpu_kmers_free(None)
        assert call_decoder(lib, dec, null_opts=True)[0] == bad and call_decoder(lib, dec, k=0)[0] == bad and call_decoder(lib, dec, k=32)[0] == bad
        assert call_decoder(lib, dec, k=31, canonical=1)[0] == _ffi.OK
        # ---- the screen
        assert call_screen(lib, good, kset)[0] == call_screen(lib, good, kset, min_percent=100, interleaved=1, keep_matched=1, min_hits=2 ** 40)[0] == _ffi.OK
        assert call_screen(lib, good, None)[0] == bad and call_screen(lib, good, kset, null_opts=True)[0] == bad
        assert call_screen(lib, dict(good, d_sequence=None), kset)[0] == bad
        rc, message = call_screen(lib, good, kset, min_percent=101)
        assert rc == bad and "min_percent" in message, (rc, message)
        rc, message = call_screen(lib, dict(good, n_records=41), kset, interleaved=1)
        assert rc == bad and "odd" in message, (rc, message)
        assert call_screen(lib, dict(good, n_records=0), kset, interleaved=1)[0] == bad         # the section as one record: odd
        n_devices = 0
        try:
            while n_devices < 64:
                lib.device_info(n_devices)
                n_devices += 1
        except RuntimeError:
            pass
        if n_devices > 1:                                                       # a set of another device
            rc, message = call_screen(lib, good, kset, device=1)
            assert rc == bad and "device" in message, (rc, message)
        assert call_screen(lib, good, kset, device=n_devices)[0] == bad
        src, o, r = _ffi.EncodeSource(**good), _ffi.ScreenOpts(), _ffi.ScreenResult()
        for args in ((None, kset._h, ctypes.byref(o), 0, ctypes.byref(h), ctypes.byref(r)), (ctypes.byref(src), kset._h, ctypes.byref(o), 0, None, ctypes.byref(r)),
                     (ctypes.byref(src), kset._h, ctypes.byref(o), 0, ctypes.byref(h), None)):
            assert lib.c.nafgpu_screen(*args, ctypes.byref(err)) == bad
        assert lib.c.nafgpu_screens_copy_to_host(None, None, 1, None) == bad
        lib.c.nafgpu_screens_free(None)
        assert call_decoder(lib, dec, kset, null_opts=True)[0] == bad and call_decoder(lib, dec, kset, min_percent=101)[0] == bad
        assert call_decoder(lib, dec, kset, min_percent=100)[0] == _ffi.OK
        err = _ffi.Error()
        assert lib.c.nafgpu_screen_decoder(dec._h, None, ctypes.byref(o), ctypes.byref(h), ctypes.byref(r), ctypes.byref(err)) == bad
        for call in (lambda: dec.kmers(0), lambda: dec.kmers(32), lambda: dec.screen(kset, min_percent=101), lambda: dec.screen(kset, min_hits=-1),
                     lambda: dec.screen(None), lambda: dec.screen("ACGT"), lambda: scr.kmers(tk.Source(), _lib=lib), lambda: scr.screen(tk.Source(), kset, _lib=lib)):
            refused(call)
        check_end_tables(lib, kset)
        # through a decoder: the sequence not decoded; a shard; no Length section; an archive that ends early
        with open_decoder(lib, blob, sequence=False) as other:
            for rc, message, _ in (call_decoder(lib, other, k=5), call_decoder(lib, other, kset)):
                assert rc == bad and "sequence" in message, (rc, message)
        with open_decoder(lib, blob, shard_count=2) as other:
            for rc, message, _ in (call_decoder(lib, other, k=5), call_decoder(lib, other, kset)):
                assert rc == bad and "shard" in message, (rc, message)
        with open_decoder(lib, golden_bytes("LuxC.naf")) as other:
            for rc, message, _ in (call_decoder(lib, other, k=5), call_decoder(lib, other, kset)):
                assert rc == bad and "nucleotide" in message, (rc, message)
        with open_decoder(lib, sc.hand_archive(1, ids=[b"a"], text=b"NNACGTTTnn")) as other:
            for rc, message, _ in (call_decoder(lib, other, k=5), call_decoder(lib, other, kset)):
                assert rc == bad and "ength" in message, (rc, message)             # the Length section is needed, as for select
        # (hand_archive writes text archives; as dna the section's size counts letters, two to a byte: ten)
        early = bytearray(sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 30], text=bytes(range(10))))
        early[4] = 0
        with open_decoder(lib, bytes(early)) as other:
            for rc, message, kind in (call_decoder(lib, other, k=3), call_decoder(lib, other, kset)):
                assert (rc, kind) == (_ffi.E_IO, _ffi.IO_UNEXPECTED_EOF) and "record 2" in message, (rc, kind, message)
            refused(lambda: other.kmers(3), EOFError)
        fits = bytearray(sc.hand_archive(3, ids=[b"a", b"b", b"c"], lengths=[4, 4, 2], text=bytes(range(10))))
        fits[4] = 0                                                             # the same archive with a last record that fits
        with open_decoder(lib, bytes(fits)) as other, other.kmers(3) as small, other.screen(small) as s:
            assert (small.n_records, s.n_records, s.n_bases) == (3, 3, 10) and s.n_hits == s.n_windows == small.n_windows


def check_end_tables(lib, kset):
    """hand-made end tables through nafgpu_kmers_build and nafgpu_screen: a selection's letters with a table of this test's own in
    device memory; the lowest offender is named"""
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
            d_table = tk.DeviceBytes(lib, table.tobytes())
            try:
                fields = dict(d_sequence=sel.d_sequence, n_bases=n, d_record_end=d_table.address, n_records=len(table))
                for rc, message in (call_build(lib, fields, k=9, canonical=1), call_screen(lib, fields, kset, min_hits=2)):
                    assert rc == status and needle in message, (what, rc, message)
            finally:
                d_table.close()


# ---------------------------------------------------------------- 6. positions and tile indices past 2^32 (MI355X only)
def big_records(n, seed=4):
    """n letters as FASTA text: 2 000 short reads, then records of 2^16 .. 2^22 letters; N sprinkled in, and every other long record
    holds copies of pieces of the first 2^20 letters, either strand"""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(0, 301, 2000)]
    while sum(lengths) < n:
        lengths.append(min(int(2 ** rng.uniform(16, 22)), n - sum(lengths)))
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
    s[rng.integers(0, n, n // 5000)] = ord("N")
    at = 0
    for i, l in enumerate(lengths):
        if l > 2 ** 16 and i % 2 and at > 2 ** 20:
            for _ in range(8):
                size, src, dst = int(rng.integers(20, 5000)), int(rng.integers(0, 2 ** 20 - 5000)), at + int(rng.integers(0, l - 5000))
                piece = s[src:src + size]
                s[dst:dst + size] = piece if rng.random() < 0.5 else np.frombuffer(revcomp(piece.tobytes()), dtype=np.uint8)
        at += l
    s = s.tobytes()
    out, at = [], 0
    for i, l in enumerate(lengths):
        out.append(b">r%d\n%s\n" % (i, s[at:at + l]))
        at += l
    return b"".join(out), s, lengths


def check_past_u32(lib, n_bases=2 ** 28, copies=17, k=13):
    text, letters, lengths = big_records(n_bases)
    archive = encode_text(text, sequence_type="dna", id=False, comment=False, sequence=True, compression_level=1, device=0, _lib=lib)
    del text
    ends = np.cumsum(lengths, dtype=np.uint64)
    head = int(np.searchsorted(ends, 2 ** 20, side="right"))                     # the records that end within the first 2^20 letters
    opts = dict(min_hits=40, min_percent=30)                                     # (a random window is in the set about once in 70)
    with open_decoder(lib, archive) as dec:
        res = dec.decode_all_device()
        assert (res.n_bases, res.n_records) == (n_bases, len(lengths)) and dec.copy_to_host(res.d_sequence, 4096) == letters[:4096]
        ref = Ref(letters[:int(ends[head - 1])], ends[:head], k)
        with dec.select(list(range(head))) as first:
            kset = first.kmers(k)
            compare_set(kset, ref, "the first 2^20 letters")
        with kset:
            with dec.screen(kset, **opts) as s:
                print("screen: %d records, %d letters, %d matched, %d hits of %d windows, %.3f ms" % (s.n_records, s.n_bases, s.n_matched, s.n_hits, s.n_windows, s.ms))
                want = compare(s, letters, ends, ref, what="2^28 letters", **opts)
                assert 0 < s.n_matched < len(lengths)
                one = (s.n_matched, s.n_kept, s.n_windows, s.n_hits, s.bases_kept)
            del letters
            windows, hits, regions, match, keep = want
            whole = np.zeros(len(lengths), dtype=REGION)
            whole["record"], whole["end"] = np.arange(len(lengths)), lengths
            kept = whole[keep.astype(bool)]
            with dec.select(list(range(res.n_records)) * copies) as sel:
                assert sel.n_bases == copies * n_bases > 2 ** 32
                with sel.screen(kset, **opts) as s:
                    print("screen past 2^32: %d records, %d letters, %d kept, %.3f ms" % (s.n_records, s.n_bases, s.n_kept, s.ms))
                    assert s.n_records == copies * len(lengths) and s.n_bases == copies * n_bases
                    assert (s.n_matched, s.n_kept, s.n_windows, s.n_hits, s.bases_kept) == tuple(copies * v for v in one)
                    got = tables(s)
                    n = len(lengths)
                    for c in range(copies):                                     # copy c: the screens of copy 0, the record shifted
                        for mine, theirs in zip(got[:2] + got[3:5], (windows, hits, match, keep)):
                            assert mine[c * n:(c + 1) * n].tobytes() == theirs.tobytes(), c
                        shifted = regions.copy()
                        shifted["record"] += np.uint64(c * n)
                        assert got[2][c * n:(c + 1) * n].tobytes() == shifted.tobytes(), c
                        shifted = kept.copy()
                        shifted["record"] += np.uint64(c * n)
                        assert got[5][c * len(kept):(c + 1) * len(kept)].tobytes() == shifted.tobytes(), c
