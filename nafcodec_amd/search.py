"""Hits / search -- where a set of short patterns (primers, adapters, restriction sites, guides) occurs in records that are
in HBM, found by the HIP kernels (include/nafgpu.h: nafgpu_search has the rules; no counterpart in the reference).

A hit is a nafgpu_region, the thing Decoder.select() takes, so the answer feeds the next stage as it is:

    with decoder.search(["AGATCGGAAGAGC"], max_mismatches=1) as hits:
        first = hits.record_hit_begin()                      # CSR over records: the hits of record k are first[k] .. first[k + 1]
        start = numpy.frombuffer(hits.regions(), dtype=REGION)["start"]
        with decoder.select(hits) as windows: ...            # every matched window as a record of its own

The tables come to the host as memoryviews; numpy.frombuffer wraps them without a copy (REGION and INFO below are the
dtypes' fields)."""
import ctypes
from ctypes import byref, c_void_p

from . import _ffi

NUCLEOTIDE, BYTES = 0, 1
MAX_PATTERNS, MAX_LENGTH, MAX_MISMATCHES = 16, 64, 3
# numpy.dtype(REGION), numpy.dtype(INFO): the layouts of nafgpu_region and nafgpu_hit_info
REGION = [("record", "<u8"), ("start", "<u8"), ("end", "<u8"), ("reverse_complement", "u1"), ("reserved", "u1", (7,))]
INFO = [("pattern", "<u4"), ("mismatches", "u1"), ("reserved", "u1", (3,))]


def _raise(rc, err):
    from .decoder import _raise as raise_error
    if rc in (_ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise_error(err)


def _alphabet(alphabet):
    if alphabet in (None, NUCLEOTIDE, "nucleotide"):
        return NUCLEOTIDE
    if alphabet in (BYTES, "bytes"):
        return BYTES
    raise ValueError("alphabet: 'nucleotide', 'bytes' or None expected, got %r" % (alphabet,))


def _arguments(patterns, alphabet, both_strands, max_mismatches, max_hits):
    """-> the patterns as NUL-terminated strings, their number, nafgpu_search_opts"""
    if isinstance(patterns, (str, bytes)):
        patterns = [patterns]
    blobs = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
    if any(b"\0" in b for b in blobs):
        raise ValueError("a pattern holds a NUL byte")
    if not 0 <= int(max_mismatches) <= 255 or int(max_hits) < 0:
        raise ValueError("max_mismatches and max_hits are not negative")
    opts = _ffi.SearchOpts(alphabet=alphabet, both_strands=int(alphabet == NUCLEOTIDE if both_strands is None else bool(both_strands)),
                           max_mismatches=int(max_mismatches), max_hits=int(max_hits))
    return b"".join(b + b"\0" for b in blobs), len(blobs), opts


class Hits:
    """What search() returns.  n_hits, n_records, n_bases, pattern_hits (a tuple, one count per pattern, both strands), ms
    (the search kernels); regions() (n_hits nafgpu_region structs, 32 bytes each), info() (n_hits nafgpu_hit_info structs, 8
    bytes each) and record_hit_begin() (n_records + 1 64-bit words) copy a table to the host.  Hits come in ascending order
    of (position, pattern, strand).  It owns its device buffers and outlives its source; they live until close()."""

    def __init__(self, lib, handle, res, n_patterns):
        self._lib, self._h = lib, handle
        self.d_regions, self.d_info, self.d_record_hit_begin = res.d_regions or None, res.d_info or None, res.d_record_hit_begin or None
        self.n_hits, self.n_records, self.n_bases = res.n_hits, res.n_records, res.n_bases
        self.pattern_hits, self.ms = tuple(res.pattern_hits[:n_patterns]), res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed hits.")
        return self._h

    def _table(self, d_ptr, n_bytes):
        handle = self._handle()
        buf = bytearray(int(n_bytes))
        if n_bytes and self._lib.c.nafgpu_hits_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf)

    def regions(self):
        """n_hits x 32 bytes: {record, start, end, reverse_complement} per hit, start and end relative to the record"""
        return self._table(self.d_regions, ctypes.sizeof(_ffi.Region) * self.n_hits)

    def info(self):
        """n_hits x 8 bytes: {pattern, mismatches} per hit"""
        return self._table(self.d_info, ctypes.sizeof(_ffi.HitInfo) * self.n_hits)

    def record_hit_begin(self):
        """n_records + 1 words: the hits of record k are [begin[k], begin[k + 1])"""
        return self._table(self.d_record_hit_begin, 8 * (self.n_records + 1)).cast("Q")

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_hits_free(h)

    def __len__(self):
        return self.n_hits

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def search(source, patterns, *, max_mismatches=0, both_strands=None, alphabet=None, max_hits=0, device=None, _lib=None):
    """Records in HBM -> the Hits of `patterns` (str or bytes, up to 16 of up to 64 letters).  `source` is whatever
    encode_device() takes: what Decoder.decode_all_device() returns, a Selection, a ParsedText, or anything with d_sequence /
    n_bases and d_record_end / n_records holding device addresses.  alphabet: "nucleotide" (None: the same) or "bytes";
    both_strands: None = on for the nucleotide alphabet, off for bytes; max_mismatches: 0 .. 3 substitutions; max_hits: 0 = no
    cap, else more hits than this is refused.  ValueError for what the rules refuse."""
    lib = _lib or _ffi.default()
    blob, n, opts = _arguments(patterns, _alphabet(alphabet), both_strands, max_mismatches, max_hits)
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    h, res, err = c_void_p(), _ffi.SearchResult(), _ffi.Error()
    rc = lib.c.nafgpu_search(byref(src), blob, len(blob), n, byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Hits(lib, h, res, n)


def _search_decoder(decoder, patterns, max_mismatches, both_strands, alphabet, max_hits):
    lib = decoder._lib
    if alphabet is None:                                     # by the archive: dna and rna as nucleotides, protein and text as bytes
        alphabet = NUCLEOTIDE if decoder._header.sequence_type <= 1 else BYTES
    blob, n, opts = _arguments(patterns, _alphabet(alphabet), both_strands, max_mismatches, max_hits)
    h, res, err = c_void_p(), _ffi.SearchResult(), _ffi.Error()
    rc = lib.c.nafgpu_search_decoder(decoder._h, blob, len(blob), n, byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Hits(lib, h, res, n)


__all__ = ["Hits", "search", "REGION", "INFO", "NUCLEOTIDE", "BYTES", "MAX_PATTERNS", "MAX_LENGTH", "MAX_MISMATCHES"]
