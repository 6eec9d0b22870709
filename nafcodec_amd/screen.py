"""KmerSet / Screens / kmers / screen -- the k-mers of a reference as a set in HBM, and records screened against it by the HIP
kernels where their letters lie (include/nafgpu.h: nafgpu_kmers_build and nafgpu_screen have the rules; no counterpart in the
reference).

A window is k letters (A, C, G, T/U in either case) of one record; its key is the 2k-bit word of its letters, with
`canonical` the lower of that and its reverse complement's, so that a read matches either strand.  The set stores the keys
themselves: membership is exact.  screen() counts, per record, the windows and those whose key is in the set (hits), gives the
span from the first to the last matching window as a region, and flags the records that match (hits >= min_hits and
hits * 100 >= min_percent * windows; with interleaved both mates match when either does).  By default the records that do
NOT match are kept, which is decontamination; keep_matched=True keeps the ones that do, which is baiting.  Decoder.select()
takes the Screens as they are, the kept records whole:

    with Decoder("phix.naf") as ref, ref.kmers(k=31) as phix, Decoder("reads.naf") as dec:
        with dec.screen(phix, interleaved=True) as s, dec.select(s) as clean:
            archive = encode_device(clean, id=True, comment=True, sequence=True, quality=True)

The tables come to the host as memoryviews; numpy.frombuffer(screens.regions(), dtype=REGION) wraps them without a copy."""
import ctypes
from ctypes import byref, c_void_p

from . import _ffi
from .search import REGION

MAX_K = 31


def _raise(rc, err):
    from .decoder import _raise as raise_error
    if rc in (_ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise_error(err)


def _source(source):
    """-> nafgpu_encode_source with the letters and the records of whatever search() takes"""
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    return src


def _kmer_options(k, canonical):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("k: 1 .. %d expected, got %d" % (MAX_K, int(k)))
    return _ffi.KmerOpts(k=int(k), canonical=int(bool(canonical)))


def _screen_options(min_hits, min_percent, interleaved, keep_matched):
    if int(min_hits) < 0:
        raise ValueError("min_hits is not negative")
    if not 0 <= int(min_percent) <= 100:
        raise ValueError("min_percent: 0 .. 100 expected, got %d" % int(min_percent))
    return _ffi.ScreenOpts(keep_matched=int(bool(keep_matched)), interleaved=int(bool(interleaved)), min_percent=int(min_percent), min_hits=int(min_hits))


class KmerSet:
    """What kmers() returns: the distinct k-mers of a source as a table in HBM.  k, canonical, n_windows (the windows of the
    source), n_kmers (their distinct keys; len()), n_bases, n_records, slots (the table's words), ms (the kernels).  It owns
    its table and outlives its source; the table lives until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        self.k, self.canonical = res.k, bool(res.canonical)
        self.n_windows, self.n_kmers, self.n_bases, self.n_records = res.n_windows, res.n_kmers, res.n_bases, res.n_records
        self.slots, self.ms = res.slots, res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed k-mer set.")
        return self._h

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_kmers_free(h)

    def __len__(self):
        return self.n_kmers

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


class Screens:
    """What screen() returns.  n_records, n_matched, n_kept, n_bases, n_windows, n_hits (sums over all records), bases_kept
    (the letters of the kept records), ms (the kernels); windows() and hits() (n_records 64-bit counts), regions()
    (n_records nafgpu_region structs {r, a, b, 0}: from the first matching window's start to the last one's end), match()
    and keep() (n_records bytes) and kept_regions() (the n_kept whole-record regions of the kept records, ascending: what
    Decoder.select() takes) copy a table to the host.  It owns its device buffers and outlives its source and its set; they
    live until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        for name, _ in _ffi.ScreenResult._fields_:
            value = getattr(res, name)
            setattr(self, name, (value or None) if name.startswith("d_") else value)

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed screens.")
        return self._h

    def _table(self, d_ptr, n_bytes):
        handle = self._handle()
        buf = bytearray(int(n_bytes))
        if n_bytes and self._lib.c.nafgpu_screens_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf)

    def windows(self):
        """n_records 64-bit counts: the windows of every record"""
        return self._table(self.d_windows, 8 * self.n_records).cast("Q")

    def hits(self):
        """n_records 64-bit counts: the windows whose key is in the set"""
        return self._table(self.d_hits, 8 * self.n_records).cast("Q")

    def regions(self):
        """n_records x 32 bytes: {record r, a, b, 0}, from the first matching window's start to the last one's end; (0, 0) without a hit"""
        return self._table(self.d_regions, ctypes.sizeof(_ffi.Region) * self.n_records)

    def match(self):
        """n_records bytes: 1 = the record (or, interleaved, its mate) matches the set"""
        return self._table(self.d_match, self.n_records).cast("B")

    def keep(self):
        """n_records bytes: 1 = kept"""
        return self._table(self.d_keep, self.n_records).cast("B")

    def kept_regions(self):
        """n_kept x 32 bytes: the whole-record regions of the kept records, ascending"""
        return self._table(self.d_kept_regions, ctypes.sizeof(_ffi.Region) * self.n_kept)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_screens_free(h)

    def __len__(self):
        return self.n_records

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


def kmers(source, k=31, canonical=True, *, device=None, _lib=None):
    """The distinct k-mers of records in HBM -> a KmerSet.  `source` is whatever search() takes: what
    Decoder.decode_all_device() returns, a Selection, a ParsedText, or anything with d_sequence / n_bases and d_record_end /
    n_records holding device addresses.  ValueError for what the rules refuse."""
    lib = _lib or _ffi.default()
    opts, src = _kmer_options(k, canonical), _source(source)
    h, res, err = c_void_p(), _ffi.KmersResult(), _ffi.Error()
    rc = lib.c.nafgpu_kmers_build(byref(src), byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return KmerSet(lib, h, res)


def _kmers_decoder(decoder, k, canonical):
    lib = decoder._lib
    opts = _kmer_options(k, canonical)
    h, res, err = c_void_p(), _ffi.KmersResult(), _ffi.Error()
    rc = lib.c.nafgpu_kmers_build_decoder(decoder._h, byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return KmerSet(lib, h, res)


def _set_handle(kmer_set):
    if not isinstance(kmer_set, KmerSet):
        raise ValueError("a KmerSet is expected: %r" % (kmer_set,))
    return kmer_set._handle()


def screen(source, kmer_set, *, min_hits=1, min_percent=0, interleaved=False, keep_matched=False, device=None, _lib=None):
    """Records in HBM against a KmerSet -> Screens.  `source` as for kmers().  min_hits, min_percent: a record matches with
    at least so many hits and so large a share of its windows; interleaved: records 2j and 2j + 1 are mates; keep_matched:
    keep what matches, not what does not.  ValueError for what the rules refuse."""
    lib = _lib or getattr(kmer_set, "_lib", None) or _ffi.default()
    opts, src = _screen_options(min_hits, min_percent, interleaved, keep_matched), _source(source)
    h, res, err = c_void_p(), _ffi.ScreenResult(), _ffi.Error()
    rc = lib.c.nafgpu_screen(byref(src), _set_handle(kmer_set), byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Screens(lib, h, res)


def _screen_decoder(decoder, kmer_set, min_hits, min_percent, interleaved, keep_matched):
    lib = decoder._lib
    opts = _screen_options(min_hits, min_percent, interleaved, keep_matched)
    h, res, err = c_void_p(), _ffi.ScreenResult(), _ffi.Error()
    rc = lib.c.nafgpu_screen_decoder(decoder._h, _set_handle(kmer_set), byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Screens(lib, h, res)


__all__ = ["KmerSet", "Screens", "kmers", "screen", "REGION", "MAX_K"]
