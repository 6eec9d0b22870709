"""Trims / trim -- the window of every record that quality trimming keeps, found by the HIP kernels where letters and
qualities lie (include/nafgpu.h: nafgpu_trim has the rules; no counterpart in the reference).

Four steps, each on what the one before left: the running-sum rule of `cutadapt -q FRONT,TAIL` and `bwa -q` (cut_front,
cut_tail), the first sliding window whose mean quality is below Q (window=(W, Q): the cut point of the 5'-to-3' window
trimmers, without their clean-up afterwards), N at either end (trim_n), and a length filter (min_length; with interleaved
both mates of a pair go when one does).  Decoder.select() takes the Trims as they are, the kept records cut to their windows:

    with Decoder("reads.naf") as dec, dec.trim(cut_tail=20, trim_n=True, min_length=30) as t, dec.select(t) as cleaned:
        archive = encode_device(cleaned, quality=True, ...)

The tables come to the host as memoryviews; numpy.frombuffer(trims.regions(), dtype=REGION) wraps them without a copy."""
import ctypes
from ctypes import byref, c_void_p

from . import _ffi
from .search import REGION

MAX_WINDOW = 64


def _raise(rc, err):
    from .decoder import _raise as raise_error
    if rc in (_ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise_error(err)


def _options(cut_front, cut_tail, window, trim_n, min_length, interleaved, quality_base):
    """-> nafgpu_trim_opts"""
    w, q = (0, 0) if window is None else (int(window[0]), int(window[1]))
    values = dict(cut_front=int(cut_front), cut_tail=int(cut_tail), window=w, window_quality=q, quality_base=int(quality_base))
    for name, value in values.items():
        if not 0 <= value <= 255:
            raise ValueError("%s: 0 .. 255 expected, got %d" % (name, value))
    if window is not None and not 1 <= w <= MAX_WINDOW:
        raise ValueError("window: (W, Q) with W in 1 .. %d expected, got W = %d" % (MAX_WINDOW, w))
    if int(min_length) < 0:
        raise ValueError("min_length is not negative")
    return _ffi.TrimOpts(trim_n=int(bool(trim_n)), interleaved=int(bool(interleaved)), min_length=int(min_length), **values)


class Trims:
    """What trim() returns.  n_records, n_kept, n_changed (records whose window is not the whole record), n_bases,
    bases_in_windows (the windows' letters, all records), bases_kept (those of the kept records), ms (the kernels);
    regions() (n_records nafgpu_region structs {k, a, b, 0}, 32 bytes each), keep() (n_records bytes, 1 = kept) and
    kept_regions() (the n_kept regions of the kept records, ascending: what Decoder.select() takes) copy a table to the host.
    It owns its device buffers and outlives its source; they live until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        self.d_regions, self.d_keep, self.d_kept_regions = res.d_regions or None, res.d_keep or None, res.d_kept_regions or None
        self.n_records, self.n_kept, self.n_changed, self.n_bases = res.n_records, res.n_kept, res.n_changed, res.n_bases
        self.bases_in_windows, self.bases_kept, self.ms = res.bases_in_windows, res.bases_kept, res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed trims.")
        return self._h

    def _table(self, d_ptr, n_bytes):
        handle = self._handle()
        buf = bytearray(int(n_bytes))
        if n_bytes and self._lib.c.nafgpu_trims_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf)

    def regions(self):
        """n_records x 32 bytes: {record k, a, b, 0}, the window [a, b) relative to the record; an empty one is (0, 0)"""
        return self._table(self.d_regions, ctypes.sizeof(_ffi.Region) * self.n_records)

    def keep(self):
        """n_records bytes: 1 = the record (and, interleaved, its mate) passes min_length"""
        return self._table(self.d_keep, self.n_records).cast("B")

    def kept_regions(self):
        """n_kept x 32 bytes: the regions of the kept records, ascending"""
        return self._table(self.d_kept_regions, ctypes.sizeof(_ffi.Region) * self.n_kept)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_trims_free(h)

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


def trim(source, *, cut_front=0, cut_tail=0, window=None, trim_n=False, min_length=0, interleaved=False, quality_base=33, device=None, _lib=None):
    """Records in HBM -> the Trims of their quality trimming.  `source` is whatever search() takes: what
    Decoder.decode_all_device() returns, a Selection, a ParsedText, or anything with d_sequence / n_bases, d_quality /
    n_quality and d_record_end / n_records holding device addresses.  cut_front, cut_tail: the cutoffs of the running sums
    (0: off); window: None or (W, Q) with W in 1 .. 64; trim_n: N at either end goes; min_length: a shorter window is not
    kept; interleaved: records 2j and 2j + 1 are mates.  ValueError for what the rules refuse."""
    lib = _lib or _ffi.default()
    opts = _options(cut_front, cut_tail, window, trim_n, min_length, interleaved, quality_base)
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_quality, src.n_quality = getattr(source, "d_quality", None) or None, int(getattr(source, "n_quality", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    h, res, err = c_void_p(), _ffi.TrimResult(), _ffi.Error()
    rc = lib.c.nafgpu_trim(byref(src), byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Trims(lib, h, res)


def _trim_decoder(decoder, cut_front, cut_tail, window, trim_n, min_length, interleaved, quality_base):
    lib = decoder._lib
    opts = _options(cut_front, cut_tail, window, trim_n, min_length, interleaved, quality_base)
    h, res, err = c_void_p(), _ffi.TrimResult(), _ffi.Error()
    rc = lib.c.nafgpu_trim_decoder(decoder._h, byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Trims(lib, h, res)


__all__ = ["Trims", "trim", "REGION", "MAX_WINDOW"]
