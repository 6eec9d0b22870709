"""Summary / summarize -- per-record letter counts, quality sums and section histograms of records that are in HBM, counted
by the HIP kernels (include/nafgpu.h: nafgpu_summarize has the rules; no counterpart in the reference).

The tables come to the host as memoryviews of 64-bit words (format "Q"); numpy.frombuffer wraps them without a copy:

    s = decoder.summarize()
    counts = numpy.frombuffer(s.counts(), dtype=numpy.uint64).reshape(-1, 8)
    gc = (counts[:, C] + counts[:, G]) / numpy.maximum(counts[:, :OTHER + 1].sum(axis=1), 1)
    picked = decoder.select([int(k) for k in numpy.nonzero(gc > 0.6)[0]])"""
import ctypes
from ctypes import byref, c_void_p

from . import _ffi

A, C, G, T, N, IUPAC, OTHER, LOWER = range(8)         # the columns of the default table


def _default_classes():
    table = bytearray([1 << OTHER]) * 256
    for column, letters in ((A, b"A"), (C, b"C"), (G, b"G"), (T, b"TU"), (N, b"N"), (IUPAC, b"RYKMSWBDHV")):
        for b in letters:
            table[b] = table[b | 0x20] = 1 << column
    for b in range(ord("a"), ord("z") + 1):
        table[b] |= 1 << LOWER
    return bytes(table)


DEFAULT_CLASSES = _default_classes()


def _opts(classes):
    if classes is None:
        return None
    classes = bytes(classes)
    if len(classes) != 256:
        raise ValueError("classes: 256 bytes expected (one mask of eight columns per byte value), got %d" % len(classes))
    opts = _ffi.SummaryOpts(use_classes=1)
    ctypes.memmove(opts.classes, classes, 256)
    return byref(opts)


def _raise(rc, err):
    from .decoder import _raise as raise_error
    if rc in (_ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise_error(err)


class Summary:
    """What summarize() returns.  n_records, n_bases, n_quality; totals (the eight column sums over all records),
    quality_total, ms (the summary kernels); counts(), quality_sum(), letter_hist(), quality_hist() copy a table to the
    host (None for a table the source has no field for).  It owns its device buffers and outlives its source; they live
    until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        self.d_counts, self.d_quality_sum = res.d_counts or None, res.d_quality_sum or None
        self.d_letter_hist, self.d_quality_hist = res.d_letter_hist or None, res.d_quality_hist or None
        self.n_records, self.n_bases, self.n_quality = res.n_records, res.n_bases, res.n_quality
        self.totals, self.quality_total, self.ms = tuple(res.totals), res.quality_total, res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed summary.")
        return self._h

    def _words(self, d_ptr, n):
        handle = self._handle()
        if d_ptr is None:
            return None
        buf = bytearray(8 * int(n))
        if n and self._lib.c.nafgpu_summary_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf).cast("Q")

    def counts(self):
        """n_records x 8 words, row-major: row k holds the eight columns of record k"""
        return self._words(self.d_counts, 8 * self.n_records)

    def quality_sum(self):
        return self._words(self.d_quality_sum, self.n_records)

    def letter_hist(self):
        """256 words: how often each byte value occurs among the letters"""
        return self._words(self.d_letter_hist, 256)

    def quality_hist(self):
        return self._words(self.d_quality_hist, 256)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_summary_free(h)

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


def summarize(source, classes=None, *, device=None, _lib=None):
    """Records in HBM -> a Summary.  `source` is whatever encode_device() takes: what Decoder.decode_all_device() returns, a
    Selection, a ParsedText, or anything with d_sequence / n_bases, d_quality / n_quality, d_record_end / n_records holding
    device addresses.  `classes`: 256 bytes, classes[b] = the columns (bits 0-7) a letter with byte value b counts in;
    None: DEFAULT_CLASSES.  ValueError for what the rules refuse."""
    lib = _lib or _ffi.default()
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_quality, src.n_quality = getattr(source, "d_quality", None) or None, int(getattr(source, "n_quality", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    h, res, err = c_void_p(), _ffi.SummaryResult(), _ffi.Error()
    rc = lib.c.nafgpu_summarize(byref(src), _opts(classes), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Summary(lib, h, res)


def _summarize_decoder(decoder, classes):
    lib = decoder._lib
    h, res, err = c_void_p(), _ffi.SummaryResult(), _ffi.Error()
    rc = lib.c.nafgpu_summarize_decoder(decoder._h, _opts(classes), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Summary(lib, h, res)


__all__ = ["Summary", "summarize", "DEFAULT_CLASSES", "A", "C", "G", "T", "N", "IUPAC", "OTHER", "LOWER"]
