"""Overlaps / overlap -- where read 1 and the reverse complement of read 2 of every pair of mates overlap, found by the HIP
kernels where the letters lie (include/nafgpu.h: nafgpu_overlap has the rules; no counterpart in the reference).

Records 2j and 2j + 1 are mates.  Every shift of read 2's reverse complement against read 1 is compared; a shift is accepted
with min_overlap matching letters, at most max_mismatches mismatches and at most max_mismatch_percent of them; the best is
the one with the fewest mismatches, then the most matches, then the lowest shift.  A found pair says how long the fragment
is, so Decoder.select() takes the Overlaps as they are, every record cut where it reads into the adapter (what `fastp` does
for pairs by default), and Decoder.merge() joins every found pair into one record (`fastp -m`, FLASH, `bbmerge`):

    with Decoder("pairs.naf") as dec, dec.overlap() as o, dec.merge(o) as merged, dec.select(o.unmerged_regions()) as rest:
        archive = encode_device(merged, quality=True, ...)

The tables come to the host as memoryviews; numpy.frombuffer(overlaps.pairs(), dtype=PAIR) wraps them without a copy."""
import ctypes
from ctypes import byref, c_void_p

from . import _ffi
from .search import REGION

MAX_LENGTH = 1024

# numpy.dtype(PAIR): the layout of nafgpu_pair_overlap
PAIR = [("shift", "<i8"), ("insert", "<u8"), ("matches", "<u4"), ("mismatches", "<u4"), ("compared", "<u4"), ("found", "u1"), ("too_long", "u1"),
        ("reserved", "u1", (2,))]


def _raise(rc, err):
    from .decoder import _raise as raise_error
    if rc in (_ffi.E_INVALID_ARG, _ffi.E_INVALID_LENGTH):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise_error(err)


def _options(min_overlap, max_mismatches, max_mismatch_percent, quality_base):
    """-> nafgpu_overlap_opts"""
    for name, value, top in (("min_overlap", min_overlap, 2 ** 32 - 1), ("max_mismatches", max_mismatches, 2 ** 32 - 1),
                             ("max_mismatch_percent", max_mismatch_percent, 100), ("quality_base", quality_base, 255)):
        if not 0 <= int(value) <= top:
            raise ValueError("%s: 0 .. %d expected, got %d" % (name, top, value))
    return _ffi.OverlapOpts(min_overlap=int(min_overlap), max_mismatches=int(max_mismatches), max_mismatch_percent=int(max_mismatch_percent),
                            quality_base=int(quality_base))


class Overlaps:
    """What overlap() returns.  n_records, n_pairs, n_found, n_too_long (pairs with a mate of more than 1 024 letters: not
    analysed), n_unmerged (the records of the pairs not found), n_cut (records whose region is shorter than the record),
    n_bases, matches, mismatches and bases_merged (sums over the found pairs), bases_after_cut (the letters of all regions),
    ms (the kernels); pairs() (n_pairs nafgpu_pair_overlap structs, 32 bytes each: numpy dtype PAIR), regions() (n_records
    nafgpu_region structs {r, 0, min(L, insert), 0}: what Decoder.select() takes) and unmerged_regions() (the whole records of
    the pairs not found, ascending) copy a table to the host.  It owns its device buffers and outlives its source; they live
    until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        self.d_pairs, self.d_regions, self.d_unmerged_regions = res.d_pairs or None, res.d_regions or None, res.d_unmerged_regions or None
        for name in ("n_records", "n_pairs", "n_bases", "n_found", "n_too_long", "n_unmerged", "n_cut", "matches", "mismatches", "bases_merged",
                     "bases_after_cut", "ms"):
            setattr(self, name, getattr(res, name))

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed overlaps.")
        return self._h

    def _table(self, d_ptr, n_bytes):
        handle = self._handle()
        buf = bytearray(int(n_bytes))
        if n_bytes and self._lib.c.nafgpu_overlaps_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf)

    def pairs(self):
        """n_pairs x 32 bytes: shift, insert, matches, mismatches, compared, found, too_long; all 0 for a pair not found"""
        return self._table(self.d_pairs, ctypes.sizeof(_ffi.PairOverlap) * self.n_pairs)

    def regions(self):
        """n_records x 32 bytes: {record r, 0, min(L, insert), 0} when r's pair is found, else the whole record"""
        return self._table(self.d_regions, ctypes.sizeof(_ffi.Region) * self.n_records)

    def unmerged_regions(self):
        """n_unmerged x 32 bytes: the whole-record regions of both mates of every pair not found, ascending"""
        return self._table(self.d_unmerged_regions, ctypes.sizeof(_ffi.Region) * self.n_unmerged)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_overlaps_free(h)

    def __len__(self):
        return self.n_pairs

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


def overlap(source, *, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, quality_base=33, device=None, _lib=None):
    """Paired records in HBM -> the Overlaps of their mates.  `source` is whatever trim() takes: what
    Decoder.decode_all_device() returns, a Selection, a ParsedText, or anything with d_sequence / n_bases and d_record_end /
    n_records holding device addresses; records 2j and 2j + 1 are mates.  quality_base is what Decoder.merge() writes the
    quality of disagreeing letters from.  ValueError for what the rules refuse."""
    lib = _lib or _ffi.default()
    opts = _options(min_overlap, max_mismatches, max_mismatch_percent, quality_base)
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    h, res, err = c_void_p(), _ffi.OverlapResult(), _ffi.Error()
    rc = lib.c.nafgpu_overlap(byref(src), byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Overlaps(lib, h, res)


def _overlap_decoder(decoder, min_overlap, max_mismatches, max_mismatch_percent, quality_base):
    lib = decoder._lib
    opts = _options(min_overlap, max_mismatches, max_mismatch_percent, quality_base)
    h, res, err = c_void_p(), _ffi.OverlapResult(), _ffi.Error()
    rc = lib.c.nafgpu_overlap_decoder(decoder._h, byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Overlaps(lib, h, res)


__all__ = ["Overlaps", "overlap", "REGION", "PAIR", "MAX_LENGTH"]
