"""Groups / group -- which records that are in HBM have equal sequences (PCR duplicates in reads, dereplication of amplicons,
identical contigs), found by the HIP kernels (include/nafgpu.h: nafgpu_group has the rules; no counterpart in the
reference).  No letter comes to the host: every record is hashed, looked up and compared with its representative letter by
letter on the device.

Decoder.select() takes the Groups as they are, the first record of every sequence:

    with Decoder("reads.naf") as dec, dec.group() as g, dec.select(g) as unique:
        archive = encode_device(unique, id=True, comment=True, sequence=True, quality=True)

The tables come to the host as memoryviews; numpy.frombuffer wraps them without a copy.  The members of every group:
numpy.argsort(group_of, kind="stable") cut at the cumulative sums of group_size."""
import ctypes
from array import array
from ctypes import byref, c_void_p

from . import _ffi

NUCLEOTIDE, BYTES = 0, 1


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


class Groups:
    """What group() returns.  n_records, n_groups, n_duplicates (records that are not the first of their sequence),
    largest_group, n_bases, rounds (table rounds: 1 unless hashes collided), ms (the kernels); representative() (per record the
    lowest record with an equal sequence), group_of(), group_first() (the representatives, ascending), group_size() copy a
    table of 64-bit words to the host, strand() one of bytes (1: equal to the representative only as its reverse complement;
    None without both_strands).  It owns its device buffers and outlives its source; they live until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        for name in ("d_representative", "d_group_of", "d_strand", "d_group_first", "d_group_size"):
            setattr(self, name, getattr(res, name) or None)
        self.n_records, self.n_groups, self.n_bases, self.largest_group = res.n_records, res.n_groups, res.n_bases, res.largest_group
        self.n_duplicates = res.n_records - res.n_groups
        self.rounds, self.ms = res.rounds, res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed groups.")
        return self._h

    def _table(self, d_ptr, n_bytes):
        handle = self._handle()
        buf = bytearray(int(n_bytes))
        if n_bytes and self._lib.c.nafgpu_groups_copy_to_host(handle, d_ptr, len(buf), (ctypes.c_uint8 * len(buf)).from_buffer(buf)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return memoryview(buf)

    def representative(self):
        """n_records words: the lowest record whose sequence equals this one's (the record itself if it is the first)"""
        return self._table(self.d_representative, 8 * self.n_records).cast("Q")

    def group_of(self):
        """n_records words: the index of the record's group"""
        return self._table(self.d_group_of, 8 * self.n_records).cast("Q")

    def strand(self):
        """n_records bytes: 1 = equal to the representative only as its reverse complement; None without both_strands"""
        if self.d_strand is None:
            self._handle()
            return None
        return self._table(self.d_strand, self.n_records).cast("B")

    def group_first(self):
        """n_groups words: the representatives, ascending"""
        return self._table(self.d_group_first, 8 * self.n_groups).cast("Q")

    def group_size(self):
        """n_groups words: the records of every group"""
        return self._table(self.d_group_size, 8 * self.n_groups).cast("Q")

    def _regions(self):
        """the representatives as whole records: a buffer of nafgpu_region structs for Decoder.select()"""
        first = self.group_first()
        words = memoryview(bytearray(ctypes.sizeof(_ffi.Region) * len(first))).cast("Q")
        if len(first):
            words[0::4] = first                              # {record, start 0, end = the record's length, forward}
            words[2::4] = memoryview(array("Q", [_ffi.REGION_END]) * len(first))
        return words.cast("B")

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_groups_free(h)

    def __len__(self):
        return self.n_groups

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


def group(source, *, both_strands=False, alphabet=None, device=None, _lib=None):
    """Records in HBM -> the Groups of records whose sequences are equal.  `source` is whatever search() takes: what
    Decoder.decode_all_device() returns, a Selection, a ParsedText, or anything with d_sequence / n_bases and d_record_end /
    n_records holding device addresses.  alphabet: "nucleotide" (None: the same; letters are equal by their 4-bit codes, so
    case and T/U are ignored) or "bytes"; both_strands: a record also equals its reverse complement.  ValueError for what the
    rules refuse."""
    lib = _lib or _ffi.default()
    opts = _ffi.GroupOpts(alphabet=_alphabet(alphabet), both_strands=int(bool(both_strands)))
    src = _ffi.EncodeSource()
    src.d_sequence, src.n_bases = getattr(source, "d_sequence", None) or None, int(getattr(source, "n_bases", 0))
    src.d_record_end, src.n_records = getattr(source, "d_record_end", None) or None, int(getattr(source, "n_records", 0))
    h, res, err = c_void_p(), _ffi.GroupResult(), _ffi.Error()
    rc = lib.c.nafgpu_group(byref(src), byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Groups(lib, h, res)


def _group_decoder(decoder, both_strands, alphabet):
    lib = decoder._lib
    if alphabet is None:                                     # by the archive: dna and rna as nucleotides, protein and text as bytes
        alphabet = NUCLEOTIDE if decoder._header.sequence_type <= 1 else BYTES
    opts = _ffi.GroupOpts(alphabet=_alphabet(alphabet), both_strands=int(bool(both_strands)))
    h, res, err = c_void_p(), _ffi.GroupResult(), _ffi.Error()
    rc = lib.c.nafgpu_group_decoder(decoder._h, byref(opts), byref(h), byref(res), byref(err))
    if rc != _ffi.OK:
        _raise(rc, err)
    return Groups(lib, h, res)


__all__ = ["Groups", "group", "NUCLEOTIDE", "BYTES"]
