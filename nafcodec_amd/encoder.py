"""Encoder -- same names, arguments and error behaviour as the reference's Python API
(nafcodec-py/nafcodec/lib.pyi:69-87, lib.rs:463-600; the Rust side: encoder/mod.rs:46-384).  Host code, like the
reference's; every section is written as Huffman-literal Zstandard blocks (include/nafgpu.h: Encoder).  With `device=` the
sections of compression levels 1 and 2 are compressed by the HIP kernels instead (same bytes), and `encode_device` writes
an archive from records that are already in HBM.  `device_lz=True` lets those device calls take the levels with LZ matches
(0 and >= 3) as well: the matches are found on the GPU, and the archive is a valid one of its own, not the host's bytes.  `parse_text` makes such records from FASTA / FASTQ text on the device, and
`encode_text` is both in one call: file in, archive out.  `mask=True` (no counterpart in the reference, whose mask writer is
commented out) accepts lower-case nucleotides and writes their runs as a Mask section."""
import ctypes
import os
from ctypes import byref, c_uint64, c_void_p

from . import _ffi
from .decoder import SEQUENCE_TYPES, Record


class Encoder:
    """lib.pyi:69-87.  `file` is a path or a binary file-like object; the archive is written by close()."""

    def __init__(self, file, sequence_type="dna", *, id=False, comment=False, sequence=False, quality=False,
                 compression_level=0, device=None, mask=False, device_lz=False, _lib=None):
        if sequence_type not in SEQUENCE_TYPES:
            raise ValueError("expected 'dna', 'rna', 'protein' or 'text', got %r" % (sequence_type,))   # lib.rs:487-495
        _check_mask(mask, sequence_type, sequence)
        self._lib = _lib or _ffi.default()
        self._file = file
        self._h = None
        if not isinstance(file, (str, bytes, os.PathLike)) and not hasattr(file, "write"):
            raise TypeError("expected a path or a binary file-like object")
        opts = _ffi.EncoderOpts()
        self._lib.c.nafgpu_encoder_opts_default(SEQUENCE_TYPES.index(sequence_type), byref(opts))
        opts.id, opts.comment, opts.sequence, opts.quality = map(int, (id, comment, sequence, quality))
        opts.compression_level, opts.mask = int(compression_level), int(bool(mask))
        opts.device_lz = int(bool(device_lz))                # read by the device calls only
        h, err = c_void_p(), _ffi.Error()
        if self._lib.c.nafgpu_encoder_new(byref(opts), byref(h), byref(err)) != _ffi.OK:
            raise _ffi.NafError.from_c(err)
        self._h = h
        if device is not None:                               # an int: the sections are compressed on that GPU (levels 1 and 2; device_lz: any)
            rc = self._lib.c.nafgpu_encoder_set_device(h, int(device))
            if rc != _ffi.OK:
                self._h = None
                self._lib.c.nafgpu_encoder_free(h)
                if rc == _ffi.E_INVALID_ARG:
                    raise ValueError("device encoding writes literal-only blocks: compression_level 1 or 2 (or device_lz=True), "
                                     "and an existing device")
                raise _ffi.NafError(rc, message="no usable HIP device")
        if isinstance(file, (str, bytes, os.PathLike)):      # fail now, as the reference does when it creates the file
            self._out = open_binary(file)
        else:
            self._out = None

    def write(self, record):
        """lib.pyi:85 -- push one record; ValueError for a missing field, an inconsistent length or an invalid letter
        (lib.rs:39-52)."""
        if self._h is None:
            raise RuntimeError("operation on closed encoder.")                         # lib.rs:584
        rec, keep = _ffi.Record(), []
        for name in ("id", "comment", "sequence", "quality"):
            value = getattr(record, name)
            if value is None:
                continue
            data = value.encode("utf-8") if isinstance(value, str) else bytes(value)
            buf = ctypes.create_string_buffer(data, len(data)) if data else ctypes.create_string_buffer(1)
            keep.append(buf)
            f = getattr(rec, name)
            f.ptr, f.len, f.present = ctypes.cast(buf, c_void_p), len(data), 1
        if record.length is not None:
            rec.length, rec.has_length = int(record.length), 1
        err = _ffi.Error()
        rc = self._lib.c.nafgpu_encoder_push(self._h, byref(rec), byref(err))
        if rc in (_ffi.E_MISSING_FIELD, _ffi.E_INVALID_LENGTH, _ffi.E_INVALID_SEQUENCE):
            raise ValueError("invalid characters found in sequence" if rc == _ffi.E_INVALID_SEQUENCE
                             else err.message.decode("utf-8", "replace"))
        if rc != _ffi.OK:
            raise _ffi.NafError.from_c(err)

    def close(self):
        """lib.pyi:86 -- build the archive (Encoder::write, mod.rs:325-384) and write it to the file."""
        if self._h is None:
            return
        h, self._h = self._h, None
        try:
            p, n, err = c_void_p(), c_uint64(), _ffi.Error()
            if self._lib.c.nafgpu_encoder_finish(h, byref(p), byref(n), byref(err)) != _ffi.OK:
                raise _ffi.NafError.from_c(err)
            data = ctypes.string_at(p, n.value)
            if self._out is not None:
                with self._out as f:
                    f.write(data)
            else:
                self._file.write(data)
        finally:
            self._lib.c.nafgpu_encoder_free(h)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()
        return False

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                self._lib.c.nafgpu_encoder_free(self._h)
            except Exception:
                pass
            self._h = None


def zstd_compress(data, device=0, lz=False, _lib=None):
    """One section's bytes -> the magicless Zstandard frame the Encoder writes for it at compression_level 1, on the GPU.
    `lz=True`: a frame of blocks with LZ sequences instead, the device matcher's own (what device_lz=True writes)."""
    return (_lib or _ffi.default()).zstd_compress(bytes(data), device, lz)


def _check_mask(mask, sequence_type, sequence):
    if mask and (sequence_type not in ("dna", "rna") or not sequence):
        raise ValueError("mask=True needs a nucleotide sequence: sequence=True and sequence_type 'dna' or 'rna'")


def encode_device(result, *, sequence_type="dna", id=False, comment=False, sequence=False, quality=False, compression_level=1,
                  device=None, threads=0, mask=False, device_lz=False, _lib=None):
    """Records in HBM -> an archive (bytes), equal to what Encoder writes when the same records are pushed one by one
    (`device_lz=True` at compression_level 0 or >= 3: equal to Encoder(device=, device_lz=True)'s).
    `result` is what Decoder.decode_all_device() returns, or anything with its fields (d_sequence / n_bases, d_quality /
    n_quality, d_record_end / n_records, d_ids / n_ids_bytes, d_comments / n_comments_bytes) holding device addresses --
    a torch tensor's data_ptr() will do.  Only the enabled fields are read.  `mask=True`: the letters may be lower case, as
    decode_all_device() leaves them; the Mask section is made from their case on the device."""
    if sequence_type not in SEQUENCE_TYPES:
        raise ValueError("expected 'dna', 'rna', 'protein' or 'text', got %r" % (sequence_type,))
    _check_mask(mask, sequence_type, sequence)
    lib = _lib or _ffi.default()
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(SEQUENCE_TYPES.index(sequence_type), byref(opts))
    opts.id, opts.comment, opts.sequence, opts.quality = map(int, (id, comment, sequence, quality))
    opts.compression_level, opts.threads, opts.mask = int(compression_level), int(threads), int(bool(mask))
    opts.device_lz = int(bool(device_lz))
    src = _ffi.EncodeSource()
    src.n_records, src.d_record_end = int(result.n_records), result.d_record_end
    if id:
        src.d_ids, src.n_ids_bytes = result.d_ids, int(result.n_ids_bytes)
    if comment:
        src.d_comments, src.n_comments_bytes = result.d_comments, int(result.n_comments_bytes)
    if sequence:
        src.d_sequence, src.n_bases = result.d_sequence, int(result.n_bases)
    if quality:
        src.d_quality, src.n_quality = result.d_quality, int(result.n_quality)
    p, n, err = c_void_p(), c_uint64(), _ffi.Error()
    rc = lib.c.nafgpu_encode_device(byref(src), byref(opts), -1 if device is None else int(device), byref(p), byref(n), byref(err))
    if rc in (_ffi.E_MISSING_FIELD, _ffi.E_INVALID_LENGTH, _ffi.E_INVALID_SEQUENCE, _ffi.E_INVALID_ARG):
        raise ValueError(err.message.decode("utf-8", "replace"))
    if rc != _ffi.OK:
        raise _ffi.NafError.from_c(err)
    try:
        return ctypes.string_at(p, n.value)
    finally:
        lib.c.nafgpu_encode_free(p)


_FORMATS = {None: 0, "auto": 0, "fasta": 1, "fastq": 2}


def _text_argument(data, n, lib):
    """-> (pointer argument, length, on device, what to keep alive)"""
    if isinstance(data, int):                                # a device address, e.g. TextResult.d_text or a tensor's data_ptr()
        if n is None:
            raise TypeError("a device pointer needs its length: parse_text(ptr, n)")
        return c_void_p(data), int(n), 1, None
    data = bytes(data) if not isinstance(data, bytes) else data
    n = len(data) if n is None else int(n)
    if n > len(data):
        raise ValueError("n is larger than the text")
    return ctypes.cast(ctypes.c_char_p(data), c_void_p), n, 0, data


def _raise_text_error(rc, err):
    if rc in (_ffi.E_MISSING_FIELD, _ffi.E_INVALID_LENGTH, _ffi.E_INVALID_SEQUENCE, _ffi.E_INVALID_ARG):
        raise ValueError(err.message.decode("utf-8", "replace"))
    raise _ffi.NafError.from_c(err)


class ParsedText:
    """What parse_text() returns: the records of a FASTA / FASTQ text in HBM, with the fields encode_device() reads
    (d_sequence / n_bases, d_quality / n_quality, d_record_end / n_records, d_ids / n_ids_bytes, d_comments /
    n_comments_bytes), and line_length (the longest sequence line), fastq, n_text, ms (the parse kernels).  The device
    buffers live until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        for name, _ in _ffi.EncodeSource._fields_:
            setattr(self, name, getattr(res.src, name))
        self.d_quality = self.d_quality or None
        self.line_length, self.n_text, self.fastq, self.ms = res.line_length, res.n_text, bool(res.fastq), res.ms

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed parse result.")
        return self._h

    def copy_to_host(self, d_ptr, n):
        buf = ctypes.create_string_buffer(max(int(n), 1))
        if self._lib.c.nafgpu_parse_copy_to_host(self._handle(), d_ptr, int(n), buf) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return buf.raw[:int(n)]

    def hash_device(self, d_ptr, n):
        out = c_uint64()
        if self._lib.c.nafgpu_parse_hash64(self._handle(), d_ptr, int(n), byref(out)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="hashing a device buffer failed")
        return out.value

    def summarize(self, classes=None, *, device=None):
        """Per-record letter counts and quality sums of the parsed records -> a Summary (nafcodec_amd.summary)."""
        from .summary import summarize
        self._handle()
        return summarize(self, classes, device=device, _lib=self._lib)

    def search(self, patterns, *, max_mismatches=0, both_strands=None, alphabet=None, max_hits=0, device=None):
        """Where `patterns` occur in the parsed records -> Hits (nafcodec_amd.search)."""
        from .search import search
        self._handle()
        return search(self, patterns, max_mismatches=max_mismatches, both_strands=both_strands, alphabet=alphabet, max_hits=max_hits, device=device,
                      _lib=self._lib)

    def group(self, *, both_strands=False, alphabet=None, device=None):
        """The parsed records whose sequences are equal -> Groups (nafcodec_amd.group)."""
        from .group import group
        self._handle()
        return group(self, both_strands=both_strands, alphabet=alphabet, device=device, _lib=self._lib)

    def trim(self, *, cut_front=0, cut_tail=0, window=None, trim_n=False, min_length=0, interleaved=False, quality_base=33, device=None):
        """The window of every parsed record that quality trimming keeps -> Trims (nafcodec_amd.trim)."""
        from .trim import trim
        self._handle()
        return trim(self, cut_front=cut_front, cut_tail=cut_tail, window=window, trim_n=trim_n, min_length=min_length, interleaved=interleaved,
                    quality_base=quality_base, device=device, _lib=self._lib)

    def kmers(self, k=31, canonical=True, *, device=None):
        """The distinct k-mers of the parsed records -> a KmerSet (nafcodec_amd.screen)."""
        from .screen import kmers
        self._handle()
        return kmers(self, k, canonical, device=device, _lib=self._lib)

    def screen(self, kmer_set, *, min_hits=1, min_percent=0, interleaved=False, keep_matched=False, device=None):
        """The parsed records against a KmerSet -> Screens (nafcodec_amd.screen)."""
        from .screen import screen
        self._handle()
        return screen(self, kmer_set, min_hits=min_hits, min_percent=min_percent, interleaved=interleaved, keep_matched=keep_matched, device=device,
                      _lib=self._lib)

    def overlap(self, *, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, quality_base=33, device=None):
        """Where the mates of every parsed pair (records 2j and 2j + 1) overlap -> Overlaps (nafcodec_amd.overlap); their
        records are the parsed ones."""
        from .overlap import overlap
        self._handle()
        return overlap(self, min_overlap=min_overlap, max_mismatches=max_mismatches, max_mismatch_percent=max_mismatch_percent,
                       quality_base=quality_base, device=device, _lib=self._lib)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_parse_free(h)

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


def parse_text(data, n=None, *, format=None, device=None, _lib=None):
    """FASTA / FASTQ text -> records in HBM, parsed by the HIP kernels (include/nafgpu.h: nafgpu_parse_text has the rules).
    `data`: bytes-like, or a device address (an int) with its length `n`, which is read where it lies.  `format`: None /
    "auto" (by the first byte), "fasta" or "fastq".  ValueError for a text the rules refuse."""
    if format not in _FORMATS:
        raise ValueError("expected None, 'auto', 'fasta' or 'fastq', got %r" % (format,))
    lib = _lib or _ffi.default()
    ptr, n, on_device, keep = _text_argument(data, n, lib)
    opts = _ffi.ParseOpts(format=_FORMATS[format], text_on_device=on_device)
    h, res, err = c_void_p(), _ffi.ParseResult(), _ffi.Error()
    rc = lib.c.nafgpu_parse_text(ptr, n, byref(opts), -1 if device is None else int(device), byref(h), byref(res), byref(err))
    del keep
    if rc != _ffi.OK:
        _raise_text_error(rc, err)
    return ParsedText(lib, h, res)


def encode_text(data, *, sequence_type="dna", id=True, comment=True, sequence=True, quality=None, mask=False, compression_level=1,
                keep_line_length=True, format=None, device=None, threads=0, device_lz=False, _lib=None):
    """FASTA / FASTQ text (bytes-like) -> an archive (bytes): parse_text and encode_device in one call, what `ennaf` does.
    `quality=None`: written if the text is FASTQ.  `keep_line_length=False`: the header says 60, and the archive is byte
    for byte what Encoder writes for the same records."""
    if sequence_type not in SEQUENCE_TYPES:
        raise ValueError("expected 'dna', 'rna', 'protein' or 'text', got %r" % (sequence_type,))
    if format not in _FORMATS:
        raise ValueError("expected None, 'auto', 'fasta' or 'fastq', got %r" % (format,))
    _check_mask(mask, sequence_type, sequence)
    lib = _lib or _ffi.default()
    ptr, n, on_device, keep = _text_argument(data, None, lib)
    if quality is None:
        quality = bytes(data[:1]) == b"@" if format in (None, "auto") else format == "fastq"
    popts = _ffi.ParseOpts(format=_FORMATS[format], text_on_device=on_device)
    opts = _ffi.EncoderOpts()
    lib.c.nafgpu_encoder_opts_default(SEQUENCE_TYPES.index(sequence_type), byref(opts))
    opts.id, opts.comment, opts.sequence, opts.quality = map(int, (id, comment, sequence, quality))
    opts.compression_level, opts.threads, opts.mask = int(compression_level), int(threads), int(bool(mask))
    opts.device_lz = int(bool(device_lz))
    p, n_out, err = c_void_p(), c_uint64(), _ffi.Error()
    rc = lib.c.nafgpu_encode_text(ptr, n, byref(popts), byref(opts), int(bool(keep_line_length)), -1 if device is None else int(device),
                                  byref(p), byref(n_out), byref(err))
    del keep
    if rc != _ffi.OK:
        _raise_text_error(rc, err)
    try:
        return ctypes.string_at(p, n_out.value)
    finally:
        lib.c.nafgpu_encode_free(p)


def open_binary(path):
    import builtins
    return builtins.open(os.fspath(path), "wb")


__all__ = ["Encoder", "ParsedText", "Record", "encode_device", "encode_text", "parse_text", "zstd_compress"]
