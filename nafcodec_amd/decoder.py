"""Decoder / Record / open -- same names, arguments and error behaviour as the reference's Python
API (nafcodec-py/nafcodec/lib.pyi:18-67, lib.rs:324-461, error mapping lib.rs:39-77)."""
import ctypes
import errno as _errno
import io
import os
from ctypes import byref, c_void_p

from . import _ffi

SEQUENCE_TYPES = ("dna", "rna", "protein", "text")


class Record:
    """lib.pyi:18-33 -- five optional fields."""
    __slots__ = ("id", "comment", "sequence", "quality", "length")

    def __init__(self, *, id=None, comment=None, sequence=None, quality=None, length=None):
        self.id, self.comment, self.sequence, self.quality, self.length = id, comment, sequence, quality, length

    def __repr__(self):
        args = ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__ if getattr(self, k) is not None)
        return "Record(%s)" % args


def _raise(err):
    """Error -> Python exception, as nafcodec-py/nafcodec/lib.rs:39-77 does."""
    e = _ffi.NafError.from_c(err)
    if e.status == _ffi.E_IO:
        if e.io_kind == _ffi.IO_NOT_FOUND:
            raise FileNotFoundError(e.os_errno or _errno.ENOENT, e.message)
        if e.io_kind == _ffi.IO_IS_A_DIRECTORY:
            raise IsADirectoryError(e.os_errno or _errno.EISDIR, e.message)
        if e.io_kind == _ffi.IO_PERMISSION_DENIED:
            raise PermissionError(e.os_errno or _errno.EACCES, e.message)
        if e.io_kind == _ffi.IO_UNEXPECTED_EOF:
            raise EOFError(e.message)
        raise OSError(e.os_errno, e.message)
    if e.status in (_ffi.E_NOM, _ffi.E_UTF8):
        raise ValueError(e.message)
    raise e


class Decoder:
    """lib.pyi:35-67.  `file` is a path or a binary file-like object."""

    def __init__(self, file, *, id=True, comment=True, sequence=True, quality=True, mask=True, buffer_size=None,
                 device=-1, spec_mask=False, shard_rank=0, shard_count=1, shard_protocol=False, _lib=None):
        self._lib = _lib or _ffi.default()
        self._h = None
        self._pending_error = None
        opts = _ffi.Opts()
        self._lib.c.nafgpu_opts_default(byref(opts))
        opts.id, opts.comment, opts.sequence, opts.quality, opts.mask = map(int, (id, comment, sequence, quality, mask))
        opts.spec_mask = int(spec_mask)
        opts.buffer_size = io.DEFAULT_BUFFER_SIZE if buffer_size is None else int(buffer_size)  # lib.rs:350-354
        opts.device = device
        opts.shard_rank, opts.shard_count = shard_rank, shard_count   # bulk device path only (decode_all_device)
        opts.shard_protocol = int(bool(shard_protocol))               # ... or the shard protocol (nafcodec_amd.sharding)
        h, err = c_void_p(), _ffi.Error()
        if isinstance(file, (str, bytes, os.PathLike)):
            path = os.fsencode(file)
            rc = self._lib.c.nafgpu_open_path(path, byref(opts), byref(h), byref(err))
        else:
            rc = self._open_filelike(file, opts, h, err)
        if rc != _ffi.OK:
            _raise(err)
        self._h = h
        self._header = _ffi.Header()
        self._lib.c.nafgpu_get_header(self._h, byref(self._header))

    def _open_filelike(self, file, opts, h, err):
        """with_reader (mod.rs:169-256) over a Python file-like, as PyFileRead does (pyfile.rs:88-187): the
        library calls back into `readinto` (or `read`) and `seek`; with a working seek it reads only the
        header and the selected sections.  An exception raised by the file object is re-raised as it is."""
        if not (hasattr(file, "readinto") or hasattr(file, "read")):
            raise TypeError("expected a path or a binary file-like object")
        pending = []                                       # exception raised inside a callback

        def on_read(_ctx, buf, cap):
            try:
                cap = int(cap)
                if hasattr(file, "readinto"):              # pyfile.rs:88-132
                    view = (ctypes.c_uint8 * cap).from_address(ctypes.addressof(buf.contents))
                    n = file.readinto(memoryview(view).cast("B"))
                    return int(n or 0)
                data = file.read(cap)                      # pyfile.rs:134-187
                if not isinstance(data, (bytes, bytearray, memoryview)):
                    raise TypeError("expected bytes from read(), found %s" % type(data).__name__)
                if len(data) > cap:
                    raise OSError(_errno.EIO, "read() returned more bytes than asked for")
                ctypes.memmove(buf, bytes(data), len(data))
                return len(data)
            except BaseException as e:                     # noqa: BLE001 -- carried across the C boundary
                pending.append(e)
                return -(getattr(e, "errno", None) or _errno.EIO)

        def on_seek(_ctx, offset, whence):
            try:
                return int(file.seek(int(offset), int(whence)))
            except BaseException as e:                     # noqa: BLE001
                pending.append(e)
                return -(getattr(e, "errno", None) or _errno.ESPIPE)

        seekable = hasattr(file, "seek")
        try:
            seekable = seekable and (file.seekable() if hasattr(file, "seekable") else True)
        except Exception:
            seekable = False
        read_cb = _ffi.READ_FN(on_read)
        seek_cb = _ffi.SEEK_FN(on_seek) if seekable else _ffi.SEEK_FN()
        rc = self._lib.c.nafgpu_open_io(read_cb, seek_cb, None, byref(opts), byref(h), byref(err))
        if pending and rc != _ffi.OK:
            raise pending[0]
        return rc

    # ---- iteration -----------------------------------------------------------------------
    def __iter__(self):
        return self

    def __next__(self):
        rec = self.read()
        if rec is None:
            raise StopIteration
        return rec

    def read(self):
        """lib.pyi:67 -- the next record, or None at the end of the archive."""
        rec = _ffi.Record()
        rc = self._lib.c.nafgpu_next(self._h, byref(rec))
        if rc == _ffi.END:
            return None
        if rc != _ffi.OK:
            err = _ffi.Error()
            self._lib.c.nafgpu_last_error(self._h, byref(err))
            _raise(err)

        def text(f):
            if not f.present:
                return None
            return ctypes.string_at(f.ptr, f.len).decode("utf-8") if f.len else ""

        return Record(id=text(rec.id), comment=text(rec.comment), sequence=text(rec.sequence),
                      quality=text(rec.quality), length=rec.length if rec.has_length else None)

    def read_batch(self, n=4096):
        """Up to `n` records in ONE call into the library (nafgpu_next_batch): the records `n` calls of read() would return, in
        order; fewer when the archive ends or the next record's bytes are not on the host yet, [] at the end.  An error
        raised by record k of the batch is raised by this call AFTER records 0 .. k-1 were collected: they are returned by
        the call, the exception is kept and raised by the next one (so no record is lost and the order of events is the
        one read() gives)."""
        if self._pending_error is not None:
            e, self._pending_error = self._pending_error, None
            raise e
        recs = (_ffi.Record * n)()
        got = ctypes.c_uint64()
        rc = self._lib.c.nafgpu_next_batch(self._h, recs, n, byref(got))

        def text(f):
            if not f.present:
                return None
            return ctypes.string_at(f.ptr, f.len).decode("utf-8") if f.len else ""

        out = [Record(id=text(r.id), comment=text(r.comment), sequence=text(r.sequence), quality=text(r.quality),
                      length=r.length if r.has_length else None) for r in recs[:got.value]]
        if rc not in (_ffi.OK, _ffi.END):
            err = _ffi.Error()
            self._lib.c.nafgpu_last_error(self._h, byref(err))
            try:
                _raise(err)
            except Exception as e:                          # noqa: BLE001
                if not out:
                    raise
                self._pending_error = e
        return out

    def __len__(self):
        return int(self._lib.c.nafgpu_remaining(self._h))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()
        return False

    def close(self):
        if self._h:
            self._lib.c.nafgpu_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- header properties (lib.pyi:56-66) ---------------------------------------------------
    @property
    def sequence_type(self):
        return SEQUENCE_TYPES[self._header.sequence_type]

    @property
    def format_version(self):
        return "v%d" % self._header.format_version

    @property
    def line_length(self):
        return int(self._header.line_length)

    @property
    def name_separator(self):
        return chr(self._header.name_separator)

    @property
    def number_of_sequences(self):
        return int(self._header.number_of_sequences)

    @property
    def flags(self):
        return int(self._header.flags)

    # ---- bulk device path (no reference counterpart: what `for r in decoder` becomes on a GPU) ----
    def decode_all_device(self):
        """Decode every selected section on the GPU; returns the nafgpu_device_result struct."""
        res = _ffi.DeviceResult()
        rc = self._lib.c.nafgpu_decode_all_device(self._h, byref(res))
        if rc != _ffi.OK:
            err = _ffi.Error()
            self._lib.c.nafgpu_last_error(self._h, byref(err))
            _raise(err)
        return res

    # ---- the shard protocol (include/nafgpu.h: nafgpu_shard_*; nafcodec_amd.sharding drives it) ----
    def _check(self, rc):
        if rc != _ffi.OK:
            err = _ffi.Error()
            self._lib.c.nafgpu_last_error(self._h, byref(err))
            _raise(err)

    def shard_begin(self):
        """-> this rank's 64-byte summary (bytes)"""
        mine = _ffi.ShardSummary()
        self._check(self._lib.c.nafgpu_shard_begin(self._h, byref(mine)))
        return bytes(mine)

    def shard_place(self, summaries):
        """summaries: the ranks' summaries back to back (bytes-like, 64 bytes per rank, rank order)"""
        buf = ctypes.create_string_buffer(bytes(summaries), len(summaries))
        self._check(self._lib.c.nafgpu_shard_place(self._h, ctypes.cast(buf, c_void_p), len(summaries) // ctypes.sizeof(_ffi.ShardSummary)))

    def shard_halo(self, section):
        """-> (recv_bytes, send_bytes, tail_ready) for section 0 (Sequence) / 1 (Quality)"""
        recv, send, ready = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        self._check(self._lib.c.nafgpu_shard_halo(self._h, section, byref(recv), byref(send), byref(ready)))
        return recv.value, send.value, bool(ready.value)

    def shard_export_tail(self, section, ptr, n):
        self._check(self._lib.c.nafgpu_shard_export_tail(self._h, section, ptr, n))

    def shard_import_halo(self, section, ptr, n):
        self._check(self._lib.c.nafgpu_shard_import_halo(self._h, section, ptr, n))

    def shard_finish(self):
        res = _ffi.DeviceResult()
        self._check(self._lib.c.nafgpu_shard_finish(self._h, byref(res)))
        return res

    def format_device(self):
        """FASTA (FASTQ when the archive has qualities and `quality` is selected) text of every record,
        built on the GPU from the decoded buffers; returns the nafgpu_text_result struct (device pointer)."""
        res = _ffi.TextResult()
        rc = self._lib.c.nafgpu_format_device(self._h, byref(res))
        if rc != _ffi.OK:
            err = _ffi.Error()
            self._lib.c.nafgpu_last_error(self._h, byref(err))
            _raise(err)
        return res

    def to_text(self):
        """format_device() copied to the host: the archive as FASTA / FASTQ bytes (what `unnaf` prints)."""
        res = self.format_device()
        return self.copy_to_host(res.d_text, res.n_text)

    def copy_to_host(self, d_ptr, n):
        buf = ctypes.create_string_buffer(int(n)) if n else ctypes.create_string_buffer(1)
        rc = self._lib.c.nafgpu_copy_to_host(self._h, d_ptr, int(n), ctypes.cast(buf, ctypes.c_void_p))
        if rc != _ffi.OK:
            raise RuntimeError("nafgpu_copy_to_host failed: %d" % rc)
        return buf.raw[:int(n)]

    def hash_device(self, d_ptr, n, first_chunk=0):
        out = ctypes.c_uint64()
        rc = self._lib.c.nafgpu_hash64_device_at(self._h, d_ptr, n, first_chunk, byref(out))
        if rc != _ffi.OK:
            raise RuntimeError("nafgpu_hash64_device failed: %d" % rc)
        return out.value

    # ---- records and regions on the device (include/nafgpu.h: nafgpu_select has the rules) ----
    def _raise_select(self, rc, err):
        if rc == _ffi.E_INVALID_ARG:
            raise ValueError(err.message.decode("utf-8", "replace"))
        _raise(err)

    def find(self, names):
        """-> for every name (str or bytes) the index of the first record with that id, or None; looked up on the GPU."""
        blobs = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
        if any(b"\0" in b for b in blobs):
            raise ValueError("a name holds a NUL byte")
        blob = b"".join(b + b"\0" for b in blobs)
        out, err = (ctypes.c_uint64 * max(len(blobs), 1))(), _ffi.Error()
        rc = self._lib.c.nafgpu_find_records(self._h, blob, len(blob), len(blobs), out, byref(err))
        if rc != _ffi.OK:
            self._raise_select(rc, err)
        return [None if v == _ffi.NOT_FOUND else int(v) for v in out[:len(blobs)]]

    def select(self, regions, *, name_regions=False):
        """Records and regions -> a Selection in HBM; region k becomes its record k.  A region is an int (a whole record),
        (record, start, end) with end=None for the record's length, or (record, start, end, "-") for the reverse strand
        (reversed and complemented; "+" is the forward one); `record` may be a name (str / bytes), resolved through find():
        KeyError when no record has it.  name_regions: every id becomes id:START-END (1-based, inclusive) and id:START-END/rc.
        Instead of a list, `regions` may be the Hits of search() or any buffer of whole nafgpu_region structs (32 bytes each:
        bytes, a memoryview, a numpy array of dtype nafcodec_amd.search.REGION): it goes to the library as it is, without a
        Python object per region.  A buffer counts as such when its items are bytes or of 32 bytes; an array of integers is
        a list of records like any other.  The Groups of group() stand for their representatives as whole records, in
        order: the first record of every sequence.  The Trims of trim() stand for their kept regions: every kept record cut
        to its window; the Screens of screen() for theirs: every kept record, whole; the Overlaps of overlap() for their regions:
        every record, cut where it reads into the adapter.  ValueError for what the rules refuse."""
        from .group import Groups
        from .overlap import Overlaps
        from .screen import Screens
        from .trim import Trims
        if isinstance(regions, Groups):
            regions = regions._regions()
        elif isinstance(regions, (Trims, Screens)):
            regions = regions.kept_regions()
        elif isinstance(regions, Overlaps):
            regions = regions.regions()
        packed = self._packed_regions(regions)
        if packed is not None:
            arr, n = packed
            return self._select(arr, n, name_regions)
        regions = [r if isinstance(r, (tuple, list)) else (r, 0, None) for r in regions]
        named = sorted({r[0] for r in regions if isinstance(r[0], (str, bytes))}, key=repr)
        index = dict(zip(named, self.find(named))) if named else {}
        arr = (_ffi.Region * max(len(regions), 1))()
        for k, r in enumerate(regions):
            if len(r) not in (3, 4) or (len(r) == 4 and r[3] not in ("+", "-")):
                raise ValueError("a region is an int, (record, start, end) or (record, start, end, '+' | '-'): %r" % (r,))
            record = r[0]
            if isinstance(record, (str, bytes)):
                record = index[record]
                if record is None:
                    raise KeyError(r[0])
            if int(record) < 0 or int(r[1]) < 0 or (r[2] is not None and int(r[2]) < 0):
                raise ValueError("negative value in region %d: %r" % (k, r))
            arr[k].record, arr[k].start = int(record), int(r[1])
            arr[k].end = _ffi.REGION_END if r[2] is None else int(r[2])
            arr[k].reverse_complement = int(len(r) == 4 and r[3] == "-")
        return self._select(arr, len(regions), name_regions)

    @staticmethod
    def _packed_regions(regions):
        """-> (pointer to nafgpu_region, their number) when `regions` is a Hits or a buffer of whole structs, else None"""
        from .search import Hits
        if isinstance(regions, Hits):
            regions = regions.regions()
        elif isinstance(regions, (list, tuple, str)):
            return None
        try:
            view = memoryview(regions)
        except TypeError:
            return None
        size = ctypes.sizeof(_ffi.Region)
        if view.itemsize not in (1, size):                   # an array of numbers (numpy.flatnonzero(...)) is a list of records, as ever
            return None
        if not view.c_contiguous or view.nbytes % size:
            raise ValueError("a buffer of regions holds whole nafgpu_region structs of %d bytes, contiguous: %d bytes given" % (size, view.nbytes))
        if view.nbytes and not view.readonly:
            raw = (ctypes.c_uint8 * view.nbytes).from_buffer(view)
        else:                                                # a read-only buffer (bytes) has no address ctypes may take: one copy
            raw = (ctypes.c_uint8 * max(view.nbytes, 1)).from_buffer_copy(view.tobytes() or b"\0")
        return ctypes.cast(raw, ctypes.POINTER(_ffi.Region)), view.nbytes // size

    def _select(self, arr, n, name_regions):
        opts = _ffi.SelectOpts(name_regions=int(bool(name_regions)))
        h, res, err = c_void_p(), _ffi.SelectResult(), _ffi.Error()
        rc = self._lib.c.nafgpu_select(self._h, arr, n, byref(opts), byref(h), byref(res), byref(err))
        if rc != _ffi.OK:
            self._raise_select(rc, err)
        return Selection(self._lib, h, res)

    def summarize(self, classes=None):
        """Per-record letter counts, quality sums and the sections' histograms of the decoded records, counted on the GPU
        (decodes first if nothing is decoded yet) -> a Summary.  `classes`: 256 bytes, see nafcodec_amd.summary."""
        from .summary import _summarize_decoder
        return _summarize_decoder(self, classes)

    def search(self, patterns, *, max_mismatches=0, both_strands=None, alphabet=None, max_hits=0):
        """Where `patterns` (str or bytes, up to 16 of up to 64 letters) occur in the decoded records, matched on the GPU
        (decodes first if nothing is decoded yet) -> Hits, whose regions select() takes.  alphabet None: by the archive
        (dna and rna as nucleotides with IUPAC sets, protein and text as bytes); both_strands None: on for nucleotides;
        max_mismatches: 0 .. 3 substitutions.  See nafcodec_amd.search."""
        from .search import _search_decoder
        return _search_decoder(self, patterns, max_mismatches, both_strands, alphabet, max_hits)

    def group(self, *, both_strands=False, alphabet=None):
        """The decoded records whose sequences are equal, found on the GPU (decodes first if nothing is decoded yet) ->
        Groups, which select() takes: the first record of every sequence.  alphabet None: by the archive (dna and rna by
        their 4-bit codes, so case and T/U are ignored; protein and text as bytes); both_strands: a record also equals its
        reverse complement.  See nafcodec_amd.group."""
        from .group import _group_decoder
        return _group_decoder(self, both_strands, alphabet)

    def trim(self, *, cut_front=0, cut_tail=0, window=None, trim_n=False, min_length=0, interleaved=False, quality_base=33):
        """The window of every decoded record that quality trimming keeps, found on the GPU (decodes first if nothing is
        decoded yet) -> Trims, which select() takes: the kept records cut to their windows.  cut_front, cut_tail: the
        running-sum cutoffs of `cutadapt -q`; window: (W, Q), the first window of W values whose mean is below Q; trim_n: N at
        either end; min_length and interleaved: which records are kept.  See nafcodec_amd.trim."""
        from .trim import _trim_decoder
        return _trim_decoder(self, cut_front, cut_tail, window, trim_n, min_length, interleaved, quality_base)

    def kmers(self, k=31, canonical=True):
        """The distinct k-mers of the decoded records as a set in HBM, built on the GPU (decodes first if nothing is decoded
        yet) -> a KmerSet, which screen() takes and which outlives this decoder.  k: 1 .. 31; canonical: a k-mer and its
        reverse complement are one key.  See nafcodec_amd.screen."""
        from .screen import _kmers_decoder
        return _kmers_decoder(self, k, canonical)

    def screen(self, kmer_set, *, min_hits=1, min_percent=0, interleaved=False, keep_matched=False):
        """The decoded records against a KmerSet, on the GPU (decodes first if nothing is decoded yet) -> Screens, which
        select() takes: the kept records, whole.  A record matches with min_hits k-mers of the set in min_percent of its
        windows; interleaved: mates match together; keep_matched: keep what matches (baiting), not what does not
        (decontamination).  See nafcodec_amd.screen."""
        from .screen import _screen_decoder
        return _screen_decoder(self, kmer_set, min_hits, min_percent, interleaved, keep_matched)

    def overlap(self, *, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, quality_base=33):
        """Where read 1 and the reverse complement of read 2 of every decoded pair of mates (records 2j and 2j + 1) overlap,
        found on the GPU (decodes first if nothing is decoded yet) -> Overlaps, which select() takes: every record cut where
        it reads into the adapter; merge() joins the found pairs.  A shift is accepted with min_overlap matches, at most
        max_mismatches mismatches and at most max_mismatch_percent of them.  See nafcodec_amd.overlap."""
        from .overlap import _overlap_decoder
        return _overlap_decoder(self, min_overlap, max_mismatches, max_mismatch_percent, quality_base)

    def merge(self, overlaps):
        """The found pairs of `overlaps` (what overlap() of THIS decoder returned) joined into one record each -> a Selection
        in HBM, in pair order: read 1, then what read 2's reverse complement adds; where both cover a position the letter
        with the higher quality wins (read 1's on a tie and without qualities) and the qualities are combined as
        include/nafgpu.h says at nafgpu_overlap.  Id and comment are read 1's.  ValueError for what the rules refuse."""
        h, res, err = c_void_p(), _ffi.SelectResult(), _ffi.Error()
        rc = self._lib.c.nafgpu_merge_pairs(self._h, overlaps._handle(), byref(h), byref(res), byref(err))
        if rc != _ffi.OK:
            self._raise_select(rc, err)
        return Selection(self._lib, h, res)


class Selection:
    """What Decoder.select() returns: records cut out of a decoded archive, in HBM, with the fields encode_device() reads
    (d_sequence / n_bases, d_quality / n_quality, d_record_end / n_records, d_ids / n_ids_bytes, d_comments /
    n_comments_bytes; None for a field the decoder did not decode), d_id_end / d_comment_end (as decode_all_device() gives
    them), n_regions and ms (the selection kernels).  A copy: it outlives the decoder; the device buffers live until close()."""

    def __init__(self, lib, handle, res):
        self._lib, self._h = lib, handle
        for name, _ in _ffi.EncodeSource._fields_:
            value = getattr(res.src, name)
            setattr(self, name, (value or None) if name.startswith("d_") else value)
        self.d_id_end, self.d_comment_end = res.d_id_end or None, res.d_comment_end or None
        self.n_regions, self.ms = res.n_regions, res.ms
        self.fastq = self.d_quality is not None

    def _handle(self):
        if self._h is None:
            raise RuntimeError("operation on closed selection.")
        return self._h

    def format_device(self, line_length=60):
        """FASTA (FASTQ when the selection has qualities) text of the selected records, built on the GPU in lines of
        `line_length` letters (0: one line); returns the nafgpu_text_result struct (d_text lives until the next call / close())."""
        res = _ffi.TextResult()
        rc = self._lib.c.nafgpu_selection_format(self._handle(), int(line_length), byref(res))
        if rc == _ffi.E_INVALID_ARG:
            raise ValueError("text output needs the sequence field")
        if rc != _ffi.OK:
            raise _ffi.NafError(rc, message="formatting a selection failed")
        return res

    def to_text(self, line_length=60):
        res = self.format_device(line_length)
        return self.copy_to_host(res.d_text, res.n_text)

    def copy_to_host(self, d_ptr, n):
        buf = ctypes.create_string_buffer(max(int(n), 1))
        if self._lib.c.nafgpu_selection_copy_to_host(self._handle(), d_ptr, int(n), buf) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="device-to-host copy failed")
        return buf.raw[:int(n)]

    def hash_device(self, d_ptr, n, first_chunk=0):
        out = ctypes.c_uint64()
        if self._lib.c.nafgpu_selection_hash64(self._handle(), d_ptr, int(n), int(first_chunk), byref(out)) != _ffi.OK:
            raise _ffi.NafError(_ffi.E_DEVICE, message="hashing a device buffer failed")
        return out.value

    def summarize(self, classes=None, *, device=None):
        """Per-record letter counts and quality sums of the selected records -> a Summary (nafcodec_amd.summary)."""
        from .summary import summarize
        self._handle()
        return summarize(self, classes, device=device, _lib=self._lib)

    def search(self, patterns, *, max_mismatches=0, both_strands=None, alphabet=None, max_hits=0, device=None):
        """Where `patterns` occur in the selected records -> Hits (nafcodec_amd.search)."""
        from .search import search
        self._handle()
        return search(self, patterns, max_mismatches=max_mismatches, both_strands=both_strands, alphabet=alphabet, max_hits=max_hits, device=device,
                      _lib=self._lib)

    def group(self, *, both_strands=False, alphabet=None, device=None):
        """The selected records whose sequences are equal -> Groups (nafcodec_amd.group)."""
        from .group import group
        self._handle()
        return group(self, both_strands=both_strands, alphabet=alphabet, device=device, _lib=self._lib)

    def trim(self, *, cut_front=0, cut_tail=0, window=None, trim_n=False, min_length=0, interleaved=False, quality_base=33, device=None):
        """The window of every selected record that quality trimming keeps -> Trims (nafcodec_amd.trim); their records are
        this selection's."""
        from .trim import trim
        self._handle()
        return trim(self, cut_front=cut_front, cut_tail=cut_tail, window=window, trim_n=trim_n, min_length=min_length, interleaved=interleaved,
                    quality_base=quality_base, device=device, _lib=self._lib)

    def kmers(self, k=31, canonical=True, *, device=None):
        """The distinct k-mers of the selected records -> a KmerSet (nafcodec_amd.screen)."""
        from .screen import kmers
        self._handle()
        return kmers(self, k, canonical, device=device, _lib=self._lib)

    def screen(self, kmer_set, *, min_hits=1, min_percent=0, interleaved=False, keep_matched=False, device=None):
        """The selected records against a KmerSet -> Screens (nafcodec_amd.screen); their records are this selection's."""
        from .screen import screen
        self._handle()
        return screen(self, kmer_set, min_hits=min_hits, min_percent=min_percent, interleaved=interleaved, keep_matched=keep_matched, device=device,
                      _lib=self._lib)

    def overlap(self, *, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, quality_base=33, device=None):
        """Where the mates of every selected pair (records 2j and 2j + 1) overlap -> Overlaps (nafcodec_amd.overlap); their
        records are this selection's."""
        from .overlap import overlap
        self._handle()
        return overlap(self, min_overlap=min_overlap, max_mismatches=max_mismatches, max_mismatch_percent=max_mismatch_percent,
                       quality_base=quality_base, device=device, _lib=self._lib)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.c.nafgpu_selection_free(h)

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


def open(file, mode="r", **options):
    """nafcodec.open (lib.pyi:89-108, nafcodec/__init__.py): "r" -> Decoder, "w" -> Encoder."""
    if mode == "r":
        return Decoder(file, **options)
    if mode == "w":
        from .encoder import Encoder
        return Encoder(file, **options)
    raise ValueError("invalid mode: %r" % (mode,))
