"""Decoder.select against format_device on the same archive.

    python tools/select_probe.py [gbases] [--once]                # redirect into profiles/select_probe.log

nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM once.  Then, in one process, medians of 20 after one
warm-up each, of the `ms` of the results (HIP events around the kernels):
  format   Decoder.format_device(): the records -> FASTA text in HBM.  The yardstick: it reads every letter once and writes it
           once, as a selection of every record does.
  (a)      every record whole
  (b)      every record on the reverse strand
  (c)      10 M regions of 100 letters at seeded random places (shorter than a 128-byte line: bytes/s, no goal)
format, (a) and (b) alternate.  (a) is checked against the writer's checksum (what the regions give is the tests' business).
--once: one call of each after the warm-up, nothing else -- for a rocprofv3 --kernel-trace --stats pass of its own."""
import ctypes
import io
import os
import statistics
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder, Selection

THREADS = 16
REGION = np.dtype([("record", "<u8"), ("start", "<u8"), ("end", "<u8"), ("rc", "u1"), ("reserved", "u1", 7)])
assert REGION.itemsize == ctypes.sizeof(_ffi.Region)


def select(lib, dec, regions):
    """nafgpu_select on a numpy array of regions (Decoder.select takes Python tuples: too slow for 10 M of them)"""
    h, res, err = ctypes.c_void_p(), _ffi.SelectResult(), _ffi.Error()
    rc = lib.c.nafgpu_select(dec._h, regions.ctypes.data_as(ctypes.POINTER(_ffi.Region)), len(regions), None, ctypes.byref(h), ctypes.byref(res),
                             ctypes.byref(err))
    if rc != _ffi.OK:
        raise RuntimeError(err.message.decode())
    return Selection(lib, h, res)


def main():
    args = sys.argv[1:]
    once = "--once" in args
    gbases = float(args[0]) if args and not args[0].startswith("--") else 1.0
    lib = _ffi.default()
    print("device:", lib.device_info(0)[0])
    arc = lib.synth(int(gbases * (1 << 30)), seed=21, with_mask=True, iupac_permille=5, threads=THREADS)
    blob = ctypes.string_at(arc.bytes, arc.n)
    seq_hash = arc.seq_hash
    lib.c.nafgpu_synth_free(ctypes.byref(arc))
    dec = Decoder(io.BytesIO(blob))
    res = dec.decode_all_device()
    del blob
    n_rec = res.n_records
    ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * n_rec), dtype=np.uint64)
    lens = np.diff(np.concatenate(([np.uint64(0)], ends)))

    whole = np.zeros(n_rec, dtype=REGION)
    whole["record"], whole["end"] = np.arange(n_rec), _ffi.REGION_END
    reverse = whole.copy()
    reverse["rc"] = 1
    rng = np.random.default_rng(5)
    n_short, width = (10_000_000 if gbases >= 0.5 else 100_000), 100
    short = np.zeros(n_short, dtype=REGION)
    short["record"] = rng.choice(np.flatnonzero(lens >= width), n_short)
    short["start"] = (rng.random(n_short) * (lens[short["record"]] - width + 1).astype(np.float64)).astype(np.uint64)
    short["end"] = short["start"] + width
    short["rc"] = rng.integers(0, 2, n_short)

    def run(regions, check=None):
        with select(lib, dec, regions) as sel:
            if check:
                check(sel)
            return sel.ms, sel.n_bases

    def is_source(sel):
        assert sel.n_bases == res.n_bases and sel.hash_device(sel.d_sequence, sel.n_bases) == seq_hash

    # warm-up of every shape, and the check: (a) is the source
    run(whole, is_source)
    run(reverse)
    run(short)
    dec.format_device()
    reps = 1 if once else 20
    t = {"format": [], "a": [], "b": [], "c": []}
    for _ in range(reps):
        text = dec.format_device()
        t["format"].append(text.ms)
        t["a"].append(run(whole)[0])
        t["b"].append(run(reverse)[0])
    for _ in range(reps):
        ms, n_short_bytes = run(short)
        t["c"].append(ms)
    print("%.2f Gbases, %d records, %d bytes of text" % (res.n_bases / 2**30, n_rec, text.n_text))
    if once:
        dec.close()
        return
    f = statistics.median(t["format"])
    for key, what, nbytes in (("format", "format_device", text.n_text), ("a", "(a) every record whole", res.n_bases),
                              ("b", "(b) every record, reverse strand", res.n_bases), ("c", "(c) %d regions of %d letters" % (n_short, width), n_short_bytes)):
        m = statistics.median(t[key])
        print("  %-36s median %8.3f ms  min %8.3f  max %8.3f   %6.0f GB/s written   x %.2f of format_device" %
              (what, m, min(t[key]), max(t[key]), nbytes / m / 1e6, m / f))
    dec.close()


if __name__ == "__main__":
    main()
