"""Decoder.summarize against format_device on the same archive.

    python tools/summary_probe.py [gbases] [--once]               # redirect into profiles/summary_probe.log

nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM once.  Then, in one process, medians of 20 after one
warm-up each, of the `ms` of the results (HIP events around the kernels):
  format     Decoder.format_device(): the records -> FASTA text in HBM.  The yardstick: it reads every letter
             once and writes it once; the summary reads every letter twice (histogram, per-record pass) and writes next to
             nothing.
  summarize  Decoder.summarize(): long records, the long route
format and summarize alternate.  Then a selection of 10 M regions of 100 letters at seeded random places is summarised: short
records, the short route.  The totals of the first summary are checked against numpy over the histogram read back.
--once: one call of each after the warm-up, nothing else -- for a rocprofv3 --kernel-trace --stats pass of its own."""
import ctypes
import io
import os
import statistics
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from nafcodec_amd import _ffi, summary as sm
from nafcodec_amd.decoder import Decoder
from select_probe import REGION, THREADS, select


def main():
    args = sys.argv[1:]
    once = "--once" in args
    gbases = float(args[0]) if args and not args[0].startswith("--") else 1.0
    lib = _ffi.default()
    print("device:", lib.device_info(0)[0])
    arc = lib.synth(int(gbases * (1 << 30)), seed=21, with_mask=True, iupac_permille=5, threads=THREADS)
    blob = ctypes.string_at(arc.bytes, arc.n)
    lib.c.nafgpu_synth_free(ctypes.byref(arc))
    dec = Decoder(io.BytesIO(blob))
    res = dec.decode_all_device()
    del blob
    n_rec = res.n_records
    ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * n_rec), dtype=np.uint64)
    lens = np.diff(np.concatenate(([np.uint64(0)], ends)))

    rng = np.random.default_rng(5)
    n_short, width = (10_000_000 if gbases >= 0.5 else 100_000), 100
    short = np.zeros(n_short, dtype=REGION)
    short["record"] = rng.choice(np.flatnonzero(lens >= width), n_short)
    short["start"] = (rng.random(n_short) * (lens[short["record"]] - width + 1).astype(np.float64)).astype(np.uint64)
    short["end"] = short["start"] + width

    # warm-up of every shape, and the check: the totals are the histogram's, the rows add up to the lengths
    with dec.summarize() as s:
        hist = np.frombuffer(s.letter_hist(), dtype=np.uint64)
        table = np.frombuffer(sm.DEFAULT_CLASSES, dtype=np.uint8)
        assert s.totals == tuple(int(hist[((table >> c) & 1) == 1].sum()) for c in range(8)) and int(hist.sum()) == res.n_bases
        rows = np.frombuffer(s.counts(), dtype=np.uint64).reshape(-1, 8)
        assert np.array_equal(rows[:, :7].sum(axis=1, dtype=np.uint64), lens) and tuple(int(v) for v in rows.sum(axis=0, dtype=np.uint64)) == s.totals
    dec.format_device()
    sel = select(lib, dec, short)
    with sel.summarize() as s:
        rows = np.frombuffer(s.counts(), dtype=np.uint64).reshape(-1, 8)
        assert s.n_records == n_short and (rows[:, :7].sum(axis=1, dtype=np.uint64) == width).all()
    reps = 1 if once else 20
    t = {"format": [], "long": [], "short": []}
    for _ in range(reps):
        text = dec.format_device()
        t["format"].append(text.ms)
        with dec.summarize() as s:
            t["long"].append(s.ms)
    for _ in range(reps):
        with sel.summarize() as s:
            t["short"].append(s.ms)
    print("%.2f Gbases, %d records, %d bytes of text" % (res.n_bases / 2**30, n_rec, text.n_text))
    if not once:
        f = statistics.median(t["format"])
        for key, what, letters in (("format", "format_device", res.n_bases), ("long", "summarize, %d records" % n_rec, res.n_bases),
                                   ("short", "summarize, %d records of %d letters" % (n_short, width), sel.n_bases)):
            m = statistics.median(t[key])
            print("  %-46s median %8.3f ms  min %8.3f  max %8.3f   %6.0f G letters/s   x %.2f of format_device" %
                  (what, m, min(t[key]), max(t[key]), letters / m / 1e6, m / f))
    sel.close()
    dec.close()


if __name__ == "__main__":
    main()
