"""Decoder.search against Decoder.summarize on the same archive.

    python tools/search_probe.py [gbases] [--once]               # redirect into profiles/search_probe.log

nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM once.  Then, in one process, medians of 20 after one
warm-up each, of the `ms` of the results (HIP events around the kernels):
  summarize  Decoder.summarize().  The yardstick: it reads every letter and writes next to nothing, as the
             search does when hits are rare.
  (a)        one 20-letter pattern, both strands, no mismatch
  (b)        the same with 2 mismatches
  (c)        sixteen 13-letter patterns, both strands, no mismatch
summarize and the three searches alternate.  Then (d): a selection of 10 M reads of 100 letters at seeded random places, as
tools/select_probe.py makes one, is searched as in (a) and summarised.  The hits of (a) are checked against numpy where the
pattern was cut from.
--once: one call of each after the warm-up, nothing else -- for a rocprofv3 --kernel-trace --stats pass of its own."""
import ctypes
import importlib
import io
import os
import statistics
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from select_probe import THREADS

REGION = np.dtype(importlib.import_module("nafcodec_amd.search").REGION)


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

    # the patterns are cut from the letters themselves (N for what is no plain letter), so each has a hit at least
    record = int(np.flatnonzero(lens >= 4096)[0])
    begin = int(ends[record] - lens[record])
    head = bytes(b if b in b"ACGT" else ord("N") for b in dec.copy_to_host(res.d_sequence + begin, 4096).upper())
    one = [head[1000:1020]]
    sixteen = [head[100 * i:100 * i + 13] for i in range(16)]
    cases = (("a", "one 20-letter pattern, both strands", one, 0), ("b", "the same, 2 mismatches", one, 2), ("c", "sixteen 13-letter patterns", sixteen, 0))

    # warm-up of every shape, and the check
    with dec.search(one) as hits:
        regions = np.frombuffer(hits.regions(), dtype=REGION)
        assert hits.n_hits >= 1 and ((regions["record"] == record) & (regions["start"] == 1000) & (regions["reverse_complement"] == 0)).any()
    for _, _, patterns, k in cases[1:]:
        dec.search(patterns, max_mismatches=k).close()
    dec.summarize().close()
    sel = dec.select(short)                                  # (a buffer of regions goes to nafgpu_select as it is)
    sel.search(one).close()
    sel.summarize().close()
    reps = 1 if once else 20
    t = {key: [] for key in ("summarize", "a", "b", "c", "d", "summarize d")}
    n_hits = {}
    for _ in range(reps):
        with dec.summarize() as s:
            t["summarize"].append(s.ms)
        for key, _, patterns, k in cases:
            with dec.search(patterns, max_mismatches=k) as hits:
                t[key].append(hits.ms)
                n_hits[key] = hits.n_hits
    for _ in range(reps):
        with sel.summarize() as s:
            t["summarize d"].append(s.ms)
        with sel.search(one) as hits:
            t["d"].append(hits.ms)
            n_hits["d"] = hits.n_hits
    print("%.2f Gbases, %d records; (d) %d reads of %d letters" % (res.n_bases / 2**30, n_rec, n_short, width))
    if not once:
        rows = [("summarize", "summarize", res.n_bases, "summarize")] + [(key, "(%s) %s" % (key, what), res.n_bases, "summarize") for key, what, _, _ in cases] + \
               [("summarize d", "summarize, the reads of (d)", sel.n_bases, "summarize d"), ("d", "(d) as (a), %d reads of %d letters" % (n_short, width), sel.n_bases, "summarize d")]
        for key, what, letters, yardstick in rows:
            m, y = statistics.median(t[key]), statistics.median(t[yardstick])
            print("  %-44s median %8.3f ms  min %8.3f  max %8.3f   %6.0f G letters/s   x %.2f of summarize   %s" %
                  (what, m, min(t[key]), max(t[key]), letters / m / 1e6, m / y, "%d hits" % n_hits[key] if key in n_hits else ""))
    sel.close()
    dec.close()


if __name__ == "__main__":
    main()
