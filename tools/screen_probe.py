"""kmers() and screen() against summarize() and search() on the same source.

    python tools/screen_probe.py [gbases] [--once]               # redirect into profiles/screen_probe.log

The query is 10 M reads of 100 letters cut from nafgpu_synth_write's letters at seeded random places, as tools/search_probe.py
makes them.  Two sets, both of the synthetic archive's own letters, so a part of the reads hits:
  small  the first 5 386 letters (a phage): a table of 16 384 slots, 128 KiB, which lies in L2
  large  the first 5.5 M letters (a bacterium): a table of 2^24 slots, 128 MiB, Infinity Cache at best
Then, in one process, medians of 20 after one warm-up each, of the `ms` of the results (HIP events around the kernels):
  summarize  yardstick: it reads the letters once and writes a row per record
  search     yardstick: one pattern of 31 letters on both strands; it reads the letters once in the same tile shape
  screen     k = 31, canonical, against the small and against the large set
  build      the build of either set (count and insert)
They alternate.  --once: one call of each after the warm-up, nothing else -- for a rocprofv3 --kernel-trace --stats pass of
its own."""
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

from nafcodec_amd import _ffi, search, summarize
from nafcodec_amd.decoder import Decoder
from select_probe import THREADS

scr = importlib.import_module("nafcodec_amd.screen")
REGION = np.dtype(scr.REGION)
SETS = (("small", 5386), ("large", 5_500_000))


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


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
    ends = np.frombuffer(dec.copy_to_host(res.d_record_end, 8 * res.n_records), dtype=np.uint64)
    lens = np.diff(np.concatenate(([np.uint64(0)], ends)))
    reps = 1 if once else 20

    rng = np.random.default_rng(5)
    n_short, width = (10_000_000 if gbases >= 0.5 else 100_000), 100
    short = np.zeros(n_short, dtype=REGION)
    short["record"] = rng.choice(np.flatnonzero(lens >= width), n_short)
    short["start"] = (rng.random(n_short) * (lens[short["record"]] - width + 1).astype(np.float64)).astype(np.uint64)
    short["end"] = short["start"] + width
    sel = dec.select(short)
    pattern = dec.copy_to_host(res.d_sequence + 1000, 31).upper()
    pattern = bytes(b if b in b"ACGT" else ord("A") for b in pattern)

    sets, t = {}, {"summarize": [], "search": []}
    for name, size in SETS:
        size = min(size, res.n_bases)
        piece = Source(d_sequence=res.d_sequence, n_bases=size, d_record_end=None, n_records=0)
        sets[name] = (piece, scr.kmers(piece, 31))           # (and the warm-up of the build)
        t["build " + name], t["screen " + name] = [], []
        sets[name][1].close()
    summarize(sel).close()
    search(sel, [pattern], both_strands=True).close()
    for name, (piece, _) in sets.items():
        sets[name] = (piece, scr.kmers(piece, 31))
        scr.screen(sel, sets[name][1]).close()
    seen = {}
    for _ in range(reps):
        with summarize(sel) as s:
            t["summarize"].append(s.ms)
        with search(sel, [pattern], both_strands=True) as hits:
            t["search"].append(hits.ms)
            seen["search"] = "%d hits" % hits.n_hits
        for name, (piece, kset) in sets.items():
            with scr.screen(sel, kset) as s:
                t["screen " + name].append(s.ms)
                seen["screen " + name] = "%d matched, %d hits of %d windows" % (s.n_matched, s.n_hits, s.n_windows)
            with scr.kmers(piece, 31) as again:
                t["build " + name].append(again.ms)
                seen["build " + name] = "%d keys of %d windows in %d slots" % (again.n_kmers, again.n_windows, again.slots)
    print("reads: %d records, %d letters" % (sel.n_records, sel.n_bases))
    if not once:
        y = {key: statistics.median(t[key]) for key in ("summarize", "search")}
        for key in t:
            m = statistics.median(t[key])
            print("  %-14s median %8.3f ms  min %8.3f  max %8.3f   x %.2f of summarize   x %.2f of search   %s" %
                  (key, m, min(t[key]), max(t[key]), m / y["summarize"], m / y["search"], seen.get(key, "")))
    for _, kset in sets.values():
        kset.close()
    sel.close()
    dec.close()


if __name__ == "__main__":
    main()
