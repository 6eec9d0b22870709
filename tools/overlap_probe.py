"""overlap() against summarize() and trim() on the same source.

    python tools/overlap_probe.py [gbases] [--once]              # redirect into profiles/overlap_probe.log

The reads are 5 M pairs of 150 letters cut from nafgpu_synth_write's letters at seeded random places: a fragment of 40 .. 520
letters, read 1 the 150 letters from its first one on, read 2 the 150 letters that end at its last one, on the reverse strand.
A fragment shorter than a read is read through: what follows it in the archive stands for the adapter.  A pair whose fragment
is shorter than 271 letters has 30 or more letters in common, so a little under half of the pairs is found.  Qualities are
drawn on the device (30 .. 40), as tools/trim_probe.py draws them.  Then, in one process, medians of 20 after one warm-up
each, of the `ms` of the results (HIP events around the kernels):
  summarize  yardstick: it reads the letters once and writes a row per record
  trim       yardstick: cut_front = cut_tail = 20 and trim_n on letters and qualities
  overlap    the defaults (min_overlap 30, 5 mismatches, 20 %)
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

from nafcodec_amd import _ffi, summarize
from nafcodec_amd.decoder import Decoder
from select_probe import THREADS

ov = importlib.import_module("nafcodec_amd.overlap")
tr = importlib.import_module("nafcodec_amd.trim")
REGION = np.dtype(ov.REGION)
READ, SHORTEST, LONGEST = 150, 40, 520


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def main():
    import torch
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
    n_pairs = 5_000_000 if gbases >= 0.5 else 50_000
    room = LONGEST + 2 * READ                                # a fragment with a read's length of letters on either side
    record = rng.choice(np.flatnonzero(lens >= room), n_pairs)
    first = (READ + rng.random(n_pairs) * (lens[record] - room + 1).astype(np.float64)).astype(np.uint64)   # the fragment's first letter
    size = rng.integers(SHORTEST, LONGEST + 1, n_pairs).astype(np.uint64)
    reads = np.zeros(2 * n_pairs, dtype=REGION)
    reads["record"] = np.repeat(record, 2)
    reads["start"][0::2] = first
    reads["start"][1::2] = first + size - READ
    reads["end"] = reads["start"] + READ
    reads["reverse_complement"][1::2] = 1
    sel = dec.select(reads)
    n = sel.n_bases
    gen = torch.Generator(device="cuda").manual_seed(5)
    q = (torch.randint(30, 41, (n,), device="cuda", dtype=torch.uint8, generator=gen) + 33).contiguous()
    torch.cuda.synchronize()
    source = Source(d_sequence=sel.d_sequence, n_bases=n, d_quality=q.data_ptr(), n_quality=n, d_record_end=sel.d_record_end, n_records=sel.n_records)
    trim = dict(cut_front=20, cut_tail=20, trim_n=True)

    t, seen = {"summarize": [], "trim": [], "overlap": []}, {}
    summarize(source).close()
    tr.trim(source, **trim).close()
    ov.overlap(source).close()
    for _ in range(reps):
        with summarize(source) as s:
            t["summarize"].append(s.ms)
        with tr.trim(source, **trim) as trims:
            t["trim"].append(trims.ms)
            seen["trim"] = "%d changed" % trims.n_changed
        with ov.overlap(source) as o:
            t["overlap"].append(o.ms)
            seen["overlap"] = "%d of %d pairs found, %d records cut, %d matches, %d mismatches" % (o.n_found, o.n_pairs, o.n_cut, o.matches, o.mismatches)
    print("reads: %d records, %d letters; %d fragments of at most %d letters" % (sel.n_records, n, int((size <= 2 * READ - 30).sum()), 2 * READ - 30))
    if not once:
        y = {key: statistics.median(t[key]) for key in ("summarize", "trim")}
        for key in t:
            m = statistics.median(t[key])
            print("  %-10s median %8.3f ms  min %8.3f  max %8.3f   %6.0f G letters/s   x %.2f of summarize   x %.2f of trim   %s" %
                  (key, m, min(t[key]), max(t[key]), n / m / 1e6, m / y["summarize"], m / y["trim"], seen.get(key, "")))
    sel.close()
    dec.close()


if __name__ == "__main__":
    main()
