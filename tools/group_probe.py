"""group() against summarize() over the same source.

    python tools/group_probe.py [gbases]                         # redirect into profiles/group_probe.log

nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM once.  Then, in one process, medians of 20 after one
warm-up each, of the `ms` of the results (HIP events, first kernel to last):
  reads   selections of 150-letter reads cut at seeded random places, as tools/select_probe.py makes them, with about 0 %,
          50 % and 99 % of the reads copies of other reads; group() on one strand and on both, beside summarize() of the same
          selection
  long    the decoded letters followed by a copy of their first 32 Mbases, cut by an end table of this tool's own (a torch
          tensor) into records of 32 Mbases: the last record is a duplicate of the first
summarize() and group() alternate.  NAFGPU_DEBUG_TIMES (behind nafgpu_test_hooks) makes the library print the split between
the hash pass, the table, the verify pass and the groups' tables of one call per case, from HIP events."""
import ctypes
import importlib
import io
import os
import statistics
import sys

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))

from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.group import group
from nafcodec_amd.summary import summarize
from select_probe import THREADS

REGION = np.dtype(importlib.import_module("nafcodec_amd.search").REGION)
WIDTH, LONG = 150, 32 << 20


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def measure(lib, what, source, reps=20):
    """medians of summarize() and group() (one strand, both) over `source`, alternating; one split per shape on stderr"""
    summarize(source).close()
    for both in (False, True):
        group(source, both_strands=both).close()
    t = {"summarize": [], False: [], True: []}
    counts = {}
    for _ in range(reps):
        with summarize(source) as s:
            t["summarize"].append(s.ms)
        for both in (False, True):
            with group(source, both_strands=both) as g:
                t[both].append(g.ms)
                counts[both] = (g.n_records, g.n_groups, g.largest_group, g.rounds)
    y = statistics.median(t["summarize"])
    gbases = source.n_bases / 1e9
    print("%s: %d records, %.3f G letters" % (what, source.n_records, gbases))
    print("  %-28s median %8.3f ms  min %8.3f  max %8.3f   %7.3f ms per Gbase" % ("summarize", y, min(t["summarize"]), max(t["summarize"]), y / gbases))
    for both in (False, True):
        m = statistics.median(t[both])
        print("  %-28s median %8.3f ms  min %8.3f  max %8.3f   %7.3f ms per Gbase   x %.2f of summarize   %d groups, the largest of %d, %d round(s)" %
              ("group, both strands" if both else "group, one strand", m, min(t[both]), max(t[both]), m / gbases, m / y, counts[both][1], counts[both][2],
               counts[both][3]))
    sys.stdout.flush()
    lib.c.nafgpu_test_hooks(1)
    os.environ["NAFGPU_DEBUG_TIMES"] = "1"
    for both in (False, True):
        group(source, both_strands=both).close()
    del os.environ["NAFGPU_DEBUG_TIMES"]
    lib.c.nafgpu_test_hooks(0)
    sys.stderr.flush()


def main():
    args = sys.argv[1:]
    gbases = float(args[0]) if args else 1.0
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
    print("%.2f Gbases decoded, %d records" % (res.n_bases / 2**30, n_rec))

    # ---- reads: n distinct reads, the other reads copies of those.  The synthetic letters repeat themselves, so reads cut at
    # random places are not distinct: three times as many are cut, and group() itself says which of them are the first of
    # their sequence on either strand
    rng = np.random.default_rng(5)
    n_reads = int(res.n_bases * 0.9) // WIDTH
    cut = np.zeros(3 * n_reads, dtype=REGION)
    cut["record"] = rng.choice(np.flatnonzero(lens >= WIDTH), len(cut))
    cut["start"] = (rng.random(len(cut)) * (lens[cut["record"]] - WIDTH + 1).astype(np.float64)).astype(np.uint64)
    cut["end"] = cut["start"] + WIDTH
    with dec.select(cut) as sel, sel.group(both_strands=True) as g:
        distinct = cut[np.frombuffer(g.group_first(), dtype=np.uint64).astype(np.int64)]
    n_reads = min(n_reads, len(distinct))
    print("%d reads cut, %d of them distinct on both strands; %d used" % (len(cut), len(distinct), n_reads))
    for rate in (0.0, 0.5, 0.99):
        n_distinct = max(int(n_reads * (1 - rate)), 1)
        places = distinct[:n_distinct]
        reads = np.concatenate((places, places[rng.integers(0, n_distinct, n_reads - n_distinct)]))
        rng.shuffle(reads)
        with dec.select(reads) as sel:
            measure(lib, "%d-letter reads, %.0f %% copies" % (WIDTH, 100 * rate), sel)

    # ---- long records: the letters and a copy of their head, cut every LONG letters by a table of this tool's own
    head = int(np.searchsorted(ends, LONG, side="left")) + 1                   # the records that hold the first LONG letters
    with dec.select(list(range(n_rec)) + [(k, 0, min(int(lens[k]), LONG - (int(ends[k]) - int(lens[k])))) for k in range(head)]) as sel:
        assert sel.n_bases == res.n_bases + LONG
        cuts = list(range(LONG, int(res.n_bases), LONG)) + [int(res.n_bases), int(res.n_bases) + LONG]
        table = torch.from_numpy(np.array(cuts, dtype=np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        src = Source(d_sequence=sel.d_sequence, n_bases=sel.n_bases, d_record_end=table.data_ptr(), n_records=len(cuts))
        with group(src) as g:
            assert g.representative()[len(cuts) - 1] == 0 and g.n_groups == len(cuts) - 1
        measure(lib, "records of %d Mbases, the last a copy of the first" % (LONG >> 20), src)
    dec.close()


if __name__ == "__main__":
    main()
