"""trim() against summarize() on the same source.

    python tools/trim_probe.py [gbases] [--once]                 # redirect into profiles/trim_probe.log

Two sources, both with qualities made on the device by torch (seeded; a tensor's data_ptr() is a section):
  reads  10 M reads of 100 letters cut from nafgpu_synth_write's letters at seeded random places, as tools/search_probe.py
         makes them; qualities of 30 .. 40, a low tail of 2 .. 14 from a random place behind letter 60 in half of the reads, a low
         first letter in a quarter
  long   the synthetic archive's own records (gbases * 2^30 letters); qualities of 30 .. 40 with a low stretch of 2 000 letters
         every 2^20 and a low tail in the first 4 096 records
Then, in one process, medians of 20 after one warm-up each, of the `ms` of the results (HIP events around the kernels):
  summarize  the yardstick: it reads both sections once and writes a row per record
  sums       cut_front = cut_tail = 20           window  window = (4, 20)           n  trim_n
  all        the three together with min_length = 30
summarize and the four trims alternate.  --once: one call of each after the warm-up, nothing else -- for a
rocprofv3 --kernel-trace --stats pass of its own."""
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

tr = importlib.import_module("nafcodec_amd.trim")
REGION = np.dtype(tr.REGION)
CASES = (("sums", dict(cut_front=20, cut_tail=20)), ("window", dict(window=(4, 20))), ("n", dict(trim_n=True)),
         ("all", dict(cut_front=20, cut_tail=20, window=(4, 20), trim_n=True, min_length=30)))


class Source:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def measure(name, source, reps, once):
    for _, opts in CASES:                                    # warm-up of every shape
        tr.trim(source, **opts).close()
    summarize(source).close()
    t, seen = {key: [] for key in ("summarize",) + tuple(c[0] for c in CASES)}, {}
    for _ in range(reps):
        with summarize(source) as s:
            t["summarize"].append(s.ms)
        for key, opts in CASES:
            with tr.trim(source, **opts) as trims:
                t[key].append(trims.ms)
                seen[key] = (trims.n_changed, trims.n_kept, trims.bases_in_windows)
    print("%s: %d records, %d letters" % (name, source.n_records, source.n_bases))
    if once:
        return
    y = statistics.median(t["summarize"])
    for key in t:
        m = statistics.median(t[key])
        print("  %-10s median %8.3f ms  min %8.3f  max %8.3f   %6.0f G letters/s   x %.2f of summarize   %s" %
              (key, m, min(t[key]), max(t[key]), source.n_bases / m / 1e6, m / y,
               "%d changed, %d kept, %d letters left" % seen[key] if key in seen else ""))


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
    gen = torch.Generator(device="cuda").manual_seed(5)
    draw = lambda lo, hi, n: torch.randint(lo, hi, (n,), device="cuda", dtype=torch.uint8, generator=gen)

    # ---- reads
    rng = np.random.default_rng(5)
    n_short, width = (10_000_000 if gbases >= 0.5 else 100_000), 100
    short = np.zeros(n_short, dtype=REGION)
    short["record"] = rng.choice(np.flatnonzero(lens >= width), n_short)
    short["start"] = (rng.random(n_short) * (lens[short["record"]] - width + 1).astype(np.float64)).astype(np.uint64)
    short["end"] = short["start"] + width
    sel = dec.select(short)
    n = sel.n_bases
    q = (draw(30, 41, n) + 33).view(n_short, width)
    where = torch.arange(width, device="cuda", dtype=torch.int32)[None, :]
    tail = torch.where(draw(0, 2, n_short) == 0, draw(60, 100, n_short).to(torch.int32), torch.full((n_short,), width, device="cuda", dtype=torch.int32))
    q = torch.where(where >= tail[:, None], (draw(2, 15, n) + 33).view(n_short, width), q)
    q[:, 0] = torch.where(draw(0, 4, n_short) == 0, torch.full((n_short,), 35, device="cuda", dtype=torch.uint8), q[:, 0])
    q = q.contiguous()
    torch.cuda.synchronize()
    measure("reads", Source(d_sequence=sel.d_sequence, n_bases=n, d_quality=q.data_ptr(), n_quality=n, d_record_end=sel.d_record_end, n_records=sel.n_records),
            reps, once)
    sel.close()
    del q

    # ---- long records
    n = res.n_bases
    q = draw(30, 41, n) + 33
    at = torch.arange(n, device="cuda", dtype=torch.int64)
    q[(at & ((1 << 20) - 1)) < 2000] = 33 + 8
    del at
    for e, l in list(zip(ends, lens))[:4096]:                # a low tail of up to 5 000 letters in the first 4 096 records
        q[int(e) - min(int(l) // 2, 5000):int(e)] = 33 + 5
    torch.cuda.synchronize()
    measure("long", Source(d_sequence=res.d_sequence, n_bases=n, d_quality=q.data_ptr(), n_quality=n, d_record_end=res.d_record_end, n_records=res.n_records),
            reps, once)
    dec.close()


if __name__ == "__main__":
    main()
