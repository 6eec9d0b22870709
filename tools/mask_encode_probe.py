"""encode_device with mask=True against the call without it, on letters that are in HBM already.

    python tools/mask_encode_probe.py [gbases] [--legs yardstick,dense,upper] [--once]     # redirect into profiles/mask_encode_probe.log

The letters: nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM twice, as a user would (lower-case runs
applied: the dense case) and with mask=False (the same letters in upper case).  Three legs, level 1, sequence only:
  yardstick  encode_device(mask=False) on the upper-case letters: the call as it was before the option existed
  dense      encode_device(mask=True) on the letters with their lower-case runs (a unit every ~1800 letters)
  upper      encode_device(mask=True) on the upper-case letters: one unit, n / 255 bytes of FF
Wall time of each call (it ends in a device synchronise), the legs alternating, median of 5 after one warm-up each.
--once: every chosen leg once after its warm-up, nothing printed but the sizes -- for a rocprofv3 --kernel-trace --stats
pass of its own (one leg per pass keeps the legs' kernels apart)."""
import ctypes
import io
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

from nafcodec_amd import _ffi
from nafcodec_amd.decoder import Decoder
from nafcodec_amd.encoder import encode_device

THREADS = 16


def main():
    args = sys.argv[1:]
    once = "--once" in args
    legs = ["yardstick", "dense", "upper"]
    if "--legs" in args:
        legs = args[args.index("--legs") + 1].split(",")
    gbases = float(args[0]) if args and not args[0].startswith("--") else 1.0
    lib = _ffi.default()
    print("device:", lib.device_info(0)[0])
    arc = lib.synth(int(gbases * (1 << 30)), seed=21, with_mask=True, iupac_permille=5, threads=THREADS)
    blob = ctypes.string_at(arc.bytes, arc.n)
    lib.c.nafgpu_synth_free(ctypes.byref(arc))
    dec_low, dec_up = Decoder(io.BytesIO(blob)), Decoder(io.BytesIO(blob), mask=False)
    low, up = dec_low.decode_all_device(), dec_up.decode_all_device()
    del blob
    calls = {"yardstick": (up, False), "dense": (low, True), "upper": (up, True)}

    def run(leg):
        res, mask = calls[leg]
        t = time.perf_counter()
        out = encode_device(res, sequence_type="dna", sequence=True, compression_level=1, device=0, threads=THREADS, mask=mask)
        return (time.perf_counter() - t) * 1e3, out

    sizes = {}
    for leg in legs:                                                        # warm-up
        sizes[leg] = len(run(leg)[1])
    reps = 1 if once else 5
    times = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg in legs:
            ms, out = run(leg)
            times[leg].append(ms)
            assert len(out) == sizes[leg]
    print("%.2f Gbases, %d records; level 1, sequence only, host plan on %d threads" % (low.n_bases / 2**30, low.n_records, THREADS))
    for leg in legs:
        print("  %-9s archive %.1f MiB%s" % (leg, sizes[leg] / 2**20, "" if once else
              "   call: median %.1f ms (%s)" % (statistics.median(times[leg]), " ".join("%.1f" % x for x in times[leg]))))
    if not once and "yardstick" in legs:
        base = statistics.median(times["yardstick"])
        for leg in legs:
            if leg != "yardstick":
                print("  %s / yardstick = %.2f" % (leg, statistics.median(times[leg]) / base))
    dec_low.close()
    dec_up.close()


if __name__ == "__main__":
    main()
