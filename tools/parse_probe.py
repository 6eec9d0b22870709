"""parse_text against format_device on the same records, and where a whole encode_text call goes.

    python tools/parse_probe.py [gbases] [--once]                 # redirect into profiles/parse_probe.log

nafgpu_synth_write(gbases * 2^30 bases, with_mask=True) decoded to HBM once.  Then, in one process:
  format   Decoder.format_device(): the records -> FASTA text in HBM (`ms` of the result: sizes + scan + write kernels)
  parse    parse_text on that text where it lies (`ms`: the parse kernels, two spans of HIP events)
alternating, medians of 5 after one warm-up each.  The yardstick is `format`, which moves the same characters (it reads them
once and writes them once; the parse reads the text three times -- summaries, counts, write -- and writes it once).
Then the text is copied to the host and encode_text(text, level 1, mask, keep_line_length) is timed as a whole (3 runs after a
warm-up) beside the parse `ms` of a parse_text from the same host text and nafgpu_encode_last_times of the call.
--once: one format and one parse after the warm-up, nothing else -- for a rocprofv3 --kernel-trace --stats pass of its own."""
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
from nafcodec_amd.encoder import encode_text, parse_text

THREADS = 16


def main():
    args = sys.argv[1:]
    once = "--once" in args
    gbases = float(args[0]) if args and not args[0].startswith("--") else 1.0
    lib = _ffi.default()
    print("device:", lib.device_info(0)[0])
    arc = lib.synth(int(gbases * (1 << 30)), seed=21, with_mask=True, iupac_permille=5, threads=THREADS)
    blob = ctypes.string_at(arc.bytes, arc.n)
    seq_hash, ends_hash = arc.seq_hash, arc.offsets_hash
    lib.c.nafgpu_synth_free(ctypes.byref(arc))
    dec = Decoder(io.BytesIO(blob))
    res = dec.decode_all_device()
    del blob

    def fmt():
        return dec.format_device()

    def parse(text):
        with parse_text(text.d_text, text.n_text, device=0) as p:
            assert p.hash_device(p.d_sequence, p.n_bases) == seq_hash and p.hash_device(p.d_record_end, 8 * p.n_records) == ends_hash
            return p.ms, p.n_records, p.line_length

    text = fmt()
    parse(text)                                                             # warm-up of both
    reps = 1 if once else 5
    t_fmt, t_parse = [], []
    for _ in range(reps):
        text = fmt()
        t_fmt.append(text.ms)
        ms, n_rec, line = parse(text)
        t_parse.append(ms)
    print("%.2f Gbases, %d records, %d bytes of text, lines of %d" % (res.n_bases / 2**30, n_rec, text.n_text, line))
    if once:
        dec.close()
        return
    f, p = statistics.median(t_fmt), statistics.median(t_parse)
    print("  format_device  median %.3f ms (%s)   %.0f GB/s of text" % (f, " ".join("%.3f" % x for x in t_fmt), text.n_text / f / 1e6))
    print("  parse_text     median %.3f ms (%s)   %.0f GB/s of text" % (p, " ".join("%.3f" % x for x in t_parse), text.n_text / p / 1e6))
    print("  parse / format = %.2f" % (p / f))
    host = dec.copy_to_host(text.d_text, text.n_text)
    dec.close()
    with parse_text(host, device=0) as q:                                   # warm-up of the upload path; its parse ms
        parse_ms = q.ms
    walls, last = [], None
    encode_text(host, mask=True, device=0, threads=THREADS)
    for _ in range(3):
        t = time.perf_counter()
        out = encode_text(host, mask=True, device=0, threads=THREADS)
        walls.append((time.perf_counter() - t) * 1e3)
        last = lib.encode_last_times()
    print("  encode_text from host text: wall median %.1f ms (%s), archive %.1f MiB" %
          (statistics.median(walls), " ".join("%.1f" % x for x in walls), len(out) / 2**20))
    print("    of which: parse kernels %.3f ms; encode stage %.1f ms (k_enc_hist %.2f, k_enc_streams + k_enc_scatter %.2f, host plan %.1f)"
          % (parse_ms, last[3], last[0], last[1], last[2]))
    print("    the rest: the text's way to the device, the archive's way back, allocation")


if __name__ == "__main__":
    main()
