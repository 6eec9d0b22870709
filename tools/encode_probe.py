"""Device encoder against the host encoder at 16 threads, on the two sections DESIGN's encode chapter quotes:
a 1 Gbase DNA sequence section (512 MiB packed) and the quality section of tools/fastq_probe.py (2 M reads x 151).

    python tools/encode_probe.py [gbases] [reads]            # writes nothing; redirect into profiles/encode_probe.log

Per section: nafgpu_encoder_finish on the host (threads = 16) and with nafgpu_encoder_set_device, wall time, median of 5
after one warm-up, alternating; nafgpu_zstd_compress of the same bytes with the split nafgpu_encode_last_times gives
(k_enc_hist, k_enc_streams + k_enc_scatter by HIP events, the host plan between them, the whole call); the bytes the
kernels move (input read twice, output written once, 4 KiB of counts per block) over the kernel time, as a share of the
8 TB/s peak.  NAFGPU_PROBE_LIBS: comma-separated experiment builds (k_enc_hist with other numbers of LDS copies) timed on
the same bytes after the product, alternating with it."""
import ctypes
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

from nafcodec_amd import _ffi

PEAK = 8e12
THREADS = 16


def finish_ms(lib, sequence_type, field, data, device):
    """one encoder: push `data` as one record, time nafgpu_encoder_finish alone -> (ms, archive bytes)"""
    opts, h, err = _ffi.EncoderOpts(), ctypes.c_void_p(), _ffi.Error()
    lib.c.nafgpu_encoder_opts_default(sequence_type, ctypes.byref(opts))
    setattr(opts, field, 1)
    opts.compression_level, opts.threads = 1, THREADS
    assert lib.c.nafgpu_encoder_new(ctypes.byref(opts), ctypes.byref(h), ctypes.byref(err)) == _ffi.OK
    rec = _ffi.Record()
    f = getattr(rec, field)
    f.ptr, f.len, f.present = data.ctypes.data, data.size, 1
    assert lib.c.nafgpu_encoder_push(h, ctypes.byref(rec), ctypes.byref(err)) == _ffi.OK, err.message
    if device is not None:
        assert lib.c.nafgpu_encoder_set_device(h, device) == _ffi.OK
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    t = time.perf_counter()
    rc = lib.c.nafgpu_encoder_finish(h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(err))
    ms = (time.perf_counter() - t) * 1e3
    assert rc == _ffi.OK, err.message
    blob = ctypes.string_at(p, n.value)
    lib.c.nafgpu_encoder_free(h)
    return ms, blob


def section(lib, libs, name, sequence_type, field, pushed, section_bytes):
    """pushed: what the encoder is given (numpy u8); section_bytes: what the section holds (numpy u8)"""
    finish_ms(lib, sequence_type, field, pushed, None)                     # warm-up, both paths
    finish_ms(lib, sequence_type, field, pushed, 0)
    host, dev, same = [], [], True
    for _ in range(5):
        a, blob_h = finish_ms(lib, sequence_type, field, pushed, None)
        b, blob_d = finish_ms(lib, sequence_type, field, pushed, 0)
        host.append(a)
        dev.append(b)
        same = same and blob_h == blob_d
    mh, md = statistics.median(host), statistics.median(dev)
    print("%s: section %.1f MiB -> archive %.1f MiB, bytes equal %s" % (name, section_bytes.size / 2**20, len(blob_h) / 2**20, same))
    print("  nafgpu_encoder_finish host, %d threads: median %.1f ms (%s)" % (THREADS, mh, " ".join("%.1f" % x for x in host)))
    print("  nafgpu_encoder_finish device 0:         median %.1f ms (%s)   host / device = %.2f" % (md, " ".join("%.1f" % x for x in dev), mh / md))
    raw = section_bytes.tobytes()
    n_blocks = (len(raw) + (128 << 10) - 1) // (128 << 10)
    rows = {}
    for rep in range(6):                                                    # first pass: warm-up; the builds alternate
        for label, L in libs:
            out = L.zstd_compress(raw, 0)
            if rep:
                rows.setdefault(label, []).append(L.encode_last_times())
    moved = 2 * len(raw) + len(out) + 4096 * n_blocks
    for label, L in libs:
        hist, streams, plan, total = (statistics.median(x[k] for x in rows[label]) for k in range(4))
        print("  nafgpu_zstd_compress [%s]: k_enc_hist %.2f ms, k_enc_streams + k_enc_scatter %.2f ms, host plan %.1f ms (%.0f %% of the call), "
              "call %.1f ms" % (label, hist, streams, plan, 100 * plan / total, total))
        print("      kernels move %.0f MB in %.2f ms = %.2f TB/s = %.0f %% of the 8 TB/s peak (k_enc_hist alone: %.2f TB/s)"
              % (moved / 1e6, hist + streams, moved / (hist + streams) / 1e9, 100 * moved / (hist + streams) / 1e9 / (PEAK / 1e12),
                 len(raw) / hist / 1e9))
    sys.stdout.flush()


def main():
    gbases = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    n_reads = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2_000_000
    lib = _ffi.default()
    libs = [("product", lib)] + [(os.path.basename(x), _ffi.Library(os.path.join(R, x)))
                                 for x in os.environ.get("NAFGPU_PROBE_LIBS", "").split(",") if x]
    print("device:", lib.device_info(0)[0])
    rng = np.random.default_rng(2)
    n_bases = int(gbases * (1 << 30)) & ~1
    idx = rng.integers(0, 1000, n_bases, dtype=np.uint16)
    ascii_ = np.frombuffer(b"ACGT", dtype=np.uint8)[idx & 3]
    ascii_[idx >= 995] = ord("N")                                           # 5 per mille of IUPAC, as the synthetic archives have
    lut = np.zeros(256, dtype=np.uint8)
    for c, v in zip(b"ACGTN", (8, 4, 2, 1, 15)):
        lut[c] = v
    codes = lut[ascii_]
    packed = codes[0::2] | (codes[1::2] << 4)
    del idx, codes
    section(lib, libs, "DNA sequence, %.2f Gbases" % gbases, 0, "sequence", ascii_, packed)
    del ascii_, packed
    qalpha = np.frombuffer(b"#8CGGGGGGGGGG<AFFFJJJJJJJJJJJJJJ", dtype=np.uint8)   # tools/fastq_probe.py
    qual = qalpha[rng.integers(0, len(qalpha), n_reads * 151)]
    section(lib, libs, "quality, %d reads x 151" % n_reads, 0, "quality", qual, qual)


if __name__ == "__main__":
    main()
