"""Device encoder with LZ sequences (device_lz) against the host encoder at level 0 and 16 threads, on three sections:
(a) 200 MB of Illumina-like ids, (b) the quality section of tools/fastq_probe.py (2 M reads x 151), (c) a 1 Gbase DNA sequence
section (512 MiB packed).

    python tools/lz_encode_probe.py [id_mb] [reads] [gbases]     # writes nothing; redirect into profiles/lz_encode_probe.log
    python tools/lz_encode_probe.py --kernels [id_mb] [reads] [gbases]
                                                                 # three nafgpu_zstd_compress_lz calls per section and nothing
                                                                 # else: the run for rocprofv3 --kernel-trace --stats

Per section: nafgpu_encoder_finish at compression_level 0 on the host (threads = 16: the yardstick) and with
nafgpu_encoder_set_device and device_lz, wall time, median of 5 after one warm-up, alternating; both archives' section against
the host's level-1 frame (h1); nafgpu_zstd_compress_lz of the same bytes with the split nafgpu_encode_last_times gives
(k_enc_hist + k_enc_lz_match + k_enc_lz_parse + k_enc_lz_hist, k_enc_lz_seqbits + k_enc_streams + k_enc_scatter, the host plan,
the whole call).  The algorithmic bytes of the match kernel are 5 per input byte (the input once, one word out) and of the
parse kernel 14 and a bit (the match words twice, the exit words written once and read about once, the input's literals in
and out, 12 bytes per sequence); the kernels' own times come from the rocprofv3 pass."""
import ctypes
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

from nafcodec_amd import _ffi

THREADS = 16


def finish_ms(lib, sequence_type, field, data, level, device):
    """one encoder: push `data` as one record, time nafgpu_encoder_finish alone -> (ms, archive bytes)"""
    opts, h, err = _ffi.EncoderOpts(), ctypes.c_void_p(), _ffi.Error()
    lib.c.nafgpu_encoder_opts_default(sequence_type, ctypes.byref(opts))
    setattr(opts, field, 1)
    opts.compression_level, opts.threads, opts.device_lz = level, THREADS, int(device is not None)
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
    size = n.value
    lib.c.nafgpu_encoder_free(h)
    return ms, size


def section(lib, name, sequence_type, field, pushed, section_bytes, kernels_only):
    """pushed: what the encoder is given (numpy u8); section_bytes: what the section holds (numpy u8)"""
    raw = section_bytes.tobytes()
    if kernels_only:
        for _ in range(3):
            out = lib.zstd_compress(raw, 0, True)
        print("%s: %d -> %d bytes" % (name, len(raw), len(out)))
        return
    finish_ms(lib, sequence_type, field, pushed, 0, None)                  # warm-up, both paths
    finish_ms(lib, sequence_type, field, pushed, 0, 0)
    host, dev = [], []
    for _ in range(5):
        a, size_h = finish_ms(lib, sequence_type, field, pushed, 0, None)
        b, size_d = finish_ms(lib, sequence_type, field, pushed, 0, 0)
        host.append(a)
        dev.append(b)
    _, size_1 = finish_ms(lib, sequence_type, field, pushed, 1, None)
    mh, md = statistics.median(host), statistics.median(dev)
    print("%s: section %d bytes (%.1f MiB); archive: device_lz %d, host level 0 (h0) %d, host level 1 (h1) %d; device / h0 = %.3f, "
          "(h0 + h1) / 2 = %d" % (name, len(raw), len(raw) / 2**20, size_d, size_h, size_1, size_d / size_h, (size_h + size_1) // 2))
    print("  nafgpu_encoder_finish host, level 0, %d threads: median %.1f ms (%s)" % (THREADS, mh, " ".join("%.1f" % x for x in host)))
    print("  nafgpu_encoder_finish device 0, device_lz:       median %.1f ms (%s)   host / device = %.2f"
          % (md, " ".join("%.1f" % x for x in dev), mh / md))
    rows = []
    for rep in range(6):                                                    # first pass: warm-up
        out = lib.zstd_compress(raw, 0, True)
        if rep:
            rows.append(lib.encode_last_times())
    hist, streams, plan, total = (statistics.median(x[k] for x in rows) for k in range(4))
    print("  nafgpu_zstd_compress_lz: hist + match + parse + literal counts %.2f ms, sequence bits + streams + scatter %.2f ms, "
          "host plan %.1f ms (%.0f %% of the call), call %.1f ms, frame %d bytes" % (hist, streams, plan, 100 * plan / total, total, len(out)))
    print("      algorithmic bytes: match %.0f MB (5 per input byte), parse %.0f MB (14 per input byte)" % (5 * len(raw) / 1e6, 14 * len(raw) / 1e6))
    sys.stdout.flush()


def illumina_ids(n_bytes):
    """`A00123:45:HXXXXDSXX:1:<tile>:<x>:<y>` NUL-terminated, tiles of 5 000 reads, x and y walking through their ranges"""
    n = n_bytes // 36 + 1
    i = np.arange(n, dtype=np.int64)
    cols = (1101 + i // 5000, 1000 + (i * 7919) % 30000, 1000 + (i * 104729) % 36000)
    out = b"\0".join(b"A00123:45:HXXXXDSXX:1:%d:%d:%d" % t for t in zip(*(c.tolist() for c in cols))) + b"\0"
    assert len(out) >= n_bytes
    return np.frombuffer(out[:n_bytes], dtype=np.uint8)


def main():
    args = [a for a in sys.argv[1:] if a != "--kernels"]
    kernels_only = "--kernels" in sys.argv[1:]
    id_mb = float(args[0]) if len(args) > 0 else 200.0
    n_reads = int(float(args[1])) if len(args) > 1 else 2_000_000
    gbases = float(args[2]) if len(args) > 2 else 1.0
    lib = _ffi.default()
    print("device:", lib.device_info(0)[0])
    rng = np.random.default_rng(2)
    ids = illumina_ids(int(id_mb * 1e6))
    section(lib, "(a) Illumina-like ids, %.0f MB" % id_mb, 3, "sequence", ids, ids, kernels_only)       # pushed as text: the same section bytes
    del ids
    qalpha = np.frombuffer(b"#8CGGGGGGGGGG<AFFFJJJJJJJJJJJJJJ", dtype=np.uint8)   # tools/fastq_probe.py
    qual = qalpha[rng.integers(0, len(qalpha), n_reads * 151)]
    section(lib, "(b) quality, %d reads x 151" % n_reads, 0, "quality", qual, qual, kernels_only)
    del qual
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
    section(lib, "(c) DNA sequence, %.2f Gbases packed" % gbases, 0, "sequence", ascii_, packed, kernels_only)


if __name__ == "__main__":
    main()
