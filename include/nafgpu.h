/*
 * nafgpu.h -- C-ABI of libnafgpu, the MI355X-native NAF decode path.
 *
 * This is the drop-in boundary for the hot path of althonos/nafcodec v0.3.1
 * (/root/reference): everything below the crate's public `Decoder` iterator --
 * container parse, per-section Zstandard decompression, 4-bit -> IUPAC unpack,
 * mask application, record slicing -- runs behind these entry points, on the GPU.
 * The reference has no FFI seam inside the path; the seam is its
 * public L3 API, so each entry point names the reference item it replaces.
 * A Rust / C++ / Python shim re-creates `Decoder`/`DecoderBuilder`/`Record` on
 * top (INTEGRATION.md shows the Rust one; include/nafcodec.hpp and
 * nafcodec_amd/ are the C++ and Python ones).
 *
 * Conventions: plain pointers and sizes only; no HIP or torch types.  Every
 * function returns NAFGPU_OK (0) or a negative nafgpu_status unless stated.
 * A decoder may move between threads but calls on one decoder must be
 * serialised by the caller (mirrors `Send + !Sync`, nafcodec/src/lib.rs:24-28).
 * Nothing here aborts or throws across the boundary.
 */
#ifndef NAFGPU_H
#define NAFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAFGPU_ABI_VERSION 2

/* ---- status / error kinds ------------------------------------------------
 * Mirrors nafcodec::Error (nafcodec/src/error.rs:4-11) plus the std::io kinds
 * the decode path raises (decoder/mod.rs:180-185, 430-435; reader.rs:108-109). */
typedef enum {
    NAFGPU_OK = 0,
    NAFGPU_END = 1,              /* Iterator::next -> None (decoder/mod.rs:447-449) */
    NAFGPU_E_IO = -1,            /* Error::Io; see nafgpu_error.io_kind */
    NAFGPU_E_NOM = -2,           /* Error::Nom; see nafgpu_error.nom_code */
    NAFGPU_E_UTF8 = -3,          /* Error::Utf8 */
    NAFGPU_E_PANIC = -4,         /* the reference panics / never returns on this input */
    NAFGPU_E_DEVICE = -5,        /* HIP runtime failure, no usable GPU, out of device memory */
    NAFGPU_E_INVALID_ARG = -6,
    NAFGPU_E_MISSING_FIELD = -7,     /* Error::MissingField (encoder/mod.rs:254,265,298,316) */
    NAFGPU_E_INVALID_LENGTH = -8,    /* Error::InvalidLength (encoder/mod.rs:273-276,303-306) */
    NAFGPU_E_INVALID_SEQUENCE = -9   /* Error::InvalidSequence (encoder/mod.rs:284-290, writer.rs:31-56) */
} nafgpu_status;

typedef enum {                   /* std::io::ErrorKind values used on the path */
    NAFGPU_IO_NONE = 0,
    NAFGPU_IO_UNEXPECTED_EOF = 1,
    NAFGPU_IO_INVALID_DATA = 2,  /* zstd stream corrupt, bad UTF-8 in text sequence/quality */
    NAFGPU_IO_NOT_FOUND = 3,
    NAFGPU_IO_IS_A_DIRECTORY = 4,
    NAFGPU_IO_PERMISSION_DENIED = 5,
    NAFGPU_IO_OTHER = 6
} nafgpu_io_kind;

typedef enum {                   /* nom::error::ErrorKind values parser.rs produces */
    NAFGPU_NOM_NONE = 0,
    NAFGPU_NOM_VERIFY = 1,       /* bad magic / separator (parser.rs:50-53, 87-91) */
    NAFGPU_NOM_MAPRES = 2,       /* bad version / sequence type (parser.rs:55-73) */
    NAFGPU_NOM_TOOLARGE = 3      /* varint overflow (parser.rs:38-45) */
} nafgpu_nom_code;

typedef struct {
    int32_t status;              /* nafgpu_status */
    int32_t io_kind;             /* nafgpu_io_kind */
    int32_t os_errno;            /* errno for NAFGPU_E_IO raised by the OS, else 0 */
    int32_t nom_code;            /* nafgpu_nom_code */
    char message[192];           /* NUL-terminated, human readable */
} nafgpu_error;

/* ---- DecoderBuilder (decoder/mod.rs:53-148) -------------------------------- */
typedef struct {
    uint8_t id;                  /* mod.rs:117  default 1 */
    uint8_t comment;             /* mod.rs:124  default 1 */
    uint8_t sequence;            /* mod.rs:131  default 1 */
    uint8_t quality;             /* mod.rs:138  default 1 */
    uint8_t mask;                /* mod.rs:145  default 1 */
    uint8_t spec_mask;           /* 0 = reference behaviour incl. the record-end mask quirk
                                    (mod.rs:410-415); 1 = lower-case every masked base */
    uint8_t shard_protocol;      /* 1: the decoder is driven through nafgpu_shard_* (below): sections WITH LZ sequences are
                                    sharded too, and the Quality section as well as the Sequence section */
    uint8_t reserved[1];
    uint64_t buffer_size;        /* mod.rs:110: accepted for API parity; sizes the host read-back window */
    int32_t device;              /* HIP device ordinal; -1 = current device */
    int32_t shard_rank;          /* multi-GPU: this process decodes shard `shard_rank` of `shard_count` */
    int32_t shard_count;         /* contiguous zstd-block ranges of the sequence section; 1 = everything */
    int32_t tile_mib;            /* decode the sequence / quality sections in tiles of about this many MiB of output, so that
                                    neither the compressed bytes nor the scratch memory -- nor, for nafgpu_next, the output --
                                    are resident whole (the reference streams any size through 4 KiB buffers, mod.rs:223);
                                    0 = when the archive would not fit in the device's free memory, and -- for nafgpu_next /
                                    nafgpu_next_batch only -- for a section of 4 GiB or more, which the iterator takes in 2 GiB
                                    tiles (the next tile's compressed bytes travel while this one is read back) */
} nafgpu_opts;

/* DecoderBuilder::new() (mod.rs:67-76) */
void nafgpu_opts_default(nafgpu_opts *opts);
/* DecoderBuilder::from_flags (mod.rs:93-101): quality/sequence/mask/comment follow `flags`
 * (a data.rs:80-97 flag byte); `id` stays on. */
void nafgpu_opts_from_flags(nafgpu_opts *opts, uint8_t flags);

/* ---- Header (data.rs:198-237) ------------------------------------------------ */
typedef struct {
    uint8_t format_version;      /* 1 | 2                          data.rs:46-50 */
    uint8_t sequence_type;       /* 0 dna, 1 rna, 2 protein, 3 text  data.rs:56-73 */
    uint8_t flags;               /* bit0 quality, 1 sequence, 2 mask, 3 length, 4 comment, 5 id,
                                    6 title, 7 extended             data.rs:80-97 */
    uint8_t name_separator;
    uint32_t reserved;
    uint64_t line_length;
    uint64_t number_of_sequences;
} nafgpu_header;

/* ---- Record (data.rs:29-40) --------------------------------------------------- */
typedef struct {
    const uint8_t *ptr;          /* host memory owned by the decoder; NOT NUL-terminated */
    uint64_t len;
    uint8_t present;             /* Option::is_some() */
    uint8_t reserved[7];
} nafgpu_field;

typedef struct {
    nafgpu_field id, comment, sequence, quality;
    uint64_t length;
    uint8_t has_length;
    uint8_t reserved[7];
} nafgpu_record;

typedef struct nafgpu_decoder nafgpu_decoder;

/* reader callbacks for nafgpu_open_io: R: Read + Seek (decoder/mod.rs:169-172, ioslice.rs) */
typedef int64_t (*nafgpu_read_fn)(void *ctx, uint8_t *buf, uint64_t cap); /* bytes read, 0 = EOF, <0 = -errno */
typedef int64_t (*nafgpu_seek_fn)(void *ctx, int64_t offset, int whence); /* new position or <0 = -errno */

/* DecoderBuilder::with_path (mod.rs:159-166) / Decoder::from_path (mod.rs:304-306) */
int nafgpu_open_path(const char *path, const nafgpu_opts *opts, nafgpu_decoder **out, nafgpu_error *err);
/* DecoderBuilder::with_bytes (mod.rs:151-156); `bytes` is borrowed until nafgpu_close */
int nafgpu_open_bytes(const uint8_t *bytes, size_t n, const nafgpu_opts *opts, nafgpu_decoder **out,
                      nafgpu_error *err);
/* DecoderBuilder::with_reader (mod.rs:169-256) */
int nafgpu_open_io(nafgpu_read_fn read, nafgpu_seek_fn seek, void *ctx, const nafgpu_opts *opts,
                   nafgpu_decoder **out, nafgpu_error *err);

/* Decoder::header (mod.rs:322-325) */
void nafgpu_get_header(const nafgpu_decoder *dec, nafgpu_header *out);
/* ExactSizeIterator::len (mod.rs:453-457): number_of_sequences - records yielded */
uint64_t nafgpu_remaining(const nafgpu_decoder *dec);
/* Iterator::next (mod.rs:444-451) -> NAFGPU_OK with *rec filled, NAFGPU_END, or an error.
 * Field pointers stay valid until the next call on this decoder; the shim copies them into
 * owned strings to honour Record<'static>.  An error does not fuse the iterator (mod.rs:391). */
int nafgpu_next(nafgpu_decoder *dec, nafgpu_record *rec);
/* Up to `cap` calls of Iterator::next (mod.rs:444-451) in one crossing of the boundary: a binding that reads millions of
 * 151-base records pays one call per few thousand of them.  Fills recs[0 .. *n) -- exactly the records, in order, that *n
 * calls of nafgpu_next would have handed out -- and returns NAFGPU_OK (with *n >= 1; *n < cap when the next record's bytes
 * are not on the host yet: call again), NAFGPU_END (*n == 0: nothing left), or the error the (*n + 1)-th call of nafgpu_next
 * would have returned: recs[0 .. *n) are valid then too, the iterator is not fused, and the next call goes on behind the
 * record that failed (mod.rs:391).  All views of one batch stay valid until the next call on this decoder. */
int nafgpu_next_batch(nafgpu_decoder *dec, nafgpu_record *recs, uint64_t cap, uint64_t *n);
/* Drop for Decoder / into_inner (mod.rs:343-350) */
void nafgpu_close(nafgpu_decoder *dec);
/* last error raised on this decoder (or by the failed open when dec == NULL is not possible:
 * open failures report through their `err` argument) */
void nafgpu_last_error(const nafgpu_decoder *dec, nafgpu_error *err);

/* ---- bulk device path (bench / GPU consumers) -------------------------------------
 * Decodes every selected section on the GPU and leaves the results in HBM.  Replaces a
 * full drain of the iterator (`for r in decoder`) without the per-record host copies. */
typedef struct {
    /* device pointers (HIP device memory owned by the decoder, valid until close / next decode_all) */
    const uint8_t *d_sequence;   /* masked ASCII bases (DNA/RNA) or raw text; length n_bases */
    const uint8_t *d_quality;    /* quality bytes; length n_quality */
    const uint64_t *d_record_end;/* inclusive prefix sum of record lengths; n_records entries */
    const uint8_t *d_ids;        /* NUL-terminated ids, concatenated */
    const uint8_t *d_comments;
    uint64_t n_bases, n_quality, n_records, n_ids_bytes, n_comments_bytes;
    uint64_t packed_bytes;       /* decoded 4-bit bytes of the sequence section (DNA/RNA), else 0 */
    uint64_t compressed_bytes;   /* compressed bytes read by the GPU over all decoded sections */
    uint64_t seq_compressed_bytes;
    uint64_t n_zstd_blocks;      /* sequence section */
    uint64_t n_huf_streams;      /* sequence section */
    uint64_t first_record;       /* shard: index of the first record that STARTS in this shard */
    uint8_t carry;               /* shard: 1 if the shard begins inside a record (its head belongs to record first_record-1) */
    uint8_t sharded;             /* 1 if shard_count > 1 was honoured (sequence section without LZ sequences) */
    uint8_t reserved[6];
    /* timing of the last decode_all, milliseconds (HIP events on the decoder's stream) */
    float ms_total;              /* first kernel launch -> last kernel done */
    float ms_huf;                /* sum over launches of the Huffman literal kernel */
    float ms_unpack;             /* 4-bit -> ASCII kernel */
    float ms_seq_lz;             /* FSE sequence decode + LZ execute kernels */
    float ms_other;
    float ms_host_plan;          /* host: frame walk + table build (outside ms_total) */
    float ms_h2d;                /* host->device upload of archive + task lists (outside ms_total) */
    uint32_t n_huf_launches;
    uint32_t reserved3;
    uint64_t lz_residue_matches; /* LZ matches the parallel passes left to the pointer-jumping stage (all sections) */
    uint64_t base_offset;        /* shard: global index of d_sequence[0] (0 unless sharded) */
    /* ids / comments split on NUL on the device (CStringReader, reader.rs:22-30): string k of d_ids is
     * d_ids[d_id_end[k-1] .. d_id_end[k] - 1) (d_id_end[k] = offset just past its NUL); at most
     * number_of_sequences strings are listed */
    const uint64_t *d_id_end;
    const uint64_t *d_comment_end;
    uint64_t n_ids, n_comments;
    /* bit s set: section s (0 ids, 1 comments, 4 sequence of a protein/text archive, 5 quality) is not valid
     * UTF-8 -- where the reference returns Error::Utf8 (reader.rs:108-109) or panics (mod.rs:362,368) */
    uint32_t utf8_invalid;
    uint32_t reserved4;
    uint64_t quality_offset;     /* shard protocol: index in the Quality section of d_quality[0] (0 otherwise) */
} nafgpu_device_result;

int nafgpu_decode_all_device(nafgpu_decoder *dec, nafgpu_device_result *out);
/* Host front end only: frame walk, table build, upload of the archive and task lists to HBM.
 * Idempotent; decode_all_device / next call it implicitly.  Lets a caller separate "compressed
 * bytes resident in HBM" from the decode itself. */
int nafgpu_upload(nafgpu_decoder *dec);

/* ---- shard protocol: ONE archive over several GPUs, sections with LZ sequences included --------
 * A section is one Zstandard frame: a block may copy from up to a window in front of it and inherits three repeat
 * offsets.  Every rank (opts.shard_rank of opts.shard_count, opts.shard_protocol = 1) walks the whole block directory
 * and decodes one contiguous block range; what a range needs from the ranges in front of it arrives in two steps:
 *
 *   nafgpu_shard_begin    entropy decode of the range (Huffman literals, FSE sequences), block sizes, and the range's
 *                         repeat-offset map -- nothing here needs the other ranks.  Fills `mine`.
 *   (all-gather of the 64-byte nafgpu_shard_summary: RCCL over xGMI; the only collective)
 *   nafgpu_shard_place    every rank now knows where its range begins in the decoded section, which repeat offsets it
 *                         inherits and how much of the window in front of it exists: literals to their places and all
 *                         matches that do not reach -- directly or through other matches -- into that window.
 *   nafgpu_shard_halo     how many bytes this rank receives from rank - 1 (recv_bytes) and sends to rank + 1
 *                         (send_bytes: the last window of its output), and whether what it sends is final already
 *                         (tail_ready; always 1 for the first rank and wherever no pending match touches the tail).
 *   nafgpu_shard_export_tail / nafgpu_shard_import_halo    the point-to-point step (ncclSend / ncclRecv): a rank whose
 *                         tail is ready sends first and receives afterwards, the others receive, finish, send.
 *                         `dst` / `src` are device (or host) buffers of send_bytes / recv_bytes; import also runs what
 *                         was waiting for the window.
 *   nafgpu_shard_finish   mask, record table placement; the result describes this rank's share of the Sequence and the
 *                         Quality sections (d_sequence / base_offset / n_bases, d_quality / quality_offset / n_quality).
 * Sections without LZ sequences take the same calls (recv_bytes = send_bytes = 0).  `section`: 0 Sequence, 1 Quality. */
typedef struct {
    uint64_t decoded[2];         /* elements (decoded zstd bytes) of this rank's block range; [0] Sequence, [1] Quality */
    uint64_t frame_tail[2];      /* of which: behind the start of the last frame that begins inside the range (all, if none does) */
    uint32_t rep_map[2][3];      /* the range's repeat-offset map: the three offsets it leaves behind, as values or as
                                    "inherited offset k minus d" tokens (plan.h: kRepToken) */
    uint8_t failed[2];           /* the rank could not decode its range (every rank then reports the error) */
    uint8_t reserved[6];
} nafgpu_shard_summary;          /* 64 bytes, no pointers: gathered as it is */
int nafgpu_shard_begin(nafgpu_decoder *dec, nafgpu_shard_summary *mine);
int nafgpu_shard_place(nafgpu_decoder *dec, const nafgpu_shard_summary *all, int n_ranks);
int nafgpu_shard_halo(nafgpu_decoder *dec, int section, uint64_t *recv_bytes, uint64_t *send_bytes, int *tail_ready);
int nafgpu_shard_export_tail(nafgpu_decoder *dec, int section, void *dst, uint64_t n);
int nafgpu_shard_import_halo(nafgpu_decoder *dec, int section, const void *src, uint64_t n);
int nafgpu_shard_finish(nafgpu_decoder *dec, nafgpu_device_result *out);

/* ---- text output on the device (what a consumer of the iterator does next, cf. unnaf) ----
 * FASTA, or FASTQ when the archive has a Quality section and opts.quality is set, of the records the
 * iterator would yield, built in HBM from the decoded buffers:
 *   FASTA  '>' id [name_separator comment] '\n', then the sequence in lines of header.line_length characters
 *   FASTQ  '@' id [name_separator comment] '\n' sequence '\n' '+' '\n' quality '\n'
 * (separator and comment only when the comment is not empty; line_length 0 = one line).  Runs
 * decode_all_device first if nothing is decoded yet.  d_text stays valid until close / the next call. */
typedef struct {
    const uint8_t *d_text;       /* device pointer */
    uint64_t n_text;             /* bytes */
    uint64_t n_records;
    float ms;                    /* sizes + scan + write kernels, HIP events */
    uint8_t fastq;
    uint8_t reserved[3];
} nafgpu_text_result;
int nafgpu_format_device(nafgpu_decoder *dec, nafgpu_text_result *out);
/* device -> host copy of `n` bytes of a buffer a result struct points to (tests, small consumers) */
int nafgpu_copy_to_host(nafgpu_decoder *dec, const void *d_ptr, uint64_t n, void *dst);
/* hipDeviceSynchronize on `device` (-1 = current) */
int nafgpu_device_synchronize(int device);
/* The library keeps the device memory of closed decoders for the next one (mapped ranges of 32 MiB and more, up to 16 GiB
 * of them idle per device; small buffers up to 64 MiB in all): this call gives all of it back to the driver -- before
 * another allocator or another process needs the device (no counterpart in the reference; -1 = current device). */
int nafgpu_trim_device_memory(int device);

/* ---- L0 replacement on its own: one NAF section payload ------------------------------
 * Replaces zstd::stream::read::Decoder + include_magicbytes(false) (decoder/mod.rs:221-223)
 * for a whole section: `src` is the magicless Zstandard frame(s), `dst` receives up to `cap`
 * decoded bytes.  Host buffers in, host buffer out; the decode runs on the GPU. */
int nafgpu_zstd_decompress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced,
                           int device, nafgpu_error *err);

/* ---- synthetic archives (format per encoder/mod.rs:334-384) ------
 * Writes a NAF v1 DNA archive with Length+Sequence (+Mask) sections whose sequence section is
 * ONE magicless zstd frame of 128 KiB Huffman-literal blocks (what `ennaf` / zstd level 1
 * produce on DNA).  Deterministic in (seed, n_bases, flags).  Host-only, multi-threaded. */
typedef struct {
    uint64_t n_bases;            /* total nucleotides */
    uint64_t seed;
    uint8_t with_mask;           /* add a Mask section (runs stay inside records) */
    uint8_t iupac_permille;      /* 0..255: per-mille of non-ACGT codes (N, R, Y, ...) */
    uint8_t part_count;          /* > 1: write only part `part_rank` of the archive (several processes write one archive
                                    together, each its share of the sequence section's zstd blocks: nafgpu_synth_archive.bytes
                                    then holds that share alone, and nafgpu_synth_head writes what goes in front) */
    uint8_t part_rank;
    uint8_t reserved[4];
    uint32_t threads;            /* 0 = hardware concurrency */
    uint32_t reserved2;
} nafgpu_synth_spec;

typedef struct {
    uint8_t *bytes;              /* malloc'ed archive; free with nafgpu_synth_free */
    uint64_t n;
    uint64_t n_records, n_bases;
    uint64_t seq_hash;           /* nafgpu_hash64 of the expected ASCII bases (after masking) */
    uint64_t offsets_hash;       /* nafgpu_hash64 of the u64 record_end table */
} nafgpu_synth_archive;

int nafgpu_synth_write(const nafgpu_synth_spec *spec, nafgpu_synth_archive *out);
/* What precedes the parts of an archive written in parts: container header, Length (and Mask) sections, the
 * sequence section's two sizes and its frame header.  seq_part_bytes = sum of the parts' sizes.  out->bytes / n:
 * that head; the archive is head followed by part 0, part 1, ...; seq_hash is 0 (the parts' values add up). */
int nafgpu_synth_head(const nafgpu_synth_spec *spec, uint64_t seq_part_bytes, nafgpu_synth_archive *out);
void nafgpu_synth_free(nafgpu_synth_archive *a);

/* ---- Encoder (EncoderBuilder / Encoder, encoder/mod.rs:46-384, writer.rs) ----------------
 * Host code: the reference's encoder is CPU code too, and the decode path above is what runs on the GPU.  Same
 * surface and checks as the reference; every section is written as one magicless Zstandard frame of 128 KiB
 * blocks -- Huffman / RLE / raw literals, and at `compression_level` 0 (the default level) or >= 3 greedy hash
 * matches coded as sequences with the predefined FSE tables (levels 1-2: literals only) -- which the reference's
 * decoder, libzstd and this library all read.  Sections are kept in memory until the archive is written (the
 * reference's `Memory` storage, storage.rs).  By default, like the reference's encoder, it writes no Mask section and
 * accepts upper-case IUPAC letters only.  With `mask` set (nucleotide sequences only: `sequence` != 0 and
 * `sequence_type` 0 or 1, else NAFGPU_E_INVALID_ARG) lower-case letters are accepted, packed as their upper-case
 * forms, and a Mask section (flag 0x04, between Length and Sequence) records their runs as MaskReader
 * (reader.rs:198-231) reads them: over the concatenated letters of all records the maximal runs of equal case,
 * alternating and starting with an unmasked one (of length 0 when the first letter is lower case), a run of length
 * l as l / 255 bytes 0xFF and one byte l % 255; nothing behind the last letter, no letters: an empty section. */
typedef struct {
    uint8_t sequence_type;       /* 0 dna, 1 rna, 2 protein, 3 text (EncoderBuilder::new, mod.rs:81-90) */
    uint8_t id, comment, sequence, quality;   /* opt-in fields (mod.rs:112-145); all 0 by default */
    uint8_t mask;                /* write a Mask section from the case of the letters (see above); 0 by default */
    uint8_t device_lz;           /* the device calls below accept compression_level 0 and >= 3 and find the LZ matches on the GPU
                                    (see "encoding on the device"); 0 by default; the host encoder ignores it */
    uint8_t reserved[1];
    int32_t compression_level;   /* mod.rs:147-157; 0 or >= 3: with LZ matches, 1-2: literals only (see above) */
    uint32_t threads;            /* blocks are encoded in parallel when the archive is written; 0 = hardware concurrency */
} nafgpu_encoder_opts;
typedef struct nafgpu_encoder nafgpu_encoder;

void nafgpu_encoder_opts_default(uint8_t sequence_type, nafgpu_encoder_opts *opts);
/* EncoderBuilder::from_flags (mod.rs:92-110): NAF flag bits 0x20 id, 0x10 comment, 0x02 sequence, 0x01 quality
 * (0x04 is ignored, as there: `mask` is set by hand) */
void nafgpu_encoder_opts_from_flags(uint8_t sequence_type, uint8_t flags, nafgpu_encoder_opts *opts);
/* EncoderBuilder::with_memory (mod.rs:161-163) */
int nafgpu_encoder_new(const nafgpu_encoder_opts *opts, nafgpu_encoder **out, nafgpu_error *err);
/* Encoder::push (mod.rs:236-323).  Only the enabled fields are read.  A record that is refused (missing field,
 * inconsistent length, invalid letter) leaves the encoder as it was -- the reference has by then written the
 * fields in front of the offending one. */
int nafgpu_encoder_push(nafgpu_encoder *enc, const nafgpu_record *rec, nafgpu_error *err);
/* Encoder::write (mod.rs:325-384) into memory: *bytes stays valid until nafgpu_encoder_free; no push afterwards */
int nafgpu_encoder_finish(nafgpu_encoder *enc, const uint8_t **bytes, uint64_t *n, nafgpu_error *err);
void nafgpu_encoder_free(nafgpu_encoder *enc);

/* ---- encoding on the device: literal-only sections (compression_level 1 and 2) --------------
 * The kernels count symbols and write the bit streams; the host decides every block from the counts with the same
 * function the host encoder uses, so the bytes are those of the host path.  Blocks with LZ sequences (levels 0 and >= 3)
 * are host-only unless opts.device_lz is set: then the three device calls below take those levels too, the matches are
 * found by kernels (inside each 128 KiB block), and the archive is a valid and deterministic one of its own -- the same
 * container, not the host encoder's bytes.  At levels 1 and 2 the flag changes nothing. */

/* L0 counterpart of nafgpu_zstd_decompress: `src` -> one magicless frame of literal-only blocks, the bytes the host
 * Encoder writes for this section at compression_level 1.  Host in, host out, the work on the GPU.  Any size: inputs
 * larger than a slab (a multiple of 64 blocks = 8 MiB, so that slabs end on chunk boundaries and stay independent)
 * go slab by slab.  *produced > cap: NAFGPU_E_INVALID_ARG with *produced set to the size needed. */
int nafgpu_zstd_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced, int device, nafgpu_error *err);
/* The same call with blocks that carry LZ sequences where that is smaller (what opts.device_lz writes for a section): one
 * magicless frame `00 50`, predefined sequence tables, every offset a new offset, no match in front of its block. */
int nafgpu_zstd_compress_lz(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t *produced, int device, nafgpu_error *err);

/* Encoder::write on the GPU for sections already pushed: call before nafgpu_encoder_finish.  device >= 0 or -1 (current):
 * finish compresses every section with the kernels; never called: host code as before.  NAFGPU_E_INVALID_ARG when the
 * encoder's compression_level is not 1 or 2 and opts.device_lz is 0, NAFGPU_E_DEVICE when there is no GPU. */
int nafgpu_encoder_set_device(nafgpu_encoder *enc, int device);

/* The way back from nafgpu_decode_all_device: records that are in HBM -> an archive, without a host push per record. */
typedef struct {
    const uint8_t *d_sequence;  uint64_t n_bases;        /* ASCII letters (DNA/RNA: upper-case IUPAC; opts->mask: lower case too) or raw text */
    const uint8_t *d_quality;   uint64_t n_quality;
    const uint64_t *d_record_end; uint64_t n_records;    /* inclusive prefix sums of record lengths */
    const uint8_t *d_ids;       uint64_t n_ids_bytes;    /* NUL-terminated, concatenated (as decode_all_device leaves them) */
    const uint8_t *d_comments;  uint64_t n_comments_bytes;
} nafgpu_encode_source;   /* a NULL pointer = that field is not written; opts->id/comment/sequence/quality must agree */
/* The archive nafgpu_encoder_finish gives when the same records are pushed one by one, byte for byte (compression_level 1
 * or 2, else NAFGPU_E_INVALID_ARG; with opts->device_lz any level, and at 0 and >= 3 the archive
 * nafgpu_encoder_set_device + finish give).  The host encoder's checks in bulk: quality total != sequence total, or a last record
 * end that is not the total: NAFGPU_E_INVALID_LENGTH; ids / comments that are not n_records NUL-terminated strings:
 * NAFGPU_E_MISSING_FIELD; a letter the nucleotide table refuses (lower case included unless opts->mask is set; with it, a
 * lower-case letter whose upper-case form is refused): NAFGPU_E_INVALID_SEQUENCE, the message names the first one.  With
 * opts->mask the Mask section's bytes are made in HBM from the letters' case (k_enc_mask_*) and compressed like every
 * other section.  On any error nothing is produced.  *bytes is malloc'ed: free it with nafgpu_encode_free. */
int nafgpu_encode_device(const nafgpu_encode_source *src, const nafgpu_encoder_opts *opts, int device,
                         uint8_t **bytes, uint64_t *n, nafgpu_error *err);
void nafgpu_encode_free(uint8_t *bytes);
/* what the calling thread's last nafgpu_zstd_compress / nafgpu_encode_device took, in milliseconds: k_enc_hist (device_lz:
 * and the match, parse and literal-count kernels) and k_enc_streams + k_enc_scatter (device_lz: and the sequence bits)
 * (HIP events, summed over slabs and sections), the host plan between them, the whole call
 * (tools/encode_probe.py) */
void nafgpu_encode_last_times(double *hist_ms, double *streams_ms, double *plan_ms, double *total_ms);

/* ---- FASTA / FASTQ text -> records in HBM -> archive (what `ennaf` does; the inverse of nafgpu_format_device) ----
 * The text is parsed by HIP kernels (parse.hip): no host loop over it, no array with an entry per line.  Rules, the
 * inverse of the text rules at nafgpu_format_device with name_separator ' ':
 *   lines    end at '\n'; the last one may lack it.  A '\r' directly in front of a '\n', or as the very last byte, goes
 *            with it; any other '\r' is data.
 *   format   0 = by the first byte ('>' FASTA, '@' FASTQ), 1 = FASTA, 2 = FASTQ.  Empty text: zero records.  Another first
 *            byte, or one that disagrees with the stated format: NAFGPU_E_INVALID_ARG.
 *   FASTA    a line that begins with '>' opens a record: id = the bytes behind '>' up to the first ' ', comment = all
 *            behind that ' ' (empty when there is none); the sequence = the bytes of the lines up to the next such line,
 *            line ends removed.  Empty lines add nothing; a '>' elsewhere in a line is data.
 *   FASTQ    four lines per record, by line index mod 4: '@' id [' ' comment] / sequence / '+' anything / quality.  A line
 *            count that is not a multiple of 4, a first line without '@', a third without '+': NAFGPU_E_INVALID_ARG, the
 *            message names the byte offset of the first offending line (of the text's end for a missing line).  A quality
 *            that is not as long as its sequence: NAFGPU_E_INVALID_LENGTH, the message names the first such record.
 *   NUL      in a header line: NAFGPU_E_INVALID_ARG with its byte offset (ids and comments are NUL-terminated).
 *   letters  are not judged here: the encode stage refuses them (NAFGPU_E_INVALID_SEQUENCE).
 * line_length = the longest sequence line (without its '\r').  On any error nothing is produced. */
typedef struct {
    uint8_t format;              /* 0 auto, 1 FASTA, 2 FASTQ */
    uint8_t text_on_device;      /* `text` is a device pointer: it is read where it lies */
    uint8_t reserved[6];
} nafgpu_parse_opts;
typedef struct nafgpu_parsed nafgpu_parsed;     /* owns the device buffers of one parse */
typedef struct {
    nafgpu_encode_source src;    /* device pointers, valid until the parse is freed: feed it to nafgpu_encode_device as it is
                                    (d_quality is NULL for FASTA) */
    uint64_t line_length;        /* longest sequence line */
    uint64_t n_text;
    uint8_t fastq, reserved[3];
    float ms;                    /* the parse kernels, HIP events */
} nafgpu_parse_result;
void nafgpu_parse_opts_default(nafgpu_parse_opts *opts);
/* host text goes to the device first (staged); opts may be NULL (auto, host text); device -1 = current */
int nafgpu_parse_text(const uint8_t *text, uint64_t n, const nafgpu_parse_opts *opts, int device,
                      nafgpu_parsed **out, nafgpu_parse_result *res, nafgpu_error *err);
int nafgpu_parse_copy_to_host(nafgpu_parsed *parsed, const void *d_ptr, uint64_t n, void *dst);
/* checksum of a device buffer, equal to nafgpu_hash64_host of the same bytes */
int nafgpu_parse_hash64(nafgpu_parsed *parsed, const void *d_ptr, uint64_t n, uint64_t *out);
void nafgpu_parse_free(nafgpu_parsed *parsed);
/* Parse and encode in one call.  With keep_line_length = 0 the archive is, byte for byte, what the host Encoder
 * writes when the same records are pushed one by one; with 1 the header carries the text's line_length instead of 60 and
 * nothing else differs.  compression_level 1 or 2 (any with opts->device_lz); opts->quality with FASTA text: NAFGPU_E_MISSING_FIELD; opts->mask as
 * for the encoders.  Fields of the text that opts does not name are dropped.  *bytes: free with nafgpu_encode_free. */
int nafgpu_encode_text(const uint8_t *text, uint64_t n, const nafgpu_parse_opts *popts, const nafgpu_encoder_opts *opts,
                       int keep_line_length, int device, uint8_t **bytes, uint64_t *n_out, nafgpu_error *err);

/* ---- records and regions of a decoded archive -> a new set of records in HBM (what a user of a decoded genome or read set does
 * first: one chromosome, bases 1 000 000-1 050 000 of a contig, the reverse strand of a gene, a list of reads by name) ----
 * The gather and the id lookup run in HIP kernels (select.hip); no decoded byte crosses to the host.  The reference has no
 * counterpart.  Rules:
 *   shape     nafgpu_select runs decode_all_device first if nothing is decoded yet.  Region k becomes output record k; regions
 *             may come in any order, may repeat and may overlap.  Zero regions: an empty selection (all counts 0), no error.
 *             The selection holds the fields the decoder was opened with; a field that was not decoded is a NULL pointer in
 *             `src` (without opts.sequence: ids, comments and record ends only, n_bases 0).  It is a COPY: it stays valid
 *             after nafgpu_close of the decoder, until nafgpu_selection_free.
 *   sequence  the letters [start, end) of the record as they lie in d_sequence: soft-masked letters stay lower case.  With
 *             reverse_complement the slice is reversed and every letter complemented, keeping its case: A<->T (A<->U in an
 *             RNA archive), C<->G, R<->Y, K<->M, B<->V, D<->H; S, W, N and '-' map to themselves -- the format's 4-bit code
 *             with its bits reversed (encoder/writer.rs:33-49); any other byte is copied unchanged.
 *   quality   the same slice, reversed when the region is reverse-complemented.
 *   names     the comment of the source record is copied, and its id; with opts->name_regions the id of EVERY region of the
 *             call (whole records included) becomes id:START-END, START = start + 1 and END = the resolved end, in decimal
 *             (`samtools faidx` coordinates), with "/rc" appended for a reverse-complemented region.  A source record without
 *             an id or comment string (the archive may list fewer strings than records) gives an empty string.
 *   refusals  NAFGPU_E_INVALID_ARG: record >= the number of records; start > the resolved end; an explicit end beyond the
 *             record's length; reverse_complement on a protein or text archive -- the message names the LOWEST offending
 *             region index (the check runs on the device, where the record lengths are); a shard, a tiled output (as
 *             nafgpu_format_device); no Length section.  The tiled-output refusal cannot be reached through today's entry
 *             points: nafgpu_select asks the engine for the whole output, as nafgpu_format_device does, so the refusal
 *             guards the engine's state and not a caller's argument, and no test reaches it.  A record whose letters lie
 *             beyond what was decoded: NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF, as nafgpu_format_device gives.  On any error
 *             nothing is produced. */
#define NAFGPU_REGION_END UINT64_MAX
typedef struct {
    uint64_t record;             /* index among the records the decoder yields */
    uint64_t start, end;         /* letters [start, end) of that record, 0-based; end = NAFGPU_REGION_END: the record's length */
    uint8_t reverse_complement;  /* nucleotide archives only */
    uint8_t reserved[7];
} nafgpu_region;
typedef struct { uint8_t name_regions; uint8_t reserved[7]; } nafgpu_select_opts;
typedef struct nafgpu_selection nafgpu_selection;      /* owns its device buffers, like nafgpu_parsed */
typedef struct {
    nafgpu_encode_source src;    /* feed it to nafgpu_encode_device as it is */
    const uint64_t *d_id_end, *d_comment_end;   /* as in nafgpu_device_result; n_regions entries each (NULL with its field) */
    uint64_t n_regions;
    float ms;                    /* the selection kernels, HIP events */
} nafgpu_select_result;
/* opts may be NULL (ids copied as they are).  An error is also kept for nafgpu_last_error. */
int nafgpu_select(nafgpu_decoder *dec, const nafgpu_region *regions, uint64_t n_regions, const nafgpu_select_opts *opts,
                  nafgpu_selection **out, nafgpu_select_result *res, nafgpu_error *err);
/* record_out[j] = the lowest record index whose id equals name j byte for byte, or UINT64_MAX when there is none (that is
 * NAFGPU_OK, not an error); equal ids in the archive resolve to the first.  Needs the ids decoded (opts.id), else
 * NAFGPU_E_INVALID_ARG; `names` must hold exactly n_names NUL-terminated strings, concatenated, in n_bytes, else
 * NAFGPU_E_INVALID_ARG.  An open-addressing table in HBM, keyed by a hash of the id bytes, built by one kernel and probed
 * by another; every hit is verified byte by byte. */
int nafgpu_find_records(nafgpu_decoder *dec, const uint8_t *names, uint64_t n_bytes, uint64_t n_names, uint64_t *record_out,
                        nafgpu_error *err);
/* The selection as text, by the rules at nafgpu_format_device (FASTQ when the selection has qualities; the name separator of
 * the source archive's header), in lines of `line_length` letters (0: one line).  d_text is owned by the selection and
 * stays valid until the next call or nafgpu_selection_free.
 * The calls on a selection return a status alone, and each status has one meaning there: NAFGPU_E_INVALID_ARG is a NULL
 * argument or, for nafgpu_selection_format, a selection without the sequence field; NAFGPU_E_DEVICE is an allocation, copy
 * or kernel that failed. */
int nafgpu_selection_format(nafgpu_selection *sel, uint64_t line_length, nafgpu_text_result *out);
int nafgpu_selection_copy_to_host(nafgpu_selection *sel, const void *d_ptr, uint64_t n, void *dst);
/* as nafgpu_hash64_device_at */
int nafgpu_selection_hash64(nafgpu_selection *sel, const void *d_ptr, uint64_t n, uint64_t first_chunk, uint64_t *out);
void nafgpu_selection_free(nafgpu_selection *sel);

/* ---- records in HBM -> a small table per record: letter counts, GC, N, soft-masked letters, quality sums (the numbers a
 * user picks records by before nafgpu_select; what `unnaf --charcount` prints) ----
 * The counting runs in HIP kernels (summary.hip); the letters stay in HBM, the tables are a few bytes per record.  The
 * reference has no counterpart.  Rules:
 *   classes   classes[b] is a mask of eight bits: a letter with byte value b adds 1 to every column whose bit is set, so
 *             columns may overlap.  opts == NULL or use_classes == 0: the default table
 *                 column 0  A a      1  C c      2  G g      3  T t U u      4  N n
 *                        5  the other IUPAC codes R Y K M S W B D H V, both cases
 *                        6  every byte that is in none of columns 0-5, '-' included
 *                        7  a .. z (lower case), in addition to the letter's own column
 *             under which columns 0-6 of a row add up to the record's length, whatever the bytes are.
 *   shape     record k is letters [d_record_end[k-1], d_record_end[k]); the same slice of d_quality gives d_quality_sum[k].
 *             Empty records have rows of zeros.  Letters behind the last record end count in the histograms only.
 *             d_record_end == NULL or n_records == 0: histograms only.  d_ids and d_comments are ignored.  All positions and
 *             counters are 64-bit; integer work only, so the result is exact whatever the schedule.
 *   totals    the column sums over all records (of the whole section when there is no record table).
 *   refusals  NAFGPU_E_INVALID_ARG: src, out or res NULL, or both d_sequence and d_quality NULL.  NAFGPU_E_INVALID_LENGTH:
 *             both sections given and n_quality != n_bases; a record end below the one in front of it or beyond the section
 *             -- checked on the device, the message names the LOWEST offending record, and no kernel reads outside the
 *             section whatever the table holds.  nafgpu_summarize_decoder decodes first if nothing is decoded yet, makes the
 *             checks of nafgpu_format_device (shard, tiled output, a section that failed), does not need the Length section
 *             (without it: histograms only) and returns NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF when the last record end lies
 *             beyond what was decoded; its error is also kept for nafgpu_last_error.  NAFGPU_E_DEVICE: an allocation, copy
 *             or kernel failed.  On any error nothing is produced. */
typedef struct { uint8_t classes[256]; uint8_t use_classes; uint8_t reserved[7]; } nafgpu_summary_opts;
typedef struct nafgpu_summary nafgpu_summary;          /* owns its device buffers, like nafgpu_selection; it outlives its source */
typedef struct {
    const uint64_t *d_counts;        /* n_records rows of 8 columns, row-major, 16-byte aligned (NULL without d_sequence or records) */
    const uint64_t *d_quality_sum;   /* n_records entries: sum of the record's quality bytes (NULL without d_quality or records) */
    const uint64_t *d_letter_hist;   /* 256 entries: how often each byte value occurs in d_sequence[0, n_bases) (NULL without it) */
    const uint64_t *d_quality_hist;  /* 256 entries over d_quality[0, n_quality) */
    uint64_t n_records, n_bases, n_quality;
    uint64_t totals[8];              /* column sums over all records, computed on the host from d_letter_hist and the table */
    uint64_t quality_total;
    float ms;                        /* the summary kernels, HIP events */
} nafgpu_summary_result;
/* device -1 = current */
int nafgpu_summarize(const nafgpu_encode_source *src, const nafgpu_summary_opts *opts, int device,
                     nafgpu_summary **out, nafgpu_summary_result *res, nafgpu_error *err);
int nafgpu_summarize_decoder(nafgpu_decoder *dec, const nafgpu_summary_opts *opts,
                             nafgpu_summary **out, nafgpu_summary_result *res, nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_summary_copy_to_host(nafgpu_summary *s, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_summary_free(nafgpu_summary *s);

/* ---- records in HBM -> where a primer, an adapter, a restriction site or a guide occurs, as regions for nafgpu_select (records
 * picked by CONTENT, as nafgpu_find_records picks them by name and nafgpu_summarize by numbers) ----
 * The matching runs in HIP kernels (search.hip); the letters stay in HBM, the answer is 40 bytes per hit and 8 per record.
 * The reference has no counterpart.  Rules:
 *   patterns  n_patterns (1 .. 16) NUL-terminated strings, concatenated, in n_bytes, as nafgpu_find_records takes its names;
 *             each 1 .. 64 letters.
 *   windows   record k is letters [d_record_end[k-1], d_record_end[k]).  A hit is a window of m = pattern-length letters that
 *             lies inside ONE record: windows never cross a record end, a record shorter than the pattern (an empty one
 *             included) has none, letters behind the last record end are not searched.  d_record_end == NULL or
 *             n_records == 0: the whole section is record 0 (n_records of the result is 1).
 *   alphabet  0, nucleotide: a letter's set is the format's 4-bit code -- A 1, C 2, G 4, T and U 8, N 15, the other IUPAC
 *             codes their unions (R 5, Y 10, K 12, M 3, S 6, W 9, B 14, D 13, H 11, V 7); either case, so the soft mask is
 *             ignored; every other byte, '-' included, has the empty set.  Pattern position j accepts a text byte when the
 *             byte's set is not empty and a subset of the pattern letter's set: N in a pattern accepts every IUPAC letter, R
 *             accepts A, G and R, and an N in the text is accepted by a pattern N only.
 *             1, bytes: a position accepts exactly its own byte.
 *   mismatches  the number of positions whose text byte is not accepted (substitutions: Hamming distance; no insertions or
 *             deletions).  A window is a hit when that number is <= max_mismatches; it goes into nafgpu_hit_info.mismatches.
 *   strands   with both_strands every pattern is also searched as its reverse complement: order reversed, every set with its
 *             four bits reversed (the complement of nafgpu_select).  Such a hit is reported in forward coordinates with
 *             reverse_complement = 1, so nafgpu_select of the region yields letters that match the pattern as written.  A
 *             palindromic site (GAATTC) is reported once per strand at the same place; equal patterns given twice are
 *             reported once each.
 *   output    hits in ascending order of (absolute start position, pattern index, strand with + first); overlapping hits
 *             are all reported.  d_regions[i] = {record, start, start + m, strand} with start relative to the record;
 *             d_record_hit_begin is the CSR row table over that order, begin[n_records] = n_hits; pattern_hits[p] counts
 *             both strands.  Zero hits: NAFGPU_OK with n_hits 0.  All positions and counts are 64-bit; integer work only,
 *             so the result is exact whatever the schedule.
 *   refusals  NAFGPU_E_INVALID_ARG: a NULL argument; n_patterns 0 or > 16; `patterns` not exactly n_patterns NUL-terminated
 *             strings in n_bytes; a pattern that is empty or longer than 64; max_mismatches > 3 or >= the shortest
 *             pattern's length; a nucleotide pattern letter outside ACGTURYKMSWBDHVN (either case); an alphabet other than 0
 *             and 1; both_strands with the bytes alphabet; d_sequence == NULL; more than max_hits hits (the message gives
 *             the count) -- where a pattern offends, the message names the LOWEST such pattern index.
 *             NAFGPU_E_INVALID_LENGTH: a record end below the one in front of it or beyond the section -- checked on the
 *             device, the message names the LOWEST offending record, and no kernel reads outside the section or the end
 *             table whatever the table holds.  NAFGPU_E_DEVICE: an allocation, copy or kernel failed.
 *             nafgpu_search_decoder decodes first if nothing is decoded yet, makes the checks of nafgpu_format_device (shard,
 *             tiled output, a section that failed), does not need the Length section, and returns NAFGPU_E_IO /
 *             NAFGPU_IO_UNEXPECTED_EOF for a record end beyond what was decoded; its error is also kept for
 *             nafgpu_last_error.  With opts == NULL its alphabet comes from the archive's sequence type (nucleotide for DNA
 *             and RNA, bytes for protein and text; one strand, no mismatches); an explicit alphabet 0 on a protein or text
 *             archive is NAFGPU_E_INVALID_ARG.  nafgpu_search with opts == NULL: all options 0.
 *             On any error nothing is produced. */
#define NAFGPU_SEARCH_MAX_PATTERNS 16
#define NAFGPU_SEARCH_MAX_LENGTH   64
#define NAFGPU_SEARCH_MAX_MISMATCHES 3
typedef struct {
    uint8_t alphabet;            /* 0 = nucleotide (IUPAC sets, case and T/U ignored), 1 = bytes (exact) */
    uint8_t both_strands;        /* nucleotide only: also report where the reverse complement of a pattern lies */
    uint8_t max_mismatches;      /* 0..3 substitutions */
    uint8_t reserved[5];
    uint64_t max_hits;           /* 0: no cap; else more hits than this is a refusal */
} nafgpu_search_opts;
typedef struct { uint32_t pattern; uint8_t mismatches; uint8_t reserved[3]; } nafgpu_hit_info;
typedef struct nafgpu_hits nafgpu_hits;                /* owns its device buffers, like nafgpu_summary; it outlives its source */
typedef struct {
    const nafgpu_region *d_regions;          /* n_hits regions, ready for nafgpu_select once copied to the host */
    const nafgpu_hit_info *d_info;           /* n_hits */
    const uint64_t *d_record_hit_begin;      /* n_records + 1: the hits of record k are [begin[k], begin[k + 1]) */
    uint64_t n_hits, n_records, n_bases;
    uint64_t pattern_hits[NAFGPU_SEARCH_MAX_PATTERNS];
    float ms;                                /* the search kernels, HIP events */
} nafgpu_search_result;
/* device -1 = current; opts may be NULL */
int nafgpu_search(const nafgpu_encode_source *src, const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns,
                  const nafgpu_search_opts *opts, int device, nafgpu_hits **out, nafgpu_search_result *res, nafgpu_error *err);
int nafgpu_search_decoder(nafgpu_decoder *dec, const uint8_t *patterns, uint64_t n_bytes, uint64_t n_patterns,
                          const nafgpu_search_opts *opts, nafgpu_hits **out, nafgpu_search_result *res, nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_hits_copy_to_host(nafgpu_hits *h, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_hits_free(nafgpu_hits *h);

/* ---- records in HBM -> the groups of records whose sequences are equal: PCR duplicates in reads, dereplication of amplicons,
 * identical contigs (records picked by being the FIRST of their sequence) ----
 * Hashing, table and comparison run in HIP kernels (group.hip); no letter comes to the host, the answer is 16 or 17 bytes per
 * record and 16 per group.  The reference has no counterpart.  Rules:
 *   key       the key of record k is the letters [d_record_end[k-1], d_record_end[k]).  Qualities, ids and comments play no
 *             part.  All empty records form one group.  Letters behind the last record end belong to no record.
 *   alphabet  0, nucleotide: two letters are equal when both are IUPAC letters (ACGTURYKMSWBDHVN, either case) with the same
 *             4-bit code, so case and T/U are ignored, as in nafgpu_search; otherwise only when they are the same byte ('-'
 *             included: it equals only itself).
 *             1, bytes: exact bytes; the soft mask distinguishes.
 *   strands   with both_strands (alphabet 0 only) a record is also equal to one whose reverse complement it is; the complement
 *             is nafgpu_select's (the code with its bits reversed; any other byte is itself).  d_strand[k] is 1 only when k
 *             differs from its representative read forward: a record that is its own reverse complement has strand 0, and so
 *             has every representative.
 *   output    d_representative[k] is the LOWEST record index whose sequence equals k's (k itself if it is the first).  Groups
 *             are numbered by ascending representative: d_group_first is ascending, d_group_size sums to n_records,
 *             d_group_of[d_group_first[g]] == g.  n_records == 0: NAFGPU_OK, all counts 0.
 *   exactness equal hashes settle nothing: every record is compared with its representative letter by letter on the device,
 *             and records whose hashes collide are sorted out in further table rounds (`rounds`; 1 unless 64-bit hashes
 *             collided).  All indices and positions are 64-bit, integer work only; the result is a function of the input
 *             alone, whatever the schedule, and no hash value appears in it.
 *   refusals  NAFGPU_E_INVALID_ARG: a NULL argument (src, opts, out, res); d_sequence == NULL; n_records > 0 with
 *             d_record_end == NULL; an alphabet other than 0 and 1; both_strands with the bytes alphabet.
 *             NAFGPU_E_INVALID_LENGTH: a record end below the one in front of it or beyond the section -- checked on the
 *             device, the message names the LOWEST offending record, and no kernel reads outside the section or the end
 *             table whatever the table holds.  NAFGPU_E_DEVICE: an allocation, copy or kernel failed.
 *             nafgpu_group_decoder decodes first if nothing is decoded yet, makes the checks of nafgpu_format_device (shard,
 *             tiled output, a section that failed), needs the Length section (else NAFGPU_E_INVALID_ARG, as nafgpu_select),
 *             and returns NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF for a record end beyond what was decoded; its error is also
 *             kept for nafgpu_last_error.  With opts == NULL its alphabet comes from the archive's sequence type (nucleotide
 *             for DNA and RNA, bytes for protein and text), one strand; an explicit alphabet 0 on a protein or text archive is
 *             NAFGPU_E_INVALID_ARG.
 *             On any error nothing is produced. */
typedef struct {
    uint8_t alphabet;            /* 0 = nucleotide (4-bit codes: case and T/U ignored), 1 = bytes (exact) */
    uint8_t both_strands;        /* nucleotide only: a record also equals its reverse complement */
    uint8_t reserved[6];
} nafgpu_group_opts;
typedef struct nafgpu_groups nafgpu_groups;            /* owns its device buffers, like nafgpu_hits; it outlives its source */
typedef struct {
    const uint64_t *d_representative;        /* n_records: the LOWEST record index whose sequence equals this one's (itself if first) */
    const uint64_t *d_group_of;              /* n_records: index of the record's group */
    const uint8_t *d_strand;                 /* n_records: 1 = equal to the representative only as its reverse complement; NULL without both_strands */
    const uint64_t *d_group_first;           /* n_groups: the representatives, ascending */
    const uint64_t *d_group_size;            /* n_groups */
    uint64_t n_records, n_groups, n_bases, largest_group;
    uint32_t rounds;                         /* table rounds run; 1 unless hashes collided */
    float ms;                                /* first kernel to last, HIP events */
} nafgpu_group_result;
/* device -1 = current */
int nafgpu_group(const nafgpu_encode_source *src, const nafgpu_group_opts *opts, int device, nafgpu_groups **out,
                 nafgpu_group_result *res, nafgpu_error *err);
int nafgpu_group_decoder(nafgpu_decoder *dec, const nafgpu_group_opts *opts, nafgpu_groups **out, nafgpu_group_result *res,
                         nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_groups_copy_to_host(nafgpu_groups *g, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_groups_free(nafgpu_groups *g);

/* ---- records in HBM -> the window of every record that quality trimming keeps, as regions for nafgpu_select (records CUT where
 * a read goes bad: the running-sum rule of `cutadapt -q` and `bwa -q`, a sliding window, N ends, a length filter) ----
 * The trimming runs in HIP kernels (trim.hip); letters and qualities stay in HBM, the answer is 33 bytes per record.  The
 * reference has no counterpart.  Rules:
 *   records   record k is positions [d_record_end[k-1], d_record_end[k]) of the sections, of length L; its letters are
 *             s[0..L), its quality values v[i] = (int) q[i] - quality_base, signed, so a byte below the base is negative.
 *             d_record_end == NULL or n_records == 0: the whole section is record 0 (n_records of the result is 1), as in
 *             nafgpu_search.  Letters behind the last record end belong to no record.  The window starts as [a, b) = [0, L);
 *             the steps run in this order, each on what the one before left.
 *   1 sums    cut_front, cut_tail; 0 turns an end off.  The rule `cutadapt -q FRONT,TAIL` and `bwa -q` state, both ends on
 *             the whole record, independently.  Front: sum = 0, best = 0, a = 0; for i = 0 .. L-1: sum += cut_front - v[i];
 *             stop if sum < 0; if sum > best then best = sum, a = i + 1.  Tail: the mirror image from i = L-1 downward with
 *             cut_tail; sum > best sets b = i.  Ties keep the shorter cut (the comparison is strict).  a >= b: the window is
 *             empty.  Sums are 64-bit signed; a record may be longer than 2^32.
 *   2 window  window = W in 1 .. 64, window_quality = Q; W = 0 turns it off.  The lowest i with a <= i, i + W <= b and
 *             v[i] + .. + v[i+W-1] < W * Q becomes b.  Without such a window (b - a < W is one such case) nothing changes.
 *             This is the cut point of the 5'-to-3' window trimmers (Trimmomatic SLIDINGWINDOW, fastp --cut_right) WITHOUT
 *             their clean-up afterwards: the output of those tools may differ by the few letters they drop or keep around
 *             that point.
 *   3 N ends  trim_n: a advances while a < b and s[a] is N or n; b retreats likewise.  An N in the middle stays.
 *   4 form    an empty window is written as a = b = 0.  keep = (b - a >= min_length); with min_length == 0 every record is
 *             kept, empty ones included.  With `interleaved` records 2j and 2j+1 are mates: both are kept only when both pass.
 *   output    d_regions[k] = {k, a, b, 0} for every record; d_keep[k]; d_kept_regions: the regions of the kept records in
 *             ascending order, n_kept of them, compacted on the device, ready for nafgpu_select once copied to the host.
 *             n_changed: records whose window is not [0, L); bases_in_windows: the sum of b - a over all records;
 *             bases_kept: the same sum over the kept records.  Integer work only: the result is a function of the input
 *             alone, whatever the schedule.
 *   refusals  NAFGPU_E_INVALID_ARG: a NULL argument, opts included; both sections NULL; a quality step (cut_front, cut_tail,
 *             window) without d_quality; trim_n without d_sequence; window > 64; interleaved with an odd number of records.
 *             NAFGPU_E_INVALID_LENGTH: both sections given and n_quality != n_bases; a record end below the one in front of
 *             it or beyond the section -- checked on the device, the message names the LOWEST offending record, and no
 *             kernel reads outside a section or the end table whatever the table holds.  NAFGPU_E_DEVICE: an allocation,
 *             copy or kernel failed.  All options off is allowed: every region is then the whole record.
 *             nafgpu_trim_decoder decodes first if nothing is decoded yet, makes the checks of nafgpu_format_device (shard,
 *             tiled output, a section that failed), needs the Length section (else NAFGPU_E_INVALID_ARG, as nafgpu_select),
 *             and returns NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF for a record end beyond what was decoded; a quality step on
 *             an archive without a Quality section is NAFGPU_E_INVALID_ARG; its error is also kept for nafgpu_last_error.
 *             On any error nothing is produced. */
#define NAFGPU_TRIM_MAX_WINDOW 64
typedef struct {
    uint8_t quality_base;        /* what a quality byte of value 0 is written as: 33 for today's FASTQ (used as given) */
    uint8_t cut_front, cut_tail; /* step 1: the cutoffs of the running sums; 0 = that end is not cut */
    uint8_t window;              /* step 2: W, 1 .. 64; 0 = off */
    uint8_t window_quality;      /* step 2: Q, a window fails when its mean is below it */
    uint8_t trim_n;              /* step 3 */
    uint8_t interleaved;         /* step 4: records 2j and 2j+1 are mates */
    uint8_t reserved;
    uint64_t min_length;         /* step 4: a record whose window is shorter is not kept */
} nafgpu_trim_opts;
typedef struct nafgpu_trims nafgpu_trims;              /* owns its device buffers, like nafgpu_hits; it outlives its source */
typedef struct {
    const nafgpu_region *d_regions;          /* n_records: {k, a, b, 0} */
    const uint8_t *d_keep;                   /* n_records: 1 = kept */
    const nafgpu_region *d_kept_regions;     /* n_kept: the regions of the kept records, ascending */
    uint64_t n_records, n_kept, n_bases;
    uint64_t n_changed;                      /* records whose window is not [0, L) */
    uint64_t bases_in_windows, bases_kept;
    float ms;                                /* the trim kernels, HIP events */
} nafgpu_trim_result;
/* device -1 = current */
int nafgpu_trim(const nafgpu_encode_source *src, const nafgpu_trim_opts *opts, int device, nafgpu_trims **out,
                nafgpu_trim_result *res, nafgpu_error *err);
int nafgpu_trim_decoder(nafgpu_decoder *dec, const nafgpu_trim_opts *opts, nafgpu_trims **out, nafgpu_trim_result *res,
                        nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_trims_copy_to_host(nafgpu_trims *t, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_trims_free(nafgpu_trims *t);

/* ---- the k-mers of a reference as a set in HBM, and records screened against it: which records hold k-mers of a known
 * sequence (a spike-in, a host, a vector: `bbduk ref= k=`, baits), as regions and a keep flag for nafgpu_select ----
 * Both run in HIP kernels (screen.hip); the letters of the reference and of the reads stay in HBM.  The reference has no
 * counterpart.  Rules:
 *   letters   A, C, G, T/U in either case are the codes 0, 1, 2, 3 (the project's 4-bit rule: soft mask and T/U play no part).
 *             Every other byte is no letter: N, the other IUPAC codes, '-', a byte at or above 128.
 *   records   record r is positions [d_record_end[r-1], d_record_end[r]) of d_sequence.  d_record_end == NULL or
 *             n_records == 0: the whole section is record 0 (n_records of the result is 1).  Letters behind the last record
 *             end belong to no record.  Only d_sequence, n_bases, d_record_end and n_records of the source are read.
 *   windows   a window is k consecutive positions of ONE record that are all letters; it never spans a record end.
 *   keys      the forward key of a window is the 2k-bit word with the first letter in the top bits; the reverse complement's
 *             is that of the letters 3 - c in reverse order.  canonical: the key is min(forward, reverse complement), so
 *             a read matches either strand of the reference; else the key is the forward one.  The set records the flag and
 *             a screen uses the set's.
 *   k         1 .. NAFGPU_KMER_MAX_K = 31: a 64-bit word holds any key and a value for an empty slot besides.  The table
 *             stores the key itself, so membership is exact: no hash value decides or appears in any output.
 *   set       nafgpu_kmers_build: n_windows: the windows of the source; n_kmers: their distinct keys; slots: the table's
 *             words, a power of two at least twice n_windows.  An empty set (n_kmers == 0: every record shorter than k, say)
 *             is NAFGPU_OK, and nothing matches it.  The set owns its table and outlives its source; it is read only after
 *             it is built, so any number of screens may use it at once.
 *   screen    per record r: d_windows[r]: its windows; d_hits[r]: those whose key is in the set; d_regions[r] = {r, a, b, 0}:
 *             a the start of the first matching window, b the end of the last one, relative to the record, (0, 0) without a
 *             hit; d_match[r] = hits >= max(min_hits, 1) and hits * 100 >= min_percent * windows; with `interleaved`
 *             records 2j and 2j+1 are mates and both match when either does; d_keep[r] = match XOR !keep_matched: by
 *             default what does NOT match is kept (decontamination), keep_matched keeps what matches (baiting).
 *             d_kept_regions: the whole-record regions {r, 0, L, 0} of the kept records in ascending order, n_kept of them,
 *             compacted on the device, ready for nafgpu_select once copied to the host.  n_matched, n_windows, n_hits:
 *             sums over all records; bases_kept: the letters of the kept records.  Integer work only: the result is a
 *             function of the input alone, whatever the schedule.
 *   refusals  NAFGPU_E_INVALID_ARG: a NULL argument, opts included; d_sequence == NULL; k of 0 or above 31; for a screen
 *             also a NULL set, a set built on another device, min_percent > 100, interleaved with an odd number of
 *             records.  NAFGPU_E_INVALID_LENGTH: a record end below the one in front of it or beyond the section --
 *             checked on the device, the message names the LOWEST offending record, and no kernel reads outside the
 *             section or the end table whatever the table holds.  NAFGPU_E_DEVICE: an allocation, copy or kernel failed.
 *             The _decoder entry points decode first if nothing is decoded yet, make the checks of nafgpu_trim_decoder
 *             (shard, tiled output, a section that failed, the Length section, NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF for a
 *             record end beyond what was decoded), need the sequence decoded and refuse a protein or text archive with
 *             NAFGPU_E_INVALID_ARG; their error is also kept for nafgpu_last_error.  On any error nothing is produced. */
#define NAFGPU_KMER_MAX_K 31
typedef struct {
    uint8_t k;                   /* 1 .. 31 */
    uint8_t canonical;           /* used as given; the Python and C++ layers default to 1 */
    uint8_t reserved[6];
} nafgpu_kmer_opts;
typedef struct nafgpu_kmers nafgpu_kmers;              /* owns its table; it outlives its source */
typedef struct {
    uint64_t n_windows;                      /* windows in the source */
    uint64_t n_kmers;                        /* distinct keys */
    uint64_t n_bases, n_records;
    uint64_t slots;                          /* words of the table */
    uint32_t k;
    uint8_t canonical;
    uint8_t reserved[3];
    float ms;                                /* the build kernels, HIP events */
} nafgpu_kmers_result;
/* device -1 = current */
int nafgpu_kmers_build(const nafgpu_encode_source *src, const nafgpu_kmer_opts *opts, int device, nafgpu_kmers **out,
                       nafgpu_kmers_result *res, nafgpu_error *err);
int nafgpu_kmers_build_decoder(nafgpu_decoder *dec, const nafgpu_kmer_opts *opts, nafgpu_kmers **out, nafgpu_kmers_result *res,
                               nafgpu_error *err);
void nafgpu_kmers_free(nafgpu_kmers *set);

typedef struct {
    uint8_t keep_matched;        /* 0: keep what does not match; 1: keep what matches */
    uint8_t interleaved;         /* records 2j and 2j+1 are mates: both match when either does */
    uint8_t min_percent;         /* 0 .. 100: a record matches only when this share of its windows hits */
    uint8_t reserved[5];
    uint64_t min_hits;           /* a record matches only with so many hits; 0 counts as 1 */
} nafgpu_screen_opts;
typedef struct nafgpu_screens nafgpu_screens;          /* owns its device buffers, like nafgpu_trims; it outlives source and set */
typedef struct {
    const uint64_t *d_windows;               /* n_records */
    const uint64_t *d_hits;                  /* n_records */
    const nafgpu_region *d_regions;          /* n_records: {r, a, b, 0} */
    const uint8_t *d_match;                  /* n_records */
    const uint8_t *d_keep;                   /* n_records: 1 = kept */
    const nafgpu_region *d_kept_regions;     /* n_kept: {r, 0, L, 0} of the kept records, ascending */
    uint64_t n_records, n_matched, n_kept, n_bases;
    uint64_t n_windows, n_hits, bases_kept;
    float ms;                                /* the screen kernels, HIP events */
} nafgpu_screen_result;
/* device -1 = current */
int nafgpu_screen(const nafgpu_encode_source *src, const nafgpu_kmers *set, const nafgpu_screen_opts *opts, int device,
                  nafgpu_screens **out, nafgpu_screen_result *res, nafgpu_error *err);
int nafgpu_screen_decoder(nafgpu_decoder *dec, const nafgpu_kmers *set, const nafgpu_screen_opts *opts, nafgpu_screens **out,
                          nafgpu_screen_result *res, nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_screens_copy_to_host(nafgpu_screens *s, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_screens_free(nafgpu_screens *s);

/* ---- paired reads in HBM -> where read 1 and the reverse complement of read 2 overlap: the cut that takes read-through
 * adapters off both mates (`fastp`'s default for pairs), as regions for nafgpu_select, and the pair joined into one fragment
 * (`fastp -m`, FLASH, `bbmerge`, `vsearch --fastq_mergepairs`) as a selection ----
 * Every shift of every pair is compared in HIP kernels (overlap.hip); the letters stay in HBM, the answer is 32 bytes per pair
 * and 32 per record.  The reference has no counterpart.  Rules:
 *   letters   A, C, G, T/U in either case are the codes 0, 1, 2, 3, as in nafgpu_screen.  Every other byte is no letter.
 *   pairs     records 2j (R1: letters x, length n1) and 2j+1 (R2: length n2) are pair j.  y is R2 reversed and complemented:
 *             y[i] = 3 - code(R2[n2-1-i]); a non-letter stays a non-letter.  Letters behind the last record end belong to no
 *             record.
 *   shifts    a shift d in -(n2-1) .. n1-1 puts y[i] under x[i+d].  The positions compared are p in [max(0,d), min(n1,d+n2));
 *             `compared` is their number.  At such a position both letters and equal is a match, both letters and different
 *             a mismatch, anything else neutral.  insert = d + n2 is the fragment's length; d < 0 is a fragment shorter than
 *             R2, where both mates read into the adapter.
 *   accepted  matches >= max(min_overlap, 1), mismatches <= max_mismatches and
 *             mismatches * 100 <= max_mismatch_percent * (matches + mismatches).
 *   best      among the accepted shifts the fewest mismatches, then the most matches, then the lowest d.  No accepted shift:
 *             the pair is not found.
 *   cap       a pair with a mate longer than NAFGPU_OVERLAP_MAX_LENGTH letters is flagged too_long: it is not analysed and
 *             not found, and it is no refusal.  A pair with an empty mate is not found.
 *   output    d_pairs[j]: shift, insert, matches, mismatches, compared, found, too_long; everything but too_long is 0 when
 *             the pair is not found.  d_regions[r] = {r, 0, min(L, insert), 0} when r's pair is found, else {r, 0, L, 0}:
 *             the adapter cut, ready for nafgpu_select once copied to the host.  d_unmerged_regions: the whole-record regions
 *             {r, 0, L, 0} of both mates of every pair not found, ascending, n_unmerged of them, compacted on the device.
 *             n_cut: records whose region is shorter than L; matches, mismatches, bases_merged (the inserts): sums over the
 *             found pairs; bases_after_cut: the letters of all regions.  Integer work only: the result is a function of the
 *             input alone, whatever the schedule.
 *   merge     nafgpu_merge_pairs: a selection with one record per FOUND pair, in pair order, of `insert` positions p.
 *             p < d (only R1 covers it): R1's byte and quality byte as they lie.  p >= n1 (only R2 covers it): the byte
 *             R2[n2-1-(p-d)] through nafgpu_select's complement table, case kept, and its quality byte.  Else both cover p,
 *             with bytes a (R1), b (R2, complemented) and quality bytes qa, qb: the letter is b if qb > qa, else a (without
 *             qualities always a); the quality byte is max(qa, qb) when a and b are letters with equal codes, otherwise
 *             quality_base + max(|qa - qb|, 2), at most 255.  Id and comment are R1's.  The selection is an ordinary one:
 *             nafgpu_encode_device, nafgpu_selection_format and the record jobs take it.
 *   refusals  NAFGPU_E_INVALID_ARG: a NULL argument, opts included; d_sequence == NULL; no record table (d_record_end == NULL
 *             or n_records == 0); an odd number of records; max_mismatch_percent > 100.  NAFGPU_E_INVALID_LENGTH: a record
 *             end below the one in front of it or beyond the section -- checked on the device, the message names the LOWEST
 *             offending record, and no kernel reads outside the section or the end table whatever the table holds.
 *             NAFGPU_E_DEVICE: an allocation, copy or kernel failed.
 *             nafgpu_overlap_decoder makes the checks of nafgpu_trim_decoder (it decodes first if nothing is decoded yet;
 *             shard, tiled output, a section that failed, the Length section, NAFGPU_E_IO / NAFGPU_IO_UNEXPECTED_EOF for a
 *             record end beyond what was decoded), needs the sequence decoded and refuses a protein or text archive with
 *             NAFGPU_E_INVALID_ARG; its error is also kept for nafgpu_last_error.
 *             nafgpu_merge_pairs refuses what nafgpu_select refuses, and with NAFGPU_E_INVALID_ARG: a NULL argument;
 *             overlaps whose n_records differs from the decoder's, that were found on another device, or whose pairs do not
 *             fit the decoder's records (the message names the LOWEST such pair); a protein or text archive; a decoder
 *             without the sequence decoded.  On any error nothing is produced. */
#define NAFGPU_OVERLAP_MAX_LENGTH 1024
typedef struct {
    uint32_t min_overlap;        /* an accepted shift has so many matches; 0 counts as 1 */
    uint32_t max_mismatches;     /* and at most so many mismatches */
    uint8_t max_mismatch_percent;   /* 0 .. 100: and at most this share of mismatches among matches + mismatches */
    uint8_t quality_base;        /* what a quality byte of value 0 is written as: 33 for today's FASTQ (used as given, by the merge) */
    uint8_t reserved[6];
} nafgpu_overlap_opts;
typedef struct {
    int64_t shift;               /* d */
    uint64_t insert;             /* d + n2 */
    uint32_t matches, mismatches, compared;
    uint8_t found, too_long;
    uint8_t reserved[2];
} nafgpu_pair_overlap;
typedef struct nafgpu_overlaps nafgpu_overlaps;        /* owns its device buffers, like nafgpu_trims; it outlives its source */
typedef struct {
    const nafgpu_pair_overlap *d_pairs;      /* n_pairs */
    const nafgpu_region *d_regions;          /* n_records: {r, 0, min(L, insert), 0}: the adapter cut */
    const nafgpu_region *d_unmerged_regions; /* n_unmerged: {r, 0, L, 0} of both mates of every pair not found, ascending */
    uint64_t n_records, n_pairs, n_bases;
    uint64_t n_found, n_too_long, n_unmerged;
    uint64_t n_cut;                          /* records whose region is shorter than L */
    uint64_t matches, mismatches;            /* sums over the found pairs */
    uint64_t bases_merged;                   /* the sum of insert over the found pairs */
    uint64_t bases_after_cut;                /* the letters of all regions */
    float ms;                                /* the overlap kernels, HIP events */
} nafgpu_overlap_result;
/* device -1 = current */
int nafgpu_overlap(const nafgpu_encode_source *src, const nafgpu_overlap_opts *opts, int device, nafgpu_overlaps **out,
                   nafgpu_overlap_result *res, nafgpu_error *err);
int nafgpu_overlap_decoder(nafgpu_decoder *dec, const nafgpu_overlap_opts *opts, nafgpu_overlaps **out,
                           nafgpu_overlap_result *res, nafgpu_error *err);
/* one record per found pair; the selection is freed with nafgpu_selection_free and outlives decoder and overlaps */
int nafgpu_merge_pairs(nafgpu_decoder *dec, const nafgpu_overlaps *overlaps, nafgpu_selection **out, nafgpu_select_result *res,
                       nafgpu_error *err);
/* n bytes from a pointer of the result; NAFGPU_E_INVALID_ARG: a NULL argument, NAFGPU_E_DEVICE: the copy failed */
int nafgpu_overlaps_copy_to_host(nafgpu_overlaps *o, const void *d_ptr, uint64_t n, void *dst);
void nafgpu_overlaps_free(nafgpu_overlaps *o);

/* order-sensitive 64-bit checksum used for full-size parity checks: sum over the 8-byte words w_j of
 * mix64(w_j ^ (j + 1) * K) -- every word is mixed non-linearly with its position before it is added, so
 * byte errors cannot cancel -- see hash64.h */
uint64_t nafgpu_hash64_host(const uint8_t *p, uint64_t n);
int nafgpu_hash64_device(const nafgpu_decoder *dec, const void *d_ptr, uint64_t n, uint64_t *out);
/* same, for a buffer that starts at 4 KiB chunk `first_chunk` of a larger object: the values of
 * consecutive shards add up (mod 2^64) to the checksum of the whole object */
int nafgpu_hash64_device_at(const nafgpu_decoder *dec, const void *d_ptr, uint64_t n, uint64_t first_chunk, uint64_t *out);
uint64_t nafgpu_hash64_host_at(const uint8_t *p, uint64_t n, uint64_t first_chunk);

/* library / device identification, for logs */
int nafgpu_abi_version(void);
/* tests and measurements only: after nafgpu_test_hooks(1) the library reads its NAFGPU_* experiment variables
 *  from the environment; by default it reads none of them. */
void nafgpu_test_hooks(int enable);
int nafgpu_device_info(int device, char *name, size_t cap, uint64_t *hbm_bytes, int *compute_units);

#ifdef __cplusplus
}
#endif
#endif /* NAFGPU_H */
