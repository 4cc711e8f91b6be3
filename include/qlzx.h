/*
 * include/qlzx.h -- C ABI of libqlzx.so, the MI355X (gfx950) QuickLZ level-3
 * codec + record CRC32 for gobeansdb.
 *
 * Two layers:
 *
 * 1. Drop-in symbols.  cgo compiles every .c of quicklz/ and includes
 *    quicklz.h (quicklz/cquicklz.go:3-8), so a drop-in replacement exports
 *    exactly the quicklz.h surface with identical semantics.  Each entry
 *    below names the reference function it replaces.  These run on the GPU
 *    (a batch of one, staged through pinned memory by the host runtime);
 *    there is no CPU codec in this library.
 *
 * 2. Batch device API (qlzx_*).  Thousands of independent value blocks per
 *    launch, device-resident inputs/outputs, per-block status.  All pointers
 *    are device pointers; `stream` is a hipStream_t (NULL = default stream).
 *    Nothing here allocates: callers pass a workspace sized by the matching
 *    *_workspace_size() call, so launches are graph-capturable.
 *    `workspace` must be 16-byte aligned: every layout places its arrays at
 *    multiples of 256 bytes from the base, and the widest access into any of
 *    them is 16 bytes (the decoder's GroupRec and BlkInfo records, the
 *    level-1 tables' uint4 rows), so no layout needs more.  A non-null base that is
 *    not 16-byte aligned returns QLZX_R_WORKSPACE before anything is launched.
 *    Exactly workspace_bytes bytes from the base are the call's to use: no
 *    byte before or past them is touched, and none needs a value on entry.
 *
 * Status codes reproduce the reference wrapper errors and add the
 * memory-safety checks the reference leaves out (quicklz.h:31 builds without
 * QLZ_MEMORY_SAFE).
 */
#ifndef QLZX_H
#define QLZX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- layer 1: quicklz.h drop-in ---------------- */

/* quicklz/quicklz.c:674-681 -- dsize from the 3/9-byte header. */
size_t qlz_size_decompressed(const char *source);
/* quicklz/quicklz.c:683-690 -- csize (header included). */
size_t qlz_size_compressed(const char *source);
/* quicklz/quicklz.c:777-836 -- decompress one block; returns dsize.
 * `scratch_decompress` (>= 16 B, QLZ_SCRATCH_DECOMPRESS) is accepted and unused.
 * A corrupt stream returns 0 instead of the reference's undefined behaviour
 * (qlzx_last_status() says why).
 * Fail-stop: the three GPU-backed drop-ins (qlz_decompress, qlz_compress,
 * crc32_write) have no error channel in their callers (quicklz/cquicklz.go:38-40,
 * store/crc32.go:81-84), so a runtime failure (no device, a HIP error) prints
 * qlzx_last_error() to stderr and abort()s instead of returning a wrong value. */
size_t qlz_decompress(const char *source, void *destination, char *scratch_decompress);
/* quicklz/quicklz.c:692-775 -- compress one block (level 3); returns csize,
 * 0 if size == 0 or size > 0xffffffff-400.  destination >= size + 400 bytes.
 * `scratch_compress` (>= 528400 B, QLZ_SCRATCH_COMPRESS) is accepted and unused. */
size_t qlz_compress(const void *source, char *destination, size_t size, char *scratch_compress);
/* quicklz/quicklz.c:31-58 -- 0:3 1:528400 2:16 3:0 6:0 7:1 8:4 9:1, else -1. */
int qlz_get_setting(int setting);
/* store/crc32.go:61-68 -- raw reflected CRC-32/IEEE table update (no
 * pre/post inversion; the Go wrapper applies ~ at store/crc32.go:78,87). */
uint32_t crc32_write(uint32_t crc, unsigned char *buf, int len);

/* ---------------- layer 2: batch device API ---------------- */

enum qlzx_status {
    QLZX_OK = 0,
    QLZX_E_SIZE_COMPRESSED = 1, /* header csize != src_len   (quicklz/cquicklz.go:90-94) */
    QLZX_E_CORRUPT = 2,         /* stream fails the QLZ_MEMORY_SAFE checks (quicklz.c:519-657) */
    QLZX_E_LEVEL = 3,           /* header level != 3 (quicklz.go:304-308 panics) */
    QLZX_E_DST_CAP = 4,         /* dsize > dst capacity (cquicklz.go:45 allocates exactly dsize) */
    QLZX_E_CRC = 5,             /* record CRC mismatch (store/datafile.go:161-168) */
    QLZX_E_HEADER = 6,          /* src_len shorter than the header */
    QLZX_E_EMPTY = 7,           /* compress of an empty value (cquicklz.go:36 panics) */
    QLZX_E_TOO_LARGE = 8,       /* compress size > 0xffffffff-400 (quicklz.c:705) */
    QLZX_E_MAX_DSIZE = 9,       /* dsize > the batch's max_dsize argument (caller contract) */
    QLZX_E_RUNTIME = 10         /* single call: no result, the GPU runtime failed (qlzx_last_error) */
};

enum qlzx_return {
    QLZX_R_OK = 0,
    QLZX_R_BAD_ARG = -1,
    QLZX_R_WORKSPACE = -2,      /* workspace too small */
    QLZX_R_HIP = -3,            /* a HIP runtime call failed */
    QLZX_R_NO_DEVICE = -4
};

/*
 * Blocks are addressed by byte offsets into one base buffer each side:
 * block i = src[src_off[i] .. src_off[i]+src_len[i]).
 */
typedef struct qlzx_blocks {
    const uint8_t *src;
    const uint64_t *src_off;
    const uint32_t *src_len;
    uint8_t *dst;
    const uint64_t *dst_off;
    uint32_t n;
} qlzx_blocks;

/* Decompress: replaces CDecompressSafe (quicklz/cquicklz.go:84-101) per block.
 *   dst_cap[i]   capacity of block i's destination (nullable: unbounded)
 *   dsize[i]     out: decompressed size (0 on error)             (nullable)
 *   status[i]    out: enum qlzx_status                           (required)
 *   crc_state[i] in: raw CRC state after header[4:24] ‖ key (store/datafile.go:66-72);
 *                nullable = no CRC
 *   crc_expect[i] in: stored record CRC (header[0:4]); nullable = no check
 *   crc_out[i]   out: ~crc_write(crc_state, compressed value)    (nullable)
 *   max_dsize    upper bound on dsize over the batch (selects kernels; blocks
 *                above the fast-path limit take the general kernel).  A block whose
 *                header dsize exceeds it is not decoded: status QLZX_E_MAX_DSIZE.
 * The record CRC is computed over the compressed bytes in the same pass that
 * decodes them (fused).
 * Values over 64 KiB (max_dsize > 65536): the batch decoder decodes every block up to 64 KiB
 * asynchronously, then each larger block in its own whole-GPU pass, one block at a time; that
 * phase reads counts back and synchronises `stream` several times per large block, so the call
 * returns only after it (blocks up to 64 KiB never do).  The workspace then also holds the
 * whole-GPU decoder's scratch: about 31.7 x max_dsize bytes (8 u16 jump levels over 1.5 x
 * max_dsize plus a u32 source index per output byte), e.g. 1.66 GB at the 50 MiB body limit.
 * qlzx_decompress_workspace_size includes it; size max_dsize from the largest header dsize
 * actually pending (as replay does), not from a configured bound.
 * Workspace of the batch decoder itself: one region per chunk in flight -- 1 for a call of one
 * chunk, 2 when K1 of the next chunk overlaps K2 of this one, 3 for calls of values over 16 KiB
 * in three chunks or more (the last chunk's K1 starts first).  A smaller workspace (at least one
 * region) still decodes, with less overlap. */
size_t qlzx_decompress_workspace_size(uint32_t n, uint32_t max_dsize);
int qlzx_decompress_batch(const qlzx_blocks *b, const uint32_t *dst_cap, uint32_t *dsize,
                          int32_t *status, const uint32_t *crc_state, const uint32_t *crc_expect,
                          uint32_t *crc_out, uint32_t max_dsize, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Compress: replaces CCompress (quicklz/cquicklz.go:23-42) per block.
 *   dst capacity per block must be >= src_len[i] + 400 (cquicklz.go:24).  The encoder may
 *                write anywhere in [0, src_len[i] + 400) of a destination (a speculative
 *                stored copy lands there before the parse decides); only [0, csize[i]) is
 *                the result, the bytes past it are unspecified.
 *   csize[i]     out: compressed size (0 + status on error)      (required)
 *   status[i]    out: enum qlzx_status                           (nullable)
 *   crc_state / crc_out: as above, over the *compressed* output (the value
 *   bytes of the record written by store/datafile.go:307-330).  Fused.
 *   max_len      upper bound on src_len over the batch
 * Values over 64 KiB (max_len > 65536) are encoded by a whole-GPU pass each, one at a time,
 * after the batch's smaller blocks; like the decoder, that phase synchronises `stream` several
 * times per large block, and the workspace grows by about 76 x max_len bytes (jump levels, sort
 * keys and scans; 3.99 GB at 50 MiB), included in qlzx_compress_workspace_size. */
#define QLZX_F_GO_COMPAT 1u /* Go quicklz.Compress(src, 3) output (quicklz.go:80-289): always a
                              9-byte header, bail-out counts the header, no 9-byte core minimum */
size_t qlzx_compress_workspace_size(uint32_t n, uint32_t max_len);
int qlzx_compress_batch(const qlzx_blocks *b, uint32_t *csize, int32_t *status,
                        const uint32_t *crc_state, uint32_t *crc_out, uint32_t max_len,
                        uint32_t flags, void *workspace, size_t workspace_bytes, void *stream);

#define QLZX_F_LEVEL1 2u    /* Go quicklz.Compress(src, 1) (quicklz.go:80-191): qlzx_compress1 only */

/* Single-block helper on the GPU with `flags` (used by the quicklz.Compress mirror);
 * same contract as qlz_compress. */
size_t qlzx_compress1(const void *source, char *destination, size_t size, uint32_t flags);

/* ---- Go quicklz level 1 (quicklz.go:80-191 and 291-431) ----
 * One lane per block with its hash tables in `workspace` (16-B aligned,
 * qlzx_go_l1_workspace_size(n) bytes for compress, qlzx_go_decompress_workspace_size(n)
 * for decompress; both bounded: launches of at most 65536 blocks reuse them).  Production gobeansdb writes level 3 through
 * cgo; these serve the Go Compress(src, 1) / Decompress surface.
 * compress:   dst capacity >= src_len + 400 per block; empty block -> QLZX_E_EMPTY
 *             (Go returns nil); output bytes = Go Compress(src, 1).
 * decompress: Go Decompress of stored streams (any level) and compressed level-1
 *             streams; QLZX_E_CORRUPT where Go would panic on an index, QLZX_E_LEVEL
 *             for compressed level 3 (use qlzx_decompress_batch) and levels 0/2. */
size_t qlzx_go_l1_workspace_size(uint32_t n);
int qlzx_go_l1_compress_batch(const qlzx_blocks *b, uint32_t *csize, int32_t *status, void *workspace,
                              size_t workspace_bytes, void *stream);
int qlzx_go_decompress_batch(const qlzx_blocks *b, const uint32_t *dst_cap, uint32_t *dsize, int32_t *status,
                             void *workspace, size_t workspace_bytes, void *stream);
/* Workspace of qlzx_go_decompress_batch (the decoder needs only the 16 KiB hashtable per
 * block; launches cover at most 65536 blocks and reuse it). */
size_t qlzx_go_decompress_workspace_size(uint32_t n);
/* Single-block Go Decompress of a stored or level-1 stream of source_len bytes into
 * destination (capacity dst_cap): returns the decompressed size (0 is a valid empty
 * result), QLZX_GO_ERROR on error; qlzx_last_status() then holds the block's
 * enum qlzx_status (QLZX_E_CORRUPT where Go panics) and qlzx_last_error() the reason. */
#define QLZX_GO_ERROR ((size_t)-1)
size_t qlzx_go_decompress1(const char *source, size_t source_len, void *destination, size_t dst_cap);

/* CRC32 of many buffers: out[i] = crc32_write(init ? init[i] : 0xffffffff, src_i) ^ (final_xor).
 * final_xor = 0 returns the raw state; 0xffffffff the store/crc32.go get() value. */
int qlzx_crc32_batch(const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                     uint32_t n, const uint32_t *init, uint32_t final_xor, uint32_t *out,
                     void *stream);

/* Synthetic workloads: block i = gen(seed, first_id + i) of src_len[i] bytes
 * written at dst + dst_off[i].  kind 0 = text-like, 1 = image-like.  Tables come from
 * gobeansdb_amd/synth.py (vocab bytes, vocab offsets[nwords+1], zipf cdf[nwords]). */
int qlzx_synth_batch(int kind, uint64_t seed, uint64_t first_id, uint8_t *dst,
                     const uint64_t *dst_off, const uint32_t *len, uint32_t n,
                     const uint8_t *vocab, const uint32_t *vocab_off, const uint32_t *zipf_cdf,
                     uint32_t nwords, void *stream);

/* ---- write-side record encode ----
 * Record CRC = ~crc_write(~0, header[4:24] ‖ key ‖ value) (store/datafile.go:66-88).
 * qlzx_compress_batch fuses the value's raw CRC (crc_state = 0, crc_out = ~raw);
 * this folds the header+key prefix in afterwards:
 *   out[i] = (raw_a[i] * x^(8 len_b[i]) ^ raw_b[i]) ^ final_xor
 * i.e. the raw state of A ‖ B from the raw state of A and the raw CRC (from 0) of B. */
int qlzx_crc32_combine(const uint32_t *raw_a, const uint32_t *raw_b, const uint32_t *len_b, uint32_t n,
                       uint32_t final_xor, uint32_t *out, void *stream);
/* dst[dst_off[i] ..+ len[i]) = src[src_off[i] ..+ len[i]) (record assembly, WriteRecord.append). */
int qlzx_copy_batch(const uint8_t *src, const uint64_t *src_off, const uint32_t *len, uint8_t *dst,
                    const uint64_t *dst_off, uint32_t n, void *stream);

/* ---- .data chunk replay ----
 * Replaces the DataStreamReader.Next loop of buildHintFromData
 * (store/datafile.go:202-277, store/bucket.go:89-117) over one chunk file that
 * is resident in device memory: the records the sequential reader would
 * return from `start` (a multiple of 256), in order, each with its offset and
 * sizeBroken (bytes skipped by the nextValid resync).  CRCs are verified
 * (store/datafile.go:161-168) as part of record discovery.
 *   max_key  MaxKeyLen (config/mc_config.go:6, 250); body_max BodyMax (50 MiB)
 *   rec_off / rec_broken: capacity size/256 + 1 entries
 *   result[0] = records found; result[1] = 1 if the reader stops on an error
 *   (unexpected EOF: partial header or truncated record) after them;
 *   result[2] = header-plausible slots, result[3] = CRC-valid slots. */
size_t qlzx_replay_workspace_size(uint64_t size);
int qlzx_replay_index(const uint8_t *data, uint64_t size, uint64_t start, uint32_t max_key, uint64_t body_max,
                      uint64_t *rec_off, uint32_t *rec_broken, uint32_t *result, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Around the batch decoder (Payload.Decompress of the FLAG_COMPRESS records, store/item.go:163-176),
 * without host parsing.  `result` is qlzx_replay_index's (result[0] = n records); `cap` the
 * capacity of rec_off and of every per-record array below.
 * qlzx_replay_plan: hdr[6 j..] = the 24-B header of record j (crc, ts, flag, ver, ksz, vsz); the
 *   compressed records in record order: comp_idx (record), comp_off/comp_len (body in `data`),
 *   comp_dsize (QuickLZ header dsize, quicklz.go:32-44; 0 if the body is shorter than a header),
 *   comp_dst_off (256-B-aligned offsets in one packed output buffer);
 *   totals[5] = {n, ncomp, max dsize, output bytes (lo, hi)} -- the only values a caller needs on
 *   the host (to size the output buffer and the decoder launch).
 * qlzx_replay_finish: after qlzx_decompress_batch over the ncomp compressed records (comp_status,
 *   comp_dsize = its dsize output): per record the flag (FLAG_COMPRESS cleared when the value
 *   decoded), value_len, where the value lives (in_out 1: outbuf + val_off, 0: data + val_off; a
 *   failed decode keeps the raw body, as the reference swallows the error) and Getvhash. */
size_t qlzx_replay_plan_workspace_size(uint32_t cap);
int qlzx_replay_plan(const uint8_t *data, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                     int32_t *hdr, uint32_t *comp_idx, uint64_t *comp_off, uint32_t *comp_len, uint32_t *comp_dsize,
                     uint64_t *comp_dst_off, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream);
int qlzx_replay_finish(const uint8_t *data, const uint64_t *rec_off, const uint32_t *result, const uint32_t *totals,
                       const uint32_t *comp_idx, const int32_t *comp_status, const uint32_t *comp_dsize,
                       const uint64_t *comp_dst_off, const uint8_t *outbuf, uint32_t cap, int32_t *flag,
                       int32_t *value_len, uint8_t *in_out, uint64_t *val_off, uint16_t *vhash, void *stream);

/* ---- batched record reads at known offsets (a multi-GET) ----
 * Replaces a loop of dataChunk.GetRecordByOffset (store/datachunk.go:150-169: readRecordAt,
 * store/datafile.go:114-170, then Payload.Decompress, store/item.go:163-176) over one chunk file
 * resident in device memory: Bucket.get -> GetRecordByPos per key of a memcache "get k1 k2 ..."
 * (store/bucket.go:405-499), GC's collision lookups (store/gc.go:300), anything driven by a hint
 * file.  Request i reads the record at rec_off[i]; requests are independent and may repeat.
 * Same shape as the replay: plan, read totals[5] back, qlzx_decompress_batch over the ncomp
 * compressed records (dst_cap = comp_dsize, no CRC arguments: the record CRC is verified in the
 * plan, before any QuickLZ header is believed), finish.  Nothing allocates; every launch goes on
 * `stream`.
 * enum qlzx_read_status: readRecordAt's checks in its order, the first failure is the verdict --
 *   ALIGN       rec_off % 256 != 0 (positions carry offsets in units of 256, store/leaf.go:56-65)
 *   EOF_HEADER  rec_off + 24 > size                 (store/datafile.go:123)
 *   KEY_SIZE    ksz == 0 || ksz > max_key           (:129, config/mc_config.go:33-35)
 *   VALUE_SIZE  vsz > body_max                      (:133)
 *   EOF_BODY    rec_off + 24 + ksz + vsz > size     (:149)
 *   CRC         ~crc(header[4:24] ‖ key ‖ value) != header[0:4]   (:161-168) */
enum qlzx_read_status {
    QLZX_RD_OK = 0,
    QLZX_RD_ALIGN,
    QLZX_RD_EOF_HEADER,
    QLZX_RD_KEY_SIZE,
    QLZX_RD_VALUE_SIZE,
    QLZX_RD_EOF_BODY,
    QLZX_RD_CRC
};
/* Workspace of qlzx_read_plan for n requests. */
size_t qlzx_read_plan_workspace_size(uint32_t n);
/* readRecordAt for every request, and the decode plan of those that passed.
 *   max_key / body_max: MaxKeyLen and BodyMax as in qlzx_replay_index (24 + max_key + body_max
 *   must stay below 4 GiB); size / 256 < 0xfffffff0.
 *   want_key / want_key_off / want_key_len (all three or none): the key the caller expects at
 *   request i, want_key[want_key_off[i] ..+ want_key_len[i]).  key_eq[i] (nullable iff no keys)
 *   = 1 iff rd_status[i] is OK and the record's key equals it (bytes.Compare,
 *   store/bucket.go:442).  A mismatch is not an error: the record is delivered and decoded, as
 *   the reference reads it before comparing (store/bucket.go:452-498 is the caller's part).
 *   rd_status[i]: enum qlzx_read_status.  hdr[6 i ..]: the stored header (crc, ts, flag, ver,
 *   ksz, vsz); zeros for ALIGN and EOF_HEADER.
 *   comp_*: as qlzx_replay_plan's, over the OK requests with FLAG_COMPRESS in request order
 *   (comp_idx = request index); capacity n each.
 *   totals[5] = {requests with rd_status OK, ncomp, max dsize, output bytes (lo, hi)}.
 * n == 0 zeroes totals and returns QLZX_R_OK. */
int qlzx_read_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t n, uint32_t max_key,
                   uint64_t body_max, const uint8_t *want_key, const uint64_t *want_key_off,
                   const uint32_t *want_key_len, int32_t *rd_status, uint8_t *key_eq, int32_t *hdr,
                   uint32_t *comp_idx, uint64_t *comp_off, uint32_t *comp_len, uint32_t *comp_dsize,
                   uint64_t *comp_dst_off, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream);
/* Payload.Decompress's outcome per request (store/item.go:163-176), after qlzx_decompress_batch
 * (comp_status, comp_dsize = its outputs).  OK requests, as qlzx_replay_finish: flag
 * (FLAG_COMPRESS cleared only when the value decoded), value_len, in_out / val_off (1: outbuf +
 * val_off, 0: data + val_off; a failed decode keeps the raw body and the flag, :167-170) and
 * Getvhash of the value as delivered.  dec_status[i]: the decoder's enum qlzx_status for a
 * compressed record (the error the reference only logs), QLZX_OK otherwise.  Failed requests get
 * flag = value_len = in_out = val_off = vhash = 0.  n == 0 returns QLZX_R_OK. */
int qlzx_read_finish(const uint8_t *data, const uint64_t *rec_off, uint32_t n, const int32_t *rd_status,
                     const uint32_t *totals, const uint32_t *comp_idx, const int32_t *comp_status,
                     const uint32_t *comp_dsize, const uint64_t *comp_dst_off, const uint8_t *outbuf,
                     int32_t *flag, int32_t *value_len, uint8_t *in_out, uint64_t *val_off, uint16_t *vhash,
                     int32_t *dec_status, void *stream);

/* ---- batched record writes (a multi-SET) ----
 * The mirror image of the batched read: Record.TryCompress (store/item.go:120-161), then
 * WriteRecord.encodeHeader / getCRC / append with the 256-B padding (store/datafile.go:66-88,
 * 307-330) for n records whose keys and values are resident in device memory, as
 * dataChunk.flush (store/datachunk.go:88-120) and AppendRecordGC (:56-79) run them once per
 * record.  Record i: value values[val_off[i] ..+ val_len[i]), key keys[key_off[i] ..+ key_len[i]),
 * flag[i], ver[i], ts[i].  Five calls, two small read-backs (totals, totals2):
 *   qlzx_write_plan; qlzx_compress_batch over the trial list (crc_state = zeros; skipped when
 *   ntry == 0); qlzx_write_decide; qlzx_compress_batch over the full list (crc_state = zeros;
 *   skipped when nfull == 0); qlzx_write_finish.
 * Device pointers only; nothing allocates; every launch goes on `stream`.  One workspace of
 * qlzx_write_plan_workspace_size(n) bytes serves the three calls (no state is carried in it).
 * enum qlzx_write_status: KEY_SIZE ksz == 0 || ksz > max_key, VALUE_SIZE vlen > body_max (the
 * limits qlzx_read_plan enforces: whatever this writes, that reads), NO_SPACE: the record would
 * end past out_cap (qlzx_write_finish; a memory-safety guard, nothing of it is written).
 * not_compress: the NotCompress set (store/item.go:114-118) as one bit per row of
 * http.DetectContentType's audio/video table (Go 1.13 net/http/sniff.go, table order) plus one
 * for every other answer; a record whose value's first bytes give a listed answer is not tried. */
enum qlzx_write_status { QLZX_WR_OK = 0, QLZX_WR_KEY_SIZE, QLZX_WR_VALUE_SIZE, QLZX_WR_NO_SPACE };
#define QLZX_NC_AUDIO_BASIC 0x01u
#define QLZX_NC_AUDIO_AIFF 0x02u
#define QLZX_NC_AUDIO_MPEG 0x04u
#define QLZX_NC_APPLICATION_OGG 0x08u
#define QLZX_NC_AUDIO_MIDI 0x10u
#define QLZX_NC_VIDEO_AVI 0x20u
#define QLZX_NC_AUDIO_WAVE 0x40u
#define QLZX_NC_OTHER 0x80u
#define QLZX_NC_DEFAULT (QLZX_NC_AUDIO_MPEG | QLZX_NC_AUDIO_WAVE) /* store/config_default.go:46-49 */
/* Workspace of the three qlzx_write_* calls for n records. */
size_t qlzx_write_plan_workspace_size(uint32_t n);
/* TryCompress's candidates and the trial list.
 *   wr_status[i]: OK, KEY_SIZE or VALUE_SIZE (24 + max_key + body_max + 9 + 256 must stay below
 *   4 GiB).  An OK record is a candidate iff ver >= 0, flag & (0x10 | 0x10000) == 0,
 *   pad256(24 + ksz + vlen) > 256 and the sniff of its value is not in not_compress.
 *   try_*: the candidates in record order (capacity n each): try_idx (record), try_off (in
 *   `values`), try_len = min(vlen, 10240), try_dst_off (256-B-aligned destinations try_len + 400
 *   apart in one packed trial buffer).
 *   totals[7] = {OK records, ntry, max try_len, trial buffer bytes (lo, hi), output bound bytes
 *   (lo, hi)}; the bound is the sum of pad256(24 + ksz + vlen + 9) over the OK records (a kept
 *   value can be a stored QuickLZ block, 9 bytes longer than the plain one).
 * n == 0 returns QLZX_R_OK; nothing is launched or written (totals included). */
int qlzx_write_plan(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len, const uint32_t *key_len,
                    const uint32_t *flag, const int32_t *ver, uint32_t n, uint32_t max_key, uint64_t body_max,
                    uint32_t not_compress, int32_t *wr_status, uint32_t *try_idx, uint64_t *try_off,
                    uint32_t *try_len, uint64_t *try_dst_off, uint32_t *totals, void *workspace,
                    size_t workspace_bytes, void *stream);
/* The ratio test and the full-recompress list, after qlzx_compress_batch over the trial list
 * (try_csize, try_status = its outputs; totals = qlzx_write_plan's, on the device).
 *   keep[k] (capacity n) = try_status[k] is QLZX_OK and float32(try_csize[k]) /
 *   float32(try_len[k]) <= 0.7f, IEEE single division and compare (store/item.go:145); a failed
 *   compress is "not compressed", as the reference's !ok branches.
 *   full_*: the kept trials with vlen > try_len, in record order (capacity n each): full_idx
 *   (record), full_off, full_len = vlen, full_dst_off (full_len + 400 apart).
 *   totals2[5] = {nkeep, nfull, max full_len, full buffer bytes (lo, hi)}.
 * n == 0 returns QLZX_R_OK; nothing is launched or written (totals2 included). */
int qlzx_write_decide(const uint64_t *val_off, const uint32_t *val_len, uint32_t n, const uint32_t *totals,
                      const uint32_t *try_idx, const uint32_t *try_len, const uint32_t *try_csize,
                      const int32_t *try_status, uint8_t *keep, uint32_t *full_idx, uint64_t *full_off,
                      uint32_t *full_len, uint64_t *full_dst_off, uint32_t *totals2, void *workspace,
                      size_t workspace_bytes, void *stream);
/* Sizes, flags, offsets, CRCs and the records themselves, after qlzx_compress_batch over the full
 * list (full_csize, full_status, full_crc = its outputs; a full compress that failed leaves the
 * value raw).  try_crc / full_crc: the compressor's crc_out for crc_state = 0.
 *   Records lie back to back in `out` (16-B aligned) from offset 0 in record order: rec_off[i] =
 *   the exclusive scan of pad256(24 + ksz + vsz) over the OK records; failed records take no
 *   space.  Each is crc ‖ ts ‖ flag ‖ ver ‖ ksz ‖ vsz ‖ key ‖ value ‖ zeros to 256, the value
 *   taken from `values`, trial_buf or full_buf (both nullable when their list is empty); the
 *   padding is written here, `out` need not be zeroed.  A record that would end past out_cap gets
 *   QLZX_WR_NO_SPACE in wr_status (in/out) and nothing of it is written.
 *   flag_out (FLAG_COMPRESS added where kept), vsz, crc = ~crc_write(~0, header[4:24] ‖ key ‖
 *   value); vhash (nullable) = Getvhash of the ORIGINAL value (CalcValueHash runs before
 *   TryCompress, store/item.go:102).  Records not written get rec_off = flag_out = vsz = crc =
 *   vhash = 0.  totals3[3] = {records written, bytes written (lo, hi)}.
 * n == 0 returns QLZX_R_OK; nothing is launched or written (totals3 included). */
int qlzx_write_finish(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len, const uint8_t *keys,
                      const uint64_t *key_off, const uint32_t *key_len, const uint32_t *flag, const int32_t *ver,
                      const uint32_t *ts, uint32_t n, const uint32_t *totals, const uint32_t *try_idx,
                      const uint32_t *try_len, const uint64_t *try_dst_off, const uint32_t *try_csize,
                      const uint32_t *try_crc, const uint8_t *keep, const uint8_t *trial_buf,
                      const uint32_t *totals2, const uint32_t *full_idx, const uint64_t *full_dst_off,
                      const uint32_t *full_csize, const int32_t *full_status, const uint32_t *full_crc,
                      const uint8_t *full_buf, uint8_t *out, uint64_t out_cap, int32_t *wr_status,
                      uint64_t *rec_off, uint32_t *flag_out, uint32_t *vsz, uint32_t *crc, uint16_t *vhash,
                      uint32_t *totals3, void *workspace, size_t workspace_bytes, void *stream);

/* ---- GC rewrite of a chunk ----
 * The record loop of GCMgr.gc (store/gc.go:268-353) over one source chunk resident in device
 * memory: every record the stream reader returned that the caller calls live is appended to the
 * destination in order, as dataChunk.AppendRecordGC -> WriteRecord.append does
 * (store/datachunk.go:56-79, store/datafile.go:307-330): the header re-encoded with its CRC
 * recomputed (store/datafile.go:66-88), zero padding to 256 B, and the next destination chunk
 * whenever recsize + writingHead > DataFileMax (store/gc.go:320-336; the reference moves once and
 * then appends whatever the size, so a record larger than data_file_max gets a chunk to itself).
 * rec_off / result / cap are qlzx_replay_index's outputs, used as qlzx_replay_plan uses them
 * (result[0] = the record count, read on the device; cap = the capacity of every per-record
 * array), so index -> qlzx_gc_plan -> qlzx_gc_rewrite needs no read-back and no synchronisation in
 * between.  rec_off is in append order; entries need not be increasing or distinct.  keep[j] != 0:
 * record j is live (the HTree / hint / collision lookups behind isNewest are the caller's).
 * chunk_head[c], c < max_chunks (1..998, MAX_NUM_CHUNK of store/data.go:15): the writingHead at
 * which destination chunk c starts (beginGCWriting, store/datachunk.go:185-199), taken as given.
 * Device pointers only; nothing allocates; every launch goes on `stream`.  One workspace of
 * qlzx_gc_workspace_size(cap, max_chunks) bytes serves both calls (no state is carried in it).
 * enum qlzx_gc_status: DROPPED keep[j] == 0; BAD_RECORD a kept record that fails readRecordAt's
 * size checks (rec_off % 256, header inside size, 1 <= ksz <= max_key, vsz <= body_max, body
 * inside size: store/datafile.go:123-149; the CRC is not a check here, see qlzx_gc_rewrite), it
 * takes no space and nothing past the failing check is read; NO_CHUNK the rotation would need
 * chunk max_chunks: that record and every later survivor; NO_SPACE the record would end past
 * out_cap (qlzx_gc_rewrite; a memory-safety guard, nothing of it is written). */
enum qlzx_gc_status { QLZX_GC_WRITTEN = 0, QLZX_GC_DROPPED, QLZX_GC_BAD_RECORD, QLZX_GC_NO_CHUNK, QLZX_GC_NO_SPACE };
/* Workspace of the two qlzx_gc_* calls. */
size_t qlzx_gc_workspace_size(uint32_t cap, uint32_t max_chunks);
/* Where every kept record goes.  data is 16-B aligned; size / 256 < 0xfffffff0; 24 + max_key +
 * body_max + 256 must stay below 4 GiB.
 *   gc_status[j]: WRITTEN (placed), DROPPED, BAD_RECORD or NO_CHUNK.
 *   new_chunk[j] / new_off[j]: the destination chunk of record j and its offset in that chunk
 *   measured from the chunk's start (the reference's newPos); 0 / 0 for a record not placed.
 *   chunk_bytes[c] / chunk_base[c] (max_chunks entries each): the bytes written into chunk c and
 *   their exclusive scan: chunk c's bytes, from its head on, lie packed at out + chunk_base[c].
 *   totals[8] = {records, keep requested, placed, chunks used (last index + 1; 0 if none placed),
 *   bytes (lo, hi), CRC mismatches (0 here), BAD_RECORD + NO_CHUNK + NO_SPACE}.
 *   The bytes never exceed pad256(size) when rec_off comes from qlzx_replay_index (its records
 *   are disjoint), so a caller may allocate that much for `out` and skip the read-back.
 * Entries j >= result[0] of the per-record arrays are not written.  cap == 0 returns QLZX_R_OK;
 * nothing is launched or written.  result[0] == 0 on the device gives zero totals. */
int qlzx_gc_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                 const uint8_t *keep, uint32_t max_key, uint64_t body_max, uint64_t data_file_max,
                 const uint64_t *chunk_head, uint32_t max_chunks, int32_t *gc_status, uint32_t *new_chunk,
                 uint64_t *new_off, uint64_t *chunk_base, uint64_t *chunk_bytes, uint32_t *totals, void *workspace,
                 size_t workspace_bytes, void *stream);
/* The records themselves, after qlzx_gc_plan (gc_status, new_chunk, new_off, chunk_base, totals =
 * its outputs, on the device).  Each WRITTEN record's 24 + ksz + vsz bytes are read once, its CRC
 * ~crc_write(~0, header[4:24] ‖ key ‖ value) is computed in the same pass, and bytes, zero
 * padding to 256 and the CRC word are written at out + chunk_base[c] + new_off - chunk_head[c];
 * `out` need not be zeroed.  data and out are 16-B aligned, and [out, out + out_cap) must not
 * overlap [data, data + size): the reference can rewrite a chunk onto itself, records written in
 * parallel cannot.
 *   crc[j]: the recomputed CRC, 0 for a record not written.  A recomputed CRC that differs from
 *   the stored word does not stop the write (WriteRecord.append always re-encodes); totals[6]
 *   counts those records.
 *   A record that would end past out_cap gets QLZX_GC_NO_SPACE in gc_status (in/out) and nothing
 *   of it is written; totals (in/out) [2], [4], [5] and [7] are adjusted.  new_chunk, new_off and
 *   the chunk arrays are inputs and keep the plan's values.
 * cap == 0 returns QLZX_R_OK; nothing is launched or written. */
int qlzx_gc_rewrite(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                    const uint64_t *chunk_head, uint32_t max_chunks, const uint32_t *new_chunk,
                    const uint64_t *new_off, const uint64_t *chunk_base, uint8_t *out, uint64_t out_cap,
                    int32_t *gc_status /* in/out */, uint32_t *crc, uint32_t *totals /* in/out */, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ---- Hint split file of a replayed chunk ----
 * getKeyHashDefalut (store/key.go:41-59) of n keys: out[i] = (uint64)fnv1a(key_i) << 32 |
 * murmur3_32(key_i, seed 0), fnv1a the sign-extending variant of store/key.go:47-55
 * (h ^= uint32(int8(b))), murmur3_32 MurmurHash3_x86_32 (little-endian 4-byte blocks, a 0..3 byte
 * tail, fmix32).  len[i] is 0..255; key i is the bytes src + off[i] .. + len[i], at any alignment.
 * n == 0 returns QLZX_R_OK. */
int qlzx_keyhash_batch(const uint8_t *src, const uint64_t *off, const uint32_t *len, uint32_t n, uint64_t *out,
                       void *stream);
/* The split file buildHintFromData (store/bucket.go:89-117) emits for a chunk, from the records
 * of a replay that are resident in device memory: HintBuffer.Set over the records in append order
 * (store/hint.go:121-161), HintBuffer.Dump's sort by (keyhash, key) (:181-208, byKeyHash.Less
 * :334-352), and hintFileWriter's head, items and index (store/hintfile.go:142-212,
 * store/hintindex.go:140-150).  One qlzx_hint_plan / qlzx_hint_write pair builds ONE split file;
 * a chunk with more than split_cap distinct keys takes one pair per split (hintChunk.setItem ->
 * rotate, store/hint.go:241-252): first += totals[0], max_offset_in = totals[3].
 * data / size / rec_off / result / cap as qlzx_gc_plan takes them (result[0] = the record count,
 * read on the device; n = min(result[0], cap)); hdr is qlzx_replay_plan's (6 ints per record: ver
 * = hdr[6j+3], ksz = hdr[6j+4], vsz = hdr[6j+5]), vhash qlzx_replay_finish's.  keyhash: NULL for
 * the default hash above of the key at data + rec_off[j] + 24, or one u64 per record (the
 * reference's replaceable getKeyHash).  Device pointers only; nothing allocates; every launch goes
 * on `stream`; no host synchronisation.  One workspace of qlzx_hint_workspace_size(cap) bytes
 * serves both calls (no state is carried in it; the radix sort's temporary storage lives there).
 * Over the records first .. n-1:
 *   - two records are one item iff keyhash and key bytes are equal; the item is the last of them
 *     below the cut (a later Set overwrites the slot);
 *   - the cut c is the first record that would be distinct item split_cap + 1 (Set returns false,
 *     store/hint.go:140-147); repeats of a taken key after the buffer is full are still taken.
 *     consumed = c - first, or n - first without a cut;
 *   - datasize = max(max_offset_in, uint32(rec_off[j]) + pad256(24 + ksz + vsz) over every taken
 *     record j < c, and uint32(rec_off[c]) when there is a cut);
 *   - items ascend by keyhash, then by key bytes, the shorter prefix first;
 *   - file: 16-B head {indexOffset i64, numKey u32, datasize u32}; per item 23 bytes {keyhash u64,
 *     chunk_id u32, offset u32, ver i32, vhash u16, ksz u8} and the key; item k at o_k = 16 + the
 *     exclusive scan of 23 + ksz; indexOffset = o_numKey; then 16 bytes {keyhash u64, offset i64}
 *     per index entry: walking the items with last = 0, item k is an entry when o_k - last >
 *     index_interval - 23 - 256 (signed 64-bit), and then last = o_k (store/hintfile.go:174-176);
 *   - a record with ksz == 0, ksz > 255 or rec_off + 24 + ksz > size is skipped: no item, no part
 *     in the cut or in datasize, nothing past the failing check is read (records from
 *     qlzx_replay_index never are).  totals[9] counts the skipped records among the consumed.
 * A run of equal keyhash is normally versions of one key and costs one key comparison per record;
 * a run with different keys (a 64-bit collision or a caller's keyhash) is ranked by one wave with
 * L^2 key comparisons for a run of L records: correct, not fast. */
#define QLZX_HINT_NO_SPACE 1
/* Workspace of the two qlzx_hint_* calls. */
size_t qlzx_hint_workspace_size(uint32_t cap);
/* The items, their order and file offsets, and the index entries.  size / 256 < 0xfffffff0;
 * split_cap >= 1 (Conf.SplitCap); index_interval = Conf.IndexIntervalSize.
 *   item_rec[k] / item_hash[k] / item_off[k]: record index, keyhash and file offset of sorted item
 *   k; index_item[m]: the item of index entry m (capacity cap each).
 *   totals[10] = {consumed, numKey, index entries, datasize, indexOffset (lo, hi), file bytes
 *   (lo, hi), 0, skipped}.  numKey == 0 (first >= n, or every record skipped): file bytes = 0, the
 *   reference never dumps an empty buffer (needDump, store/hint.go:210-212).
 * cap == 0 returns QLZX_R_OK; nothing is launched or written. */
int qlzx_hint_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                   const int32_t *hdr, const uint64_t *keyhash, uint32_t first, uint32_t split_cap,
                   int64_t index_interval, uint32_t max_offset_in, uint32_t *item_rec, uint64_t *item_hash,
                   uint64_t *item_off, uint32_t *index_item, uint32_t *totals, void *workspace, size_t workspace_bytes,
                   void *stream);
/* The file, after qlzx_hint_plan (item_rec .. totals = its outputs, on the device): head, items
 * and index, totals[6,7] bytes from `out` on; chunk_id goes into every item (buildHintFromData
 * passes 0).  `out` is 16-B aligned and need not be zeroed; no byte past the file's is written.
 * If the file exceeds out_cap nothing is written and totals[8] = QLZX_HINT_NO_SPACE, else
 * totals[8] = 0.  16 + 289 (n - first) bytes always suffice.  Whatever the plan arrays hold, every
 * access stays inside data, the arrays' cap entries and out_cap.
 * cap == 0 returns QLZX_R_OK; nothing is launched or written. */
int qlzx_hint_write(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t cap, const int32_t *hdr,
                    const uint16_t *vhash, uint32_t chunk_id, const uint32_t *item_rec, const uint64_t *item_hash,
                    const uint64_t *item_off, const uint32_t *index_item, uint8_t *out, uint64_t out_cap,
                    uint32_t *totals /* in/out */, void *workspace, size_t workspace_bytes, void *stream);

/* The merged hint file of a bucket and its collision items, from split files resident in device
 * memory: hintMgr.Merge (store/hint.go:455-508) -> merge / mergeWriter / mergeHeap.Less
 * (store/hintmerge.go) over hintFileReader.open / next and hintFileWriter.writeItem / close
 * (store/hintfile.go:57-212).  Conventions as the other qlzx_hint_* calls: device pointers only
 * (file_off / file_len / file_chunk included, one entry per source), nothing allocates, every
 * launch goes on `stream`, no host synchronisation and no read-back between plan and write, one
 * workspace of qlzx_hint_merge_workspace_size bytes serves both calls (no state is carried in it:
 * the write itself keeps nothing in it).
 * Source i is the bytes hints[file_off[i] .. + file_len[i]) at any alignment, file_chunk[i] its
 * reader's chunkID.
 *   - reading: head {indexOffset i64, numKey u32, datasize u32}; indexOffset == 0 means "no index"
 *     and the items run to the file's end; numKey is not used; an item starts at every offset from
 *     16 on below indexOffset: 23 bytes {keyhash u64, chunk u32, offset u32, ver i32, vhash u16,
 *     ksz u8} and ksz key bytes.  An item that starts below indexOffset and ends inside the file is
 *     read whole.  The stored chunk is ignored: the item's position is (file_chunk[i], offset).
 *   - QLZX_HM_BAD_FILE (totals[9] = the lowest such source): file_len < 16, the source runs past
 *     `bytes`, indexOffset negative or > file_len, an item ends past the file, or no item at all
 *     (merge dereferences a nil first item; no writer dumps an empty buffer).
 *   - merged items: one per distinct (keyhash, key bytes); among equal keys the largest CmpKey =
 *     chunk << 32 | offset wins (unsigned), on a tie the later source, then the later item; items
 *     ascend by keyhash, then by key bytes, the shorter prefix first.  For sources that ascend
 *     strictly by (keyhash, key) this is what the heap merge produces.  A source whose adjacent
 *     items do not ascend strictly is refused: QLZX_HM_UNSORTED (totals[9] = the lowest one).
 *   - QLZX_HM_TOO_MANY: the sources hold more than cap items.  Precedence: BAD_FILE, TOO_MANY,
 *     UNSORTED; with any of them numKey, index entries, file bytes and collision items are 0 and
 *     qlzx_hint_merge_write writes nothing and keeps the status.
 *   - collisions (mergeWriter.flush): every merged item whose keyhash is shared by two or more
 *     distinct keys, in merged order; CollisionTable.compareAndSet stays the caller's.
 *   - file: head with datasize = the largest of the sources' heads'; per item its 23 + ksz source
 *     bytes with bytes 8..11 replaced by item_chunk; indexOffset and the sparse index as
 *     qlzx_hint_plan states them.
 * The sources' own index sections only cut the (serial) walk over a source into stretches, and only
 * once proven: entries strictly increasing inside [16, indexOffset), every walk landing exactly on
 * the next entry, the last one reaching indexOffset.  A source that fails, or has no index, is
 * walked from 16 by one lane: correct, not fast.  The result never depends on an index section.
 * Whatever the bytes hold, every load stays inside hints[0, bytes) and the arrays' cap entries,
 * every store inside the arrays and out_cap, and every walk advances 23 bytes or more per step. */
enum qlzx_hm_status { QLZX_HM_OK = 0, QLZX_HM_NO_SPACE, QLZX_HM_BAD_FILE, QLZX_HM_TOO_MANY, QLZX_HM_UNSORTED };
/* Workspace of the two qlzx_hint_merge_* calls (`bytes` does not enter it today). */
size_t qlzx_hint_merge_workspace_size(uint64_t bytes, uint32_t n_files, uint32_t cap);
/* The plan; alone it is Merge(forGC = true): the collision items and no file.  cap = the capacity
 * of every per-item array.
 *   item_src[k]: the byte offset in `hints` of the source item that became merged item k;
 *   item_chunk[k]: its chunk id; item_off[k]: its offset in the merged file; index_item[m]: the
 *   item of index entry m; coll_item[c]: the merged item of collision item c, ascending.
 *   totals[12] = {items read, numKey, index entries, datasize, indexOffset (lo, hi), file bytes
 *   (lo, hi), status, the source the status names, collision items, 0}.
 * n_files == 0 or cap == 0 returns QLZX_R_OK; nothing is launched or written. */
int qlzx_hint_merge_plan(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                         const uint32_t *file_chunk, uint32_t n_files, uint32_t cap, int64_t index_interval,
                         uint64_t *item_src, uint32_t *item_chunk, uint64_t *item_off, uint32_t *index_item,
                         uint32_t *coll_item, uint32_t *totals, void *workspace, size_t workspace_bytes,
                         void *stream);
/* The file, after qlzx_hint_merge_plan: totals[6,7] bytes from `out` on.  `out` is 16-B aligned
 * and need not be zeroed; no byte past the file's is written.  If the file exceeds out_cap nothing
 * is written and totals[8] = QLZX_HM_NO_SPACE; a status of the plan stays.  16 + 39 cap + 22 bytes
 * always suffice when cap = (the sum of file_len - 16) / 23.  cap == 0 returns QLZX_R_OK. */
int qlzx_hint_merge_write(const uint8_t *hints, uint64_t bytes, uint32_t cap, const uint64_t *item_src,
                          const uint32_t *item_chunk, const uint64_t *item_off, const uint32_t *index_item,
                          uint8_t *out, uint64_t out_cap, uint32_t *totals /* in/out */, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Key lookups through hint files resident in device memory: hintMgr.getItem (store/hint.go:570-596)
 * -> hintChunk.get (:270-296) -> hintFileIndex.get (store/hintindex.go:28-69) over
 * hintFileReader.next (store/hintfile.go:89-124), n requests at once.  Conventions as the other
 * qlzx_hint_* calls: device pointers only, nothing allocates, every launch goes on `stream`, no
 * host synchronisation and no read-back.
 * The files are described as qlzx_hint_merge_plan's sources (one buffer, file_off / file_len at any
 * alignment, file_chunk).  THE ORDER OF THE FILES IS THE SEARCH ORDER: a binding lists a bucket as
 * getItem reaches it, newest chunk first, a chunk's splits last to first, the merged file where
 * `i <= collisions.Chunk` first holds.  file_flags[i] & QLZX_HL_FILE_MERGED marks the merged file:
 * a hit there reports the chunk stored in the item (a split hit reports file_chunk[i]), and no
 * file after it is searched.  Request i is the key keys + key_off[i] .. + key_len[i] (any length;
 * a key over 255 bytes equals no stored key and takes the same walk) with the hash keyhash[i], or,
 * keyhash == NULL, getKeyHashDefalut of the key (qlzx_keyhash_batch's kernel, into the workspace).
 * One file (hintFileIndex.get), every field little-endian and at any alignment:
 *   - the index is the (file_len - indexOffset) / 16 entries {keyhash u64, offset i64} from
 *     indexOffset on; j = sort.Search over them with Go's own loop (i, j = 0, n; h = (i + j) / 2;
 *     entry h's keyhash < the wanted one moves i = h + 1, else j = h), so j is defined on unsorted
 *     entries too.  The scan starts at entry j - 1's offset when j > 1, else at 16.
 *   - the scan reads items {keyhash u64, chunk u32, offset u32, ver i32, vhash u16, ksz u8, key}
 *     and ends after indexOffset - 16 bytes CONSUMED, not at indexOffset (after Seek the reader's
 *     own offset is still 16): from a start above 16 it walks on into the index section and reads
 *     index entries as items.  Per item: a 23-byte head or ksz key bytes that run past file_len are
 *     QLZX_HL_ERR, decided before the item is compared; keyhash below the wanted one: next item;
 *     above: QLZX_HL_MISS; equal: the key bytes decide between QLZX_HL_FOUND and the next item.
 *   - QLZX_HL_ERR also answers an index entry's offset outside [16, file_len]: the reference's
 *     behaviour there depends on the position its file descriptor was left at, and no writer
 *     produces such an entry.
 *   - QLZX_HL_BAD_FILE, what loadHintIndex would not have survived: file_len < 16, the file runs
 *     past `bytes`, indexOffset outside [16, file_len], (file_len - indexOffset) % 16 != 0.
 *   - QLZX_HL_ERR and QLZX_HL_BAD_FILE end that request's search (an error ends getItem), a hit
 *     ends it, a miss goes on to the next file.  With files every writer produces, a key whose
 *     hash lies above a file's last item usually ends in QLZX_HL_ERR once the file has two or more
 *     index entries.
 * flags: 0 is the reference as it is.  QLZX_HL_F_BOUNDED ends the scan at indexOffset by position
 * (what the code meant): a key above the last item is a miss and the search goes on.
 * Two kernels give the same results: a wave per request below QLZX_HL_LANE_FROM requests, a lane
 * per request from there on (DESIGN.md §3.6 has the two measured).  QLZX_HL_F_WAVE or
 * QLZX_HL_F_LANE (not both) names the kernel whatever n is.
 * Per request: status[i]; hit_file[i] = the file where the search ended (the last one searched for
 * a miss); for QLZX_HL_FOUND chunk / offset / ver / vhash of the item and item_src = its byte offset
 * in `hints`, else those five are 0.  totals[4] = {found, miss, err, bad_file}.
 * Whatever the bytes hold, every load stays inside hints[0, bytes) and inside the file being
 * searched, every store inside the n entries of the outputs and totals[4], and every walk advances
 * 23 bytes or more per step.
 * n == 0 or n_files == 0 returns QLZX_R_OK and nothing is launched or written: without a file every
 * request is a miss, and the outputs of that answer (all zero, totals {0, n, 0, 0}) are the
 * caller's to set. */
enum qlzx_hl_status { QLZX_HL_MISS = 0, QLZX_HL_FOUND, QLZX_HL_ERR, QLZX_HL_BAD_FILE };
#define QLZX_HL_FILE_MERGED 1u
#define QLZX_HL_F_BOUNDED 1u
#define QLZX_HL_F_LANE 2u
#define QLZX_HL_F_WAVE 4u
#define QLZX_HL_LANE_FROM 16384u
size_t qlzx_hint_lookup_workspace_size(uint32_t n, uint32_t n_files);
int qlzx_hint_lookup(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                     const uint32_t *file_chunk, const uint32_t *file_flags, uint32_t n_files, const uint8_t *keys,
                     const uint64_t *key_off, const uint32_t *key_len, const uint64_t *keyhash /* or NULL */,
                     uint32_t n, uint32_t flags, int32_t *status, uint32_t *hit_file, uint32_t *chunk,
                     uint32_t *offset, int32_t *ver, uint16_t *vhash, uint64_t *item_src, uint32_t *totals /* [4] */,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Getvhash (store/item.go:89-100, Fnv1a of utils/hash.go:8-16) of n values. */
int qlzx_vhash_batch(const uint8_t *src, const uint64_t *off, const uint32_t *len, uint32_t n, uint16_t *out,
                     void *stream);

/* enum qlzx_status of the calling thread's last single-block call (qlz_decompress,
 * qlzx_compress1, qlzx_go_decompress1). */
int qlzx_last_status(void);

/* Last error message of the calling thread (empty if none). */
const char *qlzx_last_error(void);

/* One record read in ONE request, as readRecordAt + Payload.Decompress use it
 * (store/datafile.go:161-168, store/item.go:163-176): the record CRC continued from `crc_state`
 * (crc32_write from ~0 over header[4:24] then the key) over the `vlen` value bytes is checked
 * against the stored `crc_expect` (~state == crc_expect), and only then, when `compressed`
 * (FLAG_COMPRESS), the value is decompressed into dst (dst_cap >= its dsize).  Replaces the
 * value's crc32_write and the qlz_decompress of the same GET (two GPU round trips) with one.
 * *status: QLZX_OK, QLZX_E_CRC (nothing decoded), or the decode status; *out_len: the value's
 * length after the step (vlen when not compressed, which is not copied).  Returns a qlzx_return
 * code (runtime failure). */
int qlzx_read_record1(const void *value, size_t vlen, uint32_t crc_state, uint32_t crc_expect, int compressed,
                      void *dst, size_t dst_cap, size_t *out_len, int32_t *status);

/* Library/version info: fills `buf` with a short description (arch, kernels, source hash). */
int qlzx_info(char *buf, size_t len);

/* INTERNAL test hook, inert unless the process was started with QLZX_TEST_HOOKS=1 (read once;
 * otherwise it returns QLZX_R_BAD_ARG and changes nothing).
 * For the request path behind the drop-ins (values <= 64 KiB): the next batch the
 * current device's service launches fails -- mode 1: its kernel runs but publishes no
 * completion (caught through the batch event), mode 2: the launch itself fails.  Every request
 * of that batch then fails with QLZX_R_HIP (qlzx_compress1 returns 0, the quicklz.h drop-ins
 * stop the process).  For qlzx_decompress_batch: mode 3 / 4 makes its next K1 / K2 launch fail,
 * and the call returns QLZX_R_HIP.  Returns a qlzx_return code. */
int qlzx_service_test_fault(int mode);

#ifdef __cplusplus
}
#endif
#endif
