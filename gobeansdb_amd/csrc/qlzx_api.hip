// qlzx_api.hip -- the C ABI of libqlzx.so (declared in include/qlzx.h): the batch entry points'
// argument checks and dispatch.  The whole-GPU drivers for values over 64 KiB sit with their
// kernels (qlzx_decode_huge.hip, qlzx_encode_huge.hip), the batch decoder's launcher in
// qlzx_decode_batch.hip, the workgroup encoder's (launch_encode_wg, launch_encode_wg_class) in
// qlzx_encode_wg.hip, the single-call entry points in qlzx_single.hip.  The three encoders take the
// format's rules (hash, match token, bail-out test, header) from qlzx_encode_fmt.h.  The
// position-parallel decoders (qlzx_decode_solo.h and qlzx_decode_small.h, which hold no kernel and
// run inside the request service's k_svc_decode, and qlzx_decode_huge.hip) take theirs from
// qlzx_decode_fmt.h.
//
// Unity build: the kernel sources are included here so the device tables
// (qlzx_tables.hip) link without relocatable device code.  The five record-file sources
// (replay, read, write, gc, hint) share qlzx_recfile.h; read also uses replay's k_rp_crc_long,
// ScatterComp and finish kernels.  The four hint sources (hint, hintmerge, hintlookup, htree) share
// qlzx_hint_fmt.h, hintmerge and htree also qlzx_hint_walk.h; each includes what it uses itself:
// their order here does not matter.  htree's entry points are declared in include/qlzx_htree.h.
// htree_get (the queries over a built tree, include/qlzx_htree_get.h) uses htree's HtGeo and
// comes after it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "qlzx_tables.hip"
#include "qlzx_crc.hip"
#include "qlzx_synth.hip"
#include "qlzx_decode_solo.h"
#include "qlzx_decode_small.h"
#include "qlzx_decode_batch.hip"
#include "qlzx_decode_lane8.hip"
#include "qlzx_decode_huge.hip"
#include "qlzx_encode_lane.hip"
#include "qlzx_encode_wg.hip"
#include "qlzx_encode_huge.hip"
#include "qlzx_replay.hip"
#include "qlzx_read.hip"
#include "qlzx_write.hip"
#include "qlzx_gc.hip"
#include "qlzx_hint.hip"
#include "qlzx_hintmerge.hip"
#include "qlzx_hintlookup.hip"
#include "qlzx_htree.hip"
#include "qlzx_htree_get.hip"
#include "qlzx_record.hip"
#include "qlzx_level1.hip"
#include "qlzx_host.h"
#include "qlzx_service.hip"
#include "qlzx_single.hip"

static constexpr uint32_t kMaxLaneSlabs = 4096;  // concurrent lane encoders for the general path

#ifdef QLZX_PROFILE
namespace qlzx {
int k2_profile_set(void *dev_buf);  // qlzx_k2.hip
}
extern "C" int qlzx_profile_set(void *dev_buf) {  // g_prof of both translation units
    if (const int e = (int)hipMemcpyToSymbol(HIP_SYMBOL(qlzx::g_prof), &dev_buf, sizeof(void *))) return e;
    return qlzx::k2_profile_set(dev_buf);
}
#endif

// What the record-file entry points (replay, read, write, gc, hint) repeat: `who` is the
// function's name, the error text "<who>: <what>".
static int fail_in(int code, const char *who, const char *what) {
    return fail(code, (std::string(who) + ": " + what).c_str());
}
// slot numbers are 32 bits wide in the kernels
static int check_chunk_size(const char *who, uint64_t size) {
    return size / 256 >= 0xfffffff0ull ? fail_in(QLZX_R_BAD_ARG, who, "file too large") : QLZX_R_OK;
}
// every layout places its arrays at multiples of 256 from the base, so the base's own alignment is
// what each array gets: 16 bytes, the widest access into any of them (qlzx.h, batch API preamble)
static bool workspace_aligned(const void *workspace) { return (((uintptr_t)workspace) & 15u) == 0; }
static int check_workspace(const char *who, const void *workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need) return fail_in(QLZX_R_WORKSPACE, who, "workspace too small");
    return workspace_aligned(workspace) ? QLZX_R_OK : fail_in(QLZX_R_WORKSPACE, who, "workspace not 16-byte aligned");
}
// the tail of an entry point: e = what its launcher returned (a hipError_t)
static int launched(const char *who, int e) { return e ? fail(QLZX_R_HIP, who, (hipError_t)e) : QLZX_R_OK; }

extern "C" {

const char *qlzx_last_error(void) { return t_last_error.c_str(); }

#ifndef QLZX_SRC_HASH
#define QLZX_SRC_HASH "unknown"
#endif
// the source hash of the build (gobeansdb_amd/build.py source_hash); also greppable in the binary
extern __attribute__((used)) const char qlzx_src_hash_tag[] = "qlzx-src-hash:" QLZX_SRC_HASH;

int qlzx_info(char *buf, size_t len) {
    const char *s =
        "libqlzx: QuickLZ 1.4.1 level 3 + record CRC32 for gobeansdb; target gfx950 (MI355X); "
        "decode: wave-per-block LDS history (dsize<=" QLZX_STR(QLZX_FAST_MAX_DSIZE)
        ") + lane-per-block general; encode: workgroup-per-block position-parallel "
        "(len<=" QLZX_STR(QLZX_WG_MAX_LEN) ") + lane-per-block general; src " QLZX_SRC_HASH;
    if (!buf || !len) return (int)strlen(s);
    snprintf(buf, len, "%s", s);
    return 0;
}

/* ---------------- quicklz.h drop-in: header helpers (quicklz.c:674-690) ---------------- */
size_t qlz_size_decompressed(const char *source) {
    const unsigned char *s = (const unsigned char *)source;
    return (s[0] & 2) ? ld32h(s + 5) : s[2];
}
size_t qlz_size_compressed(const char *source) {
    const unsigned char *s = (const unsigned char *)source;
    return (s[0] & 2) ? ld32h(s + 1) : s[1];
}
int qlz_get_setting(int setting) {  // quicklz.c:31-58 as built by quicklz.h:25-31
    switch (setting) {
        case 0: return 3;       // QLZ_COMPRESSION_LEVEL
        case 1: return 528400;  // QLZ_SCRATCH_COMPRESS
        case 2: return 16;      // QLZ_SCRATCH_DECOMPRESS
        case 3: return 0;       // QLZ_STREAMING_BUFFER
        case 6: return 0;       // QLZ_MEMORY_SAFE (the reference build); this library always checks
        case 7: return 1;
        case 8: return 4;
        case 9: return 1;
    }
    return -1;
}

/* ---------------- batch device API ---------------- */

size_t qlzx_decompress_workspace_size(uint32_t n, uint32_t max_dsize) {
    // two regions for batches of more than one chunk: K1/K2 of consecutive chunks overlap (three
    // for mixed sizes over three chunks or more: the last chunk's K1 starts first)
    const qlzx::BatchLayout L = qlzx::batch_layout(n, max_dsize);
    size_t ws = L.regions * L.one;
    if (max_dsize > QLZX_FAST_MAX_DSIZE)  // large values: the pending list and the whole-GPU decoder
        ws += align_up((size_t)n * sizeof(qlzx::HugeItem) + 256, 256) + qlzx::huge_ws_layout(max_dsize, nullptr, nullptr);
    return ws;
}

int qlzx_decompress_batch(const qlzx_blocks *b, const uint32_t *dst_cap, uint32_t *dsize,
                          int32_t *status, const uint32_t *crc_state, const uint32_t *crc_expect,
                          uint32_t *crc_out, uint32_t max_dsize, void *workspace,
                          size_t workspace_bytes, void *stream) {
    if (!b || !status) return fail(QLZX_R_BAD_ARG, "qlzx_decompress_batch: null blocks/status");
    if (b->n == 0) return QLZX_R_OK;
    if (!b->src || !b->src_off || !b->src_len || !b->dst || !b->dst_off)
        return fail(QLZX_R_BAD_ARG, "qlzx_decompress_batch: null block array");
    if (workspace && !workspace_aligned(workspace))
        return fail(QLZX_R_WORKSPACE, "qlzx_decompress_batch: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // no workspace: the general lane-per-block kernel for every block
    const bool fast = workspace && workspace_bytes >= qlzx::batch_layout(b->n, max_dsize).one;
    if (fast) {
        int r = qlzx::launch_decode_wave(*b, dst_cap, dsize, status, crc_state, crc_expect, crc_out,
                                         max_dsize, workspace, workspace_bytes, s);
        if (r) return fail(QLZX_R_HIP, "decode_wave launch", (hipError_t)r);
    }
    if (fast && max_dsize > QLZX_FAST_MAX_DSIZE &&
        workspace_bytes >= qlzx_decompress_workspace_size(b->n, max_dsize)) {
        // large values: the whole-GPU decoder, one value at a time (synchronises the stream)
        const size_t wave = qlzx_decompress_workspace_size(b->n, QLZX_FAST_MAX_DSIZE);
        return qlzx::launch_decode_huge(*b, crc_state, crc_expect, crc_out, status, dsize, max_dsize,
                                        (uint8_t *)workspace + wave, s);
    }
    if (!fast || max_dsize > QLZX_FAST_MAX_DSIZE) {
        const uint32_t min_dsize = fast ? QLZX_FAST_MAX_DSIZE + 1 : 0;
        hipLaunchKernelGGL(qlzx::k_dec_lane8, dim3((b->n + 255) / 256), dim3(256), 0, s, *b, dst_cap,
                           dsize, status, crc_state, crc_expect, crc_out, min_dsize, max_dsize);
        HIP_OK(hipGetLastError());
    }
    return QLZX_R_OK;
}

size_t qlzx_compress_workspace_size(uint32_t n, uint32_t max_len) {
    // at least one lane slab: QLZX_F_GO_COMPAT batches (flags are not known here) take the lane path
    size_t ws = std::max(qlzx::kLaneSlab, qlzx::encode_wg_ws_bytes(n, max_len));
    if (max_len > QLZX_WG_MAX_LEN)  // values over 64 KiB: the pending list and the whole-GPU encoder
        ws += align_up((size_t)std::max<uint32_t>(n, 1) * sizeof(qlzx::HeItem) + 256, 256) +
              qlzx::he_ws_layout(max_len, nullptr, nullptr);
    return ws;
}

int qlzx_compress_batch(const qlzx_blocks *b, uint32_t *csize, int32_t *status,
                        const uint32_t *crc_state, uint32_t *crc_out, uint32_t max_len,
                        uint32_t flags, void *workspace, size_t workspace_bytes, void *stream) {
    if (!b || !csize) return fail(QLZX_R_BAD_ARG, "qlzx_compress_batch: null blocks/csize");
    if (b->n == 0) return QLZX_R_OK;
    if (!b->src || !b->src_off || !b->src_len || !b->dst || !b->dst_off)
        return fail(QLZX_R_BAD_ARG, "qlzx_compress_batch: null block array");
    if (int r = check_workspace("qlzx_compress_batch", workspace, workspace_bytes,
                                qlzx_compress_workspace_size(b->n, max_len)))
        return r;
    hipStream_t s = (hipStream_t)stream;
    const bool wg = !(flags & QLZX_F_GO_COMPAT);
    const bool huge = max_len > QLZX_WG_MAX_LEN;  // values over 64 KiB: qlzx_encode_huge.hip
    if (wg) {
        int r = qlzx::launch_encode_wg(*b, csize, status, crc_state, crc_out, max_len, workspace, s);
        if (r) return fail(QLZX_R_HIP, "encode_wg launch", (hipError_t)r);
    }
    if (!wg) {  // the lane encoder: Go-compat batches up to 64 KiB
        const uint32_t nl = (uint32_t)std::min<size_t>(
            std::min<uint32_t>(b->n, kMaxLaneSlabs), workspace_bytes / qlzx::kLaneSlab);
        if (nl == 0) return fail(QLZX_R_WORKSPACE, "qlzx_compress_batch: no lane slab");
        hipLaunchKernelGGL(qlzx::k_encode_lane, dim3((nl + 63) / 64), dim3(64), 0, s, *b, csize, status,
                           crc_state, crc_out, (uint8_t *)workspace, nl, huge ? (uint32_t)QLZX_WG_MAX_LEN : 0u,
                           flags);
        HIP_OK(hipGetLastError());
    }
    if (huge)  // after the kernels above in stream order: the whole workspace is free again
        return qlzx::launch_encode_huge(*b, csize, status, crc_state, crc_out, flags, max_len, (uint8_t *)workspace, s);
    return QLZX_R_OK;
}

size_t qlzx_go_l1_workspace_size(uint32_t n) {
    return (size_t)std::min<uint32_t>(std::max<uint32_t>(n, 1), qlzx::kL1Chunk) * qlzx::kL1WsBlock;
}
size_t qlzx_go_decompress_workspace_size(uint32_t n) {
    return (size_t)std::min<uint32_t>(std::max<uint32_t>(n, 1), qlzx::kL1Chunk) * qlzx::kL1DecWsBlock;
}

static int check_l1_args(const qlzx_blocks *b, const void *out, void *workspace, size_t workspace_bytes,
                         size_t need, const char *who) {
    if (!b || !out) return fail(QLZX_R_BAD_ARG, who);
    if (b->n == 0) return QLZX_R_OK;
    if (!b->src || !b->src_off || !b->src_len || !b->dst || !b->dst_off) return fail(QLZX_R_BAD_ARG, who);
    if (!workspace || (((uintptr_t)workspace) & 15u) || workspace_bytes < need) return fail(QLZX_R_WORKSPACE, who);
    return QLZX_R_OK;
}

int qlzx_go_l1_compress_batch(const qlzx_blocks *b, uint32_t *csize, int32_t *status, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (int r = check_l1_args(b, csize, workspace, workspace_bytes, qlzx_go_l1_workspace_size(b ? b->n : 0),
                              "qlzx_go_l1_compress_batch"))
        return r;
    // chunks of kL1Chunk blocks reuse the workspace (same stream: in order)
    for (uint32_t first = 0; first < b->n; first += qlzx::kL1Chunk) {
        const uint32_t cnt = std::min<uint32_t>(b->n - first, qlzx::kL1Chunk);
        hipLaunchKernelGGL(qlzx::k_enc_go_l1, dim3((cnt + 63) / 64), dim3(64), 0, (hipStream_t)stream, *b, csize,
                           status, (uint8_t *)workspace, first, cnt);
        HIP_OK(hipGetLastError());
    }
    return QLZX_R_OK;
}

int qlzx_go_decompress_batch(const qlzx_blocks *b, const uint32_t *dst_cap, uint32_t *dsize, int32_t *status,
                             void *workspace, size_t workspace_bytes, void *stream) {
    if (int r = check_l1_args(b, status, workspace, workspace_bytes, qlzx_go_decompress_workspace_size(b ? b->n : 0),
                              "qlzx_go_decompress_batch"))
        return r;
    for (uint32_t first = 0; first < b->n; first += qlzx::kL1Chunk) {
        const uint32_t cnt = std::min<uint32_t>(b->n - first, qlzx::kL1Chunk);
        hipLaunchKernelGGL(qlzx::k_dec_go_l1, dim3((cnt + 63) / 64), dim3(64), 0, (hipStream_t)stream, *b, dst_cap,
                           dsize, status, (uint8_t *)workspace, first, cnt);
        HIP_OK(hipGetLastError());
    }
    return QLZX_R_OK;
}

int qlzx_crc32_batch(const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len, uint32_t n,
                     const uint32_t *init, uint32_t final_xor, uint32_t *out, void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!src || !src_off || !src_len || !out) return fail(QLZX_R_BAD_ARG, "qlzx_crc32_batch: null arg");
    hipLaunchKernelGGL(qlzx::k_crc32, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, src_off,
                       src_len, n, init, final_xor, out);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

int qlzx_synth_batch(int kind, uint64_t seed, uint64_t first_id, uint8_t *dst, const uint64_t *dst_off,
                     const uint32_t *len, uint32_t n, const uint8_t *vocab, const uint32_t *vocab_off,
                     const uint32_t *zipf_cdf, uint32_t nwords, void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!dst || !dst_off || !len || !vocab || !vocab_off || !zipf_cdf || nwords == 0)
        return fail(QLZX_R_BAD_ARG, "qlzx_synth_batch: null arg");
    hipLaunchKernelGGL(qlzx::k_synth, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, kind, seed,
                       first_id, dst, dst_off, len, n, vocab, vocab_off, zipf_cdf, nwords);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

int qlzx_crc32_combine(const uint32_t *raw_a, const uint32_t *raw_b, const uint32_t *len_b, uint32_t n,
                       uint32_t final_xor, uint32_t *out, void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!raw_a || !raw_b || !len_b || !out) return fail(QLZX_R_BAD_ARG, "qlzx_crc32_combine: null arg");
    hipLaunchKernelGGL(qlzx::k_crc_combine, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw_a, raw_b,
                       len_b, n, final_xor, out);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

int qlzx_copy_batch(const uint8_t *src, const uint64_t *src_off, const uint32_t *len, uint8_t *dst,
                    const uint64_t *dst_off, uint32_t n, void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!src || !src_off || !len || !dst || !dst_off) return fail(QLZX_R_BAD_ARG, "qlzx_copy_batch: null arg");
    hipLaunchKernelGGL(qlzx::k_copy_blocks, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, src, src_off, len,
                       dst, dst_off, n);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

size_t qlzx_replay_workspace_size(uint64_t size) { return qlzx::replay_ws_layout(size, nullptr, nullptr); }

int qlzx_replay_index(const uint8_t *data, uint64_t size, uint64_t start, uint32_t max_key, uint64_t body_max,
                      uint64_t *rec_off, uint32_t *rec_broken, uint32_t *result, void *workspace,
                      size_t workspace_bytes, void *stream) {
    if ((!data && size) || !rec_off || !rec_broken || !result)
        return fail(QLZX_R_BAD_ARG, "qlzx_replay_index: null arg");
    if (start % 256 != 0 || start > size) return fail(QLZX_R_BAD_ARG, "qlzx_replay_index: start not a slot");
    if (int r = check_chunk_size("qlzx_replay_index", size)) return r;
    if (int r = check_workspace("qlzx_replay_index", workspace, workspace_bytes, qlzx_replay_workspace_size(size))) return r;
    return launched("qlzx_replay_index", qlzx::launch_replay_index(data, size, start, max_key, body_max, rec_off,
                    rec_broken, result, workspace, (hipStream_t)stream));
}

size_t qlzx_replay_plan_workspace_size(uint32_t cap) { return qlzx::replay_plan_ws_layout(cap, nullptr, nullptr, nullptr); }

int qlzx_replay_plan(const uint8_t *data, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                     int32_t *hdr, uint32_t *comp_idx, uint64_t *comp_off, uint32_t *comp_len, uint32_t *comp_dsize,
                     uint64_t *comp_dst_off, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (!rec_off || !result || !hdr || !comp_idx || !comp_off || !comp_len || !comp_dsize || !comp_dst_off || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_replay_plan: null arg");
    // data may be null for an empty chunk: nothing is read beyond result[0] = 0 records
    if (int r = check_workspace("qlzx_replay_plan", workspace, workspace_bytes, qlzx::replay_plan_ws_layout(cap, nullptr, nullptr, nullptr))) return r;
    return launched("qlzx_replay_plan", qlzx::launch_replay_plan(data, rec_off, result, cap, hdr, comp_idx, comp_off,
                    comp_len, comp_dsize, comp_dst_off, totals, workspace, (hipStream_t)stream));
}

int qlzx_replay_finish(const uint8_t *data, const uint64_t *rec_off, const uint32_t *result, const uint32_t *totals,
                       const uint32_t *comp_idx, const int32_t *comp_status, const uint32_t *comp_dsize,
                       const uint64_t *comp_dst_off, const uint8_t *outbuf, uint32_t cap, int32_t *flag,
                       int32_t *value_len, uint8_t *in_out, uint64_t *val_off, uint16_t *vhash, void *stream) {
    if (!rec_off || !result || !totals || !comp_idx || !comp_status || !comp_dsize || !comp_dst_off || !flag ||
        !value_len || !in_out || !val_off || !vhash)
        return fail(QLZX_R_BAD_ARG, "qlzx_replay_finish: null arg");
    return launched("qlzx_replay_finish", qlzx::launch_replay_finish(data, rec_off, result, totals, comp_idx,
                    comp_status, comp_dsize, comp_dst_off, outbuf, cap, flag, value_len, in_out, val_off, vhash,
                    (hipStream_t)stream));
}

size_t qlzx_read_plan_workspace_size(uint32_t n) { return qlzx::read_ws_layout(n, nullptr, nullptr); }

int qlzx_read_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t n, uint32_t max_key,
                   uint64_t body_max, const uint8_t *want_key, const uint64_t *want_key_off,
                   const uint32_t *want_key_len, int32_t *rd_status, uint8_t *key_eq, int32_t *hdr,
                   uint32_t *comp_idx, uint64_t *comp_off, uint32_t *comp_len, uint32_t *comp_dsize,
                   uint64_t *comp_dst_off, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (!totals) return fail(QLZX_R_BAD_ARG, "qlzx_read_plan: null totals");
    if (n) {
        if ((!data && size) || !rec_off || !rd_status || !hdr || !comp_idx || !comp_off || !comp_len || !comp_dsize ||
            !comp_dst_off)
            return fail(QLZX_R_BAD_ARG, "qlzx_read_plan: null arg");
        const int nkeys = !!want_key + !!want_key_off + !!want_key_len;
        if (nkeys != 0 && nkeys != 3) return fail(QLZX_R_BAD_ARG, "qlzx_read_plan: want_key* are all three or none");
        if ((nkeys == 3) != (key_eq != nullptr))
            return fail(QLZX_R_BAD_ARG, "qlzx_read_plan: key_eq goes with the wanted keys");
        if (int r = check_chunk_size("qlzx_read_plan", size)) return r;
        if (body_max > 0xffffffffull - 24 - max_key)
            return fail(QLZX_R_BAD_ARG, "qlzx_read_plan: 24 + max_key + body_max is 4 GiB or more");
        if (int r = check_workspace("qlzx_read_plan", workspace, workspace_bytes, qlzx_read_plan_workspace_size(n))) return r;
    }
    return launched("qlzx_read_plan", qlzx::launch_read_plan(data, size, rec_off, n, max_key, body_max, want_key,
                    want_key_off, want_key_len, rd_status, key_eq, hdr, comp_idx, comp_off, comp_len, comp_dsize,
                    comp_dst_off, totals, workspace, (hipStream_t)stream));
}

int qlzx_read_finish(const uint8_t *data, const uint64_t *rec_off, uint32_t n, const int32_t *rd_status,
                     const uint32_t *totals, const uint32_t *comp_idx, const int32_t *comp_status,
                     const uint32_t *comp_dsize, const uint64_t *comp_dst_off, const uint8_t *outbuf,
                     int32_t *flag, int32_t *value_len, uint8_t *in_out, uint64_t *val_off, uint16_t *vhash,
                     int32_t *dec_status, void *stream) {
    if (n == 0) return QLZX_R_OK;
    // data and outbuf may be null: nothing of them is read when no request passed / none decoded
    if (!rec_off || !rd_status || !totals || !comp_idx || !comp_status || !comp_dsize || !comp_dst_off || !flag ||
        !value_len || !in_out || !val_off || !vhash || !dec_status)
        return fail(QLZX_R_BAD_ARG, "qlzx_read_finish: null arg");
    return launched("qlzx_read_finish", qlzx::launch_read_finish(data, rec_off, n, rd_status, totals, comp_idx,
                    comp_status, comp_dsize, comp_dst_off, outbuf, flag, value_len, in_out, val_off, vhash,
                    dec_status, (hipStream_t)stream));
}

size_t qlzx_write_plan_workspace_size(uint32_t n) { return qlzx::write_ws_layout(n, nullptr, nullptr); }

int qlzx_write_plan(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len, const uint32_t *key_len,
                    const uint32_t *flag, const int32_t *ver, uint32_t n, uint32_t max_key, uint64_t body_max,
                    uint32_t not_compress, int32_t *wr_status, uint32_t *try_idx, uint64_t *try_off,
                    uint32_t *try_len, uint64_t *try_dst_off, uint32_t *totals, void *workspace,
                    size_t workspace_bytes, void *stream) {
    if (!totals) return fail(QLZX_R_BAD_ARG, "qlzx_write_plan: null totals");
    if (n) {
        if (!values || !val_off || !val_len || !key_len || !flag || !ver || !wr_status || !try_idx || !try_off ||
            !try_len || !try_dst_off)
            return fail(QLZX_R_BAD_ARG, "qlzx_write_plan: null arg");
        if (body_max > 0xffffffffull - 24 - 9 - 256 - max_key)
            return fail(QLZX_R_BAD_ARG, "qlzx_write_plan: 24 + max_key + body_max + 9 + 256 is 4 GiB or more");
        if (int r = check_workspace("qlzx_write_plan", workspace, workspace_bytes, qlzx_write_plan_workspace_size(n))) return r;
    }
    return launched("qlzx_write_plan", qlzx::launch_write_plan(values, val_off, val_len, key_len, flag, ver, n,
                    max_key, body_max, not_compress, wr_status, try_idx, try_off, try_len, try_dst_off, totals,
                    workspace, (hipStream_t)stream));
}

int qlzx_write_decide(const uint64_t *val_off, const uint32_t *val_len, uint32_t n, const uint32_t *totals,
                      const uint32_t *try_idx, const uint32_t *try_len, const uint32_t *try_csize,
                      const int32_t *try_status, uint8_t *keep, uint32_t *full_idx, uint64_t *full_off,
                      uint32_t *full_len, uint64_t *full_dst_off, uint32_t *totals2, void *workspace,
                      size_t workspace_bytes, void *stream) {
    if (!totals2) return fail(QLZX_R_BAD_ARG, "qlzx_write_decide: null totals2");
    if (n) {
        if (!val_off || !val_len || !totals || !try_idx || !try_len || !try_csize || !try_status || !keep ||
            !full_idx || !full_off || !full_len || !full_dst_off)
            return fail(QLZX_R_BAD_ARG, "qlzx_write_decide: null arg");
        if (int r = check_workspace("qlzx_write_decide", workspace, workspace_bytes, qlzx_write_plan_workspace_size(n))) return r;
    }
    return launched("qlzx_write_decide", qlzx::launch_write_decide(val_off, val_len, n, totals, try_idx, try_len,
                    try_csize, try_status, keep, full_idx, full_off, full_len, full_dst_off, totals2, workspace,
                    (hipStream_t)stream));
}

int qlzx_write_finish(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len, const uint8_t *keys,
                      const uint64_t *key_off, const uint32_t *key_len, const uint32_t *flag, const int32_t *ver,
                      const uint32_t *ts, uint32_t n, const uint32_t *totals, const uint32_t *try_idx,
                      const uint32_t *try_len, const uint64_t *try_dst_off, const uint32_t *try_csize,
                      const uint32_t *try_crc, const uint8_t *keep, const uint8_t *trial_buf,
                      const uint32_t *totals2, const uint32_t *full_idx, const uint64_t *full_dst_off,
                      const uint32_t *full_csize, const int32_t *full_status, const uint32_t *full_crc,
                      const uint8_t *full_buf, uint8_t *out, uint64_t out_cap, int32_t *wr_status,
                      uint64_t *rec_off, uint32_t *flag_out, uint32_t *vsz, uint32_t *crc, uint16_t *vhash,
                      uint32_t *totals3, void *workspace, size_t workspace_bytes, void *stream) {
    if (!totals3) return fail(QLZX_R_BAD_ARG, "qlzx_write_finish: null totals3");
    if (n) {
        // trial_buf and full_buf may be null: nothing of them is read when their list is empty
        if (!values || !val_off || !val_len || !keys || !key_off || !key_len || !flag || !ver || !ts || !totals ||
            !try_idx || !try_len || !try_dst_off || !try_csize || !try_crc || !keep || !totals2 || !full_idx ||
            !full_dst_off || !full_csize || !full_status || !full_crc || !out || !wr_status || !rec_off ||
            !flag_out || !vsz || !crc)
            return fail(QLZX_R_BAD_ARG, "qlzx_write_finish: null arg");
        if ((uintptr_t)out & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_write_finish: out is not 16-B aligned");
        if (int r = check_workspace("qlzx_write_finish", workspace, workspace_bytes, qlzx_write_plan_workspace_size(n))) return r;
    }
    const qlzx::WrFinishArgs a{values,  keys,       trial_buf, full_buf, val_off,   key_off,  try_dst_off, full_dst_off,
                               val_len, key_len,    flag,      ts,       totals,    try_idx,  try_len,     try_csize,
                               try_crc, totals2,    full_idx,  full_csize, full_crc, ver,     full_status, keep};
    return launched("qlzx_write_finish", qlzx::launch_write_finish(a, n, out, out_cap, wr_status, rec_off, flag_out,
                    vsz, crc, vhash, totals3, workspace, (hipStream_t)stream));
}

size_t qlzx_gc_workspace_size(uint32_t cap, uint32_t max_chunks) {
    return qlzx::gc_ws_layout(cap, max_chunks, nullptr, nullptr);
}

int qlzx_gc_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                 const uint8_t *keep, uint32_t max_key, uint64_t body_max, uint64_t data_file_max,
                 const uint64_t *chunk_head, uint32_t max_chunks, int32_t *gc_status, uint32_t *new_chunk,
                 uint64_t *new_off, uint64_t *chunk_base, uint64_t *chunk_bytes, uint32_t *totals, void *workspace,
                 size_t workspace_bytes, void *stream) {
    if (cap == 0) return QLZX_R_OK;
    if ((!data && size) || !rec_off || !result || !keep || !chunk_head || !gc_status || !new_chunk || !new_off ||
        !chunk_base || !chunk_bytes || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_plan: null arg");
    if (max_chunks < 1 || max_chunks > 998) return fail(QLZX_R_BAD_ARG, "qlzx_gc_plan: max_chunks is 1 to 998");
    if ((uintptr_t)data & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_gc_plan: data is not 16-B aligned");
    if (int r = check_chunk_size("qlzx_gc_plan", size)) return r;
    if (body_max > 0xffffffffull - 24 - 256 - max_key)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_plan: 24 + max_key + body_max + 256 is 4 GiB or more");
    if (int r = check_workspace("qlzx_gc_plan", workspace, workspace_bytes, qlzx_gc_workspace_size(cap, max_chunks))) return r;
    return launched("qlzx_gc_plan", qlzx::launch_gc_plan(data, size, rec_off, result, cap, keep, max_key, body_max,
                    data_file_max, chunk_head, max_chunks, gc_status, new_chunk, new_off, chunk_base, chunk_bytes,
                    totals, workspace, (hipStream_t)stream));
}

int qlzx_gc_rewrite(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                    const uint64_t *chunk_head, uint32_t max_chunks, const uint32_t *new_chunk,
                    const uint64_t *new_off, const uint64_t *chunk_base, uint8_t *out, uint64_t out_cap,
                    int32_t *gc_status, uint32_t *crc, uint32_t *totals, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (cap == 0) return QLZX_R_OK;
    if ((!data && size) || !rec_off || !result || !chunk_head || !new_chunk || !new_off || !chunk_base ||
        (!out && out_cap) || !gc_status || !crc || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_rewrite: null arg");
    if (max_chunks < 1 || max_chunks > 998) return fail(QLZX_R_BAD_ARG, "qlzx_gc_rewrite: max_chunks is 1 to 998");
    if (((uintptr_t)data | (uintptr_t)out) & 15u)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_rewrite: data and out are not 16-B aligned");
    // records are written in parallel: a chunk cannot be rewritten onto itself
    if (size && out_cap && (uintptr_t)out < (uintptr_t)data + size && (uintptr_t)data < (uintptr_t)out + out_cap)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_rewrite: out overlaps data");
    if (int r = check_workspace("qlzx_gc_rewrite", workspace, workspace_bytes, qlzx_gc_workspace_size(cap, max_chunks))) return r;
    const qlzx::GcIn in{data, size, rec_off, chunk_head, new_off, chunk_base, new_chunk, max_chunks, out, out_cap};
    return launched("qlzx_gc_rewrite", qlzx::launch_gc_rewrite(in, result, cap, gc_status, crc, totals, workspace,
                    (hipStream_t)stream));
}

int qlzx_keyhash_batch(const uint8_t *src, const uint64_t *off, const uint32_t *len, uint32_t n, uint64_t *out,
                       void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!src || !off || !len || !out) return fail(QLZX_R_BAD_ARG, "qlzx_keyhash_batch: null arg");
    hipLaunchKernelGGL(qlzx::k_keyhash, dim3(qlzx::grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, src, off, len, n,
                       out);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

size_t qlzx_hint_workspace_size(uint32_t cap) { return qlzx::hint_ws_layout(cap, nullptr, nullptr); }

int qlzx_hint_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                   const int32_t *hdr, const uint64_t *keyhash, uint32_t first, uint32_t split_cap,
                   int64_t index_interval, uint32_t max_offset_in, uint32_t *item_rec, uint64_t *item_hash,
                   uint64_t *item_off, uint32_t *index_item, uint32_t *totals, void *workspace, size_t workspace_bytes,
                   void *stream) {
    if (cap == 0) return QLZX_R_OK;
    // keyhash may be null: the default hash of the record's key
    if ((!data && size) || !rec_off || !result || !hdr || !item_rec || !item_hash || !item_off || !index_item ||
        !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_plan: null arg");
    if (split_cap == 0) return fail(QLZX_R_BAD_ARG, "qlzx_hint_plan: split_cap is 1 or more");
    if (int r = check_chunk_size("qlzx_hint_plan", size)) return r;
    if (int r = check_workspace("qlzx_hint_plan", workspace, workspace_bytes, qlzx_hint_workspace_size(cap))) return r;
    const qlzx::HintIn in{data, size, rec_off, hdr, cap};
    return launched("qlzx_hint_plan", qlzx::launch_hint_plan(in, result, keyhash, first, split_cap, index_interval,
                    max_offset_in, item_rec, item_hash, item_off, index_item, totals, workspace,
                    (hipStream_t)stream));
}

int qlzx_hint_write(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t cap, const int32_t *hdr,
                    const uint16_t *vhash, uint32_t chunk_id, const uint32_t *item_rec, const uint64_t *item_hash,
                    const uint64_t *item_off, const uint32_t *index_item, uint8_t *out, uint64_t out_cap,
                    uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (cap == 0) return QLZX_R_OK;
    if ((!data && size) || !rec_off || !hdr || !vhash || !item_rec || !item_hash || !item_off || !index_item ||
        (!out && out_cap) || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_write: null arg");
    if ((uintptr_t)out & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_hint_write: out is not 16-B aligned");
    if (int r = check_chunk_size("qlzx_hint_write", size)) return r;
    if (int r = check_workspace("qlzx_hint_write", workspace, workspace_bytes, qlzx_hint_workspace_size(cap))) return r;
    qlzx::HintFile f{};
    f.in = qlzx::HintIn{data, size, rec_off, hdr, cap};
    f.vhash = vhash, f.item_rec = item_rec, f.index_item = index_item, f.item_hash = item_hash, f.item_off = item_off;
    f.chunk_id = chunk_id;
    return launched("qlzx_hint_write", qlzx::launch_hint_write(f, out, out_cap, totals, (hipStream_t)stream));
}

size_t qlzx_hint_merge_workspace_size(uint64_t bytes, uint32_t n_files, uint32_t cap) {
    (void)bytes;
    return qlzx::hm_ws_layout(n_files, cap, nullptr, nullptr);
}

int qlzx_hint_merge_plan(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                         const uint32_t *file_chunk, uint32_t n_files, uint32_t cap, int64_t index_interval,
                         uint64_t *item_src, uint32_t *item_chunk, uint64_t *item_off, uint32_t *index_item,
                         uint32_t *coll_item, uint32_t *totals, void *workspace, size_t workspace_bytes,
                         void *stream) {
    if (n_files == 0 || cap == 0) return QLZX_R_OK;
    if ((!hints && bytes) || !file_off || !file_len || !file_chunk || !item_src || !item_chunk || !item_off ||
        !index_item || !coll_item || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_merge_plan: null arg");
    if (int r = check_workspace("qlzx_hint_merge_plan", workspace, workspace_bytes,
                                qlzx_hint_merge_workspace_size(bytes, n_files, cap)))
        return r;
    const qlzx::HmIn in{hints, bytes, file_off, file_len, file_chunk, n_files, cap};
    return launched("qlzx_hint_merge_plan", qlzx::launch_hm_plan(in, index_interval, item_src, item_chunk, item_off,
                    index_item, coll_item, totals, workspace, (hipStream_t)stream));
}

int qlzx_hint_merge_write(const uint8_t *hints, uint64_t bytes, uint32_t cap, const uint64_t *item_src,
                          const uint32_t *item_chunk, const uint64_t *item_off, const uint32_t *index_item,
                          uint8_t *out, uint64_t out_cap, uint32_t *totals, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (cap == 0) return QLZX_R_OK;
    if ((!hints && bytes) || !item_src || !item_chunk || !item_off || !index_item || (!out && out_cap) || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_merge_write: null arg");
    if ((uintptr_t)out & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_hint_merge_write: out is not 16-B aligned");
    // the plan's workspace, for one source at the least (the write itself keeps nothing in it)
    if (int r = check_workspace("qlzx_hint_merge_write", workspace, workspace_bytes,
                                qlzx_hint_merge_workspace_size(bytes, 1, cap)))
        return r;
    const qlzx::HmFile f{hints, bytes, item_src, item_off, item_chunk, index_item};
    return launched("qlzx_hint_merge_write", qlzx::launch_hm_write(f, cap, out, out_cap, totals, (hipStream_t)stream));
}

size_t qlzx_hint_lookup_workspace_size(uint32_t n, uint32_t n_files) {
    return qlzx::hl_ws_layout(n, n_files, nullptr, nullptr);
}

int qlzx_hint_lookup(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                     const uint32_t *file_chunk, const uint32_t *file_flags, uint32_t n_files, const uint8_t *keys,
                     const uint64_t *key_off, const uint32_t *key_len, const uint64_t *keyhash, uint32_t n,
                     uint32_t flags, int32_t *status, uint32_t *hit_file, uint32_t *chunk, uint32_t *offset,
                     int32_t *ver, uint16_t *vhash, uint64_t *item_src, uint32_t *totals, void *workspace,
                     size_t workspace_bytes, void *stream) {
    if (n == 0 || n_files == 0) return QLZX_R_OK;
    // keyhash may be null: the default hash of the request's key
    if ((!hints && bytes) || !file_off || !file_len || !file_chunk || !file_flags || !keys || !key_off || !key_len ||
        !status || !hit_file || !chunk || !offset || !ver || !vhash || !item_src || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_lookup: null arg");
    constexpr uint32_t shapes = QLZX_HL_F_LANE | QLZX_HL_F_WAVE;
    if ((flags & ~(QLZX_HL_F_BOUNDED | shapes)) || (flags & shapes) == shapes)
        return fail(QLZX_R_BAD_ARG, "qlzx_hint_lookup: unknown flag, or both kernels named");
    if (int r = check_workspace("qlzx_hint_lookup", workspace, workspace_bytes,
                                qlzx_hint_lookup_workspace_size(n, n_files)))
        return r;
    const qlzx::HlIn in{hints, bytes, file_off, file_len, file_chunk, file_flags, n_files, keys, key_off, key_len,
                        keyhash, n, (flags & QLZX_HL_F_BOUNDED) != 0};
    const qlzx::HlOut out{status, hit_file, chunk, offset, ver, vhash, item_src, totals};
    const bool lane = flags & shapes ? (flags & QLZX_HL_F_LANE) != 0 : n >= QLZX_HL_LANE_FROM;
    return launched("qlzx_hint_lookup", qlzx::launch_hl(in, lane, out, workspace, (hipStream_t)stream));
}

size_t qlzx_htree_workspace_size(uint64_t bytes, uint32_t n_files, uint32_t cap, uint32_t height) {
    (void)bytes, (void)height;
    return qlzx::ht_ws_layout(n_files, cap, nullptr, nullptr);
}

int qlzx_htree_plan(const uint8_t *hints, uint64_t bytes, const uint64_t *file_off, const uint64_t *file_len,
                    const uint32_t *file_chunk, uint32_t n_files, uint32_t cap, uint32_t depth, uint32_t height,
                    uint32_t *node_count, uint16_t *node_hash, uint32_t *leaf_first, uint64_t *slot_src,
                    uint32_t *slot_chunk, uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (cap == 0) return QLZX_R_OK;
    qlzx::HtGeo g;
    if (!qlzx::ht_geo(depth, height, &g))
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_plan: depth is 0..2 and height 1..6");
    // no source is an empty tree: then the three per-source arrays may be null
    if ((!hints && bytes) || (n_files && (!file_off || !file_len || !file_chunk)) || !node_count ||
        !node_hash || !leaf_first || !slot_src || !slot_chunk || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_plan: null arg");
    if (int r = check_workspace("qlzx_htree_plan", workspace, workspace_bytes,
                                qlzx_htree_workspace_size(bytes, n_files, cap, height)))
        return r;
    const qlzx::HmIn in{hints, bytes, file_off, file_len, file_chunk, n_files, cap};
    return launched("qlzx_htree_plan", qlzx::launch_ht_plan(in, g, node_count, node_hash, leaf_first, slot_src,
                    slot_chunk, totals, workspace, (hipStream_t)stream));
}

int qlzx_htree_write(const uint8_t *hints, uint64_t bytes, uint32_t cap, uint32_t depth, uint32_t height,
                     const uint32_t *node_count, const uint16_t *node_hash, const uint32_t *leaf_first,
                     const uint64_t *slot_src, const uint32_t *slot_chunk, uint8_t *out, uint64_t out_cap,
                     uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    if (cap == 0) return QLZX_R_OK;
    qlzx::HtGeo g;
    if (!qlzx::ht_geo(depth, height, &g))
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_write: depth is 0..2 and height 1..6");
    if ((!hints && bytes) || !node_count || !node_hash || !leaf_first || !slot_src || !slot_chunk ||
        (!out && out_cap) || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_write: null arg");
    if ((uintptr_t)out & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_htree_write: out is not 16-B aligned");
    // the plan's workspace, of a plan without a source at the least (the write itself keeps nothing in it)
    if (int r = check_workspace("qlzx_htree_write", workspace, workspace_bytes,
                                qlzx_htree_workspace_size(bytes, 0, cap, height)))
        return r;
    const qlzx::HtFile f{hints, bytes, node_count, node_hash, leaf_first, slot_src, slot_chunk};
    return launched("qlzx_htree_write", qlzx::launch_ht_write(f, g, cap, out, out_cap, totals, (hipStream_t)stream));
}

// ---- include/qlzx_htree_get.h ----
// the tree every call takes: geometry, a non-null 16-B aligned image (unless empty) below 2^36 bytes
static int check_htg_tree(const char *who, const void *image, uint64_t bytes, uint32_t depth, uint32_t height,
                          qlzx::HtGeo *g) {
    if (!qlzx::ht_geo(depth, height, g)) return fail_in(QLZX_R_BAD_ARG, who, "depth is 0..2 and height 1..6");
    if (!image && bytes) return fail_in(QLZX_R_BAD_ARG, who, "null arg");
    if ((uintptr_t)image & 15u) return fail_in(QLZX_R_BAD_ARG, who, "image is not 16-B aligned");
    if (bytes >> 36) return fail_in(QLZX_R_BAD_ARG, who, "image of 2^36 bytes or more");
    return QLZX_R_OK;
}
static int htg_shape(const char *who, uint32_t flags, uint32_t n, uint64_t bytes, const qlzx::HtGeo &g, bool *lane) {
    constexpr uint32_t shapes = QLZX_HTG_F_LANE | QLZX_HTG_F_WAVE;
    if ((flags & ~shapes) || (flags & shapes) == shapes)
        return fail_in(QLZX_R_BAD_ARG, who, "unknown flag, or both kernels named");
    *lane = flags & shapes ? (flags & QLZX_HTG_F_LANE) != 0 : qlzx::htg_lane_shape(n, bytes, g);
    return QLZX_R_OK;
}

size_t qlzx_htree_index_workspace_size(uint32_t height) {
    qlzx::HtGeo g;
    return qlzx::ht_geo(0, height, &g) ? qlzx::hti_ws_layout(g.nleaf, nullptr, nullptr) : 0;
}

int qlzx_htree_index(const uint8_t *image, uint64_t bytes, uint32_t depth, uint32_t height, uint32_t *leaf_first,
                     uint32_t *totals, void *workspace, size_t workspace_bytes, void *stream) {
    qlzx::HtGeo g;
    if (int r = check_htg_tree("qlzx_htree_index", image, bytes, depth, height, &g)) return r;
    if (!leaf_first || !totals) return fail(QLZX_R_BAD_ARG, "qlzx_htree_index: null arg");
    if (int r = check_workspace("qlzx_htree_index", workspace, workspace_bytes, qlzx_htree_index_workspace_size(height)))
        return r;
    const qlzx::HtgTree T{image, bytes, nullptr, g};
    return launched("qlzx_htree_index", qlzx::launch_hti(T, leaf_first, totals, workspace, (hipStream_t)stream));
}

size_t qlzx_htree_get_workspace_size(uint32_t n) { return qlzx::htg_ws_layout(n, nullptr, nullptr); }

int qlzx_htree_get(const uint8_t *image, uint64_t bytes, const uint32_t *leaf_first, uint32_t depth, uint32_t height,
                   const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len, const uint64_t *keyhash,
                   uint32_t n, uint32_t flags, int32_t *status, uint32_t *chunk, uint32_t *offset, int32_t *ver,
                   uint16_t *vhash, uint32_t *slot, uint32_t *totals, void *workspace, size_t workspace_bytes,
                   void *stream) {
    if (n == 0) return QLZX_R_OK;
    qlzx::HtGeo g;
    if (int r = check_htg_tree("qlzx_htree_get", image, bytes, depth, height, &g)) return r;
    // keyhash may be null: the default hash of the request's key, which the three key arrays then name
    if (!leaf_first || (!keyhash && (!keys || !key_off || !key_len)) || !status || !chunk || !offset || !ver ||
        !vhash || !slot || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_get: null arg");
    bool lane;
    if (int r = htg_shape("qlzx_htree_get", flags, n, bytes, g, &lane)) return r;
    if (int r = check_workspace("qlzx_htree_get", workspace, workspace_bytes, qlzx_htree_get_workspace_size(n))) return r;
    const qlzx::HtgTree T{image, bytes, leaf_first, g};
    const qlzx::HtgOut out{status, chunk, offset, ver, vhash, slot, nullptr};
    return launched("qlzx_htree_get", qlzx::launch_htg(T, keys, key_off, key_len, keyhash, n, lane, out, workspace,
                    totals, (hipStream_t)stream));
}

size_t qlzx_gc_liveness_workspace_size(uint32_t cap) { return qlzx::gl_ws_layout(cap, nullptr, nullptr); }

int qlzx_gc_liveness(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result, uint32_t cap,
                     uint32_t max_key, uint64_t body_max, uint32_t src_chunk, const uint8_t *image, uint64_t bytes,
                     const uint32_t *leaf_first, uint32_t depth, uint32_t height, const uint64_t *keyhash,
                     uint32_t flags, uint8_t *keep, int32_t *verdict, uint16_t *vhash, int32_t *tree_ver,
                     uint32_t *slot, uint32_t *ask_idx, uint32_t *totals, void *workspace, size_t workspace_bytes,
                     void *stream) {
    if (cap == 0) return QLZX_R_OK;
    qlzx::HtGeo g;
    if (int r = check_htg_tree("qlzx_gc_liveness", image, bytes, depth, height, &g)) return r;
    if ((!data && size) || !rec_off || !result || !leaf_first || !keep || !verdict || !vhash || !tree_ver || !slot ||
        !ask_idx || !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_gc_liveness: null arg");
    if (flags & ~(uint32_t)QLZX_GL_F_BEGIN_GT_0) return fail(QLZX_R_BAD_ARG, "qlzx_gc_liveness: unknown flag");
    if ((uintptr_t)data & 15u) return fail(QLZX_R_BAD_ARG, "qlzx_gc_liveness: data is not 16-B aligned");
    if (int r = check_chunk_size("qlzx_gc_liveness", size)) return r;
    if (int r = check_workspace("qlzx_gc_liveness", workspace, workspace_bytes, qlzx_gc_liveness_workspace_size(cap)))
        return r;
    const qlzx::GlIn in{data, size, rec_off, result, cap, max_key, body_max};
    const qlzx::HtgTree T{image, bytes, leaf_first, g};
    return launched("qlzx_gc_liveness", qlzx::launch_gl(in, src_chunk, T, keyhash, flags, qlzx::htg_lane_shape(cap, bytes, g),
                    keep, verdict, vhash, tree_ver, slot, ask_idx, totals, workspace, (hipStream_t)stream));
}

size_t qlzx_htree_move_workspace_size(uint32_t cap) { return qlzx::htm_ws_layout(cap, nullptr, nullptr); }

int qlzx_htree_move(uint8_t *image, uint64_t bytes, const uint32_t *leaf_first, uint32_t depth, uint32_t height,
                    const uint32_t *result, uint32_t cap, const int32_t *verdict, const int32_t *gc_status,
                    const uint32_t *slot, const uint32_t *new_chunk, const uint64_t *new_off,
                    const uint32_t *dst_chunk_id, uint32_t max_chunks, uint32_t *totals, void *workspace,
                    size_t workspace_bytes, void *stream) {
    if (cap == 0) return QLZX_R_OK;
    qlzx::HtGeo g;
    if (int r = check_htg_tree("qlzx_htree_move", image, bytes, depth, height, &g)) return r;
    if (!leaf_first || !result || !verdict || !gc_status || !slot || !new_chunk || !new_off || !dst_chunk_id ||
        !totals)
        return fail(QLZX_R_BAD_ARG, "qlzx_htree_move: null arg");
    if (int r = check_workspace("qlzx_htree_move", workspace, workspace_bytes, qlzx_htree_move_workspace_size(cap)))
        return r;
    const qlzx::HtgTree T{image, bytes, leaf_first, g};
    const qlzx::HtmIn in{result, cap, verdict, gc_status, slot, new_chunk, new_off, dst_chunk_id, max_chunks};
    return launched("qlzx_htree_move", qlzx::launch_htm(T, image, in, totals, workspace, (hipStream_t)stream));
}

int qlzx_vhash_batch(const uint8_t *src, const uint64_t *off, const uint32_t *len, uint32_t n, uint16_t *out,
                     void *stream) {
    if (n == 0) return QLZX_R_OK;
    if (!src || !off || !len || !out) return fail(QLZX_R_BAD_ARG, "qlzx_vhash_batch: null arg");
    hipLaunchKernelGGL(qlzx::k_vhash, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, src, off, len, n,
                       out);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

int qlzx_service_test_fault(int mode) {
    // a test hook: armed only in a process started with QLZX_TEST_HOOKS=1 (read once), so no
    // caller of the release library can make another thread's drop-in call fail
    static const bool armed = [] {
        const char *e = std::getenv("QLZX_TEST_HOOKS");
        return e && e[0] == '1';
    }();
    if (!armed) return fail(QLZX_R_BAD_ARG, "qlzx_service_test_fault: test hooks are off (QLZX_TEST_HOOKS=1)");
    if (mode < 1 || mode > 4) return fail(QLZX_R_BAD_ARG, "qlzx_service_test_fault: mode is 1 to 4");
    if (mode >= 3) {  // the batch decoder's next K1 (3) or K2 (4) launch
        qlzx::g_batch_fault.store(mode, std::memory_order_release);
        return QLZX_R_OK;
    }
    Service *S = service();
    if (!S) return QLZX_R_NO_DEVICE;
    S->fault.store(mode, std::memory_order_release);
    return QLZX_R_OK;
}

}  // extern "C"
