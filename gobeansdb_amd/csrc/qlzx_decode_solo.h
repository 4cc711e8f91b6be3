// qlzx_decode_solo.h -- the latency path for ONE level-3 block (the single-call drop-ins
// qlz_decompress / qlzx_decompress1, called once per GET by store/item.go:167).
//
// The batch decoder parses with one LANE per block (K1) and decodes with one WAVE per block
// (K2b): right when 131072 blocks share the chip, but a lone 64 KiB block then walks ~2,100
// control-word groups on one lane and ~16,000 items on one wave.  Here one 1024-thread
// workgroup does the whole block, every phase position-parallel:
//
//   PARSE (the control-word chain, quicklz.c:513-530 and the token forms of 579-610)
//   1. code[x]  = token bytes - 1 if a match token started at stream byte x (2 bits each);
//   2. delta[x] = length of the control-word group that WOULD start at x (4 + 31 items), at
//                 every x at once: a speculative parse, each thread walking the match bits of
//                 the dword at x and adding code[] of each match token.  0 (no shortcut) for a
//                 dword without bit 31 (check C1) and for x within 128 B of the end, where a
//                 group may run past the stream;  j2[x] = delta[x] + delta[x + delta[x]];
//   3. one lane follows hdr -> hdr + j2[hdr] -> ... (two groups per LDS read) and lists the
//      group starts; a group without a shortcut is parsed byte by byte there as K1 parses it
//      (qlzx_decode_k1.h k_dec_parse6: checks C1, C2, the group bound, the item count);
//   4. the GroupRec {ip, m, a, b} of every listed group, in parallel.
//   DECODE (quicklz.c:531-671 restated output-parallel, as K2b does per chunk)
//   5. items: each thread decodes a contiguous run of items (token from its GroupRec), a
//      block-wide scan of the output lengths gives every item its start d; checks C3-C5;
//      the item leaves a u16 marker at d (match offset, or 1 for a literal, whose byte goes
//      straight to the destination);
//   6. fill: thread t owns output bytes [64 t, 64 t + 64): its markers are forward-filled
//      (block max-scan for the carry) into the SOURCE position of every byte (itself for a
//      literal byte, p - offset for a match byte);
//   7. pointer jumping s[p] <- s[s[p]] over the whole block until every byte points at a
//      literal (log2 of the longest copy chain rounds);
//   8. gather: out[p] = out[s[p]] (the literal bytes written in 5).
// The format's rules in these steps are qlzx_decode_fmt.h's.  Status and output equal K1 + K2b's
// on the same stream (tests/test_gpu_solo.py; hand-assembled streams:
// tests/test_gpu_crafted_streams.py).
#pragma once
#include "qlzx_decode_fmt.h"

namespace qlzx {

constexpr uint32_t kSoloWG = 64 * kBlockWaves;
constexpr uint32_t kSoloMaxCsize = 65536;            // LDS: 2-bit codes + delta + j2 per stream byte
constexpr uint32_t kSoloOwn = 64;                    // output bytes per thread: kSoloWG * 64 = 64 KiB
constexpr uint32_t kSoloGmax = QLZX_FAST_MAX_DSIZE / 31 + 2;
constexpr uint32_t kSoloIT = 16;                     // items per thread per decode round
static_assert(kSoloWG * kSoloOwn >= QLZX_FAST_MAX_DSIZE, "one output run per thread");

struct SoloLds {
    union {
        struct {
            uint32_t code[kSoloMaxCsize / 16];
            uint8_t delta[kSoloMaxCsize];
            uint8_t j2[kSoloMaxCsize];              // delta of two groups - 69 (1..187), 0: none
            uint32_t glist[kSoloGmax];
        } p;
        uint16_t s[QLZX_FAST_MAX_DSIZE];            // markers, then source positions
    };
    uint32_t wsum[kBlockWaves];
    uint32_t ngroups, klast;
    int32_t st;
    CheckAcc acc;
};
// The block being decoded (workgroup-uniform).  src and dst are 16-B aligned.
struct SoloCtx {
    const uint8_t *src;
    uint8_t *dst;
    GroupRec *recs;
    uint32_t csize, dsize, hdr, max_dsize;
};

__device__ __forceinline__ uint32_t u16_get(const uint32_t *v, uint32_t j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu; }
__device__ __forceinline__ void u16_set(uint32_t *v, uint32_t j, uint32_t x) {
    v[j >> 1] = (j & 1) ? ((v[j >> 1] & 0xffffu) | (x << 16)) : ((v[j >> 1] & 0xffff0000u) | x);
}

#ifdef QLZX_PROFILE  // phase stamps of thread 0 into the profile slots from `base` on (tools/solo_prof.py)
#define SOLO_T0 unsigned long long _st = __builtin_amdgcn_s_memtime();
#define DEC_STAMP(base, k)                                                   \
    do {                                                                     \
        if (threadIdx.x == 0 && g_prof) {                                    \
            const unsigned long long _n = __builtin_amdgcn_s_memtime();       \
            atomicAdd(&g_prof[(base) + (k)], (k) == 7 ? 1ull : _n - _st);   \
            _st = _n;                                                        \
        }                                                                    \
    } while (0)
#else
#define SOLO_T0
#define DEC_STAMP(base, k) \
    do {                   \
    } while (0)
#endif
#define SOLO_STAMP(k) DEC_STAMP(16, k)  // solo_decode: slots 16..23

// ---- 1. token codes, 16 stream bytes per word ----
__device__ __forceinline__ void solo_codes(SoloLds &L, const SoloCtx &c) {
    for (uint32_t w = threadIdx.x; w < (c.csize + 15) / 16; w += kSoloWG) {
        if (16 * w + 16 <= c.csize) {
            const uint4 q = *(const uint4 *)(c.src + 16 * w);
            L.p.code[w] = pack_codes16(q.x, q.y, q.z, q.w);
        } else {
            L.p.code[w] = pack_codes_tail(c.src + 16 * w, c.csize - 16 * w);
        }
    }
    __syncthreads();
}
// ---- 2. speculative group length at every stream byte (next candidate's dword in flight) ----
__device__ __forceinline__ void solo_delta(SoloLds &L, const SoloCtx &c) {
    const uint32_t tid = threadIdx.x, csize = c.csize;
    uint32_t x = c.hdr + tid;
    // cw = 0 within 128 B of the end: no shortcut there
    uint32_t cwn = x + 128 <= csize ? ld_dword(c.src + x) : 0u;
    for (; x < csize; x += kSoloWG) {
        const uint32_t cw = cwn;
        cwn = x + kSoloWG + 128 <= csize ? ld_dword(c.src + x + kSoloWG) : 0u;
        L.p.delta[x] = (uint8_t)spec_group_len(cw, CodeWords{L.p.code}, x);
    }
    __syncthreads();
    for (x = c.hdr + tid; x < csize; x += kSoloWG) {
        const uint32_t d1 = L.p.delta[x];
        const uint32_t d2 = d1 && x + d1 < csize ? L.p.delta[x + d1] : 0u;
        L.p.j2[x] = (uint8_t)(d2 ? d1 + d2 - 69 : 0u);
    }
    __syncthreads();
}
// ---- 3. the group chain (one lane); K1's byte-level parse where there is no shortcut ----
__device__ __forceinline__ void solo_walk(SoloLds &L, const SoloCtx &c) {
    if (threadIdx.x == 0) {
        const uint32_t gmax = groups_max(c.max_dsize < QLZX_FAST_MAX_DSIZE ? c.max_dsize : QLZX_FAST_MAX_DSIZE);
        uint32_t x = c.hdr, g = 0, klast = 31;
        int st = QLZX_OK;
        while (x + 4 <= c.csize) {  // else: stream exhausted at a control word
            const uint32_t j = L.p.j2[x], d = L.p.delta[x];
            if (j && g + 2 <= gmax) {  // two whole groups
                L.p.glist[g] = x;
                L.p.glist[g + 1] = x + d;
                g += 2;
                x += j + 69;
                continue;
            }
            if (g >= gmax) { st = QLZX_E_CORRUPT; break; }
            L.p.glist[g++] = x;
            if (d) { x += d; continue; }
            uint32_t next = x;
            st = parse_group_bytewise(ld_dword(c.src + x), x, c.csize, CodeWords{L.p.code}, klast, next);
            if (st != QLZX_OK || klast < 31) break;  // corrupt, or the stream ends inside this group
            x = next;
        }
        L.ngroups = g;
        L.klast = klast;
        L.st = chain_status(st, g);
        L.acc = check_acc_init();
    }
    __syncthreads();
}
// ---- 4. GroupRecs of the listed groups (the last one holds klast items) ----
__device__ __forceinline__ void solo_recs(SoloLds &L, const SoloCtx &c, uint32_t ng, uint32_t klast) {
    for (uint32_t g = threadIdx.x; g < ng; g += kSoloWG) {
        const uint32_t x = L.p.glist[g];
        c.recs[g] = group_rec(x, ld_dword(c.src + x), g + 1 == ng ? klast : 31u, CodeWords{L.p.code});
    }
    __threadfence();  // the records are read back by other waves below
    __syncthreads();
}
// ---- 5. items: thread tid decodes items [I0, I1), kSoloIT per round ----
struct SoloTok {  // token dword at pos from global memory: the read is clamped to the stream
    const uint8_t *src;
    uint32_t csize;
    __device__ __forceinline__ uint32_t load(bool live, uint32_t pos) const {
        return ld_dword(src + (live && pos + 4 <= csize ? pos : csize - 4));
    }
    __device__ __forceinline__ uint32_t token(uint32_t raw, uint32_t pos) const {
        return pos + 4 <= csize ? raw : raw >> (8 * (pos + 4 - csize));
    }
};
__device__ __forceinline__ void solo_items(SoloLds &L, const SoloCtx &c, uint32_t ng, uint32_t klast) {
    const uint32_t tid = threadIdx.x;
    const uint32_t nitems = (ng - 1) * 31 + klast;
    const uint32_t per = (nitems + kSoloWG - 1) / kSoloWG;
    const uint32_t I0 = min(tid * per, nitems), I1 = min(I0 + per, nitems);
    const SoloTok tok{c.src, c.csize};
    const uint32_t mysum = items_len<kSoloIT>(c.recs, ng, I0, I1, tok);
    // markers: clear the output range (the parse tables are dead: glist was read in 4)
    for (uint32_t q = tid; q < (c.dsize + 7) / 8; q += kSoloWG) *(uint4 *)(L.s + 8 * q) = make_uint4(0, 0, 0, 0);
    uint32_t total;
    const uint32_t d = block_excl<false>(mysum, L.wsum, total);
    __syncthreads();  // markers cleared, wsum read
    CheckAcc acc = check_acc_init();
    items_emit<kSoloIT>(c.recs, ng, I0, I1, d, tok, ItemCtx{c.csize, c.dsize, c.hdr, tail_start(c.dsize)}, acc,
                        [&](uint32_t p, bool ism, uint32_t off, uint32_t lit) {
                            L.s[p] = (uint16_t)(ism ? off : kLitMark);
                            if (!ism) c.dst[p] = (uint8_t)lit;
                        });
    check_acc_merge(&L.acc, acc);
    __threadfence();  // literal bytes, read back by other threads in 8
    __syncthreads();
}
// ---- 6. fill: markers -> source position of every byte of [p0, p0 + 64), two u16 per register ----
__device__ __forceinline__ void solo_store_run(SoloLds &L, uint32_t p0, const uint32_t (&sv)[kSoloOwn / 2]) {
#pragma unroll
    for (uint32_t q = 0; q < kSoloOwn / 8; q++)
        *(uint4 *)(L.s + p0 + 8 * q) = make_uint4(sv[4 * q], sv[4 * q + 1], sv[4 * q + 2], sv[4 * q + 3]);
}
__device__ __forceinline__ void solo_fill(SoloLds &L, uint32_t dsize, uint32_t (&sv)[kSoloOwn / 2]) {
    const uint32_t p0 = threadIdx.x * kSoloOwn;
    uint32_t lastp = 0;  // 1 + position of the run's last marker, 0: none
    if (p0 < dsize) {
#pragma unroll
        for (uint32_t q = 0; q < kSoloOwn / 8; q++) {
            const uint4 v = *(const uint4 *)(L.s + p0 + 8 * q);
            sv[4 * q] = v.x, sv[4 * q + 1] = v.y, sv[4 * q + 2] = v.z, sv[4 * q + 3] = v.w;
        }
#pragma unroll
        for (uint32_t j = 0; j < kSoloOwn; j++) lastp = u16_get(sv, j) ? p0 + j + 1 : lastp;
    }
    uint32_t unused;
    const uint32_t prevp = block_excl<true>(lastp, L.wsum, unused);
    uint32_t f = prevp ? L.s[prevp - 1] : kLitMark;  // position 0 always has a marker
    __syncthreads();  // every carry read before the runs are rewritten
    if (p0 < dsize) {
#pragma unroll
        for (uint32_t j = 0; j < kSoloOwn; j++) {
            const uint32_t p = p0 + j, m = u16_get(sv, j);
            f = m ? m : f;
            u16_set(sv, j, (f == kLitMark || p >= dsize) ? p : p - f);
        }
        solo_store_run(L, p0, sv);
    }
    __syncthreads();
}
// ---- 7. pointer jumping until every byte's source is a literal (s[s] == s) ----
// Entries are rewritten while others read them; any value read is an earlier link of the
// same chain, so a stale read only costs a round.
__device__ __forceinline__ void solo_jump(SoloLds &L, uint32_t dsize, uint32_t (&sv)[kSoloOwn / 2]) {
    const uint32_t p0 = threadIdx.x * kSoloOwn;
    for (;;) {
        bool ch = false;
        if (p0 < dsize) {
#pragma unroll
            for (uint32_t h = 0; h < kSoloOwn; h += 32) {  // 32 reads in flight (a literal reads itself)
                uint32_t t[32];
#pragma unroll
                for (uint32_t j = 0; j < 32; j++) t[j] = L.s[u16_get(sv, h + j)];
#pragma unroll
                for (uint32_t j = 0; j < 32; j++) {
                    const bool jump = t[j] != u16_get(sv, h + j);
                    if (jump) u16_set(sv, h + j, t[j]);
                    ch = ch || jump;
                }
            }
            if (ch) solo_store_run(L, p0, sv);
        }
        if (!__syncthreads_or(ch)) break;
    }
}
// ---- 8. gather the run's bytes from the literals and store them ----
__device__ __forceinline__ void solo_gather(uint8_t *dst, uint32_t dsize, const uint32_t (&sv)[kSoloOwn / 2]) {
    const uint32_t p0 = threadIdx.x * kSoloOwn;
    if (p0 >= dsize) return;
    const uint32_t n = min(kSoloOwn, dsize - p0);
    uint32_t out[kSoloOwn / 4];
#pragma unroll
    for (uint32_t q = 0; q < kSoloOwn / 4; q++) out[q] = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSoloOwn; j++) out[j >> 2] |= (uint32_t)dst[j < n ? u16_get(sv, j) : 0u] << (8 * (j & 3));
    if (n == kSoloOwn) {
#pragma unroll
        for (uint32_t q = 0; q < kSoloOwn / 16; q++)
            *(uint4 *)(dst + p0 + 16 * q) = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    } else {  // the short last run
        for (uint32_t j = 0; j < n; j++) dst[p0 + j] = (uint8_t)(out[j >> 2] >> (8 * (j & 3)));
    }
}

// The whole block by one 1024-thread workgroup; *status / *dsize_out are written by thread 0
// (global or LDS words).  Every return is workgroup-uniform.  src and dst are 16-B aligned: the
// callers hand over a request slot of the service (qlzx_service.hip).
__device__ __forceinline__ void solo_decode(SoloLds &L, const uint8_t *src, uint32_t len, uint8_t *dst,
                                            uint32_t dst_cap, uint32_t max_dsize, GroupRec *recs, int32_t *status,
                                            uint32_t *dsize_out) {
    const uint32_t tid = threadIdx.x;
    SOLO_T0
    SoloCtx c{src, dst, recs, 0, 0, 0, max_dsize};
    uint32_t kind;
    const int st0 = classify_block(src, len, dst_cap, max_dsize, kind, c.csize, c.dsize, c.hdr);
    if (st0 != QLZX_OK) {  // the host routes only blocks <= QLZX_FAST_MAX_DSIZE here: no kPending
        if (tid == 0) *status = st0, *dsize_out = 0;
        return;
    }
    if (kind == kBlkStored) {  // quicklz.c:808-811
        for (uint32_t p = tid; p < c.dsize; p += kSoloWG) dst[p] = src[c.hdr + p];
        if (tid == 0) *status = QLZX_OK, *dsize_out = c.dsize;
        return;
    }
    solo_codes(L, c);
    SOLO_STAMP(0);
    solo_delta(L, c);
    SOLO_STAMP(1);
    solo_walk(L, c);
    SOLO_STAMP(2);
    const uint32_t ng = L.ngroups, klast = L.klast;
    if (L.st != QLZX_OK) {
        if (tid == 0) *status = L.st, *dsize_out = 0;
        return;
    }
    solo_recs(L, c, ng, klast);
    SOLO_STAMP(3);
    solo_items(L, c, ng, klast);
    SOLO_STAMP(4);
    const bool corrupt = c.dsize > 0 && verdict_corrupt(L.acc);
    if (corrupt || c.dsize == 0) {
        if (tid == 0) *status = corrupt ? QLZX_E_CORRUPT : QLZX_OK, *dsize_out = 0;
        return;
    }
    uint32_t sv[kSoloOwn / 2];  // the thread's run of source positions
    solo_fill(L, c.dsize, sv);
    SOLO_STAMP(5);
    solo_jump(L, c.dsize, sv);
    SOLO_STAMP(6);
    solo_gather(dst, c.dsize, sv);
    if (tid == 0) *status = QLZX_OK, *dsize_out = c.dsize;
    SOLO_STAMP(7);
}

}  // namespace qlzx
