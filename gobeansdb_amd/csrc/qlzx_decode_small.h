// qlzx_decode_small.h -- the single-call latency path for small blocks (stream <= 17 KiB,
// output <= 32 KiB: the 4-16 KiB values of a GET, store/item.go:167), all in LDS.
//
// The general latency path (qlzx_decode_solo.h) keeps its parse tables for a 64 KiB stream in
// LDS and reads the stream, its GroupRecs and the literal bytes from HBM; most of its 16 KiB call
// is load latency and one lane's 85-step chain walk.  Here the whole stream, the parse tables,
// the records, the markers and the literal bytes live in LDS, and the walk is log-depth:
//
//   0. the stream is staged into LDS (zero past csize) straight from the request's slot;
//   1. info[x] for every stream byte x: the outcome of parsing a control-word group at x --
//      FULL (its 31 items fit: info = group length 35..128), END k (the stream ends before
//      item k, or item k is a token that runs past the end, check C2: the last group), BAD (no
//      bit 31, check C1).
//      Every x whose dword has bit 31 parses its group at once (candidates listed first, for balance);
//   2. jump tables by pointer doubling: J2, J4, J8, J16 (u16 next-group position, 0: none);
//   3. one lane hops J16 to list every 16th group start, then steps the last groups by info;
//      threads expand each hop's 15 inner group starts in parallel;
//   4. GroupRecs {ip, m, a, b}, then items, markers, fill, pointer jumping and gather exactly as
//      qlzx_decode_solo.h steps 4-8 (the checks C3-C5 included), with the literal bytes and
//      sources in LDS and the result written once to the destination (the caller's slot).
// The format's rules in these steps are qlzx_decode_fmt.h's.  Statuses and bytes equal the batch
// decoder's (K1 + K2, qlzx_decode_k1.h and qlzx_decode_k2.h) on the same stream, dsize-0 rule
// included (tests/test_gpu_solo.py; hand-assembled streams: tests/test_gpu_crafted_streams.py).
#pragma once
#include "qlzx_decode_solo.h"  // kSoloWG, the profile stamps' clock

namespace qlzx {

constexpr uint32_t kSmC = 17408;                 // stream bytes (csize bound of this path)
constexpr uint32_t kSmD = 32768;                 // output bytes (dsize bound)
constexpr uint32_t kSmG = kSmD / 31 + 2;         // groups_max(kSmD)
constexpr uint32_t kSmOwn = 16;                  // output bytes per thread per segment
constexpr uint32_t kSmSeg = kSmD / (kSoloWG * kSmOwn);  // 2 segments of 16 KiB
constexpr uint32_t kSmIT = 8;                    // items per thread per decode round
constexpr uint32_t kSmEnd = 0xA0, kSmBad = 0xFF;  // info codes besides FULL (35..128)
static_assert(kSmC % 16 == 0 && kSmC + 64 < 65536, "u16 positions");

struct SmallLds {
    uint32_t src[(kSmC + 64) / 4];  // the stream, zero from csize on
    uint8_t cb[kSmC + 64];          // token bytes - 1 of a match token at each byte; 4: it runs past csize (C2)
    uint16_t glist[kSmG + 16];
    union {
        struct {
            uint8_t info[kSmC + 64];
            uint16_t ja[kSmC + 64], jb[kSmC + 64];
        } p;
        struct {
            GroupRec recs[kSmG];
            uint16_t s[kSmD];       // markers, then source positions
            uint8_t out[kSmD];      // literal bytes at their output positions
        } d;
    };
    uint32_t wsum[2][kBlockWaves];
    uint32_t ngroups, klast, nhops, cursor;
    int32_t st;
    CheckAcc acc;
};
// The block being decoded (workgroup-uniform).
struct SmallCtx {
    uint8_t *dst;
    uint32_t csize, dsize, hdr, max_dsize;
};

#define SM_STAMP(k) DEC_STAMP(24, k)  // small_decode: slots 24..31
#ifdef QLZX_PROFILE  // sub-phase stamps into the general path's slots 16.. (unused here)
#define SM_SUB(k)                                                            \
    do {                                                                     \
        if (threadIdx.x == 0 && g_prof) atomicAdd(&g_prof[16 + (k)], __builtin_amdgcn_s_memtime() - _st); \
    } while (0)
#else
#define SM_SUB(k) \
    do {          \
    } while (0)
#endif

__device__ __forceinline__ uint32_t sm_dword(const SmallLds &L, uint32_t x) {  // unaligned dword
    const uint32_t w = x >> 2;
    return __builtin_amdgcn_alignbyte(L.src[w + 1], L.src[w], x & 3u);
}
__device__ __forceinline__ bool sm_full(uint32_t e) { return e >= 35u && e <= 128u; }
__device__ __forceinline__ uint32_t sm_run(uint32_t z) { return z * kSoloWG * kSmOwn + threadIdx.x * kSmOwn; }

// ---- 0. stage the stream (and 64 zero bytes past it) and its token codes ----
__device__ __forceinline__ void sm_stage(SmallLds &L, const uint8_t *src, uint32_t len) {
    for (uint32_t o = threadIdx.x * 16; o < ((len + 15) & ~15u) + 64; o += kSoloWG * 16) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (o < len) {
            q = *(const uint4 *)(src + o);
            if (o + 16 > len) {  // bytes past len are slack: zero them
                uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const int keep = (int)len - (int)(o + 4 * j);
                    w[j] = keep >= 4 ? w[j] : keep <= 0 ? 0u : (w[j] & ((1u << (8 * keep)) - 1u));
                }
                q = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        *(uint4 *)(L.src + o / 4) = q;
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
        uint32_t cw4[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            cw4[j] = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                const uint32_t x = o + 4 * j + b, c = tok_code(w4[j] >> (8 * b));
                cw4[j] |= (x + c + 1 > len ? 4u : c) << (8 * b);
            }
        }
        *(uint4 *)(L.cb + o) = make_uint4(cw4[0], cw4[1], cw4[2], cw4[3]);
    }
    __syncthreads();
}
// A stored block (quicklz.c:808-811) from the staged stream.
__device__ __forceinline__ void sm_stored(const SmallLds &L, const SmallCtx &c) {
    const uint32_t tid = threadIdx.x, dsize = c.dsize;
    if ((((uintptr_t)c.dst) & 3u) == 0) {
        for (uint32_t p = tid * 4; p < dsize; p += kSoloWG * 4) {
            const uint32_t w = sm_dword(L, c.hdr + p);
            if (p + 4 <= dsize) *(uint32_t *)(c.dst + p) = w;
            else for (uint32_t j = 0; p + j < dsize; j++) c.dst[p + j] = (uint8_t)(w >> (8 * j));
        }
    } else {
        const uint8_t *sb = (const uint8_t *)L.src;
        for (uint32_t p = tid; p < dsize; p += kSoloWG) c.dst[p] = sb[c.hdr + p];
    }
}
// ---- 1. the group that would start at every stream byte x (x + 4 <= csize) ----
// 1a. candidates: bytes whose dword has bit 31 (the rest fail C1), listed in ja for balance
__device__ __forceinline__ uint32_t sm_candidates(SmallLds &L, const SmallCtx &c) {
    const uint32_t tid = threadIdx.x;
    const uint8_t *sb = (const uint8_t *)L.src;
    uint32_t ncand, cnt = 0;
    for (uint32_t x = c.hdr + tid; x + 4 <= c.csize; x += kSoloWG) {
        const bool cand = (sb[x + 3] >> 7) != 0;
        if (!cand) L.p.info[x] = (uint8_t)kSmBad;
        cnt += cand ? 1u : 0u;
    }
    if (tid == 0) L.cursor = kSoloWG;
    uint32_t w = block_excl<false>(cnt, L.wsum[1], ncand);
    for (uint32_t x = c.hdr + tid; x + 4 <= c.csize; x += kSoloWG)
        if (sb[x + 3] >> 7) L.p.ja[w++] = (uint16_t)x;
    __syncthreads();
    return ncand;
}
// 1b. parse the group at every candidate (one dependent LDS read per match token).  All
//     lanes stay busy: a lane whose chain ends takes the next unparsed candidate from a
//     shared cursor, and a step is a handful of VALU ops (codes from cb, C2 folded in).
__device__ __forceinline__ void sm_info(SmallLds &L, const SmallCtx &c, uint32_t ncand) {
    uint32_t i = threadIdx.x, x = 0, x4 = 0, lim = 0, mrem = 0, ex = 0, cd = 0;
    auto start = [&]() {
        x = L.p.ja[i];
        x4 = x + 4;
        lim = c.csize - x4;
        mrem = sm_dword(L, x) & 0x7fffffffu;
        ex = 0;
        cd = 0;
    };
    if (i < ncand) start();
    while (i < ncand) {
        const uint32_t kend = lim - ex;  // the item index that would start at csize
        const uint32_t k = min((uint32_t)__builtin_ctz(mrem | 0x80000000u), 30u);  // no match left: 30
        bool fin = kend <= k || !mrem;   // ends before the next match / item 31, or FULL
        if (!fin) {
            // the codes of 4 bytes from this token's: a next match whose first byte is among
            // them (its code sits k2 - k + c bytes on) is taken in the same step (kept after
            // profiles/r05_small_chains_ab.txt)
            const uint32_t a = x4 + k + ex;
            const uint32_t *cbw = (const uint32_t *)L.cb;
            const uint32_t w = __builtin_amdgcn_alignbyte(cbw[(a >> 2) + 1], cbw[a >> 2], a & 3u);
            cd = w & 0xffu;
            fin = cd > 3;  // C2
            if (!fin) {
                ex += cd;
                mrem &= mrem - 1;
                const uint32_t k2 = min((uint32_t)__builtin_ctz(mrem | 0x80000000u), 30u);
                const uint32_t d = k2 - k + cd;
                if (lim - ex > k2 && mrem != 0 && d <= 3) {
                    cd = (w >> (8 * d)) & 0xffu;
                    fin = cd > 3;  // C2
                    ex += fin ? 0u : cd;
                    mrem &= fin ? mrem : mrem - 1;
                }
            }
        }
        if (fin) {
            // a token that runs past csize (cd > 3, check C2) ends the stream in front of it, at the
            // item of the lowest bit left in mrem: the checks of step 5 then find the items short
            // of dsize or the completing item not at the end (C5), as the oracle's E_CORRUPT; in
            // a core padded to 9 bytes such a token can stand in the padding, behind the item
            // that completes dsize, where the oracle never reads it
            const uint32_t ke = lim - ex, kn = min((uint32_t)__builtin_ctz(mrem | 0x80000000u), 30u);
            L.p.info[x] = (uint8_t)(cd > 3 || ke <= kn ? kSmEnd + min(ke, kn) : 35 + ex);
            i = atomicAdd(&L.cursor, 1u);
            if (i < ncand) start();
        }
    }
    __syncthreads();
}
// ---- 2. J2 .. J16 (next position after 2^k whole groups; 0: a non-FULL group on the way) ----
__device__ __forceinline__ void sm_jumps(SmallLds &L, const SmallCtx &c) {
    const uint32_t tid = threadIdx.x, csize = c.csize;
    for (uint32_t x = c.hdr + tid; x <= csize; x += kSoloWG) {
        uint32_t j = 0;
        if (x + 4 <= csize) {
            const uint32_t e1 = L.p.info[x];
            if (sm_full(e1) && x + e1 + 4 <= csize) {
                const uint32_t e2 = L.p.info[x + e1];
                if (sm_full(e2)) j = x + e1 + e2;
            }
        }
        L.p.ja[x] = (uint16_t)j;
    }
    __syncthreads();
    for (uint32_t r = 0; r < 3; r++) {  // J4 -> jb, J8 -> ja, J16 -> jb
        const uint16_t *a = (r & 1) ? L.p.jb : L.p.ja;
        uint16_t *b = (r & 1) ? L.p.ja : L.p.jb;
        for (uint32_t x = c.hdr + tid; x <= csize; x += kSoloWG) {
            const uint32_t j = a[x];
            b[x] = j ? a[j] : (uint16_t)0;
        }
        __syncthreads();
    }
}
// ---- 3. the group chain: J16 hops, then single groups to the end; the hops expanded ----
__device__ __forceinline__ void sm_walk(SmallLds &L, const SmallCtx &c) {
    if (threadIdx.x == 0) {
        const uint32_t md = min(min(c.max_dsize, c.dsize), (uint32_t)QLZX_FAST_MAX_DSIZE);
        const uint32_t gmax = groups_max(md);  // a valid stream has <= groups_max(dsize) groups
        uint32_t x = c.hdr, g = 0, klast = 31;
        int st = QLZX_OK;
        while (x + 4 <= c.csize && g + 16 <= gmax) {
            const uint32_t j = L.p.jb[x];
            if (!j) break;
            L.glist[g] = (uint16_t)x;
            g += 16;
            x = j;
        }
        L.nhops = g / 16;
        while (x + 4 <= c.csize) {  // else: stream exhausted at a control word
            if (g >= gmax) { st = QLZX_E_CORRUPT; break; }
            const uint32_t e = L.p.info[x];
            L.glist[g++] = (uint16_t)x;
            if (sm_full(e)) { x += e; continue; }
            if (e == kSmBad) { st = QLZX_E_CORRUPT; break; }  // C1
            klast = e - kSmEnd;  // the stream ends inside this group
            break;
        }
        L.ngroups = g;
        L.klast = klast;
        L.st = chain_status(st, g);
        L.acc = check_acc_init();
    }
    __syncthreads();
    if (L.st != QLZX_OK) return;
    if (threadIdx.x < L.nhops) {  // the 15 groups inside hop tid
        uint32_t x = L.glist[16 * threadIdx.x];
#pragma unroll
        for (uint32_t k = 1; k < 16; k++) {
            x += L.p.info[x];
            L.glist[16 * threadIdx.x + k] = (uint16_t)x;
        }
    }
    __syncthreads();
}
// ---- 4. GroupRecs (the last group holds klast items); markers cleared ----
__device__ __forceinline__ void sm_recs(SmallLds &L, const SmallCtx &c, uint32_t ng, uint32_t klast) {
    for (uint32_t g = threadIdx.x; g < ng; g += kSoloWG) {
        const uint32_t x = L.glist[g];  // codes <= 3: the walk checked C2
        L.d.recs[g] = group_rec(x, sm_dword(L, x), g + 1 == ng ? klast : 31u, CodeBytes{L.cb});
    }
    for (uint32_t q = threadIdx.x; q < (c.dsize + 7) / 8; q += kSoloWG) *(uint4 *)(L.d.s + 8 * q) = make_uint4(0, 0, 0, 0);
    __syncthreads();
}
// ---- 5. items: thread tid decodes items [I0, I1), kSmIT per round ----
struct SmallTok {  // token dword at pos from the staged stream: zero bytes past csize
    const SmallLds &L;
    uint32_t csize;
    __device__ __forceinline__ uint32_t load(bool live, uint32_t pos) const {
        return sm_dword(L, live && pos < csize ? pos : 0u);
    }
    __device__ __forceinline__ uint32_t token(uint32_t raw, uint32_t) const { return raw; }
};
__device__ __forceinline__ void sm_items(SmallLds &L, const SmallCtx &c, uint32_t ng, uint32_t klast) {
    const uint32_t tid = threadIdx.x;
    const uint32_t nitems = (ng - 1) * 31 + klast;
    const uint32_t per = (nitems + kSoloWG - 1) / kSoloWG;
    const uint32_t I0 = min(tid * per, nitems), I1 = min(I0 + per, nitems);
    const SmallTok tok{L, c.csize};
    const ItemCtx ic{c.csize, c.dsize, c.hdr, tail_start(c.dsize)};
    auto sink = [&](uint32_t p, bool ism, uint32_t off, uint32_t lit) {
        L.d.s[p] = (uint16_t)(ism ? off : kLitMark);
        if (!ism) L.d.out[p] = (uint8_t)lit;
    };
    CheckAcc acc = check_acc_init();
    uint32_t total;
    if (per <= kSmIT) {  // one round per thread: its items stay in registers between the passes
        Item it[kSmIT];
        decode_round<kSmIT>(L.d.recs, ng, I0, I1, tok, it);
        uint32_t d = block_excl<false>(round_len(it), L.wsum[0], total);
        emit_round(it, I0, I1, d, ic, acc, sink);
    } else {
        const uint32_t d = block_excl<false>(items_len<kSmIT>(L.d.recs, ng, I0, I1, tok), L.wsum[0], total);
        items_emit<kSmIT>(L.d.recs, ng, I0, I1, d, tok, ic, acc, sink);
    }
    // one LDS update per wave (1024 same-address atomics would serialise)
    acc.bad = __ballot(acc.bad != 0) != 0;
    acc.done = __ballot(acc.done != 0) != 0;
    acc.tail_idx = ~(uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(~acc.tail_idx), 63);
    acc.max_match = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(acc.max_match), 63);
    if ((tid & 63) == 0) check_acc_merge(&L.acc, acc);
    __syncthreads();
}
// ---- 6. fill: markers -> source position of every byte of the thread's runs ----
// (one u32 per byte in registers; the u16 LDS array is read and written 16 B at a time)
__device__ __forceinline__ void sm_load_run(const SmallLds &L, uint32_t p0, uint32_t (&v)[kSmOwn]) {
#pragma unroll
    for (uint32_t q = 0; q < kSmOwn / 8; q++) {
        const uint4 w = *(const uint4 *)(L.d.s + p0 + 8 * q);
        const uint32_t w4[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t h = 0; h < 4; h++) v[8 * q + 2 * h] = w4[h] & 0xffffu, v[8 * q + 2 * h + 1] = w4[h] >> 16;
    }
}
__device__ __forceinline__ void sm_store_run(SmallLds &L, uint32_t p0, const uint32_t (&v)[kSmOwn]) {
#pragma unroll
    for (uint32_t q = 0; q < kSmOwn / 8; q++)
        *(uint4 *)(L.d.s + p0 + 8 * q) = make_uint4(v[8 * q] | (v[8 * q + 1] << 16), v[8 * q + 2] | (v[8 * q + 3] << 16),
                                                    v[8 * q + 4] | (v[8 * q + 5] << 16), v[8 * q + 6] | (v[8 * q + 7] << 16));
}
__device__ __forceinline__ void sm_fill(SmallLds &L, uint32_t dsize, uint32_t (&sv)[kSmSeg][kSmOwn]) {
    const uint32_t nseg = (dsize + kSoloWG * kSmOwn - 1) / (kSoloWG * kSmOwn);
    uint32_t lastp[kSmSeg];
#pragma unroll
    for (uint32_t z = 0; z < kSmSeg; z++) {
        const uint32_t p0 = sm_run(z);
        lastp[z] = 0;
        if (p0 < dsize) {
            sm_load_run(L, p0, sv[z]);
#pragma unroll
            for (uint32_t j = 0; j < kSmOwn; j++) lastp[z] = sv[z][j] ? p0 + j + 1 : lastp[z];
        }
    }
    uint32_t all0, all1, fz[kSmSeg];
    const uint32_t prev0 = block_excl<true>(lastp[0], L.wsum[0], all0);
    uint32_t prev1 = 0;
    if (nseg > 1) prev1 = max(block_excl<true>(lastp[1], L.wsum[1], all1), all0);
    fz[0] = prev0 ? L.d.s[prev0 - 1] : kLitMark;  // position 0 always has a marker
    fz[1] = prev1 ? L.d.s[prev1 - 1] : kLitMark;
    __syncthreads();  // every carry read before the runs are rewritten
#pragma unroll
    for (uint32_t z = 0; z < kSmSeg; z++) {
        const uint32_t p0 = sm_run(z);
        if (p0 < dsize) {
            uint32_t f = fz[z];
#pragma unroll
            for (uint32_t j = 0; j < kSmOwn; j++) {
                const uint32_t p = p0 + j;
                f = sv[z][j] ? sv[z][j] : f;
                sv[z][j] = (f == kLitMark || p >= dsize) ? p : p - f;
            }
            sm_store_run(L, p0, sv[z]);
        }
    }
    __syncthreads();
}
// ---- 7. pointer jumping until every byte's source is a literal (s[s] == s) ----
// Entries are rewritten while others read them; any value read is an earlier link of the
// same chain, so a stale read only costs a round.  A run with no jump in a round is final
// (every source it read is a literal) and drops out.
__device__ __forceinline__ void sm_jump(SmallLds &L, uint32_t dsize, uint32_t (&sv)[kSmSeg][kSmOwn]) {
    bool fin[kSmSeg];
#pragma unroll
    for (uint32_t z = 0; z < kSmSeg; z++) fin[z] = sm_run(z) >= dsize;
    for (;;) {
        bool ch = false;
#pragma unroll
        for (uint32_t z = 0; z < kSmSeg; z++) {
            if (!fin[z]) {
                uint32_t t[kSmOwn];
                bool cz = false;
#pragma unroll
                for (uint32_t j = 0; j < kSmOwn; j++) t[j] = L.d.s[sv[z][j]];
#pragma unroll
                for (uint32_t j = 0; j < kSmOwn; j++) {
                    cz = cz || t[j] != sv[z][j];
                    sv[z][j] = t[j];
                }
                if (cz) sm_store_run(L, sm_run(z), sv[z]);
                fin[z] = !cz;
                ch = ch || cz;
            }
        }
        if (!__syncthreads_or(ch)) break;
    }
}
// ---- 8. gather the runs' bytes from the literals and store them once ----
__device__ __forceinline__ void sm_gather(const SmallLds &L, uint8_t *dst, uint32_t dsize,
                                          const uint32_t (&sv)[kSmSeg][kSmOwn]) {
    const bool al16 = (((uintptr_t)dst) & 15u) == 0;
#pragma unroll
    for (uint32_t z = 0; z < kSmSeg; z++) {
        const uint32_t p0 = sm_run(z);
        if (p0 < dsize) {
            const uint32_t n = min(kSmOwn, dsize - p0);
            uint32_t o[kSmOwn / 4];
#pragma unroll
            for (uint32_t q = 0; q < kSmOwn / 4; q++) o[q] = 0;
#pragma unroll
            for (uint32_t j = 0; j < kSmOwn; j++) o[j >> 2] |= (uint32_t)L.d.out[sv[z][j]] << (8 * (j & 3));
            if (n == kSmOwn && al16) {
                *(uint4 *)(dst + p0) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
                for (uint32_t j = 0; j < n; j++) dst[p0 + j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
}

// Returns false (workgroup-uniform) when the block is not for this path: the caller then runs
// the general latency path on the same request.  src: `len` bytes, 16-B aligned with 16 bytes of
// slack readable past len; dst: dsize bytes (16-B stores when it is 16-B aligned).
__device__ __forceinline__ bool small_decode(SmallLds &L, const uint8_t *src, uint32_t len, uint8_t *dst,
                                             uint32_t dst_cap, uint32_t max_dsize, int32_t *status,
                                             uint32_t *dsize_out) {
    const uint32_t tid = threadIdx.x;
    if (len > kSmC || (((uintptr_t)src) & 15u)) return false;
    SOLO_T0
    sm_stage(L, src, len);
    SM_SUB(0);
    SmallCtx c{dst, 0, 0, 0, max_dsize};
    uint32_t kind;
    const int st0 = classify_block((const uint8_t *)L.src, len, dst_cap, max_dsize, kind, c.csize, c.dsize, c.hdr);
    if (st0 == QLZX_OK && kind == kBlkCompressed && c.dsize > kSmD) return false;
    if (st0 != QLZX_OK) {
        if (tid == 0) *status = st0, *dsize_out = 0;
        return true;
    }
    if (kind == kBlkStored) {
        sm_stored(L, c);
        if (tid == 0) *status = QLZX_OK, *dsize_out = c.dsize;
        return true;
    }
    if (c.dsize == 0) {  // nothing to decode: C5 accepts csize == hdr or the 9-byte minimum (oracle/qlz_oracle.c:197,228)
        if (tid == 0) *status = (c.csize == c.hdr || c.csize == c.hdr + 9) ? QLZX_OK : QLZX_E_CORRUPT, *dsize_out = 0;
        return true;
    }
    SM_SUB(1);
    const uint32_t ncand = sm_candidates(L, c);
    SM_SUB(2);
    sm_info(L, c, ncand);
    SM_STAMP(0);
    sm_jumps(L, c);
    SM_STAMP(1);
    sm_walk(L, c);
    const uint32_t ng = L.ngroups, klast = L.klast;
    if (L.st != QLZX_OK) {
        if (tid == 0) *status = L.st, *dsize_out = 0;
        return true;
    }
    SM_STAMP(2);
    sm_recs(L, c, ng, klast);
    SM_STAMP(3);
    sm_items(L, c, ng, klast);
    SM_STAMP(4);
    if (verdict_corrupt(L.acc)) {
        if (tid == 0) *status = QLZX_E_CORRUPT, *dsize_out = 0;
        return true;
    }
    uint32_t sv[kSmSeg][kSmOwn];  // the thread's runs of source positions
    sm_fill(L, c.dsize, sv);
    SM_STAMP(5);
    sm_jump(L, c.dsize, sv);
    SM_STAMP(6);
    sm_gather(L, dst, c.dsize, sv);
    if (tid == 0) *status = QLZX_OK, *dsize_out = c.dsize;
    SM_STAMP(7);
    return true;
}

}  // namespace qlzx
