// qlzx_decode_fmt.h -- the level-3 format rules of the position-parallel decoders, once for the
// three of them (qlzx_decode_solo.h, qlzx_decode_small.h, qlzx_decode_huge.hip): the token length
// code and its packed tables, the speculative and the byte-level parse of a control-word group,
// the GroupRec of a listed group, and the item checks C3-C5 with their verdict, as
// qlzx_encode_fmt.h is for the encoders.  The files of the decode-only unit (qlzx_k2.hip) do not
// include it.
//
// Where a decoder keeps the stream (LDS, global memory) and its codes is its own choice: a rule
// that reads a code takes a code-reader, a functor x -> token bytes - 1 of a match token at stream
// byte x (CodeWords, CodeBytes), inlined at each use.
#pragma once
#include "qlzx_decode_batch.h"

namespace qlzx {

__device__ __forceinline__ uint32_t tok_code(uint32_t t) {  // token bytes - 1 from its first byte
    const uint32_t ty = (t & 3u) + ((t & 127u) == 3u ? 1u : 0u);
    return __builtin_amdgcn_ubfe(0x32110u, ty * 4, 4);
}
// The codes of 16 stream bytes in one word, 2 bits each (byte j at bits 2j), and the read-back.
__device__ __forceinline__ uint32_t pack_codes16(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    const uint32_t d4[4] = {d0, d1, d2, d3};
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) v |= tok_code(d4[j >> 2] >> (8 * (j & 3))) << (2 * j);
    return v;
}
__device__ __forceinline__ uint32_t pack_codes_tail(const uint8_t *p, uint32_t n) {  // the last n < 16 bytes
    uint32_t v = 0;
    for (uint32_t j = 0; j < n; j++) v |= tok_code(p[j]) << (2 * j);
    return v;
}
__device__ __forceinline__ uint32_t code_at(const uint32_t *code, uint32_t x) {
    return __builtin_amdgcn_ubfe(code[x >> 4], 2 * (x & 15u), 2);
}
struct CodeWords {  // code-reader over packed code words
    const uint32_t *code;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return code_at(code, x); }
};
struct CodeBytes {  // code-reader over one code byte per stream byte
    const uint8_t *cb;
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const { return cb[x]; }
};

// An unaligned dword of the stream.  The address is pinned to VGPRs: where it is wave-uniform
// (the chain walk starts at hdr) the compiler would otherwise emit a scalar load, which drops
// the address's low two bits; vector loads take any byte address (unaligned access mode).
__device__ __forceinline__ uint32_t ld_dword(const uint8_t *p) {
    uint64_t a = (uint64_t)(uintptr_t)p;
    asm volatile("" : "+v"(a));
    return *(const uint32_t *)(uintptr_t)a;
}

// Length of the control-word group that WOULD start at stream byte x, whose dword is cw: 4 + 31
// items + the extra bytes of its match tokens.  0 (no shortcut) without bit 31 (check C1).
template <typename Code>
__device__ __forceinline__ uint32_t spec_group_len(uint32_t cw, Code code, uint32_t x) {
    if (!(cw >> 31)) return 0;
    uint32_t mrem = cw & 0x7fffffffu, extra = 0;
    const uint32_t base = x + 4;
    while (mrem) {
        extra += code(base + __builtin_ctz(mrem) + extra);
        mrem &= mrem - 1;
    }
    return 35 + extra;
}

// K1's byte-level parse (qlzx_decode_k1.h k_dec_parse6) of the group at x, for a group without a
// shortcut: C1 (bit 31 of the control word), C2 (every token ends inside the stream).  QLZX_OK
// with klast < 31 set when the stream ends inside the group, before item klast; else next is
// the byte after its 31 items.
template <typename Code>
__device__ __forceinline__ int parse_group_bytewise(uint32_t cw, uint32_t x, uint32_t csize, Code code,
                                                    uint32_t &klast, uint32_t &next) {
    if (!(cw >> 31)) return QLZX_E_CORRUPT;  // C1
    uint32_t p = x + 4, k = 0;
    for (; k < 31 && p < csize; k++) {
        const uint32_t c = ((cw >> k) & 1u) ? code(p) : 0u;
        if (p + c + 1 > csize) return QLZX_E_CORRUPT;  // C2
        p += c + 1;
    }
    if (k < 31) klast = k;
    next = p;
    return QLZX_OK;
}
// Status of a finished chain walk that listed g groups: a stream has at least one control word.
__device__ __forceinline__ int chain_status(int st, uint32_t g) {
    return st == QLZX_OK && g == 0 ? QLZX_E_CORRUPT : st;
}

// GroupRec of the group at x holding nk items: its match bits and the two bits of each match
// token's code at the item's bit.
template <typename Code>
__device__ __forceinline__ GroupRec group_rec(uint32_t x, uint32_t cw, uint32_t nk, Code code) {
    uint32_t mrem = cw & ((1u << nk) - 1u), extra = 0, a = 0, b = 0;
    const uint32_t m = mrem;
    while (mrem) {
        const uint32_t k = __builtin_ctz(mrem);
        const uint32_t c = code(x + 4 + k + extra);
        a |= (c & 1u) << k;
        b |= (c >> 1) << k;
        extra += c;
        mrem &= mrem - 1;
    }
    return GroupRec{x, m, a, b};
}
// Stream position of item k of a group: a literal is 1 byte, a match token 1 + its code.
__device__ __forceinline__ uint32_t item_pos(const GroupRec &r, uint32_t k) {
    const uint32_t low = (1u << k) - 1u;
    return r.ip + 4 + k + __builtin_popcount(r.a & low) + 2 * __builtin_popcount(r.b & low);
}

// What the item checks leave behind, per thread and then merged for the block.
struct CheckAcc {
    uint32_t bad;        // a failed check
    uint32_t done;       // an item completed dsize
    uint32_t tail_idx;   // first literal item at or after tail_from (~0: none)
    uint32_t max_match;  // last match item
};
__host__ __device__ __forceinline__ CheckAcc check_acc_init() { return CheckAcc{0, 0, 0xffffffffu, 0}; }
__device__ __forceinline__ void check_acc_merge(CheckAcc *all, const CheckAcc &a) {
    if (a.bad) atomicOr(&all->bad, 1u);
    if (a.done) atomicOr(&all->done, 1u);
    if (a.tail_idx != 0xffffffffu) atomicMin(&all->tail_idx, a.tail_idx);
    if (a.max_match) atomicMax(&all->max_match, a.max_match);
}
// First output position of the tail, which holds literals only (quicklz.c:503).
__host__ __device__ __forceinline__ uint32_t tail_start(uint32_t dsize) {
    return dsize > QLZX_TAIL ? dsize - 1 - QLZX_TAIL : 0;
}

// Checks of item I, which starts at output byte d < dsize and stream byte pos; a match of len
// bytes off back in a token of tl bytes, or a literal (len = tl = 1):
//   C3  a match copies from inside the output: 3 <= off <= d;
//   C4  the last bytes are literals: a match ends at least 4 bytes before dsize, and no match
//       follows the first literal at or after tail_from (the verdict compares the two indices);
//   C5  the item completing dsize is the last of the stream: it ends at csize, or inside the
//       padding of a core padded to the 9-byte minimum (csize == hdr + 9).
// False when the match itself is unusable (C3, C4): its bytes have no source.
__device__ __forceinline__ bool check_item(bool ism, uint32_t off, uint32_t len, uint32_t tl, uint32_t pos,
                                           uint32_t d, uint32_t I, uint32_t dsize, uint32_t csize, uint32_t hdr,
                                           uint32_t tail_from, CheckAcc &acc) {
    const uint32_t left = dsize - d;  // > 0
    const bool ok = !(ism && (off < 3 || off > d || len + 4 > left));
    if (!ok) acc.bad = 1;
    if (!ism && d >= tail_from) acc.tail_idx = min(acc.tail_idx, I);
    if (ism) acc.max_match = max(acc.max_match, I);
    if (len == left) {
        acc.done = 1;
        const uint32_t ip_end = pos + tl;
        if (!(ip_end == csize || (ip_end < hdr + 9 && csize == hdr + 9))) acc.bad = 1;
    }
    return ok;
}
// Corrupt: a failed check; no item completing dsize (C5); a match after the first tail literal (C4).
__host__ __device__ __forceinline__ bool verdict_corrupt(const CheckAcc &a) {
    return a.bad || !a.done || (a.tail_idx != 0xffffffffu && a.max_match > a.tail_idx);
}

// ---- the item rounds of the one-workgroup decoders ----
struct Item {
    uint32_t off, len, tl, pos, lit;
    bool ism;
};
struct ItemCtx {
    uint32_t csize, dsize, hdr, tail_from;
};
constexpr uint32_t kLitMark = 1;  // marker of a literal (match offsets are >= 3)

// Items [I, I + N) of a thread that owns the items below I1 (N <= 31: a round spans at most two
// groups).  Tok: load(live, pos) issues the read of the token dword at pos, all N in flight
// before token(raw, pos) gives the first; an item past I1 has len 0.
template <uint32_t N, typename Tok>
__device__ __forceinline__ void decode_round(const GroupRec *recs, uint32_t ng, uint32_t I, uint32_t I1,
                                             const Tok &tok, Item (&it)[N]) {
    const uint32_t g0 = I / 31;
    const GroupRec r0 = recs[g0], r1 = recs[g0 + 1 < ng ? g0 + 1 : g0];
    uint32_t raw[N];
#pragma unroll
    for (uint32_t j = 0; j < N; j++) {
        const uint32_t k0 = I - 31 * g0 + j;
        const bool second = k0 >= 31, live = I + j < I1;
        const uint32_t k = second ? k0 - 31 : k0;
        const GroupRec r = second ? r1 : r0;
        it[j].pos = item_pos(r, k);
        it[j].ism = live && ((r.m >> k) & 1u) != 0;
        raw[j] = tok.load(live, it[j].pos);
    }
#pragma unroll
    for (uint32_t j = 0; j < N; j++) {
        const uint32_t t = tok.token(raw[j], it[j].pos);
        uint32_t off, mlen, tl;
        decode_tok_bf(t, off, mlen, tl);
        it[j].off = off;
        it[j].len = it[j].ism ? mlen : (I + j < I1 ? 1u : 0u);
        it[j].tl = it[j].ism ? tl : 1u;
        it[j].lit = t & 0xffu;
    }
}
template <uint32_t N>
__device__ __forceinline__ uint32_t round_len(const Item (&it)[N]) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < N; j++) s += it[j].len;
    return s;
}
// The checks of a decoded round whose first item starts at output byte d (advanced past the
// round), and sink(d, is match, offset, literal byte) for every live item: it leaves the marker at
// d (the match offset, or kLitMark) and keeps the byte of a literal.
template <uint32_t N, typename Sink>
__device__ __forceinline__ void emit_round(const Item (&it)[N], uint32_t I, uint32_t I1, uint32_t &d,
                                           const ItemCtx &c, CheckAcc &acc, Sink &&sink) {
#pragma unroll
    for (uint32_t j = 0; j < N; j++) {
        const Item &e = it[j];
        if (I + j < I1 && d < c.dsize) {  // live
            check_item(e.ism, e.off, e.len, e.tl, e.pos, d, I + j, c.dsize, c.csize, c.hdr, c.tail_from, acc);
            sink(d, e.ism, e.off, e.lit);
        }
        d += e.len;
    }
}
// The two passes over a thread's items [I0, I1), N per round: their output length, and with the
// start d of the first one known, their checks and markers.
template <uint32_t N, typename Tok>
__device__ __forceinline__ uint32_t items_len(const GroupRec *recs, uint32_t ng, uint32_t I0, uint32_t I1,
                                              const Tok &tok) {
    uint32_t sum = 0;
    for (uint32_t I = I0; I < I1; I += N) {
        Item it[N];
        decode_round<N>(recs, ng, I, I1, tok, it);
        sum += round_len(it);
    }
    return sum;
}
template <uint32_t N, typename Tok, typename Sink>
__device__ __forceinline__ void items_emit(const GroupRec *recs, uint32_t ng, uint32_t I0, uint32_t I1, uint32_t d,
                                           const Tok &tok, const ItemCtx &c, CheckAcc &acc, Sink &&sink) {
    for (uint32_t I = I0; I < I1; I += N) {
        Item it[N];
        decode_round<N>(recs, ng, I, I1, tok, it);
        emit_round(it, I, I1, d, c, acc, sink);
    }
}

// Exclusive prefix sum (or max) over a workgroup of 64 * kBlockWaves threads; `all` = the sum
// (max) of every thread.  wsum: kBlockWaves words of LDS, free again after the caller's next
// barrier.
constexpr uint32_t kBlockWaves = 16;
template <bool MAX>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t *wsum, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = MAX ? wave_incl_max(v) : wave_incl_scan(v);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t below = 0, tot = 0;
#pragma unroll
    for (uint32_t j = 0; j < kBlockWaves; j++) {
        const uint32_t x = wsum[j];
        if (MAX) {
            below = j < w ? max(below, x) : below;
            tot = max(tot, x);
        } else {
            below += j < w ? x : 0u;
            tot += x;
        }
    }
    all = tot;
    if (MAX) return max(below, wave_shr1(incl));
    return below + incl - v;
}

}  // namespace qlzx
