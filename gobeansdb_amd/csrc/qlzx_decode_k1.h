// qlzx_decode_k1.h -- K1 of the batch decoder pair (dsize <= QLZX_FAST_MAX_DSIZE), compiled in
// qlzx_k2.hip's unit only:
//
// K1 k_dec_parse6 (round 5)  one LANE per block: the serial control-word chain of
//     quicklz.c:513-671, one item STEP at a time (a literal run and the match that ends it, or a
//     control word), reading only control words and the first byte of each match token from a
//     per-lane LDS ring the lane refills itself.  The remaining control bits are kept with their
//     sentinel (cwr; 1 = group exhausted), so the item index is clz(cwr) and a literal run is
//     ctz(cwr): no per-item counters.  Emits one GroupRec {ip, cw, a, b} per control word (a, b:
//     bit-planes of token bytes - 1).
//
// Check C1 is applied exactly as by the oracle (oracle/qlz_oracle.c:180-231); a
// token cut by csize (C2) ends the item list in front of it, and K2's checks give the verdict.
#pragma once
#include "qlzx_decode_batch.h"

namespace qlzx {

// K1 k_dec_parse6 (round 5): one LANE per block walks the serial control-word chain.  Each lane
// refills its own LDS ring: an iteration writes the rounds (32 B) loaded in the previous
// iteration into the lane's slots, issues plain global loads for up to two more rounds the ring
// has room for, then takes at most `kmax` steps.  Round 4's k_dec_parse4 moved every lane of a
// wave through the same round (one LDS-DMA per round into a wave-uniform slot) and looped until
// the lane with the most steps in that round was done: the wave paid max-over-lanes steps per
// round.  Here lanes drift apart in stream position and the wave pays kmax steps per iteration.
// c2 25.1-25.3 -> 24.7-24.9 ms at kmax 16; c4 346 -> 377 GiB/s at kmax 10
// (tools/gpu_r5lr3.sh, profiles/r05_k1_lane_ring_ab.txt).
// One wave's 64 blocks (lin = the block's place in the chunk), called by the kernel below.
__device__ __forceinline__ void k1_parse_wave(uint8_t *ring, uint32_t lane, uint32_t lin, const qlzx_blocks &b,
                                              const uint32_t *dst_cap, uint32_t *dsize_out, int32_t *status,
                                              uint32_t first, uint32_t count, BlkInfo *info, GroupRec *recs,
                                              uint32_t gmax, const uint32_t *order, uint32_t max_dsize,
                                              uint32_t kmax) {
    constexpr uint32_t S = kRingSlots;
    const bool inrange = lin < count;
    const uint32_t i = inrange ? (order ? order[lin] : first + lin) : first;

    int st = QLZX_OK;
    uint32_t kind = kBlkSkip, csize = 0, dsize = 0, hdr = 0, len = 0;
    const uint8_t *src = b.src + b.src_off[i];
    if (inrange) {
        len = b.src_len[i];
        st = classify_block(src, len, dst_cap ? dst_cap[i] : 0xffffffffu, max_dsize, kind, csize, dsize, hdr);
        if (st == QLZX_OK && kind == kBlkCompressed && dsize == 0) {  // oracle/qlz_oracle.c:197,228
            st = (csize == hdr || csize == hdr + 9) ? QLZX_OK : QLZX_E_CORRUPT;
            kind = kBlkSkip;
        }
    }
    const uintptr_t a0 = (uintptr_t)src;
    const uint8_t *gbase = (const uint8_t *)(a0 & ~(uintptr_t)15);
    const uint32_t shift = (uint32_t)(a0 & 15);
    const uint32_t span = (st == QLZX_OK && kind == kBlkCompressed) ? csize : 0;
    const uint32_t last16 = span ? (span + shift - 1) >> 4 : 0;
    const uint32_t nrounds = span ? (span + shift - 1) / kRoundBytes + 1 : 0;
    const bool parsing = inrange && span > 0;

    uint32_t ip = hdr, g = 0, cwr = 1, cwg = 0, ra = 0, rb = 0, rec_ip = 0;
    GroupRec *myrec = recs + (size_t)(inrange ? lin : 0) * gmax;
    bool done_parse = !parsing;

    // ring bookkeeping: rounds [0, rl) are in the lane's slots (round r in slot r % S), rounds
    // [rl, ri) are loaded into registers and go to the slots at the next iteration
    uint32_t rl = 0, ri = 0;
    // accept up to two rounds: a round r may overwrite round r - S only once the lane reads no
    // byte below round r - S + 1 (ring_rd32 reads the aligned dwords at and after its position)
    // rounds loaded per iteration (at most; the ring can take up to S - 1 rounds past the one
    // being read).  Three rounds per iteration were slower at every step budget (c2 25.3-26.2 vs
    // 24.7 ms, c5 517-543 vs 571 GiB/s: profiles/r05_k1_lane_ring_ab.txt)
    constexpr uint32_t M = 2;
    static_assert(M == 2 || M == 3, "rounds per iteration");
    auto accept = [&]() __attribute__((always_inline)) -> uint32_t {
        const uint32_t cap = ((ip + shift) & ~3u) / kRoundBytes + S - 1;  // last round the ring can take
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < M; k++) n += (!done_parse && ri + k < nrounds && ri + k <= cap) ? 1u : 0u;
        return n;
    };
    // the M rounds from ri on (16-B pieces 2 ri ..), clamped into the stream; a lane taking fewer
    // rounds loads the stream's first piece instead (cached, never written)
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u4v g_u4;
    const uintptr_t gaddr = (uintptr_t)gbase;  // integer -> global pointer: global_load, not flat
#define K1_LD(n, k, j) (*(g_u4 *)(gaddr + (size_t)((n) > (k) ? min(ri * kPieces + 2 * (k) + (j), last16) : 0u) * 16))
#define K1_LOAD(n, v0, v1, v2, v3, v4, v5)                                                        \
    do {                                                                                          \
        v0 = K1_LD(n, 0, 0), v1 = K1_LD(n, 0, 1), v2 = K1_LD(n, 1, 0), v3 = K1_LD(n, 1, 1);        \
        if (M >= 3) v4 = K1_LD(n, 2, 0), v5 = K1_LD(n, 2, 1);                                     \
        ri += (n);                                                                                \
    } while (0)
    // rounds rl .. rl + n - 1 into their slots
#define K1_STORE(n, v0, v1, v2, v3, v4, v5)                                                       \
    do {                                                                                          \
        /* an unconditional use: the loads land here in every lane, so no later reuse of their   \
           registers waits on a vmcnt that also counts the newer loads */                         \
        asm volatile("" ::"v"(v0.x), "v"(v0.y), "v"(v0.z), "v"(v0.w), "v"(v1.x), "v"(v1.y),        \
                     "v"(v1.z), "v"(v1.w), "v"(v2.x), "v"(v2.y), "v"(v2.z), "v"(v2.w), "v"(v3.x),  \
                     "v"(v3.y), "v"(v3.z), "v"(v3.w));                                             \
        if (M >= 3) asm volatile("" ::"v"(v4.x), "v"(v4.y), "v"(v4.z), "v"(v4.w), "v"(v5.x),      \
                                 "v"(v5.y), "v"(v5.z), "v"(v5.w));                                 \
        uint8_t *sl0 = ring + (((rl & (S - 1)) * kPieces) << 10) + lane * 16;                     \
        uint8_t *sl1 = ring + ((((rl + 1) & (S - 1)) * kPieces) << 10) + lane * 16;               \
        uint8_t *sl2 = ring + ((((rl + 2) & (S - 1)) * kPieces) << 10) + lane * 16;               \
        if ((n) >= 1) *(u4v *)sl0 = v0, *(u4v *)(sl0 + 1024) = v1;                                \
        if ((n) >= 2) *(u4v *)sl1 = v2, *(u4v *)(sl1 + 1024) = v3;                                \
        if (M >= 3 && (n) >= 3) *(u4v *)sl2 = v4, *(u4v *)(sl2 + 1024) = v5;                      \
        rl += (n);                                                                                \
    } while (0)
    // One step: a control word, or a literal run (ctz of the remaining control bits, no bytes
    // read), the match that ends it and, when the next item is a match whose first byte is in the
    // same dword, that one too.  Round 6 form (87 instead of 103 vector instructions per step,
    // same checks in the same order as round 5's select-based step, in git history): a lane that
    // cannot advance leaves the loop before anything is updated, the control-word and match cases
    // update through a branch each, and the second token's byte is taken with one alignbyte.
    // c2 time unchanged (23.77 vs 23.79 ms): K1's instructions cost c2 about half their issue
    // time (+32 per step: +0.42 ms), DESIGN.md §3.
    const uint32_t lane16 = lane << 4;
    auto rd32 = [&](uint32_t x) __attribute__((always_inline)) -> uint32_t {  // ring_rd32<S>(ring, x, lane)
        constexpr uint32_t PB = S * kPieces == 8 ? 3u : S * kPieces == 4 ? 2u : 4u;  // log2(pieces of 1 KiB)
        static_assert((1u << PB) == S * kPieces, "ring address below assumes 4, 8 or 16 pieces of 1 KiB");
        const uint32_t x4 = x + 4;
        const uint32_t a1 = (__builtin_amdgcn_ubfe(x, 4, PB) << 10) | ((x & 12u) | lane16);
        const uint32_t a2 = (__builtin_amdgcn_ubfe(x4, 4, PB) << 10) | ((x4 & 12u) | lane16);
        const uint32_t lo = *(const uint32_t *)(ring + a1);
        const uint32_t hi = *(const uint32_t *)(ring + a2);
        return __builtin_amdgcn_alignbyte(hi, lo, x);
    };
    // token bytes - 1 from the token's first byte (quicklz.c:579-610): 0, 1, 1, 2 by b & 3,
    // 3 when b & 127 == 3
    auto tlc = [](uint32_t b) __attribute__((always_inline)) -> uint32_t {
        return __builtin_amdgcn_ubfe(0x94u, (b & 3u) * 2, 2) + ((b & 127u) == 3u ? 1u : 0u);
    };
    auto steps = [&]() __attribute__((always_inline)) -> uint32_t {
        const uint32_t lim = rl * kRoundBytes - shift;  // stream bytes below lim are in the ring
        uint32_t k = 0;
        if (!done_parse) {
            for (;;) {  // per-lane loop, at most kmax steps
                const bool gb = cwr == 1;
                const uint32_t run = min((uint32_t)__builtin_ctz(cwr), csize - ip);
                const uint32_t q = ip + run;
                const uint32_t rest = cwr >> run;
                // a match at q (gb: rest == 1; a run cut by the stream end: q == csize)
                const bool hasm = (rest > 1u) & (q < csize);
                const uint32_t need = gb ? 4u : 1u;
                if (ip + need > csize) {  // the stream ends here (C1/C5 are K2's or the caller's)
                    done_parse = true;
                    break;
                }
                if ((gb | hasm) & (q + need > lim)) break;  // wait for the ring
                const uint32_t w = rd32(q + shift);
                const uint32_t e = tlc(w);
                const uint32_t q2 = q + e + 1, rest2 = rest >> 1;
                const bool hasm2 = hasm & (e < 3u) & ((rest2 & 1u) != 0) & (rest2 > 1u) & (q2 < csize) & (q2 < lim);
                const uint32_t e2 = hasm2 ? tlc(__builtin_amdgcn_alignbyte(0u, w, e + 1)) : 0u;
                const bool bad = (gb & (((int32_t)w >= 0) | (g >= gmax))) | (hasm & (q2 > csize)) |
                                 (hasm2 & (q2 + e2 + 1 > csize));
                if (bad) {
                    // C1 is final.  A token that runs past csize (C2) only ends the parse in front
                    // of it: K2 then finds that the items stop short of dsize, or that the item
                    // completing dsize does not end the stream (C5), which is the oracle's
                    // E_CORRUPT as well -- but in a core padded to 9 bytes (quicklz.c:493) set
                    // bits above the last item make tokens of the padding, which the oracle,
                    // stopping at op == dsize, never reads: that stream is valid.
                    if (gb) {
                        st = QLZX_E_CORRUPT;
                    } else {
                        const bool first = q2 <= csize;  // the first token fits: the second is the cut one
                        const uint32_t idx = __builtin_clz(cwr) + run;
                        ra |= first ? (e & 1u) << idx : 0u;
                        rb |= first ? (e >> 1) << idx : 0u;
                        ip = first ? q2 : q;
                        cwr = rest >> (first ? 1u : 0u);
                    }
                    done_parse = true;
                    break;
                }
                if (gb) {
                    // the record store is invisible to the compiler's vmcnt bookkeeping: counted, it
                    // made every wait before the step loop a vmcnt(0), i.e. a wait for the loads just
                    // issued (an unseen store only makes the compiler's later vmcnt(N) waits stricter)
                    if (g > 0) {
                        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 rec = {rec_ip, cwg, ra, rb};
                        // s_nop 1: two wait states before any VALU write of the store's data
                        // registers (rec_ip .. rb are reassigned right below), which gfx940 and
                        // later need after a store of more than 64 bits; the compiler's hazard
                        // recogniser does not look into inline asm
                        asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(myrec + (g - 1)), "v"(rec)
                                     : "memory");
                    }
                    rec_ip = ip;
                    cwg = w;
                    g++;
                    ip += 4;
                    cwr = w;
                    ra = 0;
                    rb = 0;
                } else {
                    const uint32_t idx = __builtin_clz(cwr) + run;  // item index of the match
                    const uint32_t em = hasm ? e : 0u, e2m = hasm2 ? e2 : 0u;
                    ra |= ((em & 1u) | ((e2m & 1u) << 1)) << idx;
                    rb |= ((em >> 1) | (e2m & 2u)) << idx;
                    ip = q + em + e2m + (hasm ? 1u : 0u) + (hasm2 ? 1u : 0u);
                    cwr = rest >> ((hasm ? 1u : 0u) + (hasm2 ? 1u : 0u));
                }
                if (++k >= kmax) break;
            }
        }
        return k;
    };
#ifdef QLZX_PROFILE
    // profile build: outer iterations, wave step trips (max steps over lanes per iteration) and
    // lane steps (sum over lanes) per wave, in slot 0
    PROF_DECL
    auto k1prof = [&](uint32_t k) __attribute__((always_inline)) {
        uint32_t mx = k, sm = k;
        for (int o = 32; o >= 1; o >>= 1) {
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
            sm += (uint32_t)__shfl_xor((int)sm, o);
        }
        PROF_COUNT(0, 1);
        PROF_COUNT(1, mx);
        PROF_COUNT(2, sm);
    };
#define K1_STEPS() k1prof(steps())
#else
#define K1_STEPS() (void)steps()
#endif

    u4v pa0, pa1, pa2, pa3, pa4, pa5, pb0, pb1, pb2, pb3, pb4, pb5;
    uint32_t na = accept();
    K1_LOAD(na, pa0, pa1, pa2, pa3, pa4, pa5);
    uint32_t nb = 0;
    // Every iteration a lane either steps or lands a round, so csize + nrounds iterations finish
    // any stream; past that bound a lane stops as corrupt (a guard: the loop always ends).
    const uint32_t trip_cap = span + nrounds + 8;
    uint32_t trips = 0;
    auto guard = [&]() __attribute__((always_inline)) {
        trips++;
        if (!done_parse && trips > trip_cap) done_parse = true, st = QLZX_E_CORRUPT;
    };
    // two iterations per loop trip: register sets va / vb alternate, no copies of loaded data
    for (;;) {
        K1_STORE(na, pa0, pa1, pa2, pa3, pa4, pa5);
        nb = accept();
        K1_LOAD(nb, pb0, pb1, pb2, pb3, pb4, pb5);
        K1_STEPS();
        guard();
        if (__ballot(!done_parse) == 0) break;
        K1_STORE(nb, pb0, pb1, pb2, pb3, pb4, pb5);
        na = accept();
        K1_LOAD(na, pa0, pa1, pa2, pa3, pa4, pa5);
        K1_STEPS();
        guard();
        if (__ballot(!done_parse) == 0) break;
    }
#undef K1_LD
#undef K1_LOAD
#undef K1_STORE
#undef K1_STEPS
    if (parsing && st == QLZX_OK && g > 0) myrec[g - 1] = GroupRec{rec_ip, cwg, ra, rb};
    vm_sync();
#ifdef QLZX_PROFILE
    PROF_MARK(3);
    PROF_COUNT(4, 1);
    PROF_FLUSH(0);
#endif
    if (!inrange) return;
    if (st == QLZX_OK && kind == kBlkCompressed && (!done_parse || g == 0)) st = QLZX_E_CORRUPT;
    BlkInfo bi{0, 0, kind, dsize};
    if (st != QLZX_OK) {
        bi.kind = kBlkSkip;
        status[i] = st;
        if (dsize_out && st != kPending) dsize_out[i] = 0;
    } else if (kind == kBlkCompressed) {
        bi.ngroups = g;
        bi.nitems = (g - 1) * 31 + __builtin_clz(cwr);
    } else if (kind == kBlkSkip) {
        status[i] = QLZX_OK;
        if (dsize_out) dsize_out[i] = 0;
    }
    info[lin] = bi;
}

__global__ void __launch_bounds__(kParseWG) k_dec_parse6(qlzx_blocks b, const uint32_t *dst_cap, uint32_t *dsize_out,
                                                     int32_t *status, uint32_t first, uint32_t count, BlkInfo *info,
                                                     GroupRec *recs, uint32_t gmax, const uint32_t *order,
                                                     uint32_t max_dsize, uint32_t kmax) {
    constexpr uint32_t S = kRingSlots;
    __shared__ __attribute__((aligned(16))) uint8_t ring_all[(kParseWG / 64) * kRingWaveS<S>];
    const uint32_t lane = threadIdx.x & 63;
    uint8_t *ring = ring_all + (threadIdx.x >> 6) * kRingWaveS<S>;
    k1_parse_wave(ring, lane, blockIdx.x * kParseWG + threadIdx.x, b, dst_cap, dsize_out, status, first, count, info,
                  recs, gmax, order, max_dsize, kmax);
}

}  // namespace qlzx
