// qlzx_decode_k2.h -- K2 of the batch decoder pair (dsize <= QLZX_FAST_MAX_DSIZE); qlzx_k2.hip
// instantiates it without the CRC prologue, qlzx_decode_batch.hip with it:
//
// K2 k_dec_chunk4  one WAVE per block, 64 items per batch and 256 output bytes per chunk:
//     * ITEM PHASE: token position from the GroupRec, branch-free token decode, DPP scan of the
//       output lengths; item i leaves ONE u32 key (d << 16 | off) in a 256-entry marker ring
//       at slot d (off = 0 for a literal, whose byte also goes to the output window);
//     * CHUNK PHASE: lane l owns bytes c + 4l .. c + 4l + 3.  The keys grow with d, so the
//       forward fill of "the item covering byte p" is a max-scan (in-lane max + DPP max across
//       lanes + the previous chunk's carry) and the source is s = p - (key & 0xffff) for match
//       and literal bytes alike.  In-chunk sources are chased by pointer jumping over the
//       chunk's own marker slots (free once read), then every byte is gathered from the 4 KiB
//       LDS window (or, when older than the window, from the block's output in HBM).
//     The batch loop is unrolled by two with two register sets for the prefetched GroupRec and
//     token dword, so no prefetched register is copied (and waited for) at a batch boundary.
//
// Checks C3-C5 are applied exactly as by the oracle (oracle/qlz_oracle.c:180-231).
#pragma once
#include "qlzx_crc.h"
#include "qlzx_decode_batch.h"

namespace qlzx {

// ------------------------------------------------------------------------------- K2 ----
constexpr uint32_t kV4W = 4096;   // output window (LDS ring)
constexpr uint32_t kV4MR = 256;   // marker ring (u32 keys)
constexpr uint32_t kV4Bpl = 4;  // output bytes per lane per chunk
constexpr uint32_t kV4Chunk = 64 * kV4Bpl;      // 256 or 512 output bytes per chunk
static_assert(kV4Chunk <= kV4MR, "a chunk's pointer-jumping array lives in its marker slots");

template <uint32_t W = kV4W>
struct K2v4Lds {
    uint8_t win[W];
    uint32_t mk[kV4MR];
};

template <uint32_t WIN>
__device__ __forceinline__ void dec_v4_block(K2v4Lds<WIN> &L, const uint8_t *src, uint8_t *dst, uint32_t csize,
                                             const BlkInfo bi, const GroupRec *rb, int32_t *status_i,
                                             uint32_t *dsize_i, uint32_t lane) {
    constexpr uint32_t W = WIN, MR = kV4MR, CH = kV4Chunk;
    const uint32_t dsize = bi.dsize;
    if (bi.kind == kBlkStored) {  // quicklz.c:808-811
        const uint32_t hdr = (src[0] & 2u) ? 9u : 3u;
        const uint8_t *s = src + hdr;
        uint32_t p0 = 0;
        if ((((uintptr_t)dst) & 15u) == 0) {
            p0 = dsize & ~15u;
            for (uint32_t p = lane * 16; p < p0; p += 1024) {
                const uint32_t *q = (const uint32_t *)(s + p);
                *(uint4 *)(dst + p) = make_uint4(q[0], q[1], q[2], q[3]);
            }
        }
        for (uint32_t p = p0 + lane; p < dsize; p += 64) dst[p] = s[p];
        if (lane == 0) { *status_i = QLZX_OK; if (dsize_i) *dsize_i = dsize; }
        return;
    }
    for (uint32_t q = lane * 4; q < MR; q += 256) *(uint4 *)(L.mk + q) = make_uint4(0, 0, 0, 0);

    const uint32_t nitems = bi.nitems;
    const uint32_t hdr = (src[0] & 2u) ? 9u : 3u;
    const uint32_t nb = (nitems + 63) / 64;
    const uint32_t tail_from = dsize > QLZX_TAIL ? dsize - 1 - QLZX_TAIL : 0;  // op >= this: tail (quicklz.c:503)

    // token position of item (c.g, c.k) and its dword address (clamped into the stream; lanes past
    // the last item read a clamped record and are masked by v where it matters)
    auto tok_pos = [&](const GroupRec &gr, const ItemCursor &c, uint32_t &p) -> uint32_t {
        const uint32_t low = (1u << c.k) - 1u;
        const uint32_t pos = gr.ip + 4 + c.k + __builtin_popcount(gr.a & low) + 2 * __builtin_popcount(gr.b & low);
        p = min(pos, csize - 4);
        return (pos & 0x7fffffffu) | (((gr.m >> c.k) & 1u) << 31);
    };
    const uint32_t glast = bi.ngroups - 1;
    // register sets: (posm, tok) of the batch being decoded and of the next; GroupRec of the
    // batch after the decoded one and of the one after that
    ItemCursor ck{lane / 31, lane % 31};
    uint32_t posmA, tokA, posmB = 0, tokB = 0;
    GroupRec grA, grB;
    {
        const GroupRec g0 = rb[min(ck.g, glast)];
        uint32_t tp;
        posmA = tok_pos(g0, ck, tp);
        tokA = *(const uint32_t *)(src + tp);
        ck.next();
        grB = rb[min(ck.g, glast)];
        grA = grB;
    }
    PROF_DECL
    uint32_t D = 0, bt = 0, c = 0, cin = 0;
    bool tail = false, complete = false, err = false;
    // Per-lane predicates that also decide a wave-wide branch are kept as lane masks: cmp_lt and
    // its kin give a compare's mask in an SGPR pair, the masks are joined on the scalar unit and
    // in_mask() hands a mask back as the lane's bool for free.  A ballot of a bool that another
    // basic block computed costs a select and a compare on the vector unit, three times a batch.
    uint64_t pendm = 0;  // lanes whose item waits for its marker slot
    uint32_t pd = 0, pkey = 0;
    uint32_t plit = 0;

    // one batch: decode (posm, tok), prefetch the next batch's token from gr_next into
    // (posm_n, tok_n) and the GroupRec after it into gr_nn
    auto batch = [&](uint32_t posm, uint32_t tok, const GroupRec &gr_next, uint32_t &posm_n, uint32_t &tok_n,
                     GroupRec &gr_nn) __attribute__((always_inline)) {
        if (pendm) {  // a straddling batch's items not marked by a chunk yet (all start below c + CH)
            if (in_mask(pendm)) {
                L.mk[pd & (MR - 1)] = pkey;
                if (plit < 0x100u) L.win[pd & (W - 1)] = (uint8_t)plit;
            }
            pendm = 0;
        }
        const uint64_t vm = cmp_lt(lane, nitems - bt * 64);  // bt < nb: the difference is positive
        const bool v = in_mask(vm);
        {
            uint32_t tp;
            posm_n = tok_pos(gr_next, ck, tp);
            tok_n = *(const uint32_t *)(src + tp);
            ck.next();
            gr_nn = rb[min(ck.g, glast)];
        }
        const uint64_t ismm = vm & cmp_ne(posm >> 31, 0u);
        const bool ism = in_mask(ismm);
        const uint32_t pos = posm & 0x7fffffffu;
        // the last tokens: dword clamped, so the token starts pos - (csize - 4) bytes into it
        const uint32_t t = __builtin_amdgcn_alignbyte(0u, tok, __builtin_elementwise_sub_sat(pos, csize - 4));
        uint32_t off, mlen, tl;
        decode_tok_bf(t, off, mlen, tl);
        const uint32_t len = ism ? mlen : (v ? 1u : 0u);
        const uint32_t incl = wave_incl_scan(len);
        const uint32_t total = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(incl, 63));
        const uint32_t d = D + incl - len;
        const uint64_t livem = vm & cmp_lt(d, dsize);
        const bool live = in_mask(livem);
        uint64_t badm;
        if (tail || D + total > tail_from) {
            tl = ism ? tl : 1u;
            const uint64_t tail_lanes = __ballot(live && !ism && d >= tail_from);
            const uint32_t tail_lane = tail ? 0u : ff1_or(tail_lanes, 64u);  // C4: no match after it
            tail = tail || tail_lanes != 0;
            const bool mok = off >= 3 && off <= d && d + len + 4 <= dsize && lane < tail_lane;  // C3, C4
            const bool last = live && d + len == dsize;  // C5: the item completing dsize ends the stream
            const uint32_t ip_end = pos + tl;
            const bool eok = ip_end == csize || (ip_end < hdr + 9 && csize == hdr + 9);
            badm = __ballot(live && ((ism && !mok) || (last && !eok)));
            complete = __ballot(last) != 0;
        } else {
            badm = ismm & (cmp_lt(off, 3u) | cmp_lt(d, off));  // C3
        }
        if (badm) {
            err = true;
            return;
        }
        const uint32_t key = (d << 16) | (ism ? off : 0u);
        const uint64_t wrm = livem & cmp_lt(d, c + MR);
        if (in_mask(wrm)) {
            L.mk[d & (MR - 1)] = key;
            // a match's own window slot holds a byte older than the far bound (d < c + MR) that no
            // gather reads before the chunk of d overwrites it: the byte can go there unconditionally
            L.win[d & (W - 1)] = (uint8_t)t;
        }
        pendm = livem & ~wrm;
        pd = d;
        pkey = key;
        plit = ism ? 0x100u : (t & 0xffu);
        D = __builtin_amdgcn_readfirstlane(D + total);
        bt++;
        PROF_COUNT(5, 1);
    };

    // chunk phases while every item starting below c + 256 is known; true when the block is done
    auto chunks = [&]() __attribute__((always_inline)) -> bool {
        while (c < dsize && (complete || D >= c + CH)) {
            if (pendm) {  // items of the last batch that start at or above c_prev + MR
                const uint64_t wrm = pendm & cmp_lt(pd, c + MR);
                if (in_mask(wrm)) {
                    L.mk[pd & (MR - 1)] = pkey;
                    if (plit < 0x100u) L.win[pd & (W - 1)] = (uint8_t)plit;
                }
                pendm &= ~wrm;
            }
            constexpr uint32_t B = kV4Bpl;
            const uint32_t r0 = B * lane, p0 = c + r0;
            uint32_t *mkl = L.mk + ((c & (MR - 1)) + r0);
            uint32_t m[B];
#pragma unroll
            for (uint32_t h = 0; h < B; h += 4) {
                const uint4 q = *(const uint4 *)(mkl + h);
                m[h] = q.x, m[h + 1] = q.y, m[h + 2] = q.z, m[h + 3] = q.w;
            }
            uint32_t lmax = m[0];
#pragma unroll
            for (uint32_t j = 1; j < B; j++) lmax = max(lmax, m[j]);
            const uint32_t incl = wave_incl_max(lmax);
            uint32_t f = max(wave_shr1(incl), cin);
            cin = max(cin, (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(incl, 63)));
            // sources relative to the chunk (rj = s - c mod 2^32): in-chunk sources of match bytes
            // are s in [c, p), i.e. rj < r0 + j unsigned (a literal has rj = r0 + j, a source
            // below c wraps above every in-chunk value), and the pointer jumping below compares
            // and indexes the chunk's slots with rj directly
            uint32_t rj[B];
            bool qa[B], anyq = false;
#pragma unroll
            for (uint32_t j = 0; j < B; j++) {
                f = max(f, m[j]);
                rj[j] = r0 + j - (f & 0xffffu);
                qa[j] = rj[j] < r0 + j;
                anyq = anyq || qa[j];
            }
            PROF_MARK(1);
            if (__ballot(anyq)) {
                // the chunk's marker slots are free once read: they hold each byte's current source
                uint32_t *spb = L.mk + (c & (MR - 1));
#pragma unroll
                for (uint32_t h = 0; h < B; h += 4) *(uint4 *)(mkl + h) = make_uint4(rj[h], rj[h + 1], rj[h + 2], rj[h + 3]);
                do {
                    uint32_t t[B];
#pragma unroll
                    for (uint32_t j = 0; j < B; j++) t[j] = spb[qa[j] ? rj[j] : r0 + j];
                    uint64_t anym = 0;
#pragma unroll
                    for (uint32_t j = 0; j < B; j++) {
                        // a byte whose source's source is outside the chunk or a literal is final
                        qa[j] = t[j] < rj[j];
                        anym |= __ballot(qa[j]);
                        rj[j] = t[j];
                    }
                    anyq = anym != 0;
#pragma unroll
                    for (uint32_t h = 0; h < B; h += 4)
                        *(uint4 *)(mkl + h) = make_uint4(rj[h], rj[h + 1], rj[h + 2], rj[h + 3]);
                    PROF_COUNT(7, 1);
                } while (anyq);

            }
            PROF_MARK(2);
            // far: s < lo  <=>  rj < lo - c as signed (lo - c = MR - W once the window is full,
            // else -c: nothing is below the block start)
            const int32_t lo_rel = c + MR > W ? (int32_t)MR - (int32_t)W : -(int32_t)c;
            uint32_t vb[B], sv[B];
#pragma unroll
            for (uint32_t j = 0; j < B; j++) {
                sv[j] = rj[j] + c;
                vb[j] = L.win[sv[j] & (W - 1)];
            }
            int32_t mn = (int32_t)rj[0];
#pragma unroll
            for (uint32_t j = 1; j < B; j++) mn = min(mn, (int32_t)rj[j]);
            const bool far = mn < lo_rel;
            const uint32_t lo = c + lo_rel;
            PROF_COUNT(6, __ballot(far) ? 1 : 0);  // chunks with a byte older than the window
            uint32_t w[B / 4];
            if (__ballot(far)) {
#pragma unroll
                for (uint32_t j = 0; j < B; j++)
                    if (sv[j] < lo) vb[j] = dst[sv[j]];
            }
#pragma unroll
            for (uint32_t h = 0; h < B / 4; h++)
                w[h] = vb[4 * h] | (vb[4 * h + 1] << 8) | (vb[4 * h + 2] << 16) | (vb[4 * h + 3] << 24);
            *(uint32_t *)(L.win + (p0 & (W - 1))) = w[0];
#pragma unroll
            for (uint32_t h = 0; h < B; h += 4) *(uint4 *)(mkl + h) = make_uint4(0, 0, 0, 0);  // slots of c + MR ..
            PROF_MARK(3);
            if (c + CH <= dsize) {
                *(uint32_t *)(dst + p0) = w[0];
            } else {
                for (uint32_t j = 0; j < B && p0 + j < dsize; j++) dst[p0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            }
            c += CH;
            PROF_MARK(4);
        }
        return c >= dsize;
    };

    for (;;) {
        if (bt >= nb) { err = true; break; }  // stream ended before dsize (check C5)
        batch(posmA, tokA, grB, posmB, tokB, grA);
        PROF_MARK(0);
        if (err || chunks()) break;
        if (bt >= nb) { err = true; break; }
        batch(posmB, tokB, grA, posmA, tokA, grB);
        PROF_MARK(0);
        if (err || chunks()) break;
    }
    vm_sync();
    PROF_FLUSH(1);
    if (lane == 0) {
        *status_i = err ? QLZX_E_CORRUPT : QLZX_OK;
        if (dsize_i) *dsize_i = err ? 0u : dsize;
    }
}

template <bool CRC, uint32_t WIN = kV4W>
__global__ void __launch_bounds__(64) k_dec_chunk4(qlzx_blocks b, uint32_t *dsize_out, int32_t *status,
                                                   uint32_t first, uint32_t count, const BlkInfo *info,
                                                   const GroupRec *recs, uint32_t gmax, const uint32_t *list,
                                                   const uint32_t *crc_state, const uint32_t *crc_expect,
                                                   uint32_t *crc_out) {
    __shared__ __attribute__((aligned(16))) K2v4Lds<WIN> L;
    const uint32_t bx = blockIdx.x;
    if (bx >= count) return;
    const uint32_t i = list ? list[bx] : first + bx;
    if constexpr (CRC) {
        static_assert(sizeof(K2v4Lds<WIN>) >= 4096, "the slicing-by-4 CRC tables fill 4 KiB of the window");
        const uint32_t lane = threadIdx.x;
        uint32_t *tab = (uint32_t *)&L;
        for (uint32_t e = lane * 4; e < 1024; e += 256) *(uint4 *)(tab + e) = *(const uint4 *)(g_crc_slice8 + e);
        __syncthreads();
        const uint32_t c = ~wave_crc_rep<4, 1>(tab, g_crc_mul, b.src + b.src_off[i], b.src_len[i],
                                                crc_state ? crc_state[i] : 0xffffffffu, lane);
        __syncthreads();
        if (lane == 0 && crc_out) crc_out[i] = c;
        if (crc_expect && c != crc_expect[i]) {
            if (lane == 0) {
                status[i] = QLZX_E_CRC;
                if (dsize_out) dsize_out[i] = 0;
            }
            return;
        }
    }
    const BlkInfo bi = info[bx];
    if (bi.kind == kBlkSkip) return;
    dec_v4_block(L, b.src + b.src_off[i], b.dst + b.dst_off[i], b.src_len[i], bi, recs + (size_t)bx * gmax,
                 status + i, dsize_out ? dsize_out + i : nullptr, threadIdx.x);
}

}  // namespace qlzx

