// qlzx_decode_batch.h -- what the files of the fast batched level-3 decoder share (blocks with
// dsize <= QLZX_FAST_MAX_DSIZE, the 4-64 KiB values of the BASELINE configs): the types and
// constants, the workspace layout of a call, the header checks, K1's ring layout and the token
// and DPP helpers.  No kernel and no host runtime.
//
// Kernels per chunk of blocks: K1 k_dec_parse6 (qlzx_decode_k1.h; one LANE per
// block: the serial control-word chain of quicklz.c:513-671, one 16-B GroupRec per control word)
// and K2 k_dec_chunk4 (qlzx_decode_k2.h; one WAVE per block: items 64 at a time, output 256 bytes
// at a time, every byte gathered from the position it copies; the record CRC is verified first
// when asked for, store/datafile.go:161-168).  The block order and the launcher are in
// qlzx_decode_batch.hip; the single-call decoders (qlzx_decode_solo.h, qlzx_decode_small.h)
// use the same records and helpers.
#pragma once
#include "qlzx_device.h"

#ifndef QLZX_FAST_MAX_DSIZE
#define QLZX_FAST_MAX_DSIZE 65536
#endif

namespace qlzx {

struct BlkInfo {
    uint32_t ngroups;
    uint32_t nitems;
    uint32_t kind;  // 0 skip (error / general path), 1 stored, 2 compressed
    uint32_t dsize;
};
struct GroupRec {
    uint32_t ip, m, a, b;
};

constexpr int32_t kPending = -1;  // status of blocks left to the general path
constexpr uint32_t kBlkSkip = 0, kBlkStored = 1, kBlkCompressed = 2;
// K1 workgroup: one wave (the 8 KiB LDS ring per wave bounds occupancy)
constexpr uint32_t kParseWG = 64;
#ifndef QLZX_CHUNK_BLOCKS  // blocks per K1/K2 chunk for batches of values up to 16 KiB
#define QLZX_CHUNK_BLOCKS 262144
#endif
#ifndef QLZX_CHUNK_BLOCKS_MIXED  // ... and for batches whose max_dsize exceeds 16 KiB
#define QLZX_CHUNK_BLOCKS_MIXED 131072
#endif
// Chunk size by the call's max_dsize (>= 256 CUs x 8 waves x 64 lanes: K1 fills the chip).  Same-box
// A/B (profiles/r04_c2_chunk_ab.txt, r04_chunk_c5_ab.txt): c2 (1 M x 16 KiB) 27.0 ms at 262144
// vs 27.35 at 131072; c5 (mixed 4-64 KiB, 64 GiB) 549 GiB/s at 262144 vs 621 at 131072.
__host__ __device__ inline uint32_t chunk_blocks(uint32_t max_dsize) {
    return max_dsize <= 16384 ? (uint32_t)QLZX_CHUNK_BLOCKS : (uint32_t)QLZX_CHUNK_BLOCKS_MIXED;
}
constexpr uint32_t kRoundBytes = 32;  // bytes of a lane's stream per ring slot (16-B pieces)
constexpr uint32_t kPieces = kRoundBytes / 16;
// K1's LDS ring: kRingSlots rounds of kRoundBytes per lane (8 KiB per wave).  An 8-round ring
// for chunks of few waves gained 0.16 ms on c4's 4.4 ms chunk of long streams (their lanes are
// bound by the serial step chain, not by the load latency) and was dropped in round 5.
#ifndef QLZX_K1_SLOTS
#define QLZX_K1_SLOTS 4
#endif
constexpr uint32_t kRingSlots = QLZX_K1_SLOTS;
template <uint32_t S>
constexpr uint32_t kRingWaveS = S * kRoundBytes * 64;
__host__ __device__ inline uint32_t groups_max(uint32_t max_dsize) { return max_dsize / 31u + 2u; }

// Workspace of a call.  A region holds one chunk's BlkInfo and GroupRec arrays; region 0 also
// holds the block order of the whole call (list) and its counters (aux), and every region is
// `one` bytes so a caller's single region is a valid call.  Regions (what
// qlzx_decompress_workspace_size asks for): 1 for a single chunk, 2 so K1 of chunk c+1 runs
// beside K2 of chunk c, and for calls of mixed sizes over three chunks or more a third for the
// last chunk (the longest values, whose one-lane-per-block K1 is the longest): its K1 starts with
// the first one.  One early chunk: c5 rounds of 15.4 GiB 616.8 GiB/s (two runs) against 610.0
// with two and 606.3 with none; two early K1s hold enough LDS (8 KiB per K1 wave) to slow the
// first K2s 4x (profiles/r06_mixed_ab.txt).
struct BatchLayout {
    uint32_t md, gmax;           // max_dsize clamped to the fast path, GroupRecs per block
    uint32_t chunk, nchunks;     // blocks per chunk (the last may hold fewer), chunks of the call
    size_t o_rec, o_list, o_aux; // offsets in a region: GroupRecs; block order and its aux (region 0)
    size_t one;                  // bytes of a region
    uint32_t regions;
};
inline BatchLayout batch_layout(uint32_t n, uint32_t max_dsize) {
    auto a256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    BatchLayout L;
    L.md = max_dsize > QLZX_FAST_MAX_DSIZE ? QLZX_FAST_MAX_DSIZE : max_dsize;
    L.gmax = groups_max(L.md);
    const uint32_t cb = chunk_blocks(max_dsize);
    L.chunk = n < cb ? (n ? n : 1) : cb;
    L.nchunks = n <= cb ? 1u : 1u + (n - 1) / cb;
    L.o_rec = a256((size_t)L.chunk * sizeof(BlkInfo));
    L.o_list = L.o_rec + a256((size_t)L.chunk * L.gmax * sizeof(GroupRec));
    L.o_aux = L.o_list + a256((size_t)n * sizeof(uint32_t));  // block order, whole call
    L.one = L.o_aux + 1024 + 256;                              // order aux
    L.regions = L.nchunks == 1 ? 1u : max_dsize > 16384 && L.nchunks >= 3 ? 3u : 2u;
    return L;
}

// Header checks of one block of `len` bytes (quicklz.c:780-811 and the batch API's bounds):
// the status, and for QLZX_OK its kind (kBlkStored / kBlkCompressed), sizes and header length.
__device__ __forceinline__ int classify_block(const uint8_t *src, uint32_t len, uint32_t cap, uint32_t max_dsize,
                                              uint32_t &kind, uint32_t &csize, uint32_t &dsize, uint32_t &hdr) {
    kind = kBlkSkip;
    if (len < 3) return QLZX_E_HEADER;
    hdr = (src[0] & 2u) ? 9u : 3u;
    if (len < hdr) return QLZX_E_HEADER;
    const Header h = parse_header(src);
    csize = h.csize;
    dsize = h.dsize;
    if (h.csize != len) return QLZX_E_SIZE_COMPRESSED;
    if (h.level != 3) return QLZX_E_LEVEL;
    if (h.dsize > cap) return QLZX_E_DST_CAP;
    if (h.dsize > max_dsize) return QLZX_E_MAX_DSIZE;     // the caller's bound is wrong
    if (h.dsize > QLZX_FAST_MAX_DSIZE) return kPending;  // general path owns it
    if (!h.compressed) {
        if (csize < hdr + dsize) return QLZX_E_CORRUPT;
        kind = kBlkStored;
    } else {
        kind = kBlkCompressed;
    }
    return QLZX_OK;
}

// Ring layout per wave: [slot][piece][lane][16 B]; stream byte p of a lane (q = p + shift,
// shift = src & 15) lives in round q / kRoundBytes, slot round % S, piece (q / 16) % kPieces,
// byte q % 16 -- i.e. at ((q / 16) % (kPieces S)) * 1 KiB + lane * 16 + q % 16.
template <uint32_t S>
__device__ __forceinline__ uint32_t ring_off(uint32_t q, uint32_t lane) {
    return (((q >> 4) & (kPieces * S - 1)) << 10) | (lane << 4) | (q & 15u);
}
template <uint32_t S>
__device__ __forceinline__ uint32_t ring_rd32(const uint8_t *ring, uint32_t q, uint32_t lane) {
    const uint32_t qa = q & ~3u;
    const uint32_t lo = *(const uint32_t *)(ring + ring_off<S>(qa, lane));
    const uint32_t hi = *(const uint32_t *)(ring + ring_off<S>(qa + 4, lane));
    return __builtin_amdgcn_alignbyte(hi, lo, q & 3u);
}

// ------------------------------------------------------------------- K2 helpers ----
// Per-lane coordinates of item I = 64 bt + lane: group g = I / 31, index k = I % 31.
// Advanced by one batch (64 = 2 * 31 + 2) without a division.
struct ItemCursor {
    uint32_t g, k;
    __device__ __forceinline__ void next() {
        k += 2;
        const bool wrap = k >= 31;
        k = wrap ? k - 31 : k;
        g += wrap ? 3 : 2;
    }
};

// Branch-free level-3 token decode (quicklz.c:579-610).  Token type
// ty = (t & 3) + ((t & 127) == 3) selects per-type bit fields from packed tables:
//   ty 0: 1 B, off = t[2:8),  len 3          ty 1: 2 B, off = t[2:16), len 3
//   ty 2: 2 B, off = t[6:16), len = t[2:6)+3  ty 3: 3 B, off = t[7:24), len = t[2:7)+2
//   ty 4: 4 B, off = t[15:32), len = t[7:15)+3
__device__ __forceinline__ void decode_tok_bf(uint32_t t, uint32_t &off, uint32_t &len, uint32_t &tl) {
    const uint32_t ty = (t & 3u) + ((t & 127u) == 3u ? 1u : 0u);
    const uint32_t f4 = ty * 4, f6 = ty * 6;
    const uint32_t osh = __builtin_amdgcn_ubfe(0xF7622u, f4, 4);
    const uint32_t ow = __builtin_amdgcn_ubfe((6u) | (14u << 6) | (10u << 12) | (17u << 18) | (17u << 24), f6, 6);
    const uint32_t lsh = __builtin_amdgcn_ubfe(0x72200u, f4, 4);
    const uint32_t lw = __builtin_amdgcn_ubfe(0x85400u, f4, 4);
    const uint32_t la = __builtin_amdgcn_ubfe(0x32333u, f4, 4);
    tl = __builtin_amdgcn_ubfe(0x43221u, f4, 4);
    off = __builtin_amdgcn_ubfe(t, osh, ow);
    len = __builtin_amdgcn_ubfe(t, lsh, lw) + la;
}

// Inclusive prefix sum over the 64 lanes with DPP (row shifts + row broadcasts).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

// Lane masks: the lanes where a < b (unsigned) or a != b, as the compare itself leaves them in an
// SGPR pair, and the lane's own bit of a wave-uniform mask as a bool (no instruction).
constexpr int kIcmpNe = 33, kIcmpUlt = 36;  // LLVM's integer compare predicates
__device__ __forceinline__ uint64_t cmp_lt(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, kIcmpUlt); }
__device__ __forceinline__ uint64_t cmp_ne(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, kIcmpNe); }
__device__ __forceinline__ bool in_mask(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

__device__ __forceinline__ uint32_t ff1_or(uint64_t m, uint32_t dflt) {
    return m ? (uint32_t)__builtin_ctzll(m) : dflt;
}

// Inclusive max over lanes 0..lane; DPP row shifts + row broadcasts.
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}
// Value of lane - 1 (0 in lane 0): DPP wave_shr:1.
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);
}

}  // namespace qlzx
