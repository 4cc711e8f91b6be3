// qlzx_encode_fmt.h -- the level-3 format rules of the compress side, once for the three encoders
// (qlzx_encode_lane.hip, qlzx_encode_wg.hip, qlzx_encode_huge.hip), as decode_token and
// parse_header in qlzx_device.h are for the decoders.  A header of its own rather than more of
// qlzx_device.h: that one is compiled into every kernel source, the decode-only unit of
// qlzx_k2.hip included, and nothing outside the encoders needs these.
//
// How an encoder loads the bytes it hashes and compares (ld24, ld32u, he_ld32) is its own access
// strategy and stays with it.
#pragma once
#include "qlzx_device.h"

namespace qlzx {

// hash_func (quicklz.c:70) of a 3-byte fetch: the bucket of a position.
__host__ __device__ __forceinline__ uint32_t hash12(uint32_t f) { return ((f >> 12) ^ f) & (QLZX_BUCKETS - 1); }

// Positions the main loop searches and inserts: ip <= n - 1 - QLZX_TAIL (quicklz.c:204,213); the
// rest are tail literals.
__host__ __device__ inline uint32_t searched_positions(uint32_t n) { return n > QLZX_TAIL ? n - QLZX_TAIL : 0u; }

// Level-3 match token (quicklz.c:377-406) of a match of `ml` bytes `off` back: its value in t,
// returns its byte count.
__host__ __device__ __forceinline__ uint32_t match_token(uint32_t ml, uint32_t off, uint32_t &t) {
    if (ml == 3 && off <= 63) { t = off << 2; return 1; }
    if (ml == 3 && off <= 16383) { t = (off << 2) | 1u; return 2; }
    if (ml <= 18 && off <= 1023) { t = ((ml - 3) << 2) | (off << 6) | 2u; return 2; }
    if (ml <= 33) { t = ((ml - 2) << 2) | (off << 7) | 3u; return 3; }
    t = ((ml - 3) << 7) | (off << 15) | 3u;
    return 4;
}
// The nb low bytes of token t at o (one address, immediate offsets).
__device__ __forceinline__ void put_token(uint8_t *o, uint32_t t, uint32_t nb) {
    o[0] = (uint8_t)t;
    if (nb > 1) o[1] = (uint8_t)(t >> 8);
    if (nb > 2) o[2] = (uint8_t)(t >> 16);
    if (nb > 3) o[3] = (uint8_t)(t >> 24);
}

// Bail-out test (quicklz.c:218), made when the main loop starts a new control word with the input
// at ip and the output (core bytes, the new control word not counted) at op: past bail_from(n)
// input bytes, an output that is not 1/32 smaller than the input ends the parse and the value is
// stored.  bias = 9 is Go's rule, which counts the header (quicklz.go:119); the reference's is 0.
__host__ __device__ __forceinline__ uint32_t bail_from(uint32_t n) { return 3u * (n >> 2); }
template <typename U>  // uint32_t, or uint64_t where n may approach 2^32 (the whole-GPU encoder)
__host__ __device__ __forceinline__ bool bail_out(U ip, U op, uint32_t n, uint32_t bias) {
    return ip > bail_from(n) && op + bias > ip - (ip >> 5);
}

__device__ __forceinline__ void st32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// Header (quicklz.c:757-772): flags 01SSLLHC with level 3, then csize and dsize as bytes (hdr = 3,
// values under 216 bytes: quicklz.c:708-711) or as 32-bit words (hdr = 9).
__device__ __forceinline__ void write_header(uint8_t *dst, uint32_t hdr, bool compressed, uint32_t csize,
                                             uint32_t dsize) {
    if (hdr == 3) {
        dst[0] = (uint8_t)((compressed ? 1 : 0) | 0x4C);
        dst[1] = (uint8_t)csize;
        dst[2] = (uint8_t)dsize;
    } else {
        dst[0] = (uint8_t)(2 | (compressed ? 1 : 0) | 0x4C);
        st32(dst + 1, csize);
        st32(dst + 5, dsize);
    }
}

}  // namespace qlzx
