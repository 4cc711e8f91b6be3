// qlzx_recfile.h -- what the record-file kernels share (qlzx_replay.hip, qlzx_read.hip,
// qlzx_write.hip, qlzx_gc.hip, and through qlzx_hint_fmt.h the hint sources): the format's constants, readRecordAt's checks
// (store/datafile.go:114-170), the workspace carver, the wave sum, the stream compaction (three
// scan kernels behind launch_compact), the u64 offset scan k_rp_dstoff, and the long-record
// machinery: the list of records whose CRC span exceeds kRpLong, the segment accumulator, and
// the segmented write kernel k_rec_long.
#pragma once

#include <algorithm>

#include "qlzx_crc.h"
#include "qlzx_device.h"

namespace qlzx {

constexpr uint32_t kRpSlot = 256;  // records start on 256-B boundaries and are padded to them
constexpr uint32_t kRpHdr = 24;    // crc ‖ ts ‖ flag ‖ ver ‖ ksz ‖ vsz
// A wave takes ~3 us per 4 KiB stripe, so a record whose CRC span exceeds kRpLong (a false replay
// candidate can claim up to BodyMax) would be one wave's serial tail for the whole launch: those
// are listed (LongList) and cut into kRpSeg segments spread over every wave of the chip.
constexpr uint32_t kRpLong = 128u << 10;
constexpr uint32_t kRpSeg = 16u << 10;
constexpr uint32_t kScanTile = 1024;  // elements per scan tile (256 threads x 4)
constexpr uint32_t kFlagCompress = 0x00010000u;
constexpr uint32_t kBodyMax = 50u << 20;

__host__ __device__ __forceinline__ uint64_t pad256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline size_t rp_align(size_t x) { return (size_t)pad256(x); }

// the records a replay returned, never more than the arrays hold
__device__ __forceinline__ uint32_t rec_count(const uint32_t *result, uint32_t cap) {
    const uint32_t n = result[0];
    return n < cap ? n : cap;
}

// workgroups for n items at `per` items each, at most `most` (the kernels stride over the rest)
inline uint32_t grid_for(uint64_t n, uint32_t per = 256, uint32_t most = 4096) {
    return (uint32_t)std::min<uint64_t>((n + per - 1) / per, most);
}

// Carves 256-B-aligned arrays off a workspace; with base == nullptr it only sizes it (bytes()).
struct WsCarver {
    uint8_t *base;
    size_t o = 0;
    template <class T = uint8_t>
    T *take(size_t bytes) {
        T *p = base ? (T *)(base + o) : nullptr;
        o += rp_align(bytes);
        return p;
    }
    size_t bytes() const { return o; }
};

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- Getvhash (store/item.go:89-100) with the sign-extending Fnv1a (utils/hash.go:8-16) ----
__device__ __forceinline__ uint32_t fnv1a_bytes(const uint8_t *p, uint32_t n, uint32_t h) {
    for (uint32_t i = 0; i < n; i++) {
        h ^= (uint32_t)(int32_t)(int8_t)p[i];
        h *= 0x01000193u;
    }
    return h;
}
__device__ __forceinline__ uint16_t getvhash(const uint8_t *v, uint32_t l) {
    uint32_t h = l * 97u;
    if (l <= 1024) {
        h += fnv1a_bytes(v, l, 0x811c9dc5u);
    } else {  // the first and the last 512 bytes
        h += fnv1a_bytes(v, 512, 0x811c9dc5u);
        h *= 97u;
        h += fnv1a_bytes(v + l - 512, 512, 0x811c9dc5u);
    }
    return (uint16_t)h;
}

// ---- readRecordAt's checks (store/datafile.go:123-149), in the reference's order ----
// (the values are qlzx_read_plan's status codes; the other kernels map them to their own)
enum RecVerdict : int32_t {
    kRecOk = QLZX_RD_OK, kRecAlign = QLZX_RD_ALIGN, kRecEofHeader = QLZX_RD_EOF_HEADER, kRecKeySize = QLZX_RD_KEY_SIZE,
    kRecValueSize = QLZX_RD_VALUE_SIZE, kRecEofBody = QLZX_RD_EOF_BODY
};
// a record position: in units of 256 (store/leaf.go:56-65), with a whole header before the end
__device__ __forceinline__ RecVerdict rec_pos_verdict(uint64_t off, uint64_t size) {
    if (off % kRpSlot != 0) return kRecAlign;
    if (off > size || size - off < kRpHdr) return kRecEofHeader;
    return kRecOk;
}
// a header's sizes; after = the file's bytes behind the header
__device__ __forceinline__ RecVerdict rec_size_verdict(uint32_t ksz, uint32_t vsz, uint64_t after, uint32_t max_key,
                                                       uint64_t body_max) {
    if (ksz == 0 || ksz > max_key) return kRecKeySize;  // config/mc_config.go:33-35
    if ((uint64_t)vsz > body_max) return kRecValueSize;
    if (after < (uint64_t)ksz + vsz) return kRecEofBody;
    return kRecOk;
}

// ---- stream compaction: exclusive scan of per-element 0/1 flags over [0, n), three kernels ----
template <class F>
__global__ void __launch_bounds__(256) k_scan_tiles(F f, uint32_t n, uint32_t *tile_sum) {
    __shared__ uint32_t part[4];
    const uint32_t base = blockIdx.x * kScanTile;
    uint32_t c = 0;
    for (uint32_t j = threadIdx.x; j < kScanTile; j += 256)
        if (base + j < n) c += f(base + j);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// single workgroup: exclusive scan of tile sums in place; *total = sum
__global__ void __launch_bounds__(1024) k_scan_top(uint32_t *tile_sum, uint32_t ntiles, uint32_t *total) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t base = 0; base < ntiles; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < ntiles ? tile_sum[i] : 0u;
        uint32_t x = v;  // inclusive wave scan
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (int j = 0; j < 16; j++) { const uint32_t t = wsum[j]; wsum[j] = acc; acc += t; }
        }
        __syncthreads();
        const uint32_t excl = carry + wsum[w] + x - v;
        if (i < ntiles) tile_sum[i] = excl;
        __syncthreads();
        if (threadIdx.x == 1023) carry = excl + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// per tile: local exclusive ranks + the tile's offset; g(i, idx, flag) scatters
template <class F, class G>
__global__ void __launch_bounds__(256) k_scan_apply(F f, G g, uint32_t n, const uint32_t *tile_sum) {
    __shared__ uint32_t wsum[4];
    const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
    uint32_t v[4], c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = (base + j < n) ? f(base + j) : 0u;
        c += v[j];
    }
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = c;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t woff = 0;
    for (uint32_t j = 0; j < w; j++) woff += wsum[j];
    uint32_t idx = tile_sum[blockIdx.x] + woff + x - c;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (base + j < n) g(base + j, idx, v[j]);
        idx += v[j];
    }
}

// g(i, rank of i among the flagged, f(i)) for every i < n, *total = the flagged; tiles holds a
// word per tile of n.  An empty range still takes one (empty) tile: no grid is empty.
template <class F, class G>
inline void launch_compact(F f, G g, uint32_t n, uint32_t *tiles, uint32_t *total, hipStream_t s) {
    const uint32_t ntiles = std::max<uint32_t>((n + kScanTile - 1) / kScanTile, 1);
    hipLaunchKernelGGL(k_scan_tiles<F>, dim3(ntiles), dim3(256), 0, s, f, n, tiles);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, tiles, ntiles, total);
    hipLaunchKernelGGL((k_scan_apply<F, G>), dim3(ntiles), dim3(256), 0, s, f, g, n, (const uint32_t *)tiles);
}

// Destination offsets: exclusive scan of the 256-B-rounded sizes (u64) by one workgroup, and
// totals = {result[0], count, max size, bytes lo, bytes hi}.  Wave w owns the contiguous range
// [w P, (w + 1) P) and walks it twice, 64 coalesced sizes per step with the next step's load in
// flight: first its sum, then (after one scan of the 16 sums) the offsets by a wave scan with a
// carry -- no workgroup barrier per step (round 4 synchronised the workgroup four times per 1024
// sizes: 265 us for 224 K records).
__global__ void __launch_bounds__(1024) k_rp_dstoff(const uint32_t *comp_dsize, const uint32_t *ncomp_p,
                                                     uint64_t *dst_off, uint32_t *totals, const uint32_t *result) {
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t mx[16];
    const uint32_t nc = *ncomp_p, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t per = ((nc + 15) / 16 + 63) & ~63u;
    const uint32_t lo = w * per < nc ? w * per : nc, hi = lo + per < nc ? lo + per : nc;
    uint64_t sum = 0;
    uint32_t mymax = 0;
    uint32_t nxt = lo + lane < hi ? comp_dsize[lo + lane] : 0u;
    for (uint32_t i = lo; i < hi; i += 64) {
        const uint32_t d = nxt;
        nxt = i + 64 + lane < hi ? comp_dsize[i + 64 + lane] : 0u;
        sum += pad256(d);
        mymax = max(mymax, d);
    }
    for (int k = 32; k >= 1; k >>= 1) {
        sum += __shfl_xor(sum, k, 64);
        mymax = max(mymax, (uint32_t)__shfl_xor(mymax, k, 64));
    }
    if (lane == 0) wsum[w] = sum, mx[w] = mymax;
    __syncthreads();
    uint64_t carry = 0, total = 0;
    for (uint32_t j = 0; j < 16; j++) {
        carry += j < w ? wsum[j] : 0;
        total += wsum[j];
    }
    nxt = lo + lane < hi ? comp_dsize[lo + lane] : 0u;
    for (uint32_t i = lo; i < hi; i += 64) {
        const uint64_t v = i + lane < hi ? pad256(nxt) : 0;
        nxt = i + 64 + lane < hi ? comp_dsize[i + 64 + lane] : 0u;
        uint64_t x = v;  // inclusive wave scan
        for (int k = 1; k < 64; k <<= 1) {
            const uint64_t y = __shfl_up(x, k, 64);
            if (lane >= (uint32_t)k) x += y;
        }
        if (i + lane < hi) dst_off[i + lane] = carry + x - v;
        carry += __shfl(x, 63, 64);
    }
    if (threadIdx.x == 0) {
        uint32_t m = 0;
        for (int j = 0; j < 16; j++) m = max(m, mx[j]);
        totals[0] = result[0];
        totals[1] = nc;
        totals[2] = m;
        totals[3] = (uint32_t)total;
        totals[4] = (uint32_t)(total >> 32);
    }
}

// ---- long records ----
// The list a checking / assembling kernel fills (push, one lane) and a segment kernel works off:
// entry e names record idx[e]; a segment's raw CRC, shifted over the bytes after it, is XORed into
// acc[e], and done[e] counts the segments.
struct LongList {
    uint32_t *n, *idx, *acc, *done;
    __device__ __forceinline__ void push(uint32_t i) const {
        const uint32_t j = atomicAdd(n, 1u);
        idx[j] = i;
        acc[j] = 0;
        done[j] = 0;
    }
    // One lane adds a segment's shifted register to entry e.  True in the wave that completed the
    // record's last segment (of nseg): *sum is then the record's whole register.  Callers
    // initialise sum: a value undefined on the other path costs the segment kernels a VGPR.
    __device__ __forceinline__ bool add(uint32_t e, uint32_t reg, uint32_t nseg, uint32_t *sum) const {
        atomicXor(&acc[e], reg);
        __threadfence();
        if (atomicAdd(&done[e], 1u) == nseg - 1) {
            __threadfence();
            *sum = atomicOr(&acc[e], 0u);
            return true;
        }
        return false;
    }
};

// The segmented write of the listed records: every wave walks the (normally empty or tiny) list
// and takes the segments g of the global segment sequence with g = wave id (mod all waves).
// Segment r of a record is its image [r kRpSeg, (r + 1) kRpSeg); the last one runs to the
// record's last 16-B boundary and also writes the tail and the padding.  The wave that completes
// the last segment finishes the record (the CRC word).  The policy P describes a record:
//   Rec rec(i)            what the kernel needs of record i, loaded once per wave
//   bool valid(R)         false: skipped (the listing kernel saw the same answer)
//   uint32_t end(R)       the image's end, 24 + ksz + vsz
//   uint32_t segment(lds, R, r0, r1, last, lane)   writes [r0, r1) (and, when last, the tail and
//                         the padding) and returns the raw CRC register over those bytes
//   void finish(i, R, sum)   one lane; sum = the register over the whole image
template <class P>
__global__ void __launch_bounds__(256) k_rec_long(P pol, LongList ll) {
    __shared__ uint32_t tab[kCrcLdsWords];
    const uint32_t nl = *ll.n;
    if (nl == 0) return;
    load_crc_lds(tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = blockIdx.x * 4 + threadIdx.x / 64, nw = gridDim.x * 4;
    uint64_t g = 0;
    for (uint32_t e = 0; e < nl; e++) {
        const uint32_t i = ll.idx[e];
        const typename P::Rec R = pol.rec(i);
        if (!pol.valid(R)) continue;
        const uint32_t end = pol.end(R), e16 = end & ~15u;
        const uint32_t nseg = (e16 + kRpSeg - 1) / kRpSeg;
        for (uint32_t r = (uint32_t)((wid + nw - g % nw) % nw); r < nseg; r += nw) {
            const uint32_t r0 = r * kRpSeg;
            const bool last = r == nseg - 1;
            const uint32_t r1 = last ? e16 : r0 + kRpSeg;
            uint32_t reg = pol.segment(tab, R, r0, r1, last, lane);
            if (!last) reg = crc_shift(reg, end - r1);
            uint32_t sum = 0;
            if (lane == 0 && ll.add(e, reg, nseg, &sum)) pol.finish(i, R, sum);
        }
        g += nseg;
    }
}

}  // namespace qlzx
