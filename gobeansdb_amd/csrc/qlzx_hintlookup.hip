// qlzx_hintlookup.hip -- key lookups through a bucket's hint files: what
// hintMgr.getItem (store/hint.go:570-596) -> hintChunk.get (:270-296) -> hintFileIndex.get
// (store/hintindex.go:28-69) answer, for files resident in device memory.  The caller lists the
// files in the order getItem reaches them; a request walks that list until a file hits, fails
// (QLZX_HL_ERR / QLZX_HL_BAD_FILE end the search, as an error ends getItem) or is the merged one.
//
// One file, hintFileIndex.get:
//   start  Go's sort.Search over the file's 16-byte index entries (its exact loop: defined on any
//          bytes), and the scan starts at entry j - 1's offset only when j > 1, else at 16.
//   walk   hintFileReader.next from there.  The reader's own offset starts at 16 whatever the
//          Seek, so the reference stops after indexOffset - 16 bytes consumed: at file position
//          stop = indexOffset + (start - 16), inside the index section when start > 16.  An item
//          head or key that runs past the file is the error, decided before the item is compared.
//          QLZX_HL_F_BOUNDED stops at indexOffset.
//
// The format with its loads, the reader's rule (hint_next) and k_keyhash are qlzx_hint_fmt.h's;
// this file owns the head check, hl_start, hl_step, the LDS window and the two kernel shapes.
//
// Launches: k_keyhash into the workspace unless the caller brings
// hashes; k_hl_head, one lane per file: the head's checks, once; then one of two shapes of the
// same search, hl_start and the item loop being the same code over a different byte source:
//   k_hl_wave  a wave per request, below QLZX_HL_LANE_FROM requests.  The stretch is staged in LDS
//              in kHlWin-byte windows (16-B loads where a whole aligned 16 bytes lie inside the
//              file, byte loads at its edges) and walked there by all lanes alike; a window is
//              restaged whenever the next item could reach past it, so no file size or stretch
//              length is assumed.  A candidate's key bytes are compared 64 at a time.
//   k_hl_lane  a lane per request, from QLZX_HL_LANE_FROM requests on: every step of the walk is
//              a dependent global load, 64 independent walks per wave.
// A request's search is one serial chain either way (8 files: ~0.6 ms by lane, ~0.2 ms by wave),
// and the chip holds 8,192 waves but 524,288 lanes: the wave shape is 2-3 times faster while its
// requests fit the chip at once, the lane shape 4-5 times faster at 262,144 requests
// (profiles/r14_hint_lookup.json).
#include "qlzx_hint_fmt.h"

namespace qlzx {

constexpr uint32_t kHlWin = 4096;                          // bytes of one LDS window (a multiple of 16)
constexpr uint32_t kHlHold = kHlWin - 16;                  // of which file bytes: byte 22 behind any of them is in the slice
constexpr uint32_t kHlItemMax = kHintItem + kHintMaxKey;   // the longest item

struct HlIn {
    const uint8_t *hints;
    uint64_t bytes;
    const uint64_t *file_off, *file_len;
    const uint32_t *file_chunk, *file_flags;
    uint32_t n_files;
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint64_t *keyhash;
    uint32_t n, bounded;
};
struct HlOut {
    int32_t *status;
    uint32_t *hit_file, *chunk, *offset;
    int32_t *ver;
    uint16_t *vhash;
    uint64_t *item_src;
    uint32_t *totals;
};
struct HlFile {  // a file after k_hl_head: io = indexOffset, ne = its index entries
    uint64_t off, len, io, ne;
    uint32_t chunk, merged, bad, pad;
};
struct HlHit {
    int32_t status;
    uint32_t file;
    uint64_t at;  // the item's offset in its file
};

// What loadHintIndex (store/hintindex.go:71-119) needs of a file to give get an index at all.
__global__ void __launch_bounds__(256) k_hl_head(HlIn in, HlFile *files) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < in.n_files; i += gridDim.x * 256) {
        HlFile s{in.file_off[i], in.file_len[i], 0, 0, in.file_chunk[i], in.file_flags[i] & QLZX_HL_FILE_MERGED, 0, 0};
        s.bad = s.len < kHintHead || s.off > in.bytes || in.bytes - s.off < s.len;
        if (!s.bad) {
            s.io = hint_ld64(in.hints + s.off);
            if (s.io < kHintHead || s.io > s.len || (s.len - s.io) % kHintEntry != 0) s.bad = 1;
            else s.ne = (s.len - s.io) / kHintEntry;
        }
        files[i] = s;
    }
}

// sort.Search(len(arr), arr[i].keyhash >= kh) and get's `if j > 1`: where the scan starts and
// where it stops.  False: entry j - 1 names no offset inside [16, len].
__device__ __forceinline__ bool hl_start(const uint8_t *f, const HlFile &s, uint64_t kh, bool bounded, uint64_t *start,
                                         uint64_t *stop) {
    uint64_t i = 0, j = s.ne;
    while (i < j) {
        const uint64_t h = (i + j) >> 1;
        if (!(hint_ld64(f + s.io + kHintEntry * h) >= kh)) i = h + 1;
        else j = h;
    }
    *start = kHintHead;
    if (i > 1) {
        *start = hint_ld64(f + s.io + kHintEntry * (i - 1) + kEntryOffset);
        if (*start < kHintHead || *start > s.len) return false;
    }
    *stop = bounded ? s.io : s.io + (*start - kHintHead);
    return true;
}

// One step of get's loop over an item whose 23 head bytes (h = keyhash, ksz) are read: 0 = go on.
enum { kHlNext = 0, kHlMiss, kHlCandidate };
__device__ __forceinline__ int hl_step(uint64_t h, uint32_t ksz, uint64_t kh, uint32_t klen) {
    if (h > kh) return kHlMiss;
    return h == kh && ksz == klen ? kHlCandidate : kHlNext;
}

// ---- a lane per request ----
__device__ __forceinline__ int32_t hl_get_lane(const uint8_t *f, const HlFile &s, uint64_t kh, const uint8_t *key,
                                               uint32_t klen, bool bounded, uint64_t *at) {
    uint64_t p, stop;
    if (!hl_start(f, s, kh, bounded, &p, &stop)) return QLZX_HL_ERR;
    while (p < stop) {  // p <= len
        uint32_t ksz;
        if (!hint_next(s.len, p, [&](uint64_t q) { return f[q]; }, &ksz)) return QLZX_HL_ERR;
        const int t = hl_step(hint_ld64(f + p), ksz, kh, klen);
        if (t == kHlMiss) return QLZX_HL_MISS;
        if (t == kHlCandidate) {
            uint32_t d = 0;
            for (uint32_t b = 0; b < ksz; b++) d |= f[p + kHintItem + b] ^ key[b];
            if (!d) {
                *at = p;
                return QLZX_HL_FOUND;
            }
        }
        p += kHintItem + ksz;
    }
    return QLZX_HL_MISS;
}

// ---- a wave per request ----
// The window: file bytes [w0, w1) sit at LDS bytes sh + (q - w0), sh = the low four bits of the
// address of file byte w0, so that 16 aligned global bytes are 16 aligned LDS bytes.
struct HlWin {
    uint32_t *lds;  // kHlWin + 16 bytes, 16-B aligned
    uint64_t w0, w1;
    uint32_t sh;
    __device__ __forceinline__ uint32_t at(uint64_t q) const { return sh + (uint32_t)(q - w0); }
    __device__ __forceinline__ uint32_t byte(uint64_t q) const { return ((const uint8_t *)lds)[at(q)]; }
    __device__ __forceinline__ uint32_t ld32(uint64_t q) const {
        const uint32_t o = at(q);
        return __builtin_amdgcn_alignbyte(lds[(o >> 2) + 1], lds[o >> 2], o & 3u);
    }
    __device__ __forceinline__ uint64_t ld64(uint64_t q) const { return ld32(q) | ((uint64_t)ld32(q + 4) << 32); }
    // file bytes [p, min(len, end, p + kHlHold - sh)); the wave's earlier reads of the window are done
    __device__ __forceinline__ void stage(const uint8_t *f, uint64_t len, uint64_t p, uint64_t end, uint32_t lane) {
        sh = (uint32_t)((uintptr_t)(f + p) & 15u);
        w0 = p;
        w1 = len - p < kHlHold - sh ? len : p + (kHlHold - sh);
        if (end < w1) w1 = end;
        const uint32_t chunks = (sh + (uint32_t)(w1 - w0) + 15) / 16;
        for (uint32_t c = lane; c < chunks; c += 64) {
            // chunk c holds the file bytes q0 .. q0 + 15, q0 = p - sh + 16 c (below p for c = 0, sh > 0)
            uint4 v;
            if ((c > 0 || sh == 0) && w1 - w0 + sh >= 16ull * c + 16) {
                v = *(const uint4 *)(f + p + (16ull * c - sh));
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t b = 0; b < 16; b++) {
                    const uint32_t o = 16 * c + b;
                    if (o >= sh && o - sh < w1 - w0) w[b >> 2] |= (uint32_t)f[p + (o - sh)] << (8 * (b & 3));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4 *)(lds + 4 * c) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// All 64 lanes run the same walk; `key` is compared 64 bytes at a time.
__device__ __forceinline__ int32_t hl_get_wave(const uint8_t *f, const HlFile &s, uint64_t kh, const uint8_t *key,
                                               uint32_t klen, bool bounded, HlWin &w, uint32_t lane, uint64_t *at) {
    uint64_t p, stop;
    if (!hl_start(f, s, kh, bounded, &p, &stop)) return QLZX_HL_ERR;
    // an item that starts below stop ends below stop + kHlItemMax
    const uint64_t end = stop >= s.len || s.len - stop < kHlItemMax ? s.len : stop + kHlItemMax;
    w.w0 = w.w1 = 0;
    while (p < stop) {
        // the window holds the item whole, whatever its ksz, or reaches `end`
        if (w.w1 <= p || (w.w1 < end && w.w1 - p < kHlItemMax)) {
            __builtin_amdgcn_wave_barrier();
            w.stage(f, s.len, p, end, lane);
        }
        // The ksz byte is read before the rule asks for it: read between the rule's two checks it costs
        // the loop 70 instructions and 20-30 % (profiles/r15_hint_kernels_ab.txt).  Under a head that
        // the file cuts it is a byte of the slice past the window (kHlHold) and is not used.
        const uint32_t kb = w.byte(p + kItemKsz);
        uint32_t ksz;
        if (!hint_next(s.len, p, [&](uint64_t) { return kb; }, &ksz)) return QLZX_HL_ERR;
        const int t = hl_step(w.ld64(p), ksz, kh, klen);
        if (t == kHlMiss) return QLZX_HL_MISS;
        if (t == kHlCandidate) {
            uint32_t d = 0;
            for (uint32_t b = lane; b < ksz; b += 64) d |= w.byte(p + kHintItem + b) ^ key[b];
            if (!__any(d != 0)) {
                *at = p;
                return QLZX_HL_FOUND;
            }
        }
        p += kHintItem + ksz;
    }
    return QLZX_HL_MISS;
}

// hintMgr.getItem's order over the listed files: the first hit wins, an error ends the search, and
// so does the merged file, whatever it says.
template <class G>
__device__ __forceinline__ HlHit hl_files(const HlIn &in, const HlFile *files, G get) {
    HlHit r{QLZX_HL_MISS, 0, 0};
    for (uint32_t i = 0; i < in.n_files; i++) {
        const HlFile &s = files[i];
        r.file = i;
        r.status = s.bad ? (int32_t)QLZX_HL_BAD_FILE : get(in.hints + s.off, s, &r.at);
        if (r.status != QLZX_HL_MISS || s.merged) break;
    }
    return r;
}
// One lane writes request r's seven outputs.  A split hit reports its file's chunk id, a merged
// hit the chunk stored in the item (getItem: chunkID = it.Pos.ChunkID).
__device__ __forceinline__ void hl_report(const HlIn &in, const HlOut &out, const HlFile *files, uint32_t r,
                                          const HlHit &h) {
    uint32_t chunk = 0, offset = 0, ver = 0, vhash = 0;
    uint64_t src = 0;
    if (h.status == QLZX_HL_FOUND) {
        const HlFile &s = files[h.file];
        const uint8_t *p = in.hints + s.off + h.at;
        chunk = s.merged ? hint_ld32(p + kItemChunk) : s.chunk;
        offset = hint_ld32(p + kItemOffset), ver = hint_ld32(p + kItemVer);
        vhash = (uint32_t)p[kItemVhash] | ((uint32_t)p[kItemVhash + 1] << 8);
        src = s.off + h.at;
    }
    out.status[r] = h.status, out.hit_file[r] = h.file;
    out.chunk[r] = chunk, out.offset[r] = offset, out.ver[r] = (int32_t)ver, out.vhash[r] = (uint16_t)vhash;
    out.item_src[r] = src;
}
// totals = {found, miss, err, bad_file}: one more in status's slot
__device__ __forceinline__ void hl_count(uint32_t (&cnt)[4], int32_t status) {
    const uint32_t slot = status == QLZX_HL_FOUND ? 0u : status == QLZX_HL_MISS ? 1u : (uint32_t)status;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) cnt[k] += slot == k;
}
// request r: its keyhash and key
struct HlReq {
    uint64_t kh;
    const uint8_t *key;
    uint32_t klen;
    __device__ __forceinline__ HlReq(const HlIn &in, const uint64_t *hash, uint32_t r)
        : kh(hash[r]), key(in.keys + in.key_off[r]), klen(in.key_len[r]) {}
};

__global__ void __launch_bounds__(256) k_hl_lane(HlIn in, const HlFile *files, const uint64_t *hash, HlOut out) {
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < in.n; r += gridDim.x * 256) {
        const HlReq q(in, hash, r);
        const HlHit h = hl_files(in, files, [&](const uint8_t *f, const HlFile &s, uint64_t *at) {
            return hl_get_lane(f, s, q.kh, q.key, q.klen, in.bounded, at);
        });
        hl_report(in, out, files, r, h);
        hl_count(cnt, h.status);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t c = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&out.totals[k], c);
    }
}

__global__ void __launch_bounds__(256) k_hl_wave(HlIn in, const HlFile *files, const uint64_t *hash, HlOut out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4][kHlWin / 4 + 4];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    HlWin w;
    w.lds = lds[wv];
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t r = blockIdx.x * 4 + wv; r < in.n; r += gridDim.x * 4) {
        const HlReq q(in, hash, r);
        const HlHit h = hl_files(in, files, [&](const uint8_t *f, const HlFile &s, uint64_t *at) {
            return hl_get_wave(f, s, q.kh, q.key, q.klen, in.bounded, w, lane, at);
        });
        if (lane == 0) hl_report(in, out, files, r, h);
        hl_count(cnt, h.status);
    }
    if (lane == 0)
        for (uint32_t k = 0; k < 4; k++)
            if (cnt[k]) atomicAdd(&out.totals[k], cnt[k]);
}

// ---- workspace: the requests' default hashes and the files' heads ----
struct HlWs {
    uint64_t *hash;
    HlFile *files;
};
inline size_t hl_ws_layout(uint32_t n, uint32_t n_files, uint8_t *base, HlWs *w) {
    WsCarver c{base};
    HlWs t;
    t.hash = c.take<uint64_t>(8 * (size_t)n);
    t.files = c.take<HlFile>(sizeof(HlFile) * ((size_t)n_files + 1));
    if (w) *w = t;
    return c.bytes();
}

inline int launch_hl(const HlIn &in, bool lane_shape, const HlOut &out, void *ws, hipStream_t s) {
    HlWs w;
    hl_ws_layout(in.n, in.n_files, (uint8_t *)ws, &w);
    hipError_t e = hipMemsetAsync(out.totals, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    const uint64_t *hash = in.keyhash;
    if (!hash) {
        hipLaunchKernelGGL(k_keyhash, dim3(grid_for(in.n, 256, 2048)), dim3(256), 0, s, in.keys, in.key_off, in.key_len,
                           in.n, w.hash);
        hash = w.hash;
    }
    hipLaunchKernelGGL(k_hl_head, dim3(grid_for(in.n_files, 256, 2048)), dim3(256), 0, s, in, w.files);
    if (lane_shape)
        hipLaunchKernelGGL(k_hl_lane, dim3(grid_for(in.n, 256, 4096)), dim3(256), 0, s, in, (const HlFile *)w.files, hash,
                           out);
    else
        hipLaunchKernelGGL(k_hl_wave, dim3(grid_for(in.n, 4, 8192)), dim3(256), 0, s, in, (const HlFile *)w.files, hash,
                           out);
    return (int)hipGetLastError();
}

}  // namespace qlzx
