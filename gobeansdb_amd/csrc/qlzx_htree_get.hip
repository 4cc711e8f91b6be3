// qlzx_htree_get.hip -- queries over a bucket's HTree held as its .hash image in device memory
// (SURVEY §8 f1g): HTree.load's index (store/htree.go:107-144), HTree.get (:313-330 over
// SliceHeader.Get / findInBytes, store/leaf.go:81-102,155-164) for a batch of keys, the verdicts
// of GCMgr.gc (store/gc.go:280-312) for a replayed chunk, and UpdateHtreePos (:85-94) for the
// records GC moved.  The tree is the image plus leaf_first (include/qlzx_htree_get.h); geometry and
// slot rule are qlzx_htree.hip's HtGeo.
//
// Whatever the image and the arrays hold, leaf_first included: a leaf's items are cut to what lies
// inside image[0, bytes) (htg_leaf), so every load below stays there.
//
// Launches:
//   index     k_hti_count: the leaf nodes' counts, scanned: a guess of every length word's place;
//             k_hti_check: the lowest leaf whose length word is not count * item at that place
//             (all places below it are thereby proven); k_hti_walk: one lane walks from there;
//             k_hti_finish: leaf_first of the proven leaves, zeros with BAD_FILE, the totals.
//   get       k_keyhash unless the caller brings hashes, then one of two shapes of one search
//             (htg_lane_shape picks; the two totals go through one atomic per block, htg_tally):
//             k_htg_wave  a wave per key: a step compares 64 items, one per lane, each lane's
//                         eight stored bytes assembled from three aligned dwords; __ballot and
//                         its lowest bit end the step; the loop over the leaf is wave-uniform.
//             k_htg_lane  a lane per key, the leaf walked item by item.
//   liveness  k_gl_check (qlzx_gc_plan's size checks, the default keyhash), the get over the
//             records that passed, k_gl_verdict, the compaction of ask_idx, k_gl_totals.
//   move      k_htm_move: a lane per record; the leaf of a slot by a binary search of leaf_first.
#include "qlzx_hint_walk.h"
#include "qlzx_htree.h"
#include "qlzx_htree_get.h"

namespace qlzx {

struct HtgTree {
    const uint8_t *image;  // 16-B aligned
    uint64_t bytes;
    const uint32_t *leaf_first;  // nleaf + 1
    HtGeo g;
    __device__ __forceinline__ uint64_t leaves() const { return (uint64_t)kHtNode * g.nleaf; }  // the leaf section
    // what findInBytes compares, both sides through the slot rule: the low L bytes without the bucket nibbles
    __device__ __forceinline__ uint64_t cmp_mask() const {
        return (g.L >= 8 ? ~0ull : (1ull << (8 * g.L)) - 1) & (~0ull >> (4 * g.depth));
    }
};
struct HtgLeaf {
    uint64_t at;  // image byte of its first item
    uint32_t first, count;
};
// Leaf l < nleaf as leaf_first describes it, cut to the items that lie whole inside the image.
__device__ __forceinline__ HtgLeaf htg_leaf(const HtgTree &T, uint32_t l) {
    const uint32_t a = T.leaf_first[l], b = T.leaf_first[l + 1];
    HtgLeaf f;
    f.first = a;
    f.at = T.leaves() + 4ull * (l + 1) + (uint64_t)T.g.item * a;
    f.count = b > a ? b - a : 0u;
    if (f.at >= T.bytes) {
        f.count = 0;
    } else {
        const uint64_t room = (T.bytes - f.at) / T.g.item;
        if (room < f.count) f.count = (uint32_t)room;
    }
    return f;
}
// The eight bytes at image byte a, from the three aligned dwords that hold them.  They all lie
// inside an item that starts at a: (a & ~3) + 12 <= a + 16 <= a + item.
__device__ __forceinline__ uint64_t htg_ld64(const uint8_t *image, uint64_t a) {
    const uint32_t *w = (const uint32_t *)(image + (a & ~3ull));
    const uint32_t s = (uint32_t)a & 3u;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    return __builtin_amdgcn_alignbyte(w1, w0, s) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, s) << 32);
}
// bytesToItem (store/leaf.go:53-59) of the 11 bytes behind an item's stored keyhash
struct HtgItem {
    uint32_t chunk, offset, ver, vhash;
};
__device__ __forceinline__ HtgItem htg_item(const uint8_t *p) {
    HtgItem it;
    it.ver = hint_ld32(p);
    it.vhash = (uint32_t)p[4] | ((uint32_t)p[5] << 8);
    it.offset = ((uint32_t)p[6] << 8) | ((uint32_t)p[7] << 16) | ((uint32_t)p[8] << 24);
    it.chunk = (uint32_t)p[9] | ((uint32_t)p[10] << 8);
    return it;
}

// ---- get ----
// The requests: hash[r] for r < n(); n is the host's, or (liveness) a count that stays on the
// device, cut to cap.  gate (liveness): a record with gate[r] == QLZX_GL_BAD is not searched.
struct HtgReq {
    const uint64_t *hash;
    const uint32_t *n_dev;
    uint32_t cap;
    const int32_t *gate;
    __device__ __forceinline__ uint32_t n() const { return n_dev ? rec_count(n_dev, cap) : cap; }
    __device__ __forceinline__ bool open(uint32_t r) const { return !gate || gate[r] != QLZX_GL_BAD; }
};
struct HtgOut {
    int32_t *status;
    uint32_t *chunk, *offset;
    int32_t *ver;
    uint16_t *vhash;
    uint32_t *slot;
    unsigned long long *acc;  // found | miss << 32, 8-B aligned (a workspace's), zeroed by the caller
};
// One atomic per block for the two totals: with one or two per wave the launch was bound by them
// (some 13 ns per same-address atomic, 65,536 of them at 65,536 keys; profiles/r17_htree_get.json
// has the times after).  found / miss: lane 0's hold the wave's counts.
__device__ __forceinline__ void htg_tally(unsigned long long *acc, uint32_t found, uint32_t miss) {
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = found | ((unsigned long long)miss << 32);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = part[0] + part[1] + part[2] + part[3];
        if (sum) atomicAdd(acc, sum);
    }
}
// One lane writes request r's six outputs: idx = the hit's index in its leaf, or 0xffffffff.
__device__ __forceinline__ void htg_report(const HtgTree &T, const HtgLeaf &f, const HtgOut &out, uint32_t r,
                                           uint32_t idx) {
    HtgItem it{0, 0, 0, 0};
    const bool hit = idx != 0xffffffffu;
    if (hit) it = htg_item(T.image + f.at + (uint64_t)T.g.item * idx + T.g.L);
    out.status[r] = hit ? QLZX_HTG_FOUND : QLZX_HTG_MISS;
    out.chunk[r] = it.chunk, out.offset[r] = it.offset, out.ver[r] = (int32_t)it.ver, out.vhash[r] = (uint16_t)it.vhash;
    out.slot[r] = hit ? f.first + idx : QLZX_HTG_NO_SLOT;
}

__global__ void __launch_bounds__(256) k_htg_wave(HtgTree T, HtgReq q, HtgOut out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = q.n();
    const uint64_t mask = T.cmp_mask();
    uint32_t found = 0, miss = 0;
    for (uint32_t r = blockIdx.x * 4 + wv; r < n; r += gridDim.x * 4) {
        const uint64_t kh = q.hash[r];
        HtgLeaf f = htg_leaf(T, T.g.leaf(T.g.slot(kh)));
        if (!q.open(r)) f.count = 0;
        uint32_t idx = 0xffffffffu;
        for (uint32_t base = 0; base < f.count; base += 64) {  // wave-uniform: f is
            const uint32_t i = base + lane;
            bool hit = false;
            if (i < f.count) hit = ((htg_ld64(T.image, f.at + (uint64_t)T.g.item * i) ^ kh) & mask) == 0;
            const uint64_t m = __ballot(hit);
            if (m) {
                idx = base + (uint32_t)__builtin_ctzll(m);
                break;
            }
        }
        if (lane == 0) htg_report(T, f, out, r, idx);
        found += idx != 0xffffffffu, miss += idx == 0xffffffffu;
    }
    htg_tally(out.acc, found, miss);
}

__global__ void __launch_bounds__(256) k_htg_lane(HtgTree T, HtgReq q, HtgOut out) {
    const uint32_t n = q.n();
    const uint64_t mask = T.cmp_mask();
    uint32_t found = 0, miss = 0;
    for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {  // whole waves: wave_sum below
        const uint32_t r = base + threadIdx.x;
        if (r >= n) continue;
        const uint64_t kh = q.hash[r];
        HtgLeaf f = htg_leaf(T, T.g.leaf(T.g.slot(kh)));
        if (!q.open(r)) f.count = 0;
        uint32_t idx = 0xffffffffu;
        for (uint32_t i = 0; i < f.count; i++)
            if (((htg_ld64(T.image, f.at + (uint64_t)T.g.item * i) ^ kh) & mask) == 0) {
                idx = i;
                break;
            }
        htg_report(T, f, out, r, idx);
        found += idx != 0xffffffffu, miss += idx == 0xffffffffu;
    }
    htg_tally(out.acc, wave_sum(found), wave_sum(miss));
}
__global__ void k_htg_totals(uint32_t *totals, const unsigned long long *acc) {
    totals[0] = (uint32_t)*acc, totals[1] = (uint32_t)(*acc >> 32);
}

// Blocks of 256 threads for n items at `per` a block, every item with a thread (or wave) of its
// own: no cap, so the kernels' loops make one trip.  (k_keyhash and the kernels below keep their
// loops: any grid is right for them.)
inline uint32_t htq_blocks(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>((n + per - 1) / per, 1); }
// The get alone is capped, for htg_tally's sake: 2,048 blocks of four waves are the 8,192 waves
// the chip holds at once, the rest is strided over.  tests/test_gpu_htree_get.py crosses both caps.
constexpr uint32_t kHtgBlocks = 2048;
inline void launch_htg_find(const HtgTree &T, const HtgReq &q, bool lane_shape, const HtgOut &out, hipStream_t s) {
    const dim3 G(std::min(htq_blocks(q.cap, lane_shape ? 256 : 4), kHtgBlocks));
    if (lane_shape) hipLaunchKernelGGL(k_htg_lane, G, dim3(256), 0, s, T, q, out);
    else hipLaunchKernelGGL(k_htg_wave, G, dim3(256), 0, s, T, q, out);
}
// The shape by the number of keys and by the image's items per leaf (a lane walks its leaf alone)
inline bool htg_lane_shape(uint32_t n, uint64_t bytes, const HtGeo &g) {
    const uint64_t head = (uint64_t)(kHtNode + 4) * g.nleaf;
    const uint64_t items = bytes > head ? (bytes - head) / g.item : 0;
    const uint64_t leaf = items / g.nleaf;
    return leaf <= QLZX_HTG_LANE_LEAF && n >= QLZX_HTG_LANE_FROM && n >= QLZX_HTG_LANE_PER_ITEM * leaf;
}

struct HtgWs {
    unsigned long long *acc;
    uint64_t *hash;
};
inline size_t htg_ws_layout(uint32_t n, uint8_t *base, HtgWs *w) {
    WsCarver c{base};
    HtgWs t;
    t.acc = c.take<unsigned long long>(sizeof(unsigned long long));
    t.hash = c.take<uint64_t>(8 * (size_t)n);
    if (w) *w = t;
    return c.bytes();
}

inline int launch_htg(const HtgTree &T, const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                      const uint64_t *keyhash, uint32_t n, bool lane_shape, const HtgOut &out, void *ws,
                      uint32_t *totals, hipStream_t s) {
    HtgWs w;
    htg_ws_layout(n, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.acc, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    if (!keyhash) {
        hipLaunchKernelGGL(k_keyhash, dim3(htq_blocks(n, 256)), dim3(256), 0, s, keys, key_off, key_len, n, w.hash);
        keyhash = w.hash;
    }
    HtgOut o = out;
    o.acc = w.acc;
    launch_htg_find(T, HtgReq{keyhash, nullptr, n, nullptr}, lane_shape, o, s);
    hipLaunchKernelGGL(k_htg_totals, dim3(1), dim3(1), 0, s, totals, (const unsigned long long *)w.acc);
    return (int)hipGetLastError();
}

// ---- index ----
struct HtiCounters {
    uint32_t firstbad;  // the lowest leaf whose place or length the counts do not prove, nleaf = none
    uint32_t status, leaf, items;
};
// the leaf nodes' counts (0 where the image ends inside the node table)
__global__ void __launch_bounds__(256) k_hti_count(HtgTree T, unsigned long long *cnt, HtiCounters *ctr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *ctr = HtiCounters{T.g.nleaf, QLZX_HTG_OK, 0, 0};
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < T.g.nleaf; i += gridDim.x * 256) {
        const uint64_t at = (uint64_t)kHtNode * i;
        cnt[i] = T.bytes >= at + 4 ? hint_ld32(T.image + at) : 0u;
    }
}
// Leaf i's length word, were every leaf below it count * item long, sits behind
// 4 i + item * guess[i] bytes of the leaf section.  It proves the next place when it lies inside
// the image, says count * item, and the leaf's bytes lie inside the image too.
__global__ void __launch_bounds__(256) k_hti_check(HtgTree T, const unsigned long long *cnt,
                                                   const unsigned long long *guess, HtiCounters *ctr) {
    uint32_t bad = T.g.nleaf;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < T.g.nleaf; i += gridDim.x * 256) {
        const uint64_t p = T.leaves() + 4ull * i + (uint64_t)T.g.item * guess[i];  // guess < 2^52: no overflow
        bool ok = p <= T.bytes && T.bytes - p >= 4;
        if (ok) {
            const uint64_t len = hint_ld32(T.image + p);
            ok = len == cnt[i] * T.g.item && T.bytes - p - 4 >= len;
        }
        if (!ok && i < bad) bad = i;
    }
    if (bad < T.g.nleaf) atomicMin(&ctr->firstbad, bad);
}
// One lane, from the first unproven leaf on: HTree.load's second loop.  Correct, not fast.
__global__ void k_hti_walk(HtgTree T, const unsigned long long *cnt, const unsigned long long *guess,
                           uint32_t *leaf_first, HtiCounters *ctr) {
    const uint32_t f = ctr->firstbad, nleaf = T.g.nleaf;
    if (f >= nleaf) {  // every place is proven, and with it every count: their sum is below bytes / 16
        ctr->items = (uint32_t)(guess[nleaf - 1] + cnt[nleaf - 1]);
        return;
    }
    uint32_t items = (uint32_t)guess[f];
    uint64_t p = T.leaves() + 4ull * f + (uint64_t)T.g.item * items;
    for (uint32_t i = f; i < nleaf; i++) {
        bool ok = p <= T.bytes && T.bytes - p >= 4;
        uint32_t len = 0;
        if (ok) {
            len = hint_ld32(T.image + p);
            ok = len % T.g.item == 0 && T.bytes - p - 4 >= len;
        }
        if (!ok) {
            ctr->status = QLZX_HTG_BAD_FILE, ctr->leaf = i;
            return;
        }
        leaf_first[i] = items;
        items += len / T.g.item;  // item * items <= bytes < 2^36
        p += 4ull + len;
    }
    leaf_first[nleaf] = items;
    ctr->items = items;
}
__global__ void __launch_bounds__(256) k_hti_finish(HtgTree T, const unsigned long long *guess, uint32_t *leaf_first,
                                                    uint32_t *totals, const HtiCounters *ctr) {
    const HtiCounters c = *ctr;
    const bool bad = c.status != QLZX_HTG_OK;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= T.g.nleaf; i += gridDim.x * 256) {
        if (bad) leaf_first[i] = 0;
        else if (i < c.firstbad) leaf_first[i] = (uint32_t)guess[i];
        else if (i == T.g.nleaf && c.firstbad >= T.g.nleaf) leaf_first[i] = c.items;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        totals[0] = bad ? 0u : c.items, totals[1] = T.g.nleaf, totals[2] = c.status, totals[3] = bad ? c.leaf : 0u;
}

struct HtiWs {
    HtiCounters *ctr;
    unsigned long long *cnt, *guess;
    void *tmp;
    size_t tmp_bytes;
};
inline size_t hti_ws_layout(uint32_t nleaf, uint8_t *base, HtiWs *w) {
    WsCarver c{base};
    HtiWs t;
    t.ctr = c.take<HtiCounters>(sizeof(HtiCounters));
    t.cnt = c.take<unsigned long long>(8 * (size_t)nleaf);
    t.guess = c.take<unsigned long long>(8 * (size_t)nleaf);
    t.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, t.tmp_bytes, (const unsigned long long *)nullptr,
                                  (unsigned long long *)nullptr, 0ull, (size_t)nleaf,
                                  rocprim::plus<unsigned long long>());
    t.tmp = c.take(t.tmp_bytes);
    if (w) *w = t;
    return c.bytes();
}
inline int launch_hti(const HtgTree &T, uint32_t *leaf_first, uint32_t *totals, void *ws, hipStream_t s) {
    HtiWs w;
    hti_ws_layout(T.g.nleaf, (uint8_t *)ws, &w);
    const dim3 G(htq_blocks((uint64_t)T.g.nleaf + 1, 256)), B(256);
    hipLaunchKernelGGL(k_hti_count, G, B, 0, s, T, w.cnt, w.ctr);
    size_t tb = w.tmp_bytes;
    const hipError_t e = rocprim::exclusive_scan(w.tmp, tb, (const unsigned long long *)w.cnt, w.guess, 0ull,
                                                 (size_t)T.g.nleaf, rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hti_check, G, B, 0, s, T, (const unsigned long long *)w.cnt,
                       (const unsigned long long *)w.guess, w.ctr);
    hipLaunchKernelGGL(k_hti_walk, dim3(1), dim3(1), 0, s, T, (const unsigned long long *)w.cnt,
                       (const unsigned long long *)w.guess, leaf_first, w.ctr);
    hipLaunchKernelGGL(k_hti_finish, G, B, 0, s, T, (const unsigned long long *)w.guess, leaf_first, totals,
                       (const HtiCounters *)w.ctr);
    return (int)hipGetLastError();
}

// ---- liveness ----
struct GlCounters {
    unsigned long long get;  // the get's found | miss << 32: not reported
    uint32_t n, newest, other, other_del, absent, absent_kept, bad, keep;
    uint32_t nask, pad;
};
struct GlIn {
    const uint8_t *data;
    uint64_t size;
    const uint64_t *rec_off;
    const uint32_t *result;
    uint32_t cap, max_key;
    uint64_t body_max;
};
// qlzx_gc_plan's checks (k_gc_check) on every record; a record that passes is NOT_IN_TREE until
// the tree says otherwise.  hash (the workspace's) is filled only when the caller brought none.
__global__ void __launch_bounds__(256) k_gl_check(GlIn in, int32_t *verdict, uint64_t *hash) {
    const uint32_t n = rec_count(in.result, in.cap);
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        int32_t v = QLZX_GL_BAD;
        uint64_t h = 0;
        const uint64_t off = in.rec_off[j];
        if (rec_pos_verdict(off, in.size) == kRecOk) {
            const uint2 kv = *(const uint2 *)(in.data + off + 16);  // ksz, vsz
            if (rec_size_verdict(kv.x, kv.y, in.size - off - kRpHdr, in.max_key, in.body_max) == kRecOk) {
                v = QLZX_GL_NOT_IN_TREE;
                if (hash) h = hint_keyhash(in.data + off + kRpHdr, kv.x);
            }
        }
        verdict[j] = v;
        if (hash) hash[j] = h;
    }
}
struct GlOut {
    uint8_t *keep;
    int32_t *verdict;
};
// found / chunk / offset: the get's answers for the records that passed the checks
__global__ void __launch_bounds__(256) k_gl_verdict(GlIn in, uint32_t src_chunk, uint32_t begin_gt_0,
                                                    const int32_t *found, const uint32_t *chunk,
                                                    const uint32_t *offset, const int32_t *tree_ver, GlOut out,
                                                    GlCounters *cnt) {
    const uint32_t n = rec_count(in.result, in.cap);
    uint32_t c[7] = {0, 0, 0, 0, 0, 0, 0};  // newest, other, other_del, absent, absent_kept, bad, keep
    for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {  // whole waves: wave_sum below
        const uint32_t j = base + threadIdx.x;
        if (j >= n) continue;
        int32_t v = out.verdict[j];
        uint32_t keep = 0;
        if (v != QLZX_GL_BAD) {
            const uint64_t off = in.rec_off[j];
            if (found[j] == QLZX_HTG_FOUND) {
                if (chunk[j] == src_chunk && (uint64_t)offset[j] == off) {
                    v = QLZX_GL_NEWEST, keep = 1;
                } else {
                    v = QLZX_GL_OTHER_POS;
                    c[2] += tree_ver[j] < 0;
                }
            } else {
                v = QLZX_GL_NOT_IN_TREE;
                keep = begin_gt_0 && *(const int32_t *)(in.data + off + 12) < 0;  // gc.Begin > 0 && rec.Payload.Ver < 0
                c[4] += keep;
            }
        }
        out.verdict[j] = v;
        out.keep[j] = (uint8_t)keep;
        c[0] += v == QLZX_GL_NEWEST, c[1] += v == QLZX_GL_OTHER_POS, c[3] += v == QLZX_GL_NOT_IN_TREE;
        c[5] += v == QLZX_GL_BAD, c[6] += keep;
    }
    uint32_t *dst[7] = {&cnt->newest, &cnt->other, &cnt->other_del, &cnt->absent, &cnt->absent_kept, &cnt->bad, &cnt->keep};
#pragma unroll
    for (uint32_t k = 0; k < 7; k++) {
        const uint32_t x = wave_sum(c[k]);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst[k], x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->n = n;
}
struct GlAskFlag {
    const int32_t *verdict;
    const uint32_t *result;
    uint32_t cap;
    __device__ uint32_t operator()(uint32_t j) const {
        return j < rec_count(result, cap) && verdict[j] == QLZX_GL_OTHER_POS;
    }
};
struct GlAskPut {
    uint32_t *ask_idx;
    __device__ void operator()(uint32_t j, uint32_t idx, uint32_t flag) const {
        if (flag) ask_idx[idx] = j;
    }
};
__global__ void k_gl_totals(uint32_t *totals, const GlCounters *cnt) {
    totals[0] = cnt->n, totals[1] = cnt->newest, totals[2] = cnt->other, totals[3] = cnt->other_del;
    totals[4] = cnt->absent, totals[5] = cnt->absent_kept, totals[6] = cnt->bad, totals[7] = cnt->keep;
}

struct GlWs {
    GlCounters *cnt;
    uint64_t *hash;
    int32_t *found;
    uint32_t *chunk, *offset, *tiles;
};
inline size_t gl_ws_layout(uint32_t cap, uint8_t *base, GlWs *w) {
    WsCarver c{base};
    GlWs t;
    t.cnt = c.take<GlCounters>(sizeof(GlCounters));
    t.hash = c.take<uint64_t>(8 * (size_t)cap);
    t.found = c.take<int32_t>(4 * (size_t)cap);
    t.chunk = c.take<uint32_t>(4 * (size_t)cap);
    t.offset = c.take<uint32_t>(4 * (size_t)cap);
    t.tiles = c.take<uint32_t>(4 * ((size_t)cap / kScanTile + 1));
    if (w) *w = t;
    return c.bytes();
}
inline int launch_gl(const GlIn &in, uint32_t src_chunk, const HtgTree &T, const uint64_t *keyhash, uint32_t flags,
                     bool lane_shape, uint8_t *keep, int32_t *verdict, uint16_t *vhash, int32_t *tree_ver,
                     uint32_t *slot, uint32_t *ask_idx, uint32_t *totals, void *ws, hipStream_t s) {
    GlWs w;
    gl_ws_layout(in.cap, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(GlCounters), s);
    if (e != hipSuccess) return (int)e;
    const dim3 G(htq_blocks(in.cap, 256));
    hipLaunchKernelGGL(k_gl_check, G, dim3(256), 0, s, in, verdict, keyhash ? nullptr : w.hash);
    const HtgOut found{w.found, w.chunk, w.offset, tree_ver, vhash, slot, &w.cnt->get};
    launch_htg_find(T, HtgReq{keyhash ? keyhash : w.hash, in.result, in.cap, verdict}, lane_shape, found, s);
    hipLaunchKernelGGL(k_gl_verdict, G, dim3(256), 0, s, in, src_chunk,
                       (uint32_t)((flags & QLZX_GL_F_BEGIN_GT_0) != 0), (const int32_t *)w.found,
                       (const uint32_t *)w.chunk, (const uint32_t *)w.offset, (const int32_t *)tree_ver,
                       GlOut{keep, verdict}, w.cnt);
    launch_compact(GlAskFlag{verdict, in.result, in.cap}, GlAskPut{ask_idx}, in.cap, w.tiles, &w.cnt->nask, s);
    hipLaunchKernelGGL(k_gl_totals, dim3(1), dim3(1), 0, s, totals, (const GlCounters *)w.cnt);
    return (int)hipGetLastError();
}

// ---- move ----
struct HtmIn {
    const uint32_t *result;
    uint32_t cap;
    const int32_t *verdict, *gc_status;
    const uint32_t *slot, *new_chunk;
    const uint64_t *new_off;
    const uint32_t *dst_chunk_id;
    uint32_t max_chunks;
};
// Where the 11 bytes behind the stored keyhash of item `slot` start, 0 when leaf_first names no
// leaf that holds it or the item does not lie inside the image.
__device__ __forceinline__ uint64_t htm_item_at(const HtgTree &T, uint32_t slot) {
    uint32_t lo = 0, hi = T.g.nleaf;  // the last leaf that starts at or before the slot
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (T.leaf_first[mid] <= slot) lo = mid;
        else hi = mid;
    }
    if (T.leaf_first[lo] > slot || T.leaf_first[lo + 1] <= slot) return 0;
    const uint64_t at = T.leaves() + 4ull * (lo + 1) + (uint64_t)T.g.item * slot;
    if (at > T.bytes || T.bytes - at < T.g.item) return 0;
    return at + T.g.L;
}
__global__ void __launch_bounds__(256) k_htm_move(HtgTree T, uint8_t *image, HtmIn in, uint32_t *cnt) {
    const uint32_t n = rec_count(in.result, in.cap);
    uint32_t moved = 0, skipped = 0;
    for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {  // whole waves: wave_sum below
        const uint32_t j = base + threadIdx.x;
        if (j >= n || in.verdict[j] != QLZX_GL_NEWEST || in.gc_status[j] != QLZX_GC_WRITTEN) continue;
        const uint64_t off = in.new_off[j];
        const uint32_t c = in.new_chunk[j];
        const uint32_t id = c < in.max_chunks ? in.dst_chunk_id[c] : 0xffffffffu;
        const uint64_t at = off <= 0xffffffffull && off % kRpSlot == 0 && id < 65536 ? htm_item_at(T, in.slot[j]) : 0;
        if (!at) {
            skipped++;
            continue;
        }
        uint8_t *p = image + at + 6;  // itemToBytes (store/leaf.go:61-71): the position's five bytes
        p[0] = (uint8_t)(off >> 8), p[1] = (uint8_t)(off >> 16), p[2] = (uint8_t)(off >> 24);
        p[3] = (uint8_t)id, p[4] = (uint8_t)(id >> 8);
        moved++;
    }
    moved = wave_sum(moved), skipped = wave_sum(skipped);
    if ((threadIdx.x & 63) == 0) {
        if (moved) atomicAdd(&cnt[0], moved);
        if (skipped) atomicAdd(&cnt[1], skipped);
    }
}
__global__ void k_htm_totals(uint32_t *totals, const uint32_t *cnt) { totals[0] = cnt[0], totals[1] = cnt[1]; }

inline size_t htm_ws_layout(uint32_t cap, uint8_t *base, uint32_t **cnt) {
    (void)cap;
    WsCarver c{base};
    uint32_t *p = c.take<uint32_t>(2 * sizeof(uint32_t));
    if (cnt) *cnt = p;
    return c.bytes();
}
inline int launch_htm(const HtgTree &T, uint8_t *image, const HtmIn &in, uint32_t *totals, void *ws, hipStream_t s) {
    uint32_t *cnt;
    htm_ws_layout(in.cap, (uint8_t *)ws, &cnt);
    const hipError_t e = hipMemsetAsync(cnt, 0, 2 * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_htm_move, dim3(htq_blocks(in.cap, 256)), dim3(256), 0, s, T, image, in, cnt);
    hipLaunchKernelGGL(k_htm_totals, dim3(1), dim3(1), 0, s, totals, (const uint32_t *)cnt);
    return (int)hipGetLastError();
}

}  // namespace qlzx
