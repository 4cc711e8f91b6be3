// qlzx_hint_fmt.h -- what the hint-file kernels share (qlzx_hint.hip, qlzx_hintmerge.hip,
// qlzx_hintlookup.hip, qlzx_htree.hip; each includes this header itself, the merge and the tree
// through qlzx_hint_walk.h): the hint file's format (head, item and
// index entry, store/hintfile.go:19-212) with its unaligned loads and hintFileReader.next's rule
// stated once, getKeyHashDefalut and the key order, the counters and the (bytes, items) pair of a
// plan, the sort's workspace tail with its scan, the run / fix kernels over any source of keys K,
// the index pass (launch_hint_index) and the file writer k_hint_file<F> over any source of items F.
#pragma once

#include <cstring>  // rocPRIM's texture_cache_iterator.hpp calls memset without it
#include <rocprim/rocprim.hpp>

#include "qlzx_recfile.h"

namespace qlzx {

// ---- the format ----
// head:  indexOffset i64 ‖ numKey u32 ‖ datasize u32
// item:  keyhash u64 ‖ chunk u32 ‖ offset u32 ‖ ver i32 ‖ vhash u16 ‖ ksz u8 ‖ key
// index: entries of keyhash u64 ‖ item offset i64, from indexOffset to the file's end
constexpr uint32_t kHintHead = 16, kHintItem = 23, kHintMaxKey = 255, kHintEntry = 16;
constexpr uint32_t kHeadDatasize = 12;
constexpr uint32_t kItemChunk = 8, kItemOffset = 12, kItemVer = 16, kItemVhash = 20, kItemKsz = 22;
constexpr uint32_t kEntryOffset = 8;

// Unaligned loads.  Not ld_dword of qlzx_decode_fmt.h: that one pins its address to VGPRs for its loops' sake.
__device__ __forceinline__ uint32_t hint_ld32(const uint8_t *p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}
__device__ __forceinline__ uint64_t hint_ld64(const uint8_t *p) {
    return hint_ld32(p) | ((uint64_t)hint_ld32(p + 4) << 32);
}

// hintFileReader.next (store/hintfile.go:89-127) at position p of a file of len bytes, p <= len:
// the item's ksz, or false when its head or its key runs past the file.  byte(q) reads file byte q
// and is called once, for ksz, after the head is known to lie inside the file.  The next item
// starts at p + kHintItem + ksz: every step advances 23 bytes or more.
template <class B>
__device__ __forceinline__ bool hint_next(uint64_t len, uint64_t p, B byte, uint32_t *ksz) {
    if (len - p < kHintItem) return false;
    *ksz = byte(p + kItemKsz);
    return len - p - kHintItem >= *ksz;
}

// ---- getKeyHashDefalut (store/key.go:41-59): fnv1a(key) << 32 | murmur3_32(key, 0) ----
// One key per lane.  The sign-extending Fnv1a (fnv1a_bytes' quirk) is serial per byte, MurmurHash3
// x86_32 takes a little-endian dword per round: a key that starts on a 4-B boundary (every record
// key does: 24 bytes into a 256-B slot) is read a dword at a time, two rounds' loads in flight.
__device__ __forceinline__ uint32_t mm3_round(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = (k << 15) | (k >> 17);
    k *= 0x1b873593u;
    h ^= k;
    h = (h << 13) | (h >> 19);
    return h * 5u + 0xe6546b64u;
}
__device__ __forceinline__ uint32_t fnv_dword(uint32_t h, uint32_t w) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
        h ^= (uint32_t)(int32_t)(int8_t)(w >> (8 * b));
        h *= 0x01000193u;
    }
    return h;
}
__device__ uint64_t hint_keyhash(const uint8_t *p, uint32_t n) {
    uint32_t f = 0x811c9dc5u, m = 0;
    const uint32_t nb = n / 4;
    if (((uintptr_t)p & 3u) == 0) {
        const uint32_t *q = (const uint32_t *)p;
        uint32_t nx = nb ? q[0] : 0u;
        for (uint32_t i = 0; i < nb; i++) {
            const uint32_t w = nx;
            nx = i + 1 < nb ? q[i + 1] : 0u;
            f = fnv_dword(f, w);
            m = mm3_round(m, w);
        }
    } else {
        for (uint32_t i = 0; i < nb; i++) {
            const uint8_t *b = p + 4 * i;
            const uint32_t w = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
            f = fnv_dword(f, w);
            m = mm3_round(m, w);
        }
    }
    uint32_t k = 0;
    for (uint32_t i = 4 * nb; i < n; i++) {
        const uint32_t b = p[i];
        f ^= (uint32_t)(int32_t)(int8_t)b;
        f *= 0x01000193u;
        k |= b << (8 * (i & 3));
    }
    if (n & 3u) {
        k *= 0xcc9e2d51u;
        k = (k << 15) | (k >> 17);
        k *= 0x1b873593u;
        m ^= k;
    }
    m ^= n;
    m ^= m >> 16;
    m *= 0x85ebca6bu;
    m ^= m >> 13;
    m *= 0xc2b2ae35u;
    m ^= m >> 16;
    return ((uint64_t)f << 32) | m;
}

__global__ void __launch_bounds__(256) k_keyhash(const uint8_t *src, const uint64_t *off, const uint32_t *len,
                                                 uint32_t n, uint64_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        out[i] = hint_keyhash(src + off[i], len[i]);
}

// memcmp order with the shorter prefix first (Go's string <): < 0, 0, > 0.
__device__ int hint_key_cmp(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb) {
    const uint32_t n = na < nb ? na : nb;
    uint32_t i = 0;
    if ((((uintptr_t)a | (uintptr_t)b) & 3u) == 0)
        while (i + 4 <= n && *(const uint32_t *)(a + i) == *(const uint32_t *)(b + i)) i += 4;
    for (; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na == nb ? 0 : na < nb ? -1 : 1;
}

// ---- a plan's counters, its (bytes, items) pairs and the workspace tail of its sort ----
struct HintCounters {
    uint32_t nv, nlist, cut1, nk, r0, nidx, datasize, nbelow;  // cut1 = the cut record + 1, 0 without a cut
    unsigned long long ibytes;                                 // the items' bytes: indexOffset - 16
};
struct HintAcc {  // (bytes, items) summed together by one scan
    unsigned long long b, c;
};
struct HintAccPlus {
    __host__ __device__ HintAcc operator()(const HintAcc &x, const HintAcc &y) const {
        return HintAcc{x.b + y.b, x.c + y.c};
    }
};

// rocPRIM's temporary storage for every count up to `most` that a call may sort or scan: it is not
// monotone in the count (a small input takes another algorithm), so the largest need over `most`
// and every power of two below it
inline size_t hint_tmp_bytes(size_t most) {
    size_t tmp_bytes = 0;
    for (size_t q = most; q; q = q & (q - 1) ? (size_t)1 << (63 - __builtin_clzll(q)) : q >> 1) {
        size_t sort_tmp = 0, scan_tmp = 0, acc_tmp = 0;
        (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                        (const uint32_t *)nullptr, (uint32_t *)nullptr, q, 0, 64);
        (void)rocprim::exclusive_scan(nullptr, scan_tmp, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, q,
                                      rocprim::plus<uint32_t>());
        (void)rocprim::exclusive_scan(nullptr, acc_tmp, (const HintAcc *)nullptr, (HintAcc *)nullptr, HintAcc{0, 0},
                                      q, HintAccPlus());
        tmp_bytes = std::max(tmp_bytes, std::max(std::max(sort_tmp, scan_tmp), acc_tmp));
    }
    return tmp_bytes;
}

// What both plans carve last, m entries each: the sort's pairs, the flags and their scans, rocPRIM's
// temporary.  key_in is the second half of `acc`, a (bytes, items) array of m entries or more that
// the plan does not use while it sorts.
struct HintSortWs {
    uint64_t *key_in, *key_s;
    uint32_t *val_in, *val_s, *val_r, *list, *fa, *fb;  // fa / fb: a flag array and its scan, three times
    uint8_t *fl, *gh;
    void *tmp;
    size_t tmp_bytes;
    void carve(WsCarver &c, size_t m, HintAcc *acc, size_t tmp_need) {
        key_in = acc ? (uint64_t *)acc + m : nullptr;
        key_s = c.take<uint64_t>(8 * m);
        val_in = c.take<uint32_t>(4 * m);
        val_s = c.take<uint32_t>(4 * m);
        val_r = c.take<uint32_t>(4 * m);
        list = c.take<uint32_t>(4 * m);
        fa = c.take<uint32_t>(4 * m);
        fb = c.take<uint32_t>(4 * m);
        fl = c.take(m);
        gh = c.take(m);
        tmp_bytes = tmp_need;
        tmp = c.take(tmp_bytes);
    }
    // the exclusive scan of n elements through tmp: u32 flags under rocprim::plus, HintAcc under HintAccPlus
    template <class T, class Op>
    hipError_t scan(const T *from, T *to, size_t n, Op op, hipStream_t s) const {
        size_t tb = tmp_bytes;
        return rocprim::exclusive_scan(tmp, tb, from, to, T{}, n, op, s);
    }
    hipError_t sort(const uint32_t *vin, uint32_t *vout, size_t n, hipStream_t s) const {  // key_in -> key_s, stable
        size_t tb = tmp_bytes;
        return rocprim::radix_sort_pairs(tmp, tb, (const uint64_t *)key_in, key_s, vin, vout, n, 0, 64, s);
    }
};

// ---- (keyhash, key, append) order and the groups of a sorted plan ----
// K names the keys: K::key(r, &bytes) = the length of key r, 0 (and bytes = nullptr) when r has none.
// fl[i]: bit 0 = first of its run of equal keyhash, bit 1 = same keyhash as its predecessor but
// other key bytes (such a run is listed for k_hint_fix).  gh[i] = a group (one item) starts here,
// val_r = the records in (keyhash, key, append) order: both final for every run without bit 1.
template <class K>
__global__ void __launch_bounds__(256) k_hint_runs(K in, const uint64_t *key_s, const uint32_t *val_s,
                                                   uint8_t *fl, uint8_t *gh, uint32_t *val_r, uint32_t *list,
                                                   HintCounters *cnt) {
    const uint32_t nv = cnt->nv;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
        const uint32_t r = val_s[i];
        const bool head = i == 0 || key_s[i] != key_s[i - 1];
        bool kdiff = false;
        if (!head) {
            const uint8_t *a, *b;
            const uint32_t na = in.key(val_s[i - 1], &a), nb = in.key(r, &b);
            kdiff = hint_key_cmp(a, na, b, nb) != 0;
        }
        fl[i] = (uint8_t)(head | (kdiff << 1));
        gh[i] = head | kdiff;
        val_r[i] = r;
        if (kdiff) list[atomicAdd(&cnt->nlist, 1u)] = i;
    }
}

// The slow path: a run of equal keyhash with different keys (a 64-bit collision, or a caller's
// keyhash array).  Every listed position finds its run; the run's first listed position ranks it:
// lane by lane, an element's place is the number of elements before it in (key, append) order,
// L^2 key comparisons for a run of L.  A run's positions are in append order (the sort is stable).
template <class K>
__global__ void __launch_bounds__(256) k_hint_fix(K in, const uint32_t *val_s, const uint8_t *fl, uint8_t *gh,
                                                  uint32_t *val_r, const uint32_t *list, const HintCounters *cnt) {
    const uint32_t nv = cnt->nv, nl = cnt->nlist < nv ? cnt->nlist : nv, lane = threadIdx.x & 63;
    for (uint32_t e = blockIdx.x * 4 + threadIdx.x / 64; e < nl; e += gridDim.x * 4) {
        const uint32_t i = list[e];
        uint32_t s = i - 1;  // fl[0] has bit 0: the walk ends at or before 0
        bool mine = true;
        while (!(fl[s] & 1)) {
            if (fl[s] & 2) {
                mine = false;  // an earlier listed position of this run ranks it
                break;
            }
            s--;
        }
        if (!mine) continue;
        uint32_t end = i + 1;
        while (end < nv && !(fl[end] & 1)) end++;
        for (uint32_t a = s + lane; a < end; a += 64) {
            const uint32_t ra = val_s[a];
            const uint8_t *ka;
            const uint32_t na = in.key(ra, &ka);
            uint32_t rank = 0;
            bool dup = false;
            for (uint32_t b = s; b < end; b++) {
                const uint32_t rb = val_s[b];
                const uint8_t *kb;
                const uint32_t nb = in.key(rb, &kb);
                const int c = hint_key_cmp(kb, nb, ka, na);
                rank += c < 0 || (c == 0 && b < a);
                dup |= c == 0 && b < a;
            }
            val_r[s + rank] = ra;
            gh[s + rank] = !dup;
        }
    }
}

// ---- the index (store/hintfile.go:174-176) ----
// From `last`, the next entry is the first item k with o_k - last > thr.  J[k] = the entry after
// item k (nk = none), r0 = the first one (last = 0).
__device__ __forceinline__ uint32_t hint_succ(const uint64_t *item_off, uint32_t lo, uint32_t nk, uint64_t last,
                                              int64_t thr) {
    uint32_t hi = nk;  // the first k in [lo, nk) with o_k - last > thr: o is increasing
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)(item_off[mid] - last) > thr) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__global__ void __launch_bounds__(256) k_hint_next(const uint64_t *item_off, int64_t thr, uint32_t M, uint32_t *J,
                                                   uint32_t *iflag, HintCounters *cnt) {
    const uint32_t nk = cnt->nk;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k <= M; k += gridDim.x * 256) {
        J[k] = k < nk ? hint_succ(item_off, k + 1, nk, item_off[k], thr) : nk;
        iflag[k] = 0;
        if (k == 0) cnt->r0 = hint_succ(item_off, 0, nk, 0, thr);
    }
}
__global__ void k_hint_seed(const HintCounters *cnt, uint32_t *iflag) { iflag[cnt->r0] = 1; }
__global__ void __launch_bounds__(256) k_hint_double(const HintCounters *cnt, const uint32_t *J, uint32_t *J2,
                                                     uint32_t *iflag) {
    const uint32_t nk = cnt->nk;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k <= nk; k += gridDim.x * 256) {
        const uint32_t j = J[k];
        if (iflag[k]) iflag[j] = 1;
        J2[k] = J[j];
    }
}
__global__ void __launch_bounds__(256) k_hint_index(const uint32_t *iflag, const uint32_t *ipos, uint32_t *index_item,
                                                    HintCounters *cnt) {
    const uint32_t nk = cnt->nk;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k <= nk; k += gridDim.x * 256) {
        if (k < nk && iflag[k]) index_item[ipos[k]] = k;
        if (k == nk) cnt->nidx = ipos[k];
    }
}
// The index entries of the cnt->nk <= M items at item_off: successors, the walk from the first one by
// pointer doubling (as k_rp_double), compaction into index_item; cnt->nidx = their number.  Uses
// w.val_in / w.val_s as the two successor arrays and w.fa / w.fb as the flags and their scan.
inline hipError_t launch_hint_index(const uint64_t *item_off, int64_t index_interval, uint32_t M, const HintSortWs &w,
                                    HintCounters *cnt, uint32_t *index_item, hipStream_t s) {
    const dim3 G(grid_for((uint64_t)M + 1, 256, 2048)), B(256);
    const int64_t thr = (int64_t)((uint64_t)index_interval - kHintItem - 256);
    uint32_t *J = w.val_in, *J2 = w.val_s;
    hipLaunchKernelGGL(k_hint_next, G, B, 0, s, item_off, thr, M, J, w.fa, cnt);
    hipLaunchKernelGGL(k_hint_seed, dim3(1), dim3(1), 0, s, (const HintCounters *)cnt, w.fa);
    for (uint64_t reach = 1; reach < (uint64_t)M + 1; reach <<= 1) {
        hipLaunchKernelGGL(k_hint_double, G, B, 0, s, (const HintCounters *)cnt, (const uint32_t *)J, J2, w.fa);
        std::swap(J, J2);
    }
    if (const hipError_t e = w.scan(w.fa, w.fb, (size_t)M + 1, rocprim::plus<uint32_t>(), s)) return e;
    hipLaunchKernelGGL(k_hint_index, G, B, 0, s, (const uint32_t *)w.fa, (const uint32_t *)w.fb, index_item, cnt);
    return hipSuccess;
}

// ---- the file writer ----
struct HintTot {  // the plan's totals: items, index entries, datasize, indexOffset, file bytes
    uint32_t nk, nidx, datasize;
    uint64_t io, fb;
};
// One item's 23 header bytes as dwords (h0 .. h5; a zero dword pads the funnel shift) and its key.
struct HintCur {
    uint32_t k, ksz;
    uint64_t o, next;
    uint32_t h0, h1, h2, h3, h4, h5;
    const uint8_t *key;
};
// F names the items of a plan (HintFile, HmFile).  The plan arrays may hold anything (they are the
// caller's between the two calls): F keeps every read of its own inside its arrays' cap entries
// and inside its bytes, the writer below every k below t.nk <= cap.
//   item_off, index_item     the plan's arrays, cap entries
//   void head(k, HintCur &)  item k's header dwords, ksz and key into a zeroed cursor
//   uint64_t keyhash(k)      item k's keyhash
//   uint32_t status(prev, fits)   totals[8] after the write
template <class F>
__device__ __forceinline__ void hint_cur_load(const F &f, const HintTot &t, uint32_t k, HintCur &c) {
    c.k = k;
    c.o = f.item_off[k];
    c.next = k + 1 < t.nk ? f.item_off[k + 1] : t.io;
    c.ksz = 0, c.key = nullptr;
    c.h0 = 0, c.h1 = 0, c.h2 = 0, c.h3 = 0, c.h4 = 0, c.h5 = 0;
    f.head(k, c);
}
__device__ __forceinline__ uint32_t hint_funnel(uint32_t lo, uint32_t hi, uint32_t r) {  // bytes r.. of hi:lo
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * r));
}
// header dword i by selects (0 past the header): an array indexed at run time would live in scratch
__device__ __forceinline__ uint32_t hint_h(const HintCur &c, uint32_t i) {
    return i == 0 ? c.h0 : i == 1 ? c.h1 : i == 2 ? c.h2 : i == 3 ? c.h3 : i == 4 ? c.h4 : i == 5 ? c.h5 : 0u;
}
__device__ __forceinline__ uint32_t hint_item_byte(const HintCur &c, uint64_t rel) {
    if (rel < kHintItem) return (hint_h(c, (uint32_t)rel >> 2) >> (8 * (rel & 3))) & 0xffu;
    return rel - kHintItem < c.ksz ? c.key[rel - kHintItem] : 0u;
}
// Index entry e = (keyhash, offset) of item index_item[e]: the dword at byte d of the index, d a
// multiple of 4 (an entry is 16 bytes: a dword lies inside the index or past its end).  d inside
// the index means d / 16 < nidx <= cap (k_hint_file's cut); an entry that names no item is zeros.
template <class F>
__device__ __forceinline__ uint32_t hint_index_dword(const F &f, const HintTot &t, uint64_t d) {
    if (d >= t.fb - t.io) return 0;
    const uint32_t k = f.index_item[d / kHintEntry], r = (uint32_t)d % kHintEntry;
    const uint64_t x = k < t.nk ? (r < kEntryOffset ? f.keyhash(k) : f.item_off[k]) : 0;
    return (uint32_t)(x >> (8 * (r & 4)));
}
// The file's dword at byte position p >= 16 (bytes past the file's end come out as zeros).
template <class F>
__device__ __forceinline__ uint32_t hint_file_dword(const F &f, const HintTot &t, uint64_t p, HintCur &c) {
    if (p >= t.io) {
        const uint64_t d = p - t.io;
        const uint32_t lo = hint_index_dword(f, t, d & ~3ull);
        return (d & 3u) ? hint_funnel(lo, hint_index_dword(f, t, (d & ~3ull) + 4), d & 3u) : lo;
    }
    while (p >= c.next && c.k + 1 < t.nk) hint_cur_load(f, t, c.k + 1, c);
    if (p >= c.o && p + 4 <= c.next) {  // the whole dword inside one item's header or key
        const uint64_t rel = p - c.o;
        const uint32_t hd = (uint32_t)rel >> 2;
        if (rel + 4 <= kHintItem) return hint_funnel(hint_h(c, hd), hint_h(c, hd + 1), rel & 3);
        if (rel >= kHintItem && rel - kHintItem + 4 <= c.ksz) return hint_ld32(c.key + (rel - kHintItem));
    }
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; b++) {  // across a header / key / item / index boundary
        const uint64_t q = p + b;
        if (q >= t.io) {
            const uint64_t d = q - t.io;
            w |= ((hint_index_dword(f, t, d & ~3ull) >> (8 * (d & 3u))) & 0xffu) << (8 * b);
            continue;
        }
        while (q >= c.next && c.k + 1 < t.nk) hint_cur_load(f, t, c.k + 1, c);
        if (q >= c.o) w |= hint_item_byte(c, q - c.o) << (8 * b);
    }
    return w;
}

// A lane per 16 bytes of the file, grid-stride: the last item at or before the chunk's first byte
// by a binary search over item_off, then four dwords and one aligned 16-B store (the file's last,
// partial chunk: dwords, then at most three single bytes).  Nothing is written when the file does
// not fit out_cap; totals[8] says so.
template <class F>
__global__ void __launch_bounds__(256) k_hint_file(const F f, uint32_t cap, uint8_t *out, uint64_t out_cap,
                                                   uint32_t *totals) {
    // items and index entries never exceed the arrays' cap, whatever totals holds
    const HintTot t{totals[1] < cap ? totals[1] : cap, totals[2] < cap ? totals[2] : cap, totals[3],
                    (uint64_t)totals[4] | ((uint64_t)totals[5] << 32),
                    (uint64_t)totals[6] | ((uint64_t)totals[7] << 32)};
    const bool fits = t.fb <= out_cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[8] = f.status(totals[8], fits);
    // a file the arrays cannot describe (totals not the plan's) is cut to what they can
    if (!fits || t.nk == 0 || t.io < kHintHead || t.fb < t.io || t.fb - t.io > (uint64_t)kHintEntry * t.nidx) return;
    const uint64_t nchunks = (t.fb + 15) / 16;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < nchunks; g += (uint64_t)gridDim.x * 256) {
        const uint64_t x = 16 * g;
        uint32_t w[4];
        if (g == 0) {
            w[0] = (uint32_t)t.io, w[1] = (uint32_t)(t.io >> 32), w[2] = t.nk, w[3] = t.datasize;
        } else {
            HintCur c;
            if (x < t.io) {
                uint32_t lo = 0, hi = t.nk;  // the last item with o_k <= x (o_0 = 16 <= x)
                while (hi - lo > 1) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (f.item_off[mid] <= x) lo = mid;
                    else hi = mid;
                }
                hint_cur_load(f, t, lo, c);
            } else {
                c.k = t.nk, c.ksz = 0, c.o = t.io, c.next = t.io, c.key = nullptr;
            }
#pragma unroll
            for (uint32_t d = 0; d < 4; d++) w[d] = hint_file_dword(f, t, x + 4 * d, c);
        }
        const uint64_t left = t.fb - x;
        if (left >= 16) {
            *(uint4 *)(out + x) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (uint32_t d = 0; d < 4; d++) {
                if (4 * d + 4 <= left) *(uint32_t *)(out + x + 4 * d) = w[d];
                else
                    for (uint32_t b = 4 * d; b < left && b < 4 * d + 4; b++)
                        out[x + b] = (uint8_t)(w[d] >> (8 * (b & 3)));
            }
        }
    }
}

}  // namespace qlzx
