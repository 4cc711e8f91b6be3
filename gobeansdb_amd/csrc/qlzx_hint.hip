// qlzx_hint.hip -- the hint split file of a replayed chunk: what buildHintFromData
// (store/bucket.go:89-117) produces from the records the stream reader returns, for one chunk
// resident in device memory.  HintBuffer.Set (store/hint.go:121-161) keeps one item per
// (keyhash, key), the last Set wins, and refuses a new key once SplitCap items exist;
// HintBuffer.Dump (:181-208) sorts the items by (keyhash, key) (byKeyHash.Less, :334-352) and
// hintFileWriter (store/hintfile.go:142-212) writes head, items and the sparse index
// (store/hintindex.go:140-150).  The key hash is getKeyHashDefalut (store/key.go:41-59).
//
// Two calls, nothing read back in between:
//   plan   k_hint_hash: the guards and the key hash of every record from `first`; the valid ones
//          compacted (a scan) and radix-sorted by keyhash, stably, so equal hashes stay in append
//          order; k_hint_runs: a run of equal hash whose neighbours all carry the same key bytes
//          (versions of one key: the common case) is already in (keyhash, key, append) order;
//          a run with different keys goes to k_hint_fix, where one wave ranks it by key bytes;
//          the split's cut is the (split_cap + 1)-th first appearance of a key (a scan over the
//          records); an item is its group's last member below the cut; a u64 scan of 23 + ksz
//          gives the file offsets; the index entries are a greedy successor walk over those
//          offsets, marked by pointer doubling (as k_rp_double) and compacted by a scan;
//   write  k_hint_file: a lane per 16 bytes of the file, assembled in registers from the item
//          fields and the key bytes and stored with one aligned 16-B store.
#include <rocprim/rocprim.hpp>

#include "qlzx_recfile.h"

namespace qlzx {

constexpr uint32_t kHintHead = 16, kHintItem = 23, kHintMaxKey = 255;

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

// ---- plan ----
struct HintIn {
    const uint8_t *data;
    uint64_t size;
    const uint64_t *rec_off;
    const int32_t *hdr;
    uint32_t cap;
    __device__ __forceinline__ uint32_t key(uint32_t r, const uint8_t **k) const;
};
// The key of record r, or ksz = 0 when a guard fails (nothing past the failing check is read).
__device__ __forceinline__ uint32_t hint_key(const HintIn &in, uint32_t r, const uint8_t **key) {
    const uint32_t ksz = (uint32_t)in.hdr[6 * (size_t)r + 4];
    *key = nullptr;
    if (ksz == 0 || ksz > kHintMaxKey) return 0;
    const uint64_t off = in.rec_off[r];
    if (off > in.size || in.size - off < (uint64_t)kRpHdr + ksz) return 0;
    *key = in.data + off + kRpHdr;
    return ksz;
}
__device__ __forceinline__ uint32_t HintIn::key(uint32_t r, const uint8_t **k) const { return hint_key(*this, r, k); }
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

// t = j - first over [0, M): vf[t] = record j is in range and passes the guards, hash[t] its keyhash.
__global__ void __launch_bounds__(256) k_hint_hash(HintIn in, const uint32_t *result, const uint64_t *keyhash,
                                                   uint32_t first, uint32_t M, uint64_t *hash, uint32_t *vf) {
    const uint32_t n = rec_count(result, in.cap);
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < M; t += gridDim.x * 256) {
        const uint32_t j = first + t;
        uint32_t ok = 0;
        uint64_t h = 0;
        if (j < n) {
            const uint8_t *key;
            const uint32_t ksz = hint_key(in, j, &key);
            if (ksz) {
                ok = 1;
                h = keyhash ? keyhash[j] : hint_keyhash(key, ksz);
            }
        }
        vf[t] = ok;
        hash[t] = h;
    }
}

// The valid records first, in append order, as (keyhash, record) pairs; the other M - nv entries
// behind them with the largest key, so that the stable sort leaves them behind every record.
__global__ void __launch_bounds__(256) k_hint_compact(const uint64_t *hash, const uint32_t *vf, const uint32_t *vpos,
                                                      uint32_t first, uint32_t M, uint64_t *key_in, uint32_t *val_in,
                                                      HintCounters *cnt) {
    const uint32_t nv = vpos[M - 1] + vf[M - 1];
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < M; t += gridDim.x * 256) {
        const uint32_t p = vpos[t];
        if (vf[t]) key_in[p] = hash[t], val_in[p] = first + t;
        else key_in[nv + (t - p)] = ~0ull, val_in[nv + (t - p)] = 0xffffffffu;
        if (t == M - 1) cnt->nv = nv;
    }
}

// fl[i]: bit 0 = first of its run of equal keyhash, bit 1 = same keyhash as its predecessor but
// other key bytes (such a run is listed for k_hint_fix).  gh[i] = a group (one item) starts here,
// val_r = the records in (keyhash, key, append) order: both final for every run without bit 1.
// K names the keys: K::key(r, &bytes) = the length (qlzx_hintmerge.hip sorts hint items with it).
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

// isnew[j - first] = 1 where record j is the first appearance of its key
__global__ void __launch_bounds__(256) k_hint_first(const uint8_t *gh, const uint32_t *val_r, uint32_t first,
                                                    uint32_t M, uint32_t *isnew, const HintCounters *cnt) {
    const uint32_t nv = cnt->nv;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nv; i += gridDim.x * 256) {
        const uint32_t t = val_r[i] - first;
        if (gh[i] && t < M) isnew[t] = 1;
    }
}
// the cut: the record that would be distinct key split_cap + 1 (HintBuffer.Set returns false)
__global__ void __launch_bounds__(256) k_hint_cut(const uint32_t *isnew, const uint32_t *newpos, uint32_t first,
                                                  uint32_t M, uint32_t split_cap, HintCounters *cnt) {
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < M; t += gridDim.x * 256)
        if (isnew[t] && newpos[t] == split_cap) cnt->cut1 = first + t + 1;
}
__device__ __forceinline__ uint32_t hint_cut(const HintCounters *cnt, uint32_t n) {
    return cnt->cut1 ? cnt->cut1 - 1 : n;
}

// Sorted position i carries an item iff its record is its group's last below the cut; every record
// below the cut, overwritten or not, raises datasize (store/hint.go:156-159).
__global__ void __launch_bounds__(256) k_hint_items(HintIn in, const uint32_t *result, const uint8_t *gh,
                                                    const uint32_t *val_r, uint32_t M, HintAcc *itemv,
                                                    HintCounters *cnt) {
    const uint32_t n = rec_count(result, in.cap), nv = cnt->nv, c = hint_cut(cnt, n);
    uint32_t dmax = 0, nbelow = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        HintAcc v{0, 0};
        if (i < nv) {
            const uint32_t r = val_r[i];
            if (r < c) {
                const uint32_t ksz = (uint32_t)in.hdr[6 * (size_t)r + 4], vsz = (uint32_t)in.hdr[6 * (size_t)r + 5];
                const uint32_t end = (uint32_t)in.rec_off[r] + (uint32_t)pad256((uint64_t)kRpHdr + ksz + vsz);
                dmax = max(dmax, end);
                nbelow++;
                if (i + 1 == nv || gh[i + 1] || val_r[i + 1] >= c) v = HintAcc{kHintItem + ksz, 1};
            }
        }
        itemv[i] = v;
    }
    for (int m = 32; m >= 1; m >>= 1) dmax = max(dmax, (uint32_t)__shfl_xor(dmax, m, 64));
    nbelow = wave_sum(nbelow);
    if ((threadIdx.x & 63) == 0 && nbelow) {
        atomicMax(&cnt->datasize, dmax);
        atomicAdd(&cnt->nbelow, nbelow);
    }
}

__global__ void __launch_bounds__(256) k_hint_emit(const HintAcc *itemv, const HintAcc *items, const uint64_t *key_s,
                                                   const uint32_t *val_r, uint32_t M, uint32_t *item_rec,
                                                   uint64_t *item_hash, uint64_t *item_off, HintCounters *cnt) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const HintAcc v = itemv[i], x = items[i];
        if (v.c) {
            item_rec[x.c] = val_r[i];
            item_hash[x.c] = key_s[i];
            item_off[x.c] = kHintHead + x.b;
        }
        if (i == M - 1) cnt->nk = (uint32_t)(x.c + v.c), cnt->ibytes = x.b + v.b;
    }
}

// The index (store/hintfile.go:174-176): from `last`, the next entry is the first item k with
// o_k - last > thr.  J[k] = the entry after item k (nk = none), r0 = the first one (last = 0).
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

__global__ void k_hint_totals(const uint64_t *rec_off, const uint32_t *result, uint32_t cap, uint32_t first,
                              uint32_t max_offset_in, uint32_t *totals, const HintCounters *cnt) {
    const uint32_t n = rec_count(result, cap);
    uint32_t consumed = 0, skipped = 0, nk = 0, nidx = 0, datasize = max_offset_in;
    uint64_t io = kHintHead;
    if (cnt) {  // cnt == nullptr: no record in range
        const uint32_t c = hint_cut(cnt, n);
        consumed = c > first ? c - first : 0;
        skipped = consumed - cnt->nbelow;
        nk = cnt->nk, nidx = cnt->nidx;
        datasize = max(datasize, cnt->datasize);
        if (cnt->cut1) datasize = max(datasize, (uint32_t)rec_off[c]);  // store/hint.go:143-145
        io += cnt->ibytes;
    }
    const uint64_t fb = nk ? io + 16ull * nidx : 0;
    totals[0] = consumed, totals[1] = nk, totals[2] = nidx, totals[3] = datasize;
    totals[4] = (uint32_t)io, totals[5] = (uint32_t)(io >> 32);
    totals[6] = (uint32_t)fb, totals[7] = (uint32_t)(fb >> 32);
    totals[8] = 0, totals[9] = skipped;
}

// ---- write ----
struct HintFile {
    HintIn in;
    const uint16_t *vhash;
    const uint32_t *item_rec, *index_item;
    const uint64_t *item_hash, *item_off;
    uint32_t chunk_id;
    // totals[8] after the write: whether the file fits is all this writer reports
    __device__ __forceinline__ uint32_t status(uint32_t, bool fits) const { return fits ? 0u : 1u; }
};
struct HintTot {  // the plan's totals: items, index entries, datasize, indexOffset, file bytes
    uint32_t nk, nidx, datasize;
    uint64_t io, fb;
};
// One item's 23 header bytes as dwords (h0 .. h5; a zero dword pads the funnel shift) and its key; whatever the
// plan arrays hold, every read stays inside the arrays' cap entries and the key inside `data`.
struct HintCur {
    uint32_t k, ksz;
    uint64_t o, next;
    uint32_t h0, h1, h2, h3, h4, h5;
    const uint8_t *key;
};
__device__ __forceinline__ void hint_cur_load(const HintFile &f, const HintTot &t, uint32_t k, HintCur &c) {
    c.k = k;
    c.o = f.item_off[k];
    c.next = k + 1 < t.nk ? f.item_off[k + 1] : t.io;
    const uint32_t r = f.item_rec[k];
    const uint64_t kh = f.item_hash[k];
    c.ksz = 0, c.key = nullptr;
    c.h0 = (uint32_t)kh, c.h1 = (uint32_t)(kh >> 32), c.h2 = f.chunk_id;
    c.h3 = 0, c.h4 = 0, c.h5 = 0;
    if (r < f.in.cap) {
        c.ksz = hint_key(f.in, r, &c.key);
        c.h3 = (uint32_t)f.in.rec_off[r];
        c.h4 = (uint32_t)f.in.hdr[6 * (size_t)r + 3];
        c.h5 = (uint32_t)f.vhash[r] | (c.ksz << 16);
    }
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
// multiple of 4 (an entry is 16 bytes: a dword lies inside the index or past its end).
__device__ __forceinline__ uint32_t hint_index_dword(const HintFile &f, const HintTot &t, uint64_t d) {
    if (d >= t.fb - t.io) return 0;
    const uint32_t k = f.index_item[d >> 4], r = (uint32_t)d & 15u;
    const uint64_t x = k < t.nk ? (r < 8 ? f.item_hash[k] : f.item_off[k]) : 0;
    return (uint32_t)(x >> (8 * (r & 4)));
}
// The file's dword at byte position p >= 16 (bytes past the file's end come out as zeros).  F is
// HintFile or another source of items with its own hint_cur_load and hint_index_dword.
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
        if (rel >= kHintItem && rel - kHintItem + 4 <= c.ksz) {
            uint32_t w;
            __builtin_memcpy(&w, c.key + (rel - kHintItem), 4);
            return w;
        }
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
    const HintTot t{totals[1] < cap ? totals[1] : cap, totals[2] < cap ? totals[2] : cap, totals[3],
                    (uint64_t)totals[4] | ((uint64_t)totals[5] << 32),
                    (uint64_t)totals[6] | ((uint64_t)totals[7] << 32)};
    const bool fits = t.fb <= out_cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[8] = f.status(totals[8], fits);
    // a file the arrays cannot describe (totals not the plan's) is cut to what they can
    if (!fits || t.nk == 0 || t.io < kHintHead || t.fb < t.io || t.fb - t.io > 16ull * t.nidx) return;
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

// ---- workspace: the counters, the sort's pairs, the flags and their scans, rocPRIM's temporary ----
struct HintWs {
    HintCounters *cnt;
    uint64_t *hash, *key_in, *key_s;  // hash ‖ key_in are reused as itemv once the sort is done
    HintAcc *itemv, *items;
    uint32_t *val_in, *val_s, *val_r, *list, *fa, *fb;  // fa / fb: a flag array and its scan, three times
    uint8_t *fl, *gh;
    void *tmp;
    size_t tmp_bytes;
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
inline size_t hint_ws_layout(uint32_t cap, uint8_t *base, HintWs *w) {
    const size_t m = (size_t)cap + 2;
    const size_t tmp_bytes = hint_tmp_bytes((size_t)cap + 1);  // the calls take cap - first and one more
    WsCarver c{base};
    HintWs t;
    t.cnt = c.take<HintCounters>(sizeof(HintCounters));
    t.hash = c.take<uint64_t>(16 * m);
    t.key_in = t.hash ? t.hash + m : nullptr;
    t.itemv = (HintAcc *)t.hash;
    t.items = c.take<HintAcc>(16 * m);
    t.key_s = c.take<uint64_t>(8 * m);
    t.val_in = c.take<uint32_t>(4 * m);
    t.val_s = c.take<uint32_t>(4 * m);
    t.val_r = c.take<uint32_t>(4 * m);
    t.list = c.take<uint32_t>(4 * m);
    t.fa = c.take<uint32_t>(4 * m);
    t.fb = c.take<uint32_t>(4 * m);
    t.fl = c.take(m);
    t.gh = c.take(m);
    t.tmp_bytes = tmp_bytes;
    t.tmp = c.take(t.tmp_bytes);
    if (w) *w = t;
    return c.bytes();
}

inline int launch_hint_plan(const HintIn &in, const uint32_t *result, const uint64_t *keyhash, uint32_t first,
                            uint32_t split_cap, int64_t index_interval, uint32_t max_offset_in, uint32_t *item_rec,
                            uint64_t *item_hash, uint64_t *item_off, uint32_t *index_item, uint32_t *totals, void *ws,
                            hipStream_t s) {
    if (first >= in.cap) {  // no record in range, whatever result[0] says
        hipLaunchKernelGGL(k_hint_totals, dim3(1), dim3(1), 0, s, in.rec_off, result, in.cap, first, max_offset_in,
                           totals, (const HintCounters *)nullptr);
        return (int)hipGetLastError();
    }
    HintWs w;
    hint_ws_layout(in.cap, (uint8_t *)ws, &w);
    const uint32_t M = in.cap - first;
    const dim3 G(grid_for((uint64_t)M + 1, 256, 2048)), B(256);
    hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(HintCounters), s);
    if (e != hipSuccess) return (int)e;
    size_t tb;
    auto scan32 = [&](size_t n) {
        tb = w.tmp_bytes;
        return rocprim::exclusive_scan(w.tmp, tb, (const uint32_t *)w.fa, w.fb, 0u, n, rocprim::plus<uint32_t>(), s);
    };
    // valid records and their hashes, compacted, sorted by keyhash (stable: append order inside a run)
    hipLaunchKernelGGL(k_hint_hash, G, B, 0, s, in, result, keyhash, first, M, w.hash, w.fa);
    if ((e = scan32(M)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_compact, G, B, 0, s, (const uint64_t *)w.hash, (const uint32_t *)w.fa,
                       (const uint32_t *)w.fb, first, M, w.key_in, w.val_in, w.cnt);
    tb = w.tmp_bytes;
    e = rocprim::radix_sort_pairs(w.tmp, tb, (const uint64_t *)w.key_in, w.key_s, (const uint32_t *)w.val_in, w.val_s,
                                  (size_t)M, 0, 64, s);
    if (e != hipSuccess) return (int)e;
    // (keyhash, key, append) order and the groups
    hipLaunchKernelGGL(k_hint_runs<HintIn>, G, B, 0, s, in, (const uint64_t *)w.key_s, (const uint32_t *)w.val_s, w.fl, w.gh,
                       w.val_r, w.list, w.cnt);
    hipLaunchKernelGGL(k_hint_fix<HintIn>, dim3(1024), B, 0, s, in, (const uint32_t *)w.val_s, (const uint8_t *)w.fl, w.gh,
                       w.val_r, (const uint32_t *)w.list, (const HintCounters *)w.cnt);
    // the cut
    if ((e = hipMemsetAsync(w.fa, 0, 4 * (size_t)M, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_first, G, B, 0, s, (const uint8_t *)w.gh, (const uint32_t *)w.val_r, first, M, w.fa,
                       (const HintCounters *)w.cnt);
    if ((e = scan32(M)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_cut, G, B, 0, s, (const uint32_t *)w.fa, (const uint32_t *)w.fb, first, M, split_cap,
                       w.cnt);
    // the items and their file offsets
    hipLaunchKernelGGL(k_hint_items, G, B, 0, s, in, result, (const uint8_t *)w.gh, (const uint32_t *)w.val_r, M,
                       w.itemv, w.cnt);
    tb = w.tmp_bytes;
    e = rocprim::exclusive_scan(w.tmp, tb, (const HintAcc *)w.itemv, w.items, HintAcc{0, 0}, (size_t)M, HintAccPlus(),
                                s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_emit, G, B, 0, s, (const HintAcc *)w.itemv, (const HintAcc *)w.items,
                       (const uint64_t *)w.key_s, (const uint32_t *)w.val_r, M, item_rec, item_hash, item_off, w.cnt);
    // the index entries: successors, the walk from the first one by pointer doubling, compaction
    const int64_t thr = (int64_t)((uint64_t)index_interval - kHintItem - 256);
    uint32_t *J = w.val_in, *J2 = w.val_s;
    hipLaunchKernelGGL(k_hint_next, G, B, 0, s, (const uint64_t *)item_off, thr, M, J, w.fa, w.cnt);
    hipLaunchKernelGGL(k_hint_seed, dim3(1), dim3(1), 0, s, (const HintCounters *)w.cnt, w.fa);
    for (uint64_t reach = 1; reach < (uint64_t)M + 1; reach <<= 1) {
        hipLaunchKernelGGL(k_hint_double, G, B, 0, s, (const HintCounters *)w.cnt, (const uint32_t *)J, J2, w.fa);
        std::swap(J, J2);
    }
    if ((e = scan32((size_t)M + 1)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_index, G, B, 0, s, (const uint32_t *)w.fa, (const uint32_t *)w.fb, index_item, w.cnt);
    hipLaunchKernelGGL(k_hint_totals, dim3(1), dim3(1), 0, s, in.rec_off, result, in.cap, first, max_offset_in, totals,
                       (const HintCounters *)w.cnt);
    return (int)hipGetLastError();
}

inline int launch_hint_write(const HintFile &f, uint8_t *out, uint64_t out_cap, uint32_t *totals, hipStream_t s) {
    // 16 + 289 (n - first) bytes at the most: 23 + 250 of an item and 16 of its index entry
    const uint64_t chunks = ((uint64_t)kHintHead + 289ull * f.in.cap + 15) / 16;
    hipLaunchKernelGGL(k_hint_file<HintFile>, dim3(grid_for(chunks, 256, 2048)), dim3(256), 0, s, f, f.in.cap, out, out_cap, totals);
    return (int)hipGetLastError();
}

}  // namespace qlzx
