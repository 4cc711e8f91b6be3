// qlzx_hint.hip -- the hint split file of a replayed chunk: what buildHintFromData
// (store/bucket.go:89-117) produces from the records the stream reader returns, for one chunk
// resident in device memory.  HintBuffer.Set (store/hint.go:121-161) keeps one item per
// (keyhash, key), the last Set wins, and refuses a new key once SplitCap items exist;
// HintBuffer.Dump (:181-208) sorts the items by (keyhash, key) (byKeyHash.Less, :334-352) and
// hintFileWriter (store/hintfile.go:142-212) writes head, items and the sparse index
// (store/hintindex.go:140-150).  The key hash is getKeyHashDefalut (store/key.go:41-59).
//
// The sort's workspace tail, the run / fix kernels, the index pass and the file writer are
// qlzx_hint_fmt.h's; this file owns the source of keys over a replay's records (HintIn), the plan
// kernels from k_hint_hash to k_hint_emit and k_hint_totals, the writer's source of items (HintFile),
// the workspace layout and the two launchers.
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
#include "qlzx_hint_fmt.h"

namespace qlzx {

// ---- plan ----
struct HintIn {
    const uint8_t *data;
    uint64_t size;
    const uint64_t *rec_off;
    const int32_t *hdr;
    uint32_t cap;
    // The key of record r, or ksz = 0 when a guard fails (nothing past the failing check is read).
    __device__ __forceinline__ uint32_t key(uint32_t r, const uint8_t **key) const {
        const uint32_t ksz = (uint32_t)hdr[6 * (size_t)r + 4];
        *key = nullptr;
        if (ksz == 0 || ksz > kHintMaxKey) return 0;
        const uint64_t off = rec_off[r];
        if (off > size || size - off < (uint64_t)kRpHdr + ksz) return 0;
        *key = data + off + kRpHdr;
        return ksz;
    }
};

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
            const uint32_t ksz = in.key(j, &key);
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
    const uint64_t fb = nk ? io + (uint64_t)kHintEntry * nidx : 0;
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
    __device__ __forceinline__ uint64_t keyhash(uint32_t k) const { return item_hash[k]; }
    // item_rec[k] may be any number: a record past the arrays' cap leaves position, version, vhash and key empty
    __device__ __forceinline__ void head(uint32_t k, HintCur &c) const {
        const uint32_t r = item_rec[k];
        const uint64_t kh = item_hash[k];
        c.h0 = (uint32_t)kh, c.h1 = (uint32_t)(kh >> 32), c.h2 = chunk_id;
        if (r < in.cap) {
            c.ksz = in.key(r, &c.key);
            c.h3 = (uint32_t)in.rec_off[r];
            c.h4 = (uint32_t)in.hdr[6 * (size_t)r + 3];
            c.h5 = (uint32_t)vhash[r] | (c.ksz << 16);
        }
    }
};

// ---- workspace: the counters, the hashes and the (bytes, items) pairs, the sort's tail ----
struct HintWs : HintSortWs {
    HintCounters *cnt;
    uint64_t *hash;  // hash ‖ key_in are reused as itemv once the sort is done
    HintAcc *itemv, *items;
};
inline size_t hint_ws_layout(uint32_t cap, uint8_t *base, HintWs *w) {
    const size_t m = (size_t)cap + 2;
    WsCarver c{base};
    HintWs t;
    t.cnt = c.take<HintCounters>(sizeof(HintCounters));
    t.itemv = c.take<HintAcc>(16 * m);
    t.hash = (uint64_t *)t.itemv;
    t.items = c.take<HintAcc>(16 * m);
    t.carve(c, m, t.itemv, hint_tmp_bytes((size_t)cap + 1));  // the calls take cap - first and one more
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
    // valid records and their hashes, compacted, sorted by keyhash (stable: append order inside a run)
    hipLaunchKernelGGL(k_hint_hash, G, B, 0, s, in, result, keyhash, first, M, w.hash, w.fa);
    if ((e = w.scan(w.fa, w.fb, M, rocprim::plus<uint32_t>(), s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_compact, G, B, 0, s, (const uint64_t *)w.hash, (const uint32_t *)w.fa,
                       (const uint32_t *)w.fb, first, M, w.key_in, w.val_in, w.cnt);
    if ((e = w.sort(w.val_in, w.val_s, M, s)) != hipSuccess) return (int)e;
    // (keyhash, key, append) order and the groups
    hipLaunchKernelGGL(k_hint_runs<HintIn>, G, B, 0, s, in, (const uint64_t *)w.key_s, (const uint32_t *)w.val_s, w.fl, w.gh,
                       w.val_r, w.list, w.cnt);
    hipLaunchKernelGGL(k_hint_fix<HintIn>, dim3(1024), B, 0, s, in, (const uint32_t *)w.val_s, (const uint8_t *)w.fl, w.gh,
                       w.val_r, (const uint32_t *)w.list, (const HintCounters *)w.cnt);
    // the cut
    if ((e = hipMemsetAsync(w.fa, 0, 4 * (size_t)M, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_first, G, B, 0, s, (const uint8_t *)w.gh, (const uint32_t *)w.val_r, first, M, w.fa,
                       (const HintCounters *)w.cnt);
    if ((e = w.scan(w.fa, w.fb, M, rocprim::plus<uint32_t>(), s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_cut, G, B, 0, s, (const uint32_t *)w.fa, (const uint32_t *)w.fb, first, M, split_cap,
                       w.cnt);
    // the items and their file offsets
    hipLaunchKernelGGL(k_hint_items, G, B, 0, s, in, result, (const uint8_t *)w.gh, (const uint32_t *)w.val_r, M,
                       w.itemv, w.cnt);
    if ((e = w.scan(w.itemv, w.items, M, HintAccPlus(), s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hint_emit, G, B, 0, s, (const HintAcc *)w.itemv, (const HintAcc *)w.items,
                       (const uint64_t *)w.key_s, (const uint32_t *)w.val_r, M, item_rec, item_hash, item_off, w.cnt);
    // the index entries
    if ((e = launch_hint_index(item_off, index_interval, M, w, w.cnt, index_item, s)) != hipSuccess) return (int)e;
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
