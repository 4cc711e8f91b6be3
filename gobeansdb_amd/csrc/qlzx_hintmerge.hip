// qlzx_hintmerge.hip -- the merged hint file and the collision items of a bucket:
// what hintMgr.Merge (store/hint.go:455-508) -> merge (store/hintmerge.go:96-159) produces from the
// bucket's split files, for files resident in device memory.  The reference pops a heap keyed
// (keyhash, key, CmpKey) over one hintFileReader per source; mergeWriter keeps, per keyhash, the
// last item of every distinct key, hands runs with two or more keys to the collision table and
// writes the rest through hintFileWriter.  For sources that ascend strictly by (keyhash, key) that
// is: one item per distinct (keyhash, key), the one with the largest CmpKey, in (keyhash, key)
// order.  A source that does not ascend is refused.
//
// The format with its loads and the reader's rule (hint_next), the sort's workspace tail, the
// run / fix kernels, the index pass and the file writer are qlzx_hint_fmt.h's; the source heads,
// stretches and walks are qlzx_hint_walk.h's (qlzx_htree.hip reads its sources the same way); this
// file owns the two sort keys, the collision flags, winners, emit and
// totals, the writer's source of items (HmFile), the workspace layout and the two launchers.
//
// Two calls, nothing read back in between:
//   plan   launch_hm_walk (qlzx_hint_walk.h).  k_hm_head: every source's head.  The item starts of a source are a serial chain (ksz
//          sits at byte 22 of an item), so a source is cut into stretches at the entries of its own
//          sparse index, one lane per stretch: k_hm_count walks a stretch and must land exactly on
//          the next entry (the last one on indexOffset); entries that are not strictly increasing
//          inside [16, indexOffset), or a walk that misses, leave the source unproven, and
//          k_hm_settle then walks it from 16 with one lane (as a source without an index is
//          walked): correct, not fast.  A scan of the counts, k_hm_fill walks again and writes
//          every item's position and source; k_hm_sorted compares neighbours of one source.
//          Then the item numbers are sorted by CmpKey and, stably, by keyhash: a run of equal hash
//          is in position order and k_hint_runs / k_hint_fix's "last of its group wins" applies.
//   write  k_hint_file over HmFile: an item's 23 bytes come from its source with the chunk replaced.
#include "qlzx_hint_walk.h"

namespace qlzx {

// The key of item r: pos[r] is an item k_hm_fill found whole inside its file.
struct HmKey {
    const uint8_t *hints;
    const uint64_t *pos;
    uint32_t cap;
    __device__ __forceinline__ uint32_t key(uint32_t r, const uint8_t **k) const {
        *k = nullptr;
        if (r >= cap) return 0;
        const uint8_t *p = hints + pos[r];
        *k = p + kHintItem;
        return p[kItemKsz];
    }
};

// HintBuffer.Dump and merge write strictly ascending files; the sequential merge of anything else
// depends on the order of its steps.
__global__ void __launch_bounds__(256) k_hm_sorted(HmKey K, const uint32_t *sid, HmCounters *hm) {
    if (hm->status != QLZX_HM_OK) return;
    const uint32_t N = (uint32_t)hm->n;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x + 1; k < N; k += gridDim.x * 256) {
        if (sid[k] != sid[k - 1]) continue;
        const uint64_t ha = hint_ld64(K.hints + K.pos[k - 1]), hb = hint_ld64(K.hints + K.pos[k]);
        bool asc = ha < hb;
        if (ha == hb) {
            const uint8_t *a, *b;
            const uint32_t na = K.key(k - 1, &a), nb = K.key(k, &b);
            asc = hint_key_cmp(a, na, b, nb) < 0;
        }
        if (!asc) atomicMax(&hm->uns_inv, ~sid[k]);
    }
}
// The first sort's pairs (CmpKey, item); behind the nv items the largest key, which a stable sort
// leaves behind every item.  The final status and nv (0 with any status) are settled here.
__global__ void __launch_bounds__(256) k_hm_cmpkey(HmIn in, const uint64_t *pos, const uint32_t *sid, uint64_t *key_in,
                                                   uint32_t *val_in, HintCounters *cnt, HmCounters *hm) {
    const uint32_t status = hm->status == QLZX_HM_OK && hm->uns_inv ? (uint32_t)QLZX_HM_UNSORTED : hm->status;
    const uint32_t nv = status == QLZX_HM_OK ? (uint32_t)hm->n : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt->nv = nv, hm->fin = status;
        if (status == QLZX_HM_UNSORTED) hm->src = ~hm->uns_inv;
    }
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < in.cap; k += gridDim.x * 256) {
        const bool v = k < nv;
        key_in[k] = v ? ((uint64_t)in.file_chunk[sid[k]] << 32) | hint_ld32(in.hints + pos[k] + kItemOffset) : ~0ull;
        val_in[k] = v ? k : 0xffffffffu;
    }
}
__global__ void __launch_bounds__(256) k_hm_hashkey(HmIn in, const uint64_t *pos, const uint32_t *val_s,
                                                    uint64_t *key_in, const HintCounters *cnt) {
    const uint32_t nv = cnt->nv;
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < in.cap; j += gridDim.x * 256) {
        const uint32_t r = val_s[j];
        key_in[j] = j < nv && r < in.cap ? hint_ld64(in.hints + pos[r]) : ~0ull;
    }
}
// cf[i] = a second or later key of its keyhash starts at sorted position i (mergeWriter.write's
// num += 1): a run with such a position is a collision (flush, num > 1).
__global__ void __launch_bounds__(256) k_hm_cflag(const uint64_t *key_s, const uint8_t *gh, uint32_t cap, uint32_t *cf,
                                                  const HintCounters *cnt) {
    const uint32_t nv = cnt->nv;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= cap; i += gridDim.x * 256)
        cf[i] = i > 0 && i < nv && gh[i] && key_s[i] == key_s[i - 1];
}
// Sorted position i carries a merged item iff it is its group's last; cw[i] = it is a collision
// item (cfs = the scan of cf: a run [s, e) of one keyhash holds cfs[e] - cfs[s] later keys).
__global__ void __launch_bounds__(256) k_hm_winners(HmKey K, const uint64_t *key_s, const uint8_t *gh,
                                                    const uint32_t *val_r, const uint32_t *cfs, uint32_t *cw,
                                                    HintAcc *itemv, const HintCounters *cnt) {
    const uint32_t nv = cnt->nv;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < K.cap; i += gridDim.x * 256) {
        HintAcc v{0, 0};
        uint32_t c = 0;
        if (i < nv && (i + 1 == nv || gh[i + 1])) {
            const uint8_t *key;
            v = HintAcc{kHintItem + K.key(val_r[i], &key), 1};
            const uint64_t h = key_s[i];
            uint32_t lo = 0, hi = i;  // s: the first position with key_s >= h
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (key_s[mid] < h) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t s = lo;
            lo = i + 1, hi = nv;  // e: the first position with key_s > h
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (key_s[mid] <= h) lo = mid + 1;
                else hi = mid;
            }
            c = cfs[lo] != cfs[s];
        }
        itemv[i] = v;
        cw[i] = c;
    }
}
__global__ void __launch_bounds__(256) k_hm_emit(HmIn in, const uint64_t *pos, const uint32_t *sid,
                                                 const HintAcc *itemv, const HintAcc *items, const uint32_t *val_r,
                                                 const uint32_t *cw, const uint32_t *cws, uint64_t *item_src,
                                                 uint32_t *item_chunk, uint64_t *item_off, uint32_t *coll_item,
                                                 HintCounters *cnt, HmCounters *hm) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < in.cap; i += gridDim.x * 256) {
        const HintAcc v = itemv[i], x = items[i];
        const uint32_t r = val_r[i];
        if (v.c && x.c < in.cap && r < in.cap) {
            item_src[x.c] = pos[r];
            item_chunk[x.c] = in.file_chunk[sid[r]];
            item_off[x.c] = kHintHead + x.b;
            if (cw[i] && cws[i] < in.cap) coll_item[cws[i]] = (uint32_t)x.c;
        }
        if (i == in.cap - 1) {
            cnt->nk = (uint32_t)(x.c + v.c), cnt->ibytes = x.b + v.b;
            hm->ncoll = cws[i] + cw[i];
        }
    }
}
__global__ void k_hm_totals(uint32_t *totals, const HintCounters *cnt, const HmCounters *hm) {
    const bool ok = hm->fin == QLZX_HM_OK;
    const uint32_t nk = ok ? cnt->nk : 0u, nidx = ok ? cnt->nidx : 0u;
    const uint64_t io = kHintHead + (ok ? cnt->ibytes : 0ull), fb = nk ? io + (uint64_t)kHintEntry * nidx : 0;
    totals[0] = (uint32_t)(hm->n < 0xffffffffull ? hm->n : 0xffffffffull);
    totals[1] = nk, totals[2] = nidx, totals[3] = cnt->datasize;
    totals[4] = (uint32_t)io, totals[5] = (uint32_t)(io >> 32);
    totals[6] = (uint32_t)fb, totals[7] = (uint32_t)(fb >> 32);
    totals[8] = hm->fin, totals[9] = hm->src;
    totals[10] = ok ? hm->ncoll : 0u, totals[11] = 0;
}

// ---- write: k_hint_file's items come from the sources ----
struct HmFile {
    const uint8_t *hints;
    uint64_t bytes;
    const uint64_t *item_src, *item_off;
    const uint32_t *item_chunk, *index_item;
    // the plan's verdict stays; otherwise whether the file fits (QLZX_HM_NO_SPACE)
    __device__ __forceinline__ uint32_t status(uint32_t prev, bool fits) const {
        return prev > QLZX_HM_NO_SPACE ? prev : fits ? (uint32_t)QLZX_HM_OK : (uint32_t)QLZX_HM_NO_SPACE;
    }
    // item k's source bytes, or nullptr when item_src[k] (not the plan's) leaves no whole item head
    __device__ __forceinline__ const uint8_t *item(uint32_t k) const {
        const uint64_t o = item_src[k];
        return o <= bytes && bytes - o >= kHintItem ? hints + o : nullptr;
    }
    __device__ __forceinline__ uint64_t keyhash(uint32_t k) const {
        const uint8_t *p = item(k);
        return p ? hint_ld64(p) : 0;
    }
    // the source's 23 bytes with the chunk replaced; the key only when it lies inside `hints`
    __device__ __forceinline__ void head(uint32_t k, HintCur &c) const {
        c.h2 = item_chunk[k];
        if (const uint8_t *p = item(k)) {
            c.h0 = hint_ld32(p), c.h1 = hint_ld32(p + 4), c.h3 = hint_ld32(p + kItemOffset), c.h4 = hint_ld32(p + kItemVer);
            c.h5 = (uint32_t)p[kItemVhash] | ((uint32_t)p[kItemVhash + 1] << 8) | ((uint32_t)p[kItemKsz] << 16);
            if (bytes - (uint64_t)(p - hints) - kHintItem >= p[kItemKsz]) c.ksz = p[kItemKsz], c.key = p + kHintItem;
        }
    }
};

// ---- workspace: the counters, the sources, the stretches, the items' positions, the sort's tail ----
// a / b: stretch counts and their scan; then key_in (a's second half) and itemv / items
struct HmWs : HintSortWs, HmWalkWs {};
inline size_t hm_ws_layout(uint32_t n_files, uint32_t cap, uint8_t *base, HmWs *w) {
    const size_t m = (size_t)cap + 2, sm = (size_t)cap + n_files + 2;
    WsCarver c{base};
    HmWs t;
    t.cnt = c.take<HintCounters>(sizeof(HintCounters));
    t.hm = c.take<HmCounters>(sizeof(HmCounters));
    t.src = c.take<HmSrc>(sizeof(HmSrc) * (size_t)n_files);
    t.unproven = c.take<uint32_t>(4 * (size_t)n_files);
    t.sv = c.take<HintAcc>(16 * (size_t)n_files);
    t.sb = c.take<HintAcc>(16 * (size_t)n_files);
    t.a = c.take<HintAcc>(16 * sm);
    t.b = c.take<HintAcc>(16 * sm);
    t.pos = c.take<uint64_t>(8 * m);
    t.sid = c.take<uint32_t>(4 * m);
    t.carve(c, m, t.a, std::max(hint_tmp_bytes(sm), hint_tmp_bytes(n_files)));
    if (w) *w = t;
    return c.bytes();
}

inline int launch_hm_plan(const HmIn &in, int64_t index_interval, uint64_t *item_src, uint32_t *item_chunk,
                          uint64_t *item_off, uint32_t *index_item, uint32_t *coll_item, uint32_t *totals, void *ws,
                          hipStream_t s) {
    HmWs w;
    hm_ws_layout(in.n_files, in.cap, (uint8_t *)ws, &w);
    const uint32_t M = in.cap;
    const dim3 G(grid_for((uint64_t)M + 1, 256, 2048)), B(256);
    hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(HintCounters), s);
    if (e != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(w.hm, 0, sizeof(HmCounters), s)) != hipSuccess) return (int)e;
    // the sources' items: heads, stretches, counts, positions
    const auto acc_scan = [&](const HintAcc *from, HintAcc *to, size_t n) { return w.scan(from, to, n, HintAccPlus(), s); };
    if ((e = launch_hm_walk<false>(in, w, acc_scan, s)) != hipSuccess) return (int)e;
    const HmKey K{in.hints, w.pos, in.cap};
    hipLaunchKernelGGL(k_hm_sorted, G, B, 0, s, K, (const uint32_t *)w.sid, w.hm);
    // by CmpKey, then stably by keyhash: a run of equal hash is in position order
    hipLaunchKernelGGL(k_hm_cmpkey, G, B, 0, s, in, (const uint64_t *)w.pos, (const uint32_t *)w.sid, w.key_in, w.val_in,
                       w.cnt, w.hm);
    if ((e = w.sort(w.val_in, w.val_s, M, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hm_hashkey, G, B, 0, s, in, (const uint64_t *)w.pos, (const uint32_t *)w.val_s, w.key_in,
                       (const HintCounters *)w.cnt);
    if ((e = w.sort(w.val_s, w.val_in, M, s)) != hipSuccess) return (int)e;
    // (keyhash, key, position) order and the groups
    hipLaunchKernelGGL(k_hint_runs<HmKey>, G, B, 0, s, K, (const uint64_t *)w.key_s, (const uint32_t *)w.val_in, w.fl,
                       w.gh, w.val_r, w.list, w.cnt);
    hipLaunchKernelGGL(k_hint_fix<HmKey>, dim3(1024), B, 0, s, K, (const uint32_t *)w.val_in, (const uint8_t *)w.fl,
                       w.gh, w.val_r, (const uint32_t *)w.list, (const HintCounters *)w.cnt);
    // the merged items, the collision items among them, the file offsets
    hipLaunchKernelGGL(k_hm_cflag, G, B, 0, s, (const uint64_t *)w.key_s, (const uint8_t *)w.gh, M, w.fa,
                       (const HintCounters *)w.cnt);
    if ((e = w.scan(w.fa, w.fb, (size_t)M + 1, rocprim::plus<uint32_t>(), s)) != hipSuccess) return (int)e;
    HintAcc *itemv = w.a, *items = w.b;
    hipLaunchKernelGGL(k_hm_winners, G, B, 0, s, K, (const uint64_t *)w.key_s, (const uint8_t *)w.gh,
                       (const uint32_t *)w.val_r, (const uint32_t *)w.fb, w.fa, itemv, (const HintCounters *)w.cnt);
    if ((e = w.scan(w.fa, w.fb, M, rocprim::plus<uint32_t>(), s)) != hipSuccess) return (int)e;
    if ((e = w.scan(itemv, items, M, HintAccPlus(), s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hm_emit, G, B, 0, s, in, (const uint64_t *)w.pos, (const uint32_t *)w.sid,
                       (const HintAcc *)itemv, (const HintAcc *)items, (const uint32_t *)w.val_r,
                       (const uint32_t *)w.fa, (const uint32_t *)w.fb, item_src, item_chunk, item_off, coll_item, w.cnt,
                       w.hm);
    // the index entries
    if ((e = launch_hint_index(item_off, index_interval, M, w, w.cnt, index_item, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hm_totals, dim3(1), dim3(1), 0, s, totals, (const HintCounters *)w.cnt,
                       (const HmCounters *)w.hm);
    return (int)hipGetLastError();
}

inline int launch_hm_write(const HmFile &f, uint32_t cap, uint8_t *out, uint64_t out_cap, uint32_t *totals,
                           hipStream_t s) {
    // a file that fits has at most out_cap / 16 + 1 chunks
    hipLaunchKernelGGL(k_hint_file<HmFile>, dim3(std::max(grid_for(out_cap / 16 + 1, 256, 2048), 1u)), dim3(256), 0, s,
                       f, cap, out, out_cap, totals);
    return (int)hipGetLastError();
}

}  // namespace qlzx
