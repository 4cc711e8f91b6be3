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
// run / fix kernels, the index pass and the file writer are qlzx_hint_fmt.h's; this file owns the
// source heads, stretches and walks, the two sort keys, the collision flags, winners, emit and
// totals, the writer's source of items (HmFile), the workspace layout and the two launchers.
//
// Two calls, nothing read back in between:
//   plan   k_hm_head: every source's head.  The item starts of a source are a serial chain (ksz
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
#include "qlzx_hint_fmt.h"

namespace qlzx {

struct HmIn {
    const uint8_t *hints;
    uint64_t bytes;
    const uint64_t *file_off, *file_len;
    const uint32_t *file_chunk;
    uint32_t n_files, cap;
};
struct HmSrc {  // a source after k_hm_head: io = where its items end, ne = the index entries to prove
    uint64_t off, len, io;
    uint32_t ne, bad;
};
struct HmCounters {
    unsigned long long n;             // the items the sources hold
    uint32_t bad_inv, uns_inv;        // ~(the lowest bad / unsorted source), 0 = none
    uint32_t status, fin, src, ncoll;  // status: after k_hm_fill; fin: the plan's verdict
};

// hintFileReader.open (store/hintfile.go:57-87).  A source that cannot yield an item is bad.
__global__ void __launch_bounds__(256) k_hm_head(HmIn in, HmSrc *src, uint32_t *unproven, HintAcc *sv,
                                                 HintCounters *cnt, HmCounters *hm) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < in.n_files; i += gridDim.x * 256) {
        HmSrc s{in.file_off[i], in.file_len[i], 0, 0, 0};
        s.bad = s.len < kHintHead || s.off > in.bytes || in.bytes - s.off < s.len;
        if (!s.bad) {
            const uint8_t *f = in.hints + s.off;
            const int64_t ix = (int64_t)hint_ld64(f);
            atomicMax(&cnt->datasize, hint_ld32(f + kHeadDatasize));
            if (ix < 0 || (uint64_t)ix > s.len) {
                s.bad = 1;
            } else if (ix == 0) {
                s.io = s.len;  // "has no index": the items run to the file's end
            } else {
                s.io = (uint64_t)ix;
                // more entries than items fit below indexOffset, or than cap: no proof can hold
                const uint64_t ne = (s.len - s.io) / kHintEntry;
                if (s.io > kHintHead && ne <= (s.io - kHintHead) / kHintItem && ne <= in.cap) s.ne = (uint32_t)ne;
            }
            if (s.io <= kHintHead) s.bad = 1;  // no item: merge dereferences a nil first item
        }
        if (s.bad) atomicMax(&hm->bad_inv, ~i);
        src[i] = s;
        unproven[i] = 0;
        sv[i] = HintAcc{(unsigned long long)s.ne + 1, 0};  // its stretches
    }
}

// The stretches: source i owns [sb[i].b, sb[i].b + ne_i + 1).  Should the sources claim more index
// entries than cap (then they hold more than cap items, or some claim is wrong), nothing is
// proven: one stretch per source.
struct HmStr {
    const HmSrc *src;
    const HintAcc *sv, *sb;
    const uint32_t *unproven;
    uint32_t n_files, cap;
    __device__ __forceinline__ uint64_t count(bool *flat) const {
        const uint64_t S = sb[n_files - 1].b + sv[n_files - 1].b;
        *flat = S > (uint64_t)cap + n_files;
        return *flat ? n_files : S;
    }
    __device__ __forceinline__ void locate(uint64_t g, bool flat, uint32_t *i, uint32_t *m) const {
        if (flat) {
            *i = (uint32_t)g, *m = 0;
            return;
        }
        uint32_t lo = 0, hi = n_files;  // the last source with sb[i].b <= g
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (sb[mid].b <= g) lo = mid;
            else hi = mid;
        }
        *i = lo, *m = (uint32_t)(g - sb[lo].b);
    }
};

// hintFileReader.next from p while p < stop <= len: emit(j, p) per item; false when an item's head
// or key runs past the file.
template <class E>
__device__ __forceinline__ bool hm_walk(const uint8_t *f, uint64_t len, uint64_t *p_io, uint64_t stop, uint64_t *n,
                                        E emit) {
    uint64_t p = *p_io, j = 0;
    bool ok = true;
    while (p < stop) {
        uint32_t ksz;
        if (!hint_next(len, p, [&](uint64_t q) { return f[q]; }, &ksz)) { ok = false; break; }
        emit(j, p);
        p += kHintItem + ksz;
        j++;
    }
    *p_io = p, *n = j;
    return ok;
}
// Stretch m of a source with ne entries to prove: from entry m - 1 (16 for m = 0) to entry m
// (indexOffset for m = ne).  False when the bounds break the rule "strictly increasing inside
// [16, indexOffset)".  Entry m is 16 bytes at io + 16 m: {keyhash, offset i64}; a negative offset
// reads as a large one and fails.
__device__ __forceinline__ bool hm_stretch(const uint8_t *f, const HmSrc &s, uint32_t m, uint64_t *start,
                                           uint64_t *stop) {
    *start = m == 0 ? kHintHead : hint_ld64(f + s.io + (uint64_t)kHintEntry * (m - 1) + kEntryOffset);
    *stop = m == s.ne ? s.io : hint_ld64(f + s.io + (uint64_t)kHintEntry * m + kEntryOffset);
    if (*start < kHintHead || *start >= s.io || *stop > s.io) return false;
    if (m < s.ne && *stop >= s.io) return false;
    return m == 0 ? *start <= *stop : *start < *stop;
}
// The items of stretch (i, m), counted or emitted.  proven = false walks the whole source in its
// stretch 0.  Returns false when the stretch does not hold what it must (see the callers).
template <class E>
__device__ __forceinline__ bool hm_items(const HmIn &in, const HmSrc &s, uint32_t m, bool proven, uint64_t *n,
                                         E emit) {
    *n = 0;
    if (s.bad) return true;
    const uint8_t *f = in.hints + s.off;
    uint64_t p = kHintHead, stop = s.io;
    if (proven) {
        if (!hm_stretch(f, s, m, &p, &stop)) return false;
    } else if (m) {
        return true;
    }
    const bool last = !proven || m == s.ne;
    if (!hm_walk(f, s.len, &p, stop, n, emit)) return false;
    return last || p == stop;  // the last item may run past indexOffset: the reader takes it whole
}

__global__ void __launch_bounds__(256) k_hm_count(HmIn in, HmStr st, uint32_t *unproven, HintAcc *sc,
                                                  HmCounters *hm) {
    bool flat;
    const uint64_t S = st.count(&flat);
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < S; g += (uint64_t)gridDim.x * 256) {
        uint32_t i, m;
        st.locate(g, flat, &i, &m);
        const HmSrc s = st.src[i];
        const bool proven = !flat && s.ne != 0;
        uint64_t n;
        if (!hm_items(in, s, m, proven, &n, [](uint64_t, uint64_t) {})) {
            n = 0;
            if (proven) unproven[i] = 1;
            else atomicMax(&hm->bad_inv, ~i);  // walked from 16: an item ends past the file
        }
        sc[g] = HintAcc{n, 0};
    }
}
// An unproven source, walked from 16 by the lane of its stretch 0; its other stretches hold nothing.
__global__ void __launch_bounds__(256) k_hm_settle(HmIn in, HmStr st, HintAcc *sc, HmCounters *hm) {
    bool flat;
    const uint64_t S = st.count(&flat);
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < S; g += (uint64_t)gridDim.x * 256) {
        uint32_t i, m;
        st.locate(g, flat, &i, &m);
        if (flat || !st.unproven[i]) continue;
        uint64_t n;
        if (!hm_items(in, st.src[i], m, false, &n, [](uint64_t, uint64_t) {})) {
            n = 0;
            atomicMax(&hm->bad_inv, ~i);
        }
        sc[g] = HintAcc{n, 0};
    }
}
// pos[k] / sid[k]: where item k starts in `hints` and its source, in (source, item) order.  The
// first status is decided here by every lane alike: nothing is filled unless the sources are good
// and hold at most cap items.
__global__ void __launch_bounds__(256) k_hm_fill(HmIn in, HmStr st, const HintAcc *sc, const HintAcc *so, uint64_t *pos,
                                                 uint32_t *sid, HmCounters *hm) {
    bool flat;
    const uint64_t S = st.count(&flat);
    const uint64_t N = so[S - 1].b + sc[S - 1].b;
    const uint32_t status = hm->bad_inv ? QLZX_HM_BAD_FILE : N > in.cap ? QLZX_HM_TOO_MANY : QLZX_HM_OK;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hm->n = N, hm->status = status;
        hm->src = status == QLZX_HM_BAD_FILE ? ~hm->bad_inv : 0u;
    }
    if (status != QLZX_HM_OK) return;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < S; g += (uint64_t)gridDim.x * 256) {
        uint32_t i, m;
        st.locate(g, flat, &i, &m);
        const HmSrc s = st.src[i];
        const uint64_t base = so[g].b;
        uint64_t n;
        hm_items(in, s, m, !flat && s.ne != 0 && !st.unproven[i], &n, [&](uint64_t j, uint64_t p) {
            if (base + j < in.cap) pos[base + j] = s.off + p, sid[base + j] = i;
        });
    }
}

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
struct HmWs : HintSortWs {
    HintCounters *cnt;
    HmCounters *hm;
    HmSrc *src;
    uint32_t *unproven, *sid;
    HintAcc *sv, *sb;  // the sources' stretch counts and their scan
    HintAcc *a, *b;    // stretch counts and their scan; then key_in (a's second half) and itemv / items
    uint64_t *pos;
};
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
    const dim3 GF(grid_for(in.n_files, 256, 2048)), GS(grid_for((uint64_t)in.cap + in.n_files, 256, 2048));
    hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(HintCounters), s);
    if (e != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(w.hm, 0, sizeof(HmCounters), s)) != hipSuccess) return (int)e;
    // the sources' items: heads, stretches, counts, positions
    hipLaunchKernelGGL(k_hm_head, GF, B, 0, s, in, w.src, w.unproven, w.sv, w.cnt, w.hm);
    if ((e = w.scan(w.sv, w.sb, in.n_files, HintAccPlus(), s)) != hipSuccess) return (int)e;
    const HmStr st{w.src, w.sv, w.sb, w.unproven, in.n_files, in.cap};
    hipLaunchKernelGGL(k_hm_count, GS, B, 0, s, in, st, w.unproven, w.a, w.hm);
    hipLaunchKernelGGL(k_hm_settle, GS, B, 0, s, in, st, w.a, w.hm);
    // the scan covers the most stretches there can be; the kernels read the first S sums only
    if ((e = w.scan(w.a, w.b, (size_t)in.cap + in.n_files, HintAccPlus(), s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_hm_fill, GS, B, 0, s, in, st, (const HintAcc *)w.a, (const HintAcc *)w.b, w.pos, w.sid, w.hm);
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
