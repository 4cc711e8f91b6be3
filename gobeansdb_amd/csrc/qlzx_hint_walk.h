// qlzx_hint_walk.h -- the items of hint files resident in device memory, found without a serial
// pass: what qlzx_hintmerge.hip and qlzx_htree.hip share (each includes this header itself).
//
// The item starts of a source are a serial chain (ksz sits at byte 22 of an item), so a source is
// cut into stretches at the entries of its own sparse index, one lane per stretch:
//   k_hm_head    every source's head.
//   k_hm_count   walks a stretch and must land exactly on the next entry (the last one on
//                indexOffset); entries that are not strictly increasing inside [16, indexOffset),
//                or a walk that misses, leave the source unproven.
//   k_hm_settle  walks an unproven source from 16 with one lane (as a source without an index is
//                walked): correct, not fast.
//   k_hm_fill    after a scan of the counts, walks again and writes every item's position and
//                source, in (source, item) order; settles the first status.
// The two users differ in one rule: the merge dereferences a first item, so a source without any
// item is bad there (k_hm_head<false>); updateHtreeFromHint's loop just ends (k_hm_head<true>).
#pragma once

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

// hintFileReader.open (store/hintfile.go:57-87).  A source that cannot yield an item is bad unless
// kEmptyOk.
template <bool kEmptyOk>
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
            if (!kEmptyOk && s.io <= kHintHead) s.bad = 1;  // no item: merge dereferences a nil first item
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

// What the discovery keeps in a workspace: the counters, the sources, their stretch counts with
// the scan (sv / sb), the stretches' item counts with the scan (a / b), the items' positions.
struct HmWalkWs {
    HintCounters *cnt;
    HmCounters *hm;
    HmSrc *src;
    uint32_t *unproven, *sid;
    HintAcc *sv, *sb;
    HintAcc *a, *b;
    uint64_t *pos;
};
// The four kernels and their two scans; scan(from, to, n) is the exclusive HintAcc scan on s.
// Afterwards hm->n / status / src are settled and pos / sid hold the hm->n items (status OK only).
template <bool kEmptyOk, class Scan>
inline hipError_t launch_hm_walk(const HmIn &in, const HmWalkWs &w, Scan scan, hipStream_t s) {
    const dim3 B(256), GF(grid_for(in.n_files, 256, 2048)), GS(grid_for((uint64_t)in.cap + in.n_files, 256, 2048));
    hipLaunchKernelGGL(k_hm_head<kEmptyOk>, GF, B, 0, s, in, w.src, w.unproven, w.sv, w.cnt, w.hm);
    if (const hipError_t e = scan(w.sv, w.sb, (size_t)in.n_files)) return e;
    const HmStr st{w.src, w.sv, w.sb, w.unproven, in.n_files, in.cap};
    hipLaunchKernelGGL(k_hm_count, GS, B, 0, s, in, st, w.unproven, w.a, w.hm);
    hipLaunchKernelGGL(k_hm_settle, GS, B, 0, s, in, st, w.a, w.hm);
    // the scan covers the most stretches there can be; the kernels read the first S sums only
    if (const hipError_t e = scan(w.a, w.b, (size_t)in.cap + in.n_files)) return e;
    hipLaunchKernelGGL(k_hm_fill, GS, B, 0, s, in, st, (const HintAcc *)w.a, (const HintAcc *)w.b, w.pos, w.sid, w.hm);
    return hipSuccess;
}

}  // namespace qlzx
