// qlzx_htree.hip -- a bucket's HTree and its .hash dump from hint files resident in device memory
// (SURVEY §8 f1f): what bucket open does with the split files, updateHtreeFromHint per file
// (store/bucket.go:119-151, :207-230) -> HTree.set / remove (store/htree.go:211-311) over
// SliceHeader.Set / Remove (store/leaf.go:120-153), then HTree.Update (updateNodes, :332-359) and
// HTree.dump (:146-203).  The reference replays the items one by one through a linear find per
// leaf under the tree's mutex.  Here the items are ops t = 0, 1, ... in (source, file) order and
// the tree is a function of them:
//   - the slot of an op is its keyhash without the bucket nibbles: (leaf, the low L bytes that
//     findInBytes compares), one 64-bit value since 8 L + 4 p >= 64;
//   - a slot is present iff its last op is a set (ver > 0), with that op's data;
//   - Set on an existing slot rewrites in place, Remove shifts the tail down, a later Set appends:
//     a leaf's bytes are its present slots ascending by incarnation start, the first set after
//     the slot's last remove;
//   - a leaf node's (count, hash) is a sum over its present slots: every add of a replaced or
//     removed item is taken back by the reference's running += / -=.
//
// The sources are read as qlzx_hintmerge.hip reads them (qlzx_hint_walk.h; a source without any
// item is valid here), the sorts and scans run through qlzx_hint_fmt.h's workspace tail.
//
// Two calls, nothing read back in between:
//   plan   the ops' positions (launch_hm_walk); k_ht_key: (slot, op) pairs, sorted stably: a run
//          of one slot is in op order and the runs of one leaf are adjacent.  k_ht_runs: the last
//          position of a run decides whether the slot is present and walks back over the sets
//          before it to its incarnation start; pairs ((leaf, start), data op), absent slots
//          behind every present one.  The second sort is the file order.  k_ht_slots: slot_src /
//          slot_chunk and the slot's hash term; a scan of the terms.  k_ht_leaves: leaf_first by a
//          binary search per leaf, the leaf node from leaf_first and the scanned terms (no atomic
//          on a node).  k_ht_level per upper level, bottom up.
//   write  k_ht_file: a lane per 16 bytes of the file: the leaf by a binary search over the
//          leaves' file offsets (4 l + item * leaf_first[l]), then the bytes from a cursor.
#include "qlzx_hint_walk.h"
#include "qlzx_htree.h"

namespace qlzx {

static_assert((int)QLZX_HT_OK == (int)QLZX_HM_OK && (int)QLZX_HT_NO_SPACE == (int)QLZX_HM_NO_SPACE &&
                  (int)QLZX_HT_BAD_FILE == (int)QLZX_HM_BAD_FILE && (int)QLZX_HT_TOO_MANY == (int)QLZX_HM_TOO_MANY,
              "k_hm_fill settles the status both plans report");

constexpr uint32_t kHtMaxDepth = 2, kHtMaxHeight = 6, kHtItemHead = 11, kHtNode = 6, kHtBigHash = 256;

// Conf.TreeDepth / TreeHeight and what InitTree derives (store/config.go:82-96).
struct HtGeo {
    uint32_t depth, height, L, item;  // item = L + 11: the bytes of a leaf's item
    uint32_t nleaf, leaf_base;        // 16^(height-1) leaves; their nodes start at leaf_base
    __host__ __device__ static uint32_t level_base(uint32_t l) { return (uint32_t)(((1ull << (4 * l)) - 1) / 15); }
    __device__ __forceinline__ uint64_t slot(uint64_t keyhash) const { return keyhash & (~0ull >> (4 * depth)); }
    __device__ __forceinline__ uint32_t leaf(uint64_t slot) const {
        const uint32_t p = depth + height - 1;
        return p ? (uint32_t)(slot >> (64 - 4 * p)) : 0u;
    }
};
inline bool ht_geo(uint32_t depth, uint32_t height, HtGeo *g) {
    if (depth > kHtMaxDepth || height < 1 || height > kHtMaxHeight) return false;
    static const uint32_t lens[8] = {8, 8, 7, 7, 6, 6, 5, 5};  // KHASH_LENS
    const uint32_t L = lens[depth + height - 1];
    *g = HtGeo{depth, height, L, L + kHtItemHead, 1u << (4 * (height - 1)), HtGeo::level_base(height - 1)};
    return true;
}

struct HtCounters {
    uint32_t nset, nslots;  // the ops with ver > 0; the present slots
};

// op t's item: pos[t] is an item k_hm_fill found whole inside its file
struct HtOps {
    const uint8_t *hints;
    const uint64_t *pos;
    uint32_t cap;
    __device__ __forceinline__ const uint8_t *item(uint32_t t) const { return t < cap ? hints + pos[t] : nullptr; }
    __device__ __forceinline__ bool is_set(uint32_t t) const {
        const uint8_t *p = item(t);
        return p && (int32_t)hint_ld32(p + kItemVer) > 0;
    }
};

// The first sort's pairs (slot, op); behind the nv ops the largest key, which a stable sort leaves
// behind every op.  nv (0 with any status) is settled here.
__global__ void __launch_bounds__(256) k_ht_key(HtOps O, HtGeo g, uint64_t *key_in, uint32_t *val_in,
                                                HintCounters *cnt, const HmCounters *hm, HtCounters *ht) {
    const uint32_t nv = hm->status == QLZX_HT_OK ? (uint32_t)(hm->n < O.cap ? hm->n : O.cap) : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->nv = nv;
    uint32_t nset = 0;
    for (uint32_t base = blockIdx.x * 256; base < O.cap; base += gridDim.x * 256) {  // whole waves: wave_sum below
        const uint32_t k = base + threadIdx.x;
        if (k >= O.cap) continue;
        const bool v = k < nv;
        key_in[k] = v ? g.slot(hint_ld64(O.item(k))) : ~0ull;
        val_in[k] = k;
        nset += v && O.is_set(k);
    }
    nset = wave_sum(nset);
    if ((threadIdx.x & 63) == 0 && nset) atomicAdd(&ht->nset, nset);
}

// Sorted position i ends the run of its slot iff the next position holds another slot.  That
// position's op is the slot's last: a set makes the slot present with that op's data, and the
// sets before it back to the slot's last remove (or the run's start) are one incarnation, whose
// first op placed the slot in its leaf.  The second sort's pairs ((leaf, that op), data op);
// every other position gets the largest key.
__global__ void __launch_bounds__(256) k_ht_runs(HtOps O, HtGeo g, const uint64_t *key_s, const uint32_t *val_s,
                                                 uint64_t *key_in, uint32_t *val_in, const HintCounters *cnt,
                                                 HtCounters *ht) {
    const uint32_t nv = cnt->nv;
    uint32_t npresent = 0;
    for (uint32_t base = blockIdx.x * 256; base < O.cap; base += gridDim.x * 256) {
        const uint32_t i = base + threadIdx.x;
        if (i >= O.cap) continue;
        uint64_t k2 = ~0ull;
        uint32_t v2 = 0xffffffffu;
        if (i < nv) {
            const uint64_t slot = key_s[i];
            const uint32_t t1 = val_s[i];
            if ((i + 1 == nv || key_s[i + 1] != slot) && O.is_set(t1)) {
                uint32_t j = i;
                while (j > 0 && key_s[j - 1] == slot && O.is_set(val_s[j - 1])) j--;
                k2 = ((uint64_t)g.leaf(slot) << 32) | val_s[j];
                v2 = t1;
                npresent++;
            }
        }
        key_in[i] = k2;
        val_in[i] = v2;
    }
    npresent = wave_sum(npresent);
    if ((threadIdx.x & 63) == 0 && npresent) atomicAdd(&ht->nslots, npresent);
}

// After the second sort position k < nslots is slot k of the file.  term[k] = its share of its
// leaf node's hash (setToLeaf, store/htree.go:224), 0 from nslots on (cap + 1 entries).
__global__ void __launch_bounds__(256) k_ht_slots(HtOps O, const uint32_t *sid, const uint32_t *file_chunk,
                                                  uint32_t n_files, const uint32_t *val_s, uint64_t *slot_src,
                                                  uint32_t *slot_chunk, uint32_t *term, const HtCounters *ht) {
    const uint32_t ns = ht->nslots < O.cap ? ht->nslots : O.cap;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k <= O.cap; k += gridDim.x * 256) {
        uint32_t x = 0;
        if (k < ns) {
            const uint32_t t = val_s[k];
            if (const uint8_t *p = O.item(t)) {
                const uint32_t f = sid[t];
                slot_src[k] = O.pos[t];
                slot_chunk[k] = f < n_files ? file_chunk[f] : 0u;
                const uint32_t vhash = (uint32_t)p[kItemVhash] | ((uint32_t)p[kItemVhash + 1] << 8);
                x = vhash * (hint_ld32(p + 4) & 0xffffu);  // uint16(keyhash >> 32)
            }
        }
        term[k] = x;
    }
}

// The first of the ns sorted keys that is not below (leaf << 32).
__device__ __forceinline__ uint32_t ht_leaf_lower(const uint64_t *key_s, uint32_t ns, uint32_t leaf) {
    const uint64_t want = (uint64_t)leaf << 32;
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_s[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// leaf_first and the leaf nodes; terms = the exclusive scan of term.
__global__ void __launch_bounds__(256) k_ht_leaves(HtGeo g, const uint64_t *key_s, const uint32_t *terms, uint32_t cap,
                                                   uint32_t *leaf_first, uint32_t *node_count, uint16_t *node_hash,
                                                   const HtCounters *ht) {
    const uint32_t ns = ht->nslots < cap ? ht->nslots : cap;
    for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l <= g.nleaf; l += gridDim.x * 256) {
        const uint32_t lo = ht_leaf_lower(key_s, ns, l);
        leaf_first[l] = lo;
        if (l < g.nleaf) {
            const uint32_t hi = ht_leaf_lower(key_s, ns, l + 1);
            node_count[g.leaf_base + l] = hi - lo;
            node_hash[g.leaf_base + l] = (uint16_t)(terms[hi] - terms[lo]);
        }
    }
}
// updateNodes (store/htree.go:338-359) for the 16^level nodes of one level above the leaves.
__global__ void __launch_bounds__(256) k_ht_level(uint32_t level, uint32_t *node_count, uint16_t *node_hash) {
    const uint32_t n = 1u << (4 * level), at = HtGeo::level_base(level), below = HtGeo::level_base(level + 1);
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        uint32_t count = 0;
        for (uint32_t i = 0; i < 16; i++) count += node_count[below + 16 * j + i];
        uint16_t hash = 0;
        for (uint32_t i = 0; i < 16; i++) {
            if (count > kHtBigHash) hash = (uint16_t)(hash * 97u);
            hash = (uint16_t)(hash + node_hash[below + 16 * j + i]);
        }
        node_count[at + j] = count;
        node_hash[at + j] = hash;
    }
}
__global__ void k_ht_totals(uint32_t *totals, HtGeo g, uint32_t cap, const HintCounters *cnt, const HmCounters *hm,
                            const HtCounters *ht) {
    const bool ok = hm->status == QLZX_HT_OK;
    const uint32_t n = ok ? cnt->nv : 0u, ns = ok ? (ht->nslots < cap ? ht->nslots : cap) : 0u;
    const uint64_t fb = ok ? (uint64_t)(kHtNode + 4) * g.nleaf + (uint64_t)g.item * ns : 0;
    totals[0] = n, totals[1] = ok ? ht->nset : 0u, totals[2] = ok ? n - ht->nset : 0u, totals[3] = ns;
    totals[4] = g.nleaf;
    totals[5] = (uint32_t)fb, totals[6] = (uint32_t)(fb >> 32);
    totals[7] = hm->src, totals[8] = hm->status, totals[9] = 0;
}

// ---- write ----
// The plan's arrays are the caller's between the two calls and may hold anything: a slot number is
// used only below ns <= cap, a leaf_first entry only cut to ns, slot_src only when a whole item
// head lies inside `hints`; what they cannot describe comes out as zeros.
struct HtFile {
    const uint8_t *hints;
    uint64_t bytes;
    const uint32_t *node_count;
    const uint16_t *node_hash;
    const uint32_t *leaf_first;  // nleaf + 1
    const uint64_t *slot_src;
    const uint32_t *slot_chunk;
};
struct HtCur {
    uint32_t leaf, first, count;  // the leaf, its first slot, its slots
    uint64_t start, end;          // its bytes in the leaf section: the length field at start
    uint32_t k;                   // the slot whose bytes are loaded below (0xffffffff = none)
    uint64_t kh, t0;              // keyhash; ver, vhash, offset >> 8 (its low two bytes)
    uint32_t t1;                  // offset >> 24, chunk u16
};
__device__ __forceinline__ uint32_t ht_first(const HtFile &f, uint32_t ns, uint32_t l) {
    const uint32_t x = f.leaf_first[l];
    return x < ns ? x : ns;
}
// where leaf l's length field starts in the leaf section, l <= nleaf
__device__ __forceinline__ uint64_t ht_leaf_at(const HtFile &f, const HtGeo &g, uint32_t ns, uint32_t l) {
    return 4ull * l + (uint64_t)g.item * ht_first(f, ns, l);
}
__device__ __forceinline__ void ht_cur_leaf(const HtFile &f, const HtGeo &g, uint32_t ns, uint32_t l, HtCur &c) {
    const uint32_t a = ht_first(f, ns, l), b = ht_first(f, ns, l + 1);
    c.leaf = l, c.first = a, c.count = b > a ? b - a : 0u;
    c.start = 4ull * l + (uint64_t)g.item * a;
    c.end = 4ull * (l + 1) + (uint64_t)g.item * b;
}
// itemToBytes (store/leaf.go:61-71) of slot k, as the three words ht_item_byte picks from
__device__ __forceinline__ void ht_cur_item(const HtFile &f, uint32_t k, HtCur &c) {
    c.k = k, c.kh = 0, c.t0 = 0, c.t1 = (f.slot_chunk[k] & 0xffffu) << 8;
    const uint64_t o = f.slot_src[k];
    if (o > f.bytes || f.bytes - o < kHintItem) return;
    const uint8_t *p = f.hints + o;
    const uint32_t off = hint_ld32(p + kItemOffset);
    const uint32_t vhash = (uint32_t)p[kItemVhash] | ((uint32_t)p[kItemVhash + 1] << 8);
    c.kh = hint_ld64(p);
    c.t0 = hint_ld32(p + kItemVer) | ((uint64_t)vhash << 32) | ((uint64_t)((off >> 8) & 0xffffu) << 48);
    c.t1 |= off >> 24;
}
// The file's byte q < 10 nleaf + item * ns.
__device__ __forceinline__ uint32_t ht_file_byte(const HtFile &f, const HtGeo &g, uint32_t ns, uint64_t q, HtCur &c) {
    const uint64_t nodes = (uint64_t)kHtNode * g.nleaf;
    if (q < nodes) {
        const uint32_t n = (uint32_t)(q / kHtNode), r = (uint32_t)(q % kHtNode);
        const uint32_t x = r < 4 ? f.node_count[g.leaf_base + n] >> (8 * r) : (uint32_t)f.node_hash[g.leaf_base + n] >> (8 * (r - 4));
        return x & 0xffu;
    }
    const uint64_t y = q - nodes;
    if (c.leaf == 0xffffffffu) {
        uint32_t lo = 0, hi = g.nleaf;  // the last leaf that starts at or before y
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ht_leaf_at(f, g, ns, mid) <= y) lo = mid;
            else hi = mid;
        }
        ht_cur_leaf(f, g, ns, lo, c);
    }
    while (y >= c.end && c.leaf + 1 < g.nleaf) ht_cur_leaf(f, g, ns, c.leaf + 1, c);
    if (y < c.start || y >= c.end) return 0;
    const uint64_t r = y - c.start;
    if (r < 4) return (uint32_t)(((uint64_t)g.item * c.count) >> (8 * r)) & 0xffu;
    const uint64_t idx = (r - 4) / g.item;
    const uint32_t b = (uint32_t)((r - 4) % g.item);
    if (idx >= c.count) return 0;
    const uint32_t k = c.first + (uint32_t)idx;  // below first + count <= ns
    if (k != c.k) ht_cur_item(f, k, c);
    const uint32_t t = b - g.L;
    const uint64_t x = b < g.L ? c.kh >> (8 * b) : t < 8 ? c.t0 >> (8 * t) : (uint64_t)c.t1 >> (8 * (t - 8));
    return (uint32_t)x & 0xffu;
}
// A lane per 16 bytes of the file, grid-stride: one aligned 16-B store (the file's last, partial
// chunk: dwords, then at most three single bytes).  Nothing is written when the plan refused its
// sources or the file does not fit out_cap; totals[8] says so.
__global__ void __launch_bounds__(256) k_ht_file(const HtFile f, HtGeo g, uint32_t cap, uint8_t *out, uint64_t out_cap,
                                                 uint32_t *totals) {
    const uint32_t ns = totals[3] < cap ? totals[3] : cap, prev = totals[8];
    const uint64_t fb = (uint64_t)(kHtNode + 4) * g.nleaf + (uint64_t)g.item * ns;
    const bool fits = fb <= out_cap;
    // thread 0's store may be seen by another block's load of totals[8]: it never crosses NO_SPACE
    if (blockIdx.x == 0 && threadIdx.x == 0 && prev <= QLZX_HT_NO_SPACE)
        totals[8] = fits ? (uint32_t)QLZX_HT_OK : (uint32_t)QLZX_HT_NO_SPACE;
    if (!fits || prev > QLZX_HT_NO_SPACE) return;
    const uint64_t nchunks = (fb + 15) / 16;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (uint64_t)gridDim.x * 256) {
        const uint64_t x = 16 * i, left = fb - x;
        HtCur c;
        c.leaf = 0xffffffffu, c.k = 0xffffffffu;
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (b < left) w[b / 4] |= ht_file_byte(f, g, ns, x + b, c) << (8 * (b & 3));
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

// ---- workspace: the discovery's arrays, the tree's counters, the sort's tail ----
// a / b: stretch counts and their scan; then key_in (a's second half)
struct HtWs : HintSortWs, HmWalkWs {
    HtCounters *ht;
};
inline size_t ht_ws_layout(uint32_t n_files, uint32_t cap, uint8_t *base, HtWs *w) {
    const size_t m = (size_t)cap + 2, sm = (size_t)cap + n_files + 2;
    WsCarver c{base};
    HtWs t;
    t.cnt = c.take<HintCounters>(sizeof(HintCounters));
    t.hm = c.take<HmCounters>(sizeof(HmCounters));
    t.ht = c.take<HtCounters>(sizeof(HtCounters));
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

inline int launch_ht_plan(const HmIn &in, const HtGeo &g, uint32_t *node_count, uint16_t *node_hash,
                          uint32_t *leaf_first, uint64_t *slot_src, uint32_t *slot_chunk, uint32_t *totals, void *ws,
                          hipStream_t s) {
    HtWs w;
    ht_ws_layout(in.n_files, in.cap, (uint8_t *)ws, &w);
    const uint32_t M = in.cap;
    const dim3 G(grid_for((uint64_t)M + 1, 256, 2048)), B(256);
    hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(HintCounters), s);
    if (e != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(w.hm, 0, sizeof(HmCounters), s)) != hipSuccess) return (int)e;
    if ((e = hipMemsetAsync(w.ht, 0, sizeof(HtCounters), s)) != hipSuccess) return (int)e;
    // the ops: every source's items in (source, file) order; no source is no op, status OK
    if (in.n_files) {
        const auto acc_scan = [&](const HintAcc *from, HintAcc *to, size_t n) { return w.scan(from, to, n, HintAccPlus(), s); };
        if ((e = launch_hm_walk<true>(in, w, acc_scan, s)) != hipSuccess) return (int)e;
    }
    const HtOps O{in.hints, w.pos, in.cap};
    // by slot, stably: a slot's ops in op order, a leaf's slots together
    hipLaunchKernelGGL(k_ht_key, G, B, 0, s, O, g, w.key_in, w.val_in, w.cnt, (const HmCounters *)w.hm, w.ht);
    if ((e = w.sort(w.val_in, w.val_s, M, s)) != hipSuccess) return (int)e;
    // the present slots by (leaf, incarnation start): the file's order
    hipLaunchKernelGGL(k_ht_runs, G, B, 0, s, O, g, (const uint64_t *)w.key_s, (const uint32_t *)w.val_s, w.key_in,
                       w.val_in, (const HintCounters *)w.cnt, w.ht);
    if ((e = w.sort(w.val_in, w.val_s, M, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ht_slots, G, B, 0, s, O, (const uint32_t *)w.sid, in.file_chunk, in.n_files,
                       (const uint32_t *)w.val_s, slot_src, slot_chunk, w.fa, (const HtCounters *)w.ht);
    if ((e = w.scan(w.fa, w.fb, (size_t)M + 1, rocprim::plus<uint32_t>(), s)) != hipSuccess) return (int)e;
    // the nodes: the leaves, then every level above them
    hipLaunchKernelGGL(k_ht_leaves, dim3(grid_for((uint64_t)g.nleaf + 1, 256, 2048)), B, 0, s, g,
                       (const uint64_t *)w.key_s, (const uint32_t *)w.fb, M, leaf_first, node_count, node_hash,
                       (const HtCounters *)w.ht);
    for (uint32_t level = g.height - 1; level-- > 0;)
        hipLaunchKernelGGL(k_ht_level, dim3(grid_for(1ull << (4 * level), 256, 2048)), B, 0, s, level, node_count,
                           node_hash);
    hipLaunchKernelGGL(k_ht_totals, dim3(1), dim3(1), 0, s, totals, g, M, (const HintCounters *)w.cnt,
                       (const HmCounters *)w.hm, (const HtCounters *)w.ht);
    return (int)hipGetLastError();
}

inline int launch_ht_write(const HtFile &f, const HtGeo &g, uint32_t cap, uint8_t *out, uint64_t out_cap,
                           uint32_t *totals, hipStream_t s) {
    // a file that fits has at most out_cap / 16 + 1 chunks
    hipLaunchKernelGGL(k_ht_file, dim3(std::max(grid_for(out_cap / 16 + 1, 256, 2048), 1u)), dim3(256), 0, s, f, g, cap,
                       out, out_cap, totals);
    return (int)hipGetLastError();
}

}  // namespace qlzx
