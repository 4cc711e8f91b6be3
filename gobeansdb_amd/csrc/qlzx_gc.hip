// qlzx_gc.hip -- the GC rewrite of a chunk: the record loop of GCMgr.gc
// (store/gc.go:268-353) for one source chunk resident in device memory.  The records the stream
// reader returns (qlzx_replay_index's rec_off / result) are filtered by the caller's liveness
// mask and every kept record is appended to the destination in order, as
// dataChunk.AppendRecordGC -> WriteRecord.append does (store/datachunk.go:56-79,
// store/datafile.go:307-330): header re-encoded with its CRC recomputed (store/datafile.go:66-88),
// zero padding to 256 B, and the next destination chunk whenever recsize + writingHead >
// DataFileMax (store/gc.go:320-336).
//
// Two calls, nothing read back in between:
//   plan     k_gc_check: readRecordAt's size checks (qlzx_recfile.h; no CRC) on every kept
//            record and its padded size; k_rp_dstoff: the u64 exclusive scan S of the sizes;
//            k_gc_cut: the rotation is a greedy cut of S, one wave finds each destination chunk's
//            first record by a 64-way search over S; k_gc_place: (chunk, offset) per record;
//   rewrite  k_gc_copy: a wave per placed record reads its bytes once (aligned 16-B loads: source
//            and destination both start on 256-B boundaries), computes the CRC in the same pass
//            (wave_crc's stripe layout, anchored at the end of the span as wr_span's) and writes
//            them with aligned 16-B stores, padding included, the CRC word last; records with a
//            CRC span over kRpLong are cut into kRpSeg segments over the chip (k_rec_long<GcLong>).
#include "qlzx_recfile.h"

namespace qlzx {

struct GcCounters {
    uint32_t n, nkeep, nbad, nnochunk, nplaced, nch, end, nlong, nfail, nmis;
    unsigned long long bytes, failbytes;
    uint32_t t5[6];  // k_rp_dstoff's totals; pads the struct to a multiple of 16 bytes
};

// ---- plan ----
// Per record: DROPPED, BAD_RECORD or WRITTEN (so far: the cut may still say NO_CHUNK), and
// sz[j] = its padded size, 0 for a record that takes no space.
__global__ void __launch_bounds__(256) k_gc_check(const uint8_t *data, uint64_t size, const uint64_t *rec_off,
                                                  const uint32_t *result, uint32_t cap, const uint8_t *keep,
                                                  uint32_t max_key, uint64_t body_max, int32_t *gc_status,
                                                  uint32_t *sz, GcCounters *cnt) {
    const uint32_t n = rec_count(result, cap);
    uint32_t nkeep = 0, nbad = 0;
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        int32_t st = QLZX_GC_DROPPED;
        uint32_t s = 0;
        if (keep[j]) {
            nkeep++;
            st = QLZX_GC_BAD_RECORD;
            const uint64_t off = rec_off[j];
            if (rec_pos_verdict(off, size) == kRecOk) {
                const uint2 kv = *(const uint2 *)(data + off + 16);  // ksz, vsz
                if (rec_size_verdict(kv.x, kv.y, size - off - kRpHdr, max_key, body_max) == kRecOk) {
                    st = QLZX_GC_WRITTEN;
                    s = (uint32_t)pad256((uint64_t)kRpHdr + kv.x + kv.y);
                }
            }
            nbad += st == QLZX_GC_BAD_RECORD;
        }
        gc_status[j] = st;
        sz[j] = s;
    }
    nkeep = wave_sum(nkeep), nbad = wave_sum(nbad);
    if ((threadIdx.x & 63) == 0) {
        if (nkeep) atomicAdd(&cnt->nkeep, nkeep);
        if (nbad) atomicAdd(&cnt->nbad, nbad);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->n = n;
}

// The first j in [lo, hi) with S[j] + sz[j] - sb > room, hi when there is none.  S + sz is
// non-decreasing, so each round the 64 lanes probe the last index of 64 equal parts of the range
// and the first part whose probe passes holds the answer.
__device__ uint32_t gc_search(const uint64_t *S, const uint32_t *sz, uint32_t lo, uint32_t hi, uint64_t sb,
                              uint64_t room, uint32_t lane) {
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63) / 64;
        const uint64_t last = (uint64_t)lo + (uint64_t)(lane + 1) * step - 1;
        const uint32_t p = last < hi ? (uint32_t)last : hi - 1;
        const uint64_t m = __ballot(S[p] + sz[p] - sb > room);
        if (m == 0) return hi;
        const uint32_t L = (uint32_t)__builtin_ctzll(m);
        const uint64_t nlo = (uint64_t)lo + (uint64_t)L * step, nhi = nlo + step - 1;
        hi = nhi < hi ? (uint32_t)nhi : hi - 1;  // the probe that passed: the answer is at most here
        lo = (uint32_t)nlo;
    }
    return lo;
}

// One wave.  Destination chunk c holds the records [first[c], first[c + 1]); the record that
// does not fit (recsize + head > data_file_max) opens the next chunk and is appended there
// whatever its size (the reference moves once).  chunk_base / chunk_bytes for every c below
// max_chunks; cnt->nch chunks were opened, cnt->end = the first record left without a chunk.
__global__ void __launch_bounds__(64) k_gc_cut(const uint64_t *S, const uint32_t *sz, const uint64_t *chunk_head,
                                               uint32_t max_chunks, uint64_t data_file_max, uint64_t *chunk_base,
                                               uint64_t *chunk_bytes, uint32_t *first, GcCounters *cnt) {
    const uint32_t lane = threadIdx.x;
    const uint32_t n = cnt->n;
    const uint64_t total = (uint64_t)cnt->t5[3] | ((uint64_t)cnt->t5[4] << 32);
    uint32_t c = 0, b = 0, end = n;
    uint64_t sf = 0, sb = 0;  // S[first[c]]; the bytes before record b
    const uint64_t h0 = chunk_head[0];
    uint64_t room = h0 > data_file_max ? 0 : data_file_max - h0;
    if (lane == 0) first[0] = 0;
    for (;;) {
        const uint32_t j = gc_search(S, sz, b, n, sb, room, lane);
        if (j == n) break;
        if (c + 1 == max_chunks) {
            end = j;
            break;
        }
        const uint64_t sj = S[j], szj = sz[j];
        if (lane == 0) chunk_base[c] = sf, chunk_bytes[c] = sj - sf;
        c++;
        if (lane == 0) first[c] = j;
        const uint64_t h = chunk_head[c];
        room = h > data_file_max || szj > data_file_max - h ? 0 : data_file_max - h - szj;
        sf = sj;
        sb = sj + szj;
        b = j + 1;
    }
    const uint64_t send = end == n ? total : S[end];
    if (lane == 0) {
        chunk_base[c] = sf, chunk_bytes[c] = send - sf;
        first[c + 1] = end;
        cnt->nch = c + 1;
        cnt->end = end;
        cnt->bytes = send;
    }
    for (uint32_t k = c + 1 + lane; k < max_chunks; k += 64) chunk_base[k] = send, chunk_bytes[k] = 0;
}

__global__ void __launch_bounds__(256) k_gc_place(const uint64_t *S, const uint32_t *first,
                                                  const uint64_t *chunk_head, const uint64_t *chunk_base,
                                                  int32_t *gc_status, uint32_t *new_chunk, uint64_t *new_off,
                                                  GcCounters *cnt) {
    const uint32_t n = cnt->n, nch = cnt->nch, end = cnt->end;
    uint32_t nplaced = 0, nnochunk = 0;
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        uint32_t c = 0;
        uint64_t o = 0;
        if (gc_status[j] == QLZX_GC_WRITTEN) {
            if (j >= end) {
                gc_status[j] = QLZX_GC_NO_CHUNK;
                nnochunk++;
            } else {
                uint32_t lo = 0, hi = nch;  // the last chunk whose first record is at or before j
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) / 2;
                    if (first[mid] <= j) lo = mid;
                    else hi = mid;
                }
                c = lo;
                o = chunk_head[c] + (S[j] - chunk_base[c]);
                nplaced++;
            }
        }
        new_chunk[j] = c;
        new_off[j] = o;
    }
    nplaced = wave_sum(nplaced), nnochunk = wave_sum(nnochunk);
    if ((threadIdx.x & 63) == 0) {
        if (nplaced) atomicAdd(&cnt->nplaced, nplaced);
        if (nnochunk) atomicAdd(&cnt->nnochunk, nnochunk);
    }
}

__global__ void k_gc_totals(uint32_t *totals, const GcCounters *cnt) {
    totals[0] = cnt->n;
    totals[1] = cnt->nkeep;
    totals[2] = cnt->nplaced;
    totals[3] = cnt->bytes ? cnt->nch : 0u;
    totals[4] = (uint32_t)cnt->bytes;
    totals[5] = (uint32_t)(cnt->bytes >> 32);
    totals[6] = 0;
    totals[7] = cnt->nbad + cnt->nnochunk;
}

// ---- rewrite ----
// The four 16-B chunks of the piece at record offset p that lie inside the span (zeros below r0).
__device__ __forceinline__ void gc_piece_load(const uint8_t *src, int64_t p, uint32_t r0, uint4 (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t xc = p + 16 * k;
        v[k] = xc >= (int64_t)r0 ? *(const uint4 *)(src + xc) : make_uint4(0, 0, 0, 0);
    }
}
// Copies the bytes [r0, r1) of the record at src to dst (r0, r1 multiples of 16; src and dst
// 16-B aligned; the CRC word, bytes 0..3, is left to the caller) and returns the raw CRC register
// of src[max(r0, 4), r1) from state 0, with the initial state ~0 folded into dword 1 when r0 == 0.
// wave_crc's layout anchored at the END of the span, as wr_span: lane l owns the 64-B piece l of
// every 4 KiB stripe of the virtual stream zeros ‖ src[r0, r1), one register over its pieces
// (x^(8*4032) between stripes), the 64 registers merged in a 6-level tree.  Every piece starts on
// a 16-B boundary of the record, so each of its four 16-B chunks lies wholly inside or outside
// the span: one aligned 16-B load and one aligned 16-B store per chunk.
// The next stripe's piece is loaded before the current one's CRC (a chain of dependent LDS
// lookups) runs, so a wave waits for the longer of the two latencies, not their sum.
__device__ uint32_t gc_span(const uint32_t *lds, const uint8_t *src, uint8_t *dst, uint32_t r0, uint32_t r1,
                            uint32_t lane) {
    const uint32_t *t8 = lds, *mul = lds + 8 * 256;
    const uint32_t nst = (r1 - r0 + kStripe - 1) / kStripe;
    const int64_t base = (int64_t)r1 - (int64_t)nst * kStripe;
    uint32_t c = 0;
    uint4 v[4], nx[4];
    if (nst) gc_piece_load(src, base + kPiece * lane, r0, nx);
    for (uint32_t t = 0; t < nst; t++) {
        const int64_t p = base + (int64_t)t * kStripe + kPiece * lane;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = nx[k];
        if (t + 1 < nst) gc_piece_load(src, p + kStripe, r0, nx);
        c = crc_mul_tab(mul + 6 * 1024, c);
        if (p + (int64_t)kPiece <= (int64_t)r0) continue;  // all leading zeros
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t xc = p + 16 * k;
            if (xc < (int64_t)r0) continue;
            uint32_t *d = (uint32_t *)(dst + xc);
            if (xc == 0) {  // the CRC word comes last (as store_rec_chunk); the initial state goes over dword 1
                d[1] = v[k].y, d[2] = v[k].z, d[3] = v[k].w;
                v[k].x = 0;
                v[k].y ^= 0xffffffffu;
            } else {
                *(uint4 *)d = v[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c = crc_slice8(t8, c, v[k].x, v[k].y);
            c = crc_slice8(t8, c, v[k].z, v[k].w);
        }
    }
    return crc_lane_merge(mul, c);
}

// The record's last bytes src[e16, end), fewer than 16, as four dwords (zeros past the end); never
// reads past `avail` = the bytes of the source buffer from src on.  Independent of the span: the
// callers load it before gc_span runs.
__device__ __forceinline__ uint4 gc_tail_load(const uint8_t *src, uint64_t avail, uint32_t e16, uint32_t end) {
    uint32_t w[4] = {0, 0, 0, 0};
    const uint32_t nb = end - e16;
    if (nb && avail - e16 >= 16) {
        const uint4 v = *(const uint4 *)(src + e16);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t in = nb > 4 * k ? nb - 4 * k : 0;  // bytes of dword k inside the record
            if (in < 4) w[k] &= in ? (1u << (8 * in)) - 1u : 0u;
        }
    } else {
#pragma unroll
        for (uint32_t b = 0; b < 15; b++)
            if (b < nb) w[b >> 2] |= (uint32_t)src[e16 + b] << (8 * (b & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// reg continued over the tail's end - e16 bytes, and the 16-B chunks from e16 to the padded end
// written, the padding zeros included.
__device__ uint32_t gc_tail(const uint32_t *t8, uint4 tail, uint8_t *dst, uint32_t e16, uint32_t end, uint32_t rsz,
                            uint32_t reg, uint32_t lane) {
    const uint32_t w[4] = {tail.x, tail.y, tail.z, tail.w};
#pragma unroll
    for (uint32_t b = 0; b < 15; b++)
        if (b < end - e16) reg = crc_byte(t8, reg, (w[b >> 2] >> (8 * (b & 3))) & 0xffu);
    const uint32_t xc = e16 + 16 * lane;
    if (xc < rsz) *(uint4 *)(dst + xc) = lane == 0 ? tail : make_uint4(0, 0, 0, 0);
    return reg;
}

struct GcIn {
    const uint8_t *data;
    uint64_t size;
    const uint64_t *rec_off, *chunk_head, *new_off, *chunk_base;
    const uint32_t *new_chunk;
    uint32_t max_chunks;
    uint8_t *out;
    uint64_t out_cap;
};
struct GcRec {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t avail;  // bytes of `data` from src on
    uint32_t end, rsz, stored;
    int32_t st;  // WRITTEN, or why not
};
// Record j in two dependent steps of loads, so that k_gc_copy can run them ahead of the record it
// is copying: GcIdx = its entries of the per-record arrays, GcHdr = what those lead to (the
// stored header and its chunk's base and head).  gc_rec then repeats the checks that keep every
// access inside `data` and `out` whatever the arrays hold.
struct GcIdx {
    int32_t st;
    uint32_t c;
    uint64_t off, noff;
};
struct GcHdr {
    bool ok;  // the header lies inside `data` and the chunk index inside the chunk arrays
    uint32_t stored, ksz, vsz;
    uint64_t cbase, chead;
};
__device__ __forceinline__ GcIdx gc_idx(const GcIn &in, const int32_t *gc_status, uint32_t j, uint32_t n) {
    GcIdx I;
    I.st = QLZX_GC_DROPPED, I.c = 0, I.off = 0, I.noff = 0;
    if (j < n) I.st = gc_status[j], I.c = in.new_chunk[j], I.off = in.rec_off[j], I.noff = in.new_off[j];
    return I;
}
__device__ __forceinline__ GcHdr gc_hdr(const GcIn &in, const GcIdx &I) {
    GcHdr H;
    H.stored = 0, H.ksz = 0, H.vsz = 0, H.cbase = 0, H.chead = 0;
    H.ok = I.st == QLZX_GC_WRITTEN && I.off % kRpSlot == 0 && I.off <= in.size && in.size - I.off >= kRpHdr &&
           I.c < in.max_chunks;
    if (H.ok) {
        const uint32_t *h = (const uint32_t *)(in.data + I.off);
        H.stored = h[0];
        const uint2 kv = *(const uint2 *)(h + 4);
        H.ksz = kv.x, H.vsz = kv.y;
        H.cbase = in.chunk_base[I.c], H.chead = in.chunk_head[I.c];
    }
    return H;
}
__device__ __forceinline__ GcRec gc_rec(const GcIn &in, const GcIdx &I, const GcHdr &H) {
    GcRec R;
    R.src = nullptr, R.dst = nullptr, R.avail = 0, R.end = 0, R.rsz = 0, R.stored = H.stored;
    R.st = QLZX_GC_BAD_RECORD;
    if (!H.ok) return R;
    R.src = in.data + I.off;
    R.avail = in.size - I.off;
    const uint64_t end = (uint64_t)kRpHdr + H.ksz + H.vsz;
    if (H.ksz == 0 || end > R.avail || end > 0xffffff00ull) return R;
    R.end = (uint32_t)end;
    R.rsz = (uint32_t)pad256(end);
    const uint64_t pos = H.cbase + (I.noff - H.chead);
    R.st = QLZX_GC_NO_SPACE;
    if (pos % kRpSlot != 0 || pos > in.out_cap || in.out_cap - pos < R.rsz) return R;
    R.dst = in.out + pos;
    R.st = QLZX_GC_WRITTEN;
    return R;
}

// k_gc_copy: a wave per record, grid-stride.  A record that would end past out_cap gets
// QLZX_GC_NO_SPACE and nothing of it is written; one whose CRC span exceeds kRpLong goes to the
// long list (k_rec_long<GcLong>).  What leads to a record's bytes is two dependent loads deep (its array entries,
// then its header and chunk), so a wave loads the entries of its record after next and the header
// of its next record before it copies the current one: in the steady state a record waits for its
// own bytes only.
__global__ void __launch_bounds__(256) k_gc_copy(GcIn in, const uint32_t *result, uint32_t cap, int32_t *gc_status,
                                                 uint32_t *crc, GcCounters *cnt, LongList ll) {
    __shared__ uint32_t tab[kCrcLdsWords];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = rec_count(result, cap);
    const uint32_t j0 = blockIdx.x * 4 + threadIdx.x / 64, stride = gridDim.x * 4;
    GcIdx I0 = gc_idx(in, gc_status, j0, n), I1 = gc_idx(in, gc_status, j0 + stride, n);
    GcHdr H0 = gc_hdr(in, I0);
    load_crc_lds(tab);
    __syncthreads();
    uint32_t nfail = 0, nmis = 0;
    unsigned long long failbytes = 0;
    for (uint32_t j = j0; j < n; j += stride) {
        const GcIdx I = I0;
        const GcHdr H = H0;
        I0 = I1;
        const uint64_t j2 = (uint64_t)j + 2 * (uint64_t)stride;
        I1 = gc_idx(in, gc_status, j2 < n ? (uint32_t)j2 : n, n);
        H0 = gc_hdr(in, I0);
        if (I.st != QLZX_GC_WRITTEN) {
            if (lane == 0) crc[j] = 0;
            continue;
        }
        const GcRec R = gc_rec(in, I, H);
        if (R.st != QLZX_GC_WRITTEN) {
            if (lane == 0) gc_status[j] = R.st, crc[j] = 0;
            nfail++;
            failbytes += R.rsz;
            continue;
        }
        if (R.end - 4 > kRpLong) {
            if (lane == 0) ll.push(j);
            continue;
        }
        const uint32_t e16 = R.end & ~15u;
        const uint4 tail = gc_tail_load(R.src, R.avail, e16, R.end);
        uint32_t reg = gc_span(tab, R.src, R.dst, 0, e16, lane);
        reg = gc_tail(tab, tail, R.dst, e16, R.end, R.rsz, reg, lane);
        if (lane == 0) {
            *(uint32_t *)R.dst = ~reg;
            crc[j] = ~reg;
        }
        nmis += ~reg != R.stored;
    }
    if (lane == 0) {
        if (nfail) {
            atomicAdd(&cnt->nfail, nfail);
            atomicAdd(&cnt->failbytes, failbytes);
        }
        if (nmis) atomicAdd(&cnt->nmis, nmis);
    }
}

// k_rec_long's policy: a long record's segments are spans of its source bytes, the last one with
// the tail (loaded before the span runs, as in k_gc_copy).
struct GcLong {
    GcIn in;
    uint32_t *crc, *nmis;
    using Rec = GcRec;
    __device__ Rec rec(uint32_t j) const {
        GcIdx I;  // k_gc_copy lists WRITTEN records only
        I.st = QLZX_GC_WRITTEN, I.c = in.new_chunk[j], I.off = in.rec_off[j], I.noff = in.new_off[j];
        return gc_rec(in, I, gc_hdr(in, I));
    }
    __device__ bool valid(const Rec &R) const { return R.st == QLZX_GC_WRITTEN; }  // k_gc_copy's answer again
    __device__ uint32_t end(const Rec &R) const { return R.end; }
    __device__ uint32_t segment(const uint32_t *lds, const Rec &R, uint32_t r0, uint32_t r1, bool last,
                                uint32_t lane) const {
        uint4 tail = make_uint4(0, 0, 0, 0);
        if (last) tail = gc_tail_load(R.src, R.avail, r1, R.end);
        const uint32_t reg = gc_span(lds, R.src, R.dst, r0, r1, lane);
        return last ? gc_tail(lds, tail, R.dst, r1, R.end, R.rsz, reg, lane) : reg;
    }
    __device__ void finish(uint32_t j, const Rec &R, uint32_t sum) const {
        *(uint32_t *)R.dst = ~sum;
        crc[j] = ~sum;
        if (~sum != R.stored) atomicAdd(nmis, 1u);
    }
};

__global__ void k_gc_totals2(uint32_t *totals, const uint32_t *result, const GcCounters *cnt) {
    if (result[0] == 0) {
        for (int k = 0; k < 8; k++) totals[k] = 0;
        return;
    }
    const uint64_t bytes = ((uint64_t)totals[4] | ((uint64_t)totals[5] << 32)) - cnt->failbytes;
    totals[2] -= cnt->nfail;
    totals[4] = (uint32_t)bytes;
    totals[5] = (uint32_t)(bytes >> 32);
    totals[6] = cnt->nmis;
    totals[7] += cnt->nfail;
}

// ---- workspace: the counters, the sizes and their scan, the chunks' first records, the long list ----
struct GcWs {
    GcCounters *cnt;
    uint32_t *sz, *first, *lng, *lacc, *ldone;
    uint64_t *S;
};
inline size_t gc_ws_layout(uint32_t cap, uint32_t max_chunks, uint8_t *base, GcWs *w) {
    WsCarver c{base};
    GcWs t;
    t.cnt = c.take<GcCounters>(sizeof(GcCounters));
    t.sz = c.take<uint32_t>(4 * (size_t)cap);
    t.first = c.take<uint32_t>(4 * ((size_t)max_chunks + 1));
    t.lng = c.take<uint32_t>(4 * (size_t)cap);
    t.lacc = c.take<uint32_t>(4 * (size_t)cap);
    t.ldone = c.take<uint32_t>(4 * (size_t)cap);
    t.S = c.take<uint64_t>(8 * (size_t)cap);
    if (w) *w = t;
    return c.bytes();
}

inline int launch_gc_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, const uint32_t *result,
                          uint32_t cap, const uint8_t *keep, uint32_t max_key, uint64_t body_max,
                          uint64_t data_file_max, const uint64_t *chunk_head, uint32_t max_chunks, int32_t *gc_status,
                          uint32_t *new_chunk, uint64_t *new_off, uint64_t *chunk_base, uint64_t *chunk_bytes,
                          uint32_t *totals, void *ws, hipStream_t s) {
    GcWs w;
    gc_ws_layout(cap, max_chunks, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(GcCounters), s);
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = grid_for(cap);
    hipLaunchKernelGGL(k_gc_check, dim3(grid), dim3(256), 0, s, data, size, rec_off, result, cap, keep, max_key,
                       body_max, gc_status, w.sz, w.cnt);
    // S: the exclusive scan of the padded sizes (0 for a record that takes no space)
    hipLaunchKernelGGL(k_rp_dstoff, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.sz, (const uint32_t *)&w.cnt->n,
                       w.S, &w.cnt->t5[0], (const uint32_t *)&w.cnt->n);
    hipLaunchKernelGGL(k_gc_cut, dim3(1), dim3(64), 0, s, (const uint64_t *)w.S, (const uint32_t *)w.sz, chunk_head,
                       max_chunks, data_file_max, chunk_base, chunk_bytes, w.first, w.cnt);
    hipLaunchKernelGGL(k_gc_place, dim3(grid), dim3(256), 0, s, (const uint64_t *)w.S, (const uint32_t *)w.first,
                       chunk_head, (const uint64_t *)chunk_base, gc_status, new_chunk, new_off, w.cnt);
    hipLaunchKernelGGL(k_gc_totals, dim3(1), dim3(1), 0, s, totals, (const GcCounters *)w.cnt);
    return (int)hipGetLastError();
}

inline int launch_gc_rewrite(const GcIn &in, const uint32_t *result, uint32_t cap, int32_t *gc_status, uint32_t *crc,
                             uint32_t *totals, void *ws, hipStream_t s) {
    GcWs w;
    gc_ws_layout(cap, in.max_chunks, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(GcCounters), s);
    if (e != hipSuccess) return (int)e;
    const LongList ll{&w.cnt->nlong, w.lng, w.lacc, w.ldone};
    hipLaunchKernelGGL(k_gc_copy, dim3(grid_for(cap, 4, 2048)), dim3(256), 0, s, in, result, cap, gc_status, crc,
                       w.cnt, ll);
    hipLaunchKernelGGL(k_rec_long<GcLong>, dim3(2048), dim3(256), 0, s, GcLong{in, crc, &w.cnt->nmis}, ll);
    hipLaunchKernelGGL(k_gc_totals2, dim3(1), dim3(1), 0, s, totals, result, (const GcCounters *)w.cnt);
    return (int)hipGetLastError();
}

}  // namespace qlzx
