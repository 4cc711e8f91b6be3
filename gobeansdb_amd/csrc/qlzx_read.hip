// qlzx_read.hip -- batched record reads at offsets the caller already knows (a multi-GET):
// readRecordAt (store/datafile.go:114-170) for every request of a list, as
// dataChunk.GetRecordByOffset runs it once per key of a memcache "get k1 k2 ..."
// (store/bucket.go:405-499, store/datachunk.go:150-169) and GC's collision path does
// (store/gc.go:300), then Payload.Decompress (store/item.go:163-176) through the batch decoder.
//
// Three steps around qlzx_decompress_batch, like the replay's:
//   check   k_rd_check: per request the size checks in readRecordAt's order and the record CRC;
//           records with a CRC span over kRpLong go through k_rp_crc_long (qlzx_replay.hip),
//           listed by request index (LongList, qlzx_recfile.h);
//   plan    the requests that passed and carry FLAG_COMPRESS, compacted in request order
//           (launch_compact and k_rp_dstoff of qlzx_recfile.h, the replay's ScatterComp);
//   finish  the replay's finish kernels under a validity predicate: failed requests get zeros.
// The CRC is checked BEFORE the plan, not fused into the decoder: it is readRecordAt's order, and
// the QuickLZ header of a body that fails its CRC (it can claim up to BodyMax) must never size
// the output buffer or route the batch to the whole-GPU decoder.
#include "qlzx_recfile.h"

namespace qlzx {

struct RdCounters {
    uint32_t nlong, nok, ncomp, pad[5];
};

// k_rd_check: a wave takes 64 consecutive requests at a time (the launch shape of k_rp_scan: the
// CRC tables in LDS once per workgroup, a grid-stride loop over 64-request groups).  One header
// load per lane classifies them; the survivors are CRCed one at a time by the whole wave
// (wave_crc: any alignment and length).  The first failing check of readRecordAt's order is the
// verdict (rec_pos_verdict, then rec_size_verdict, then the CRC):
//   rec_off % 256 != 0                QLZX_RD_ALIGN       positions are in units of 256, store/leaf.go:56-65
//   rec_off + 24 > size               QLZX_RD_EOF_HEADER  store/datafile.go:123
//   ksz == 0 || ksz > max_key         QLZX_RD_KEY_SIZE    :129, config/mc_config.go:33-35
//   vsz > body_max                    QLZX_RD_VALUE_SIZE  :133
//   rec_off + 24 + ksz + vsz > size   QLZX_RD_EOF_BODY    :149
//   ~crc(header[4:24] ‖ key ‖ value) != header[0:4]   QLZX_RD_CRC   :161-168
// hdr[6 i ..] is the stored header (zeros for ALIGN / EOF_HEADER: nothing was read).  With wanted
// keys, key_eq[i] = 1 iff the request is OK and its key equals the wanted one (bytes.Compare,
// store/bucket.go:442); a long record's key_eq is provisional until k_rp_crc_long's verdict.
__global__ void __launch_bounds__(256) k_rd_check(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t n,
                                                  uint32_t max_key, uint64_t body_max, const uint8_t *want_key,
                                                  const uint64_t *want_key_off, const uint32_t *want_key_len,
                                                  int32_t *rd_status, uint8_t *key_eq, int32_t *hdr, RdCounters *cnt,
                                                  LongList ll) {
    __shared__ uint32_t tab[kCrcLdsWords];
    load_crc_lds(tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ngroups = (n + 63) / 64;
    uint32_t nok = 0;
    for (uint32_t g = blockIdx.x * 4 + threadIdx.x / 64; g < ngroups; g += gridDim.x * 4) {
        const uint32_t i = g * 64 + lane;
        const bool in = i < n;
        const uint64_t off = in ? rec_off[i] : 0;
        int32_t st = QLZX_RD_ALIGN;
        uint32_t h[6] = {0, 0, 0, 0, 0, 0};
        if (in) {
            RecVerdict v = rec_pos_verdict(off, size);
            if (v == kRecOk) {
                const uint2 *q = (const uint2 *)(data + off);  // records are 256-B aligned
                const uint2 a = q[0], b = q[1], c = q[2];
                h[0] = a.x, h[1] = a.y, h[2] = b.x, h[3] = b.y, h[4] = c.x, h[5] = c.y;
                v = rec_size_verdict(h[4], h[5], size - off - kRpHdr, max_key, body_max);
            }
            st = v;  // QLZX_RD_OK so far: the CRC decides
#pragma unroll
            for (int k = 0; k < 6; k++) hdr[6 * (uint64_t)i + k] = (int32_t)h[k];
            if (st != QLZX_RD_OK) {
                rd_status[i] = st;
                if (key_eq) key_eq[i] = 0;
            }
        }
        uint64_t m = __ballot(in && st == QLZX_RD_OK);
        while (m) {
            const uint32_t L = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t ic = g * 64 + L;
            const uint8_t *rec = data + __shfl(off, L, 64);
            const uint32_t crc0 = __shfl(h[0], L, 64), ksz = __shfl(h[4], L, 64), vsz = __shfl(h[5], L, 64);
            uint32_t keq = 0;
            if (want_key && want_key_len[ic] == ksz) {
                const uint8_t *wk = want_key + want_key_off[ic];
                bool diff = false;
                for (uint32_t b = lane; b < ksz; b += 64) diff |= rec[kRpHdr + b] != wk[b];
                keq = __ballot(diff) == 0;
            }
            const uint32_t len = 20 + ksz + vsz;  // header[4:24] ‖ key ‖ value
            if (len > kRpLong) {
                if (lane == 0) {
                    ll.push(ic);
                    if (key_eq) key_eq[ic] = (uint8_t)keq;
                }
                continue;
            }
            const uint32_t reg = wave_crc(tab, rec + 4, len, 0xffffffffu, lane);
            if (lane == 0) {
                const bool ok = (reg ^ 0xffffffffu) == crc0;
                rd_status[ic] = ok ? QLZX_RD_OK : QLZX_RD_CRC;
                if (key_eq) key_eq[ic] = (uint8_t)(ok && keq);
                nok += ok;
            }
        }
    }
    if (lane == 0 && nok) atomicAdd(&cnt->nok, nok);
}

// k_rp_crc_long's policy for a list of request indices
struct RdLongReqs {
    const uint64_t *rec_off;
    int32_t *rd_status;
    uint8_t *key_eq;
    uint32_t *nok;
    __device__ const uint8_t *rec(const uint8_t *data, uint32_t i) const { return data + rec_off[i]; }
    __device__ void verdict(const uint8_t *h, uint32_t i, uint32_t, uint32_t, uint32_t reg) const {
        const bool ok = (reg ^ 0xffffffffu) == *(const uint32_t *)h;
        rd_status[i] = ok ? QLZX_RD_OK : QLZX_RD_CRC;
        if (ok) atomicAdd(nok, 1u);
        else if (key_eq) key_eq[i] = 0;
    }
};

struct RdCompFlag {  // request i passed and its record carries FLAG_COMPRESS (hdr = k_rd_check's)
    const int32_t *rd_status, *hdr;
    __device__ uint32_t operator()(uint32_t i) const {
        return rd_status[i] == QLZX_RD_OK && ((uint32_t)hdr[6 * (uint64_t)i + 2] & kFlagCompress) ? 1u : 0u;
    }
};
struct RdOkRequests {  // the finish kernels' predicate: n requests, the failed ones get zeros
    uint32_t count;
    const int32_t *rd_status;
    __device__ uint32_t n() const { return count; }
    __device__ bool ok(uint32_t i) const { return rd_status[i] == QLZX_RD_OK; }
};

// ---- workspace: the counters, the long list with its accumulators, the scan tiles ----
struct RdWs {
    RdCounters *cnt;
    uint32_t *lng, *lacc, *ldone, *tiles;
};
inline size_t read_ws_layout(uint32_t n, uint8_t *base, RdWs *w) {
    WsCarver c{base};
    RdWs t;
    t.cnt = c.take<RdCounters>(sizeof(RdCounters));
    t.lng = c.take<uint32_t>(4 * (size_t)n);
    t.lacc = c.take<uint32_t>(4 * (size_t)n);
    t.ldone = c.take<uint32_t>(4 * (size_t)n);
    t.tiles = c.take<uint32_t>(4 * ((size_t)n / kScanTile + 2));
    if (w) *w = t;
    return c.bytes();
}

inline int launch_read_plan(const uint8_t *data, uint64_t size, const uint64_t *rec_off, uint32_t n, uint32_t max_key,
                            uint64_t body_max, const uint8_t *want_key, const uint64_t *want_key_off,
                            const uint32_t *want_key_len, int32_t *rd_status, uint8_t *key_eq, int32_t *hdr,
                            uint32_t *comp_idx, uint64_t *comp_off, uint32_t *comp_len, uint32_t *comp_dsize,
                            uint64_t *comp_dst_off, uint32_t *totals, void *ws, hipStream_t s) {
    if (n == 0) return (int)hipMemsetAsync(totals, 0, 5 * sizeof(uint32_t), s);
    RdWs w;
    read_ws_layout(n, (uint8_t *)ws, &w);
    hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(RdCounters), s);
    if (e != hipSuccess) return (int)e;
    const LongList ll{&w.cnt->nlong, w.lng, w.lacc, w.ldone};
    hipLaunchKernelGGL(k_rd_check, dim3(grid_for((n + 63) / 64, 4, 2048)), dim3(256), 0, s, data, size, rec_off, n,
                       max_key, body_max, want_key, want_key_off, want_key_len, rd_status, key_eq, hdr, w.cnt, ll);
    hipLaunchKernelGGL(k_rp_crc_long<RdLongReqs>, dim3(2048), dim3(256), 0, s, data,
                       RdLongReqs{rec_off, rd_status, key_eq, &w.cnt->nok}, ll);
    // the compressed survivors in request order, then their destination offsets and the totals
    launch_compact(RdCompFlag{rd_status, hdr}, ScatterComp{data, rec_off, comp_idx, comp_len, comp_dsize, comp_off}, n,
                   w.tiles, &w.cnt->ncomp, s);
    hipLaunchKernelGGL(k_rp_dstoff, dim3(1), dim3(1024), 0, s, (const uint32_t *)comp_dsize,
                       (const uint32_t *)&w.cnt->ncomp, comp_dst_off, totals, (const uint32_t *)&w.cnt->nok);
    return (int)hipGetLastError();
}

inline int launch_read_finish(const uint8_t *data, const uint64_t *rec_off, uint32_t n, const int32_t *rd_status,
                              const uint32_t *totals, const uint32_t *comp_idx, const int32_t *cstatus,
                              const uint32_t *cdsize, const uint64_t *cdst_off, const uint8_t *outbuf, int32_t *flag,
                              int32_t *value_len, uint8_t *in_out, uint64_t *val_off, uint16_t *vh,
                              int32_t *dec_status, hipStream_t s) {
    if (n == 0) return 0;
    static_assert(QLZX_OK == 0, "dec_status is cleared with a memset");
    const hipError_t e = hipMemsetAsync(dec_status, 0, (size_t)n * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = grid_for(n);
    const RdOkRequests ok{n, rd_status};
    hipLaunchKernelGGL(k_rp_finish_vals<RdOkRequests>, dim3(grid), dim3(256), 0, s, data, rec_off, ok, flag, value_len,
                       in_out, val_off);
    hipLaunchKernelGGL(k_rp_finish_comp, dim3(grid), dim3(256), 0, s, totals + 1, comp_idx, cstatus, cdsize, cdst_off,
                       flag, value_len, in_out, val_off, dec_status);
    hipLaunchKernelGGL(k_rp_vhash2<RdOkRequests>, dim3(grid), dim3(256), 0, s, data, outbuf, ok,
                       (const uint8_t *)in_out, (const uint64_t *)val_off, (const int32_t *)value_len, vh);
    return (int)hipGetLastError();
}

}  // namespace qlzx
