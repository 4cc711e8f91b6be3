// qlzx_write.hip -- batched record writes (a multi-SET), the mirror image of qlzx_read.hip:
// Record.TryCompress (store/item.go:120-161) for every value of a list, then
// WriteRecord.encodeHeader / getCRC / append with the 256-B padding (store/datafile.go:66-88,
// 307-330), as dataChunk.flush runs them once per queued record (store/datachunk.go:88-120).
//
// Three steps around two qlzx_compress_batch calls:
//   plan    k_wr_plan: per record the size limits qlzx_read_plan enforces and TryCompress's
//           candidate test with http.DetectContentType's audio/video rows on the value's first
//           bytes; the candidates compacted in record order (launch_compact) into the
//           trial list, each destination len + 400 apart (k_rp_dstoff);
//   decide  k_wr_decide: float32(csize) / float32(try_len) <= 0.7 per trial; the kept ones longer
//           than the trial, compacted into the full-recompress list;
//   finish  sizes, flags and offsets (k_wr_sizes, k_wr_apply, k_rp_dstoff), then k_wr_assemble: a
//           wave per record writes header, key, value, CRC word and padding; a plain value's CRC
//           is computed in the pass that copies it, a compressed value's comes from the compressor
//           (fused, state 0) and is combined with the prefix's; records with a CRC span over
//           kRpLong are cut into kRpSeg segments over the chip (k_rec_long<WrLong>).
#include "qlzx_recfile.h"

namespace qlzx {

constexpr uint32_t kFlagClientCompress = 0x00000010u;
constexpr uint32_t kTryCompressSize = 10u << 10;  // store/item.go:139
constexpr uint32_t kWrPad = 400;                  // compress destinations: len + 400 (quicklz.h)

struct WrCounters {
    uint32_t nok, nkeep, nlong, nwritten, n, zero;
    unsigned long long bound, bytes;
    uint32_t t5[10];  // k_rp_dstoff's totals; pads the struct to a multiple of 16 bytes
};

// The row of http.DetectContentType's audio/video table (Go 1.13 net/http/sniff.go, in table
// order: audio/basic, audio/aiff, audio/mpeg, application/ogg, audio/midi, video/avi, audio/wave)
// the value's first bytes match, 7 for any other answer.  The first matching row decides; a value
// shorter than a row's pattern cannot match it.
__device__ __forceinline__ uint32_t wr_sniff(const uint8_t *v, uint32_t len) {
    uint8_t b[12];
#pragma unroll
    for (uint32_t k = 0; k < 12; k++) b[k] = k < len ? v[k] : 0;
    auto eq4 = [&](uint32_t o, char c0, char c1, char c2, char c3) {
        return b[o] == (uint8_t)c0 && b[o + 1] == (uint8_t)c1 && b[o + 2] == (uint8_t)c2 && b[o + 3] == (uint8_t)c3;
    };
    if (len >= 4 && eq4(0, '.', 's', 'n', 'd')) return 0;
    if (len >= 12 && eq4(0, 'F', 'O', 'R', 'M') && eq4(8, 'A', 'I', 'F', 'F')) return 1;
    if (len >= 3 && b[0] == 'I' && b[1] == 'D' && b[2] == '3') return 2;
    if (len >= 5 && eq4(0, 'O', 'g', 'g', 'S') && b[4] == 0) return 3;
    if (len >= 8 && eq4(0, 'M', 'T', 'h', 'd') && eq4(4, 0, 0, 0, 6)) return 4;
    if (len >= 12 && eq4(0, 'R', 'I', 'F', 'F') && eq4(8, 'A', 'V', 'I', ' ')) return 5;
    if (len >= 12 && eq4(0, 'R', 'I', 'F', 'F') && eq4(8, 'W', 'A', 'V', 'E')) return 6;
    return 7;
}

// plan: the verdict and the candidate flag of every record; the count of OK records and the sum
// of their output bounds pad256(24 + ksz + vlen + 9) (a kept value can be a stored QuickLZ block,
// 9 bytes longer than the plain one).
__global__ void __launch_bounds__(256) k_wr_plan(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len,
                                                 const uint32_t *key_len, const uint32_t *flag, const int32_t *ver,
                                                 uint32_t n, uint32_t max_key, uint64_t body_max, uint32_t not_compress,
                                                 int32_t *wr_status, uint8_t *cand, WrCounters *cnt) {
    uint32_t nok = 0;
    unsigned long long bound = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t ksz = key_len[i], vlen = val_len[i];
        int32_t st = QLZX_WR_OK;
        if (ksz == 0 || ksz > max_key) st = QLZX_WR_KEY_SIZE;
        else if ((uint64_t)vlen > body_max) st = QLZX_WR_VALUE_SIZE;
        bool c = false;
        if (st == QLZX_WR_OK) {
            const uint64_t plain = (uint64_t)kRpHdr + ksz + vlen;
            nok++;
            bound += pad256(plain + 9);
            c = ver[i] >= 0 && (flag[i] & (kFlagClientCompress | kFlagCompress)) == 0 && pad256(plain) > kRpSlot;
            if (c) c = ((not_compress >> wr_sniff(values + val_off[i], vlen)) & 1u) == 0;
        }
        wr_status[i] = st;
        cand[i] = c;
    }
    nok = wave_sum(nok), bound = wave_sum(bound);
    if ((threadIdx.x & 63) == 0 && nok) {
        atomicAdd(&cnt->nok, nok);
        atomicAdd(&cnt->bound, bound);
    }
}

struct WrCandFlag {
    const uint8_t *cand;
    __device__ uint32_t operator()(uint32_t i) const { return cand[i]; }
};
struct ScatterTry {  // trial k = the k-th candidate: min(vlen, 10 KiB) of its value
    const uint64_t *val_off;
    const uint32_t *val_len;
    uint32_t *try_idx, *try_len, *cap;
    uint64_t *try_off;
    __device__ void operator()(uint32_t i, uint32_t idx, uint32_t v) const {
        if (!v) return;
        const uint32_t t = val_len[i] < kTryCompressSize ? val_len[i] : kTryCompressSize;
        try_idx[idx] = i;
        try_off[idx] = val_off[i];
        try_len[idx] = t;
        cap[idx] = t + kWrPad;
    }
};
// k_rp_dstoff's totals {first, count, max cap, bytes lo, hi} -> max length; the plan adds its bound
__global__ void k_wr_totals(uint32_t *totals, const WrCounters *cnt, int with_bound) {
    totals[2] = totals[1] ? totals[2] - kWrPad : 0u;
    if (with_bound) {
        totals[5] = (uint32_t)cnt->bound;
        totals[6] = (uint32_t)(cnt->bound >> 32);
    }
}

// decide: keep[k] = the trial compressed and float32(csize) / float32(try_len) <= 0.7
// (store/item.go:145: IEEE single division and compare); a failed compress is "not compressed".
__global__ void __launch_bounds__(256) k_wr_decide(const uint32_t *totals, const uint32_t *try_len,
                                                   const uint32_t *try_csize, const int32_t *try_status, uint8_t *keep,
                                                   WrCounters *cnt) {
    const uint32_t ntry = totals[1];
    uint32_t nkeep = 0;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < ntry; k += gridDim.x * 256) {
        const bool kp = try_status[k] == QLZX_OK && __fdiv_rn((float)try_csize[k], (float)try_len[k]) <= 0.7f;
        keep[k] = kp;
        nkeep += kp;
    }
    nkeep = wave_sum(nkeep);
    if ((threadIdx.x & 63) == 0 && nkeep) atomicAdd(&cnt->nkeep, nkeep);
}
struct WrFullFlag {  // a kept trial that saw only the first 10 KiB: recompress the whole value
    const uint32_t *totals, *try_idx, *try_len, *val_len;
    const uint8_t *keep;
    __device__ uint32_t operator()(uint32_t k) const {
        return k < totals[1] && keep[k] && val_len[try_idx[k]] > try_len[k] ? 1u : 0u;
    }
};
struct ScatterFull {
    const uint32_t *try_idx, *val_len;
    const uint64_t *val_off;
    uint32_t *full_idx, *full_len, *cap;
    uint64_t *full_off;
    __device__ void operator()(uint32_t k, uint32_t idx, uint32_t v) const {
        if (!v) return;
        const uint32_t i = try_idx[k];
        full_idx[idx] = i;
        full_off[idx] = val_off[i];
        full_len[idx] = val_len[i];
        cap[idx] = val_len[i] + kWrPad;
    }
};

// ---- finish ----
// Where a record's stored value comes from: sel 0 = values, 1 = the trial buffer, 2 = the full
// buffer; vcrc = the compressor's fused raw CRC of it (sel != 0).
__global__ void __launch_bounds__(256) k_wr_sizes(const uint64_t *val_off, const uint32_t *val_len,
                                                  const uint32_t *key_len, const uint32_t *flag,
                                                  const int32_t *wr_status, uint32_t n, uint32_t *flag_out,
                                                  uint32_t *vsz, uint32_t *sz, uint32_t *sel, uint64_t *soff,
                                                  WrCounters *cnt) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const bool ok = wr_status[i] == QLZX_WR_OK;
        flag_out[i] = ok ? flag[i] : 0u;
        vsz[i] = ok ? val_len[i] : 0u;
        sz[i] = ok ? kRpHdr + key_len[i] + val_len[i] : 0u;
        sel[i] = 0;
        soff[i] = val_off[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->n = n;
}
// threads [0, ntry): kept trials whose output is the value; [ntry, ntry + nfull): the full
// compresses that succeeded (a failed one leaves the value raw, as the reference's !ok branch)
__global__ void __launch_bounds__(256) k_wr_apply(const uint32_t *totals, const uint32_t *try_idx,
                                                  const uint32_t *try_len, const uint64_t *try_dst_off,
                                                  const uint32_t *try_csize, const uint32_t *try_crc,
                                                  const uint8_t *keep, const uint32_t *totals2,
                                                  const uint32_t *full_idx, const uint64_t *full_dst_off,
                                                  const uint32_t *full_csize, const int32_t *full_status,
                                                  const uint32_t *full_crc, const uint32_t *val_len,
                                                  const uint32_t *key_len, uint32_t *flag_out, uint32_t *vsz,
                                                  uint32_t *sz, uint32_t *sel, uint64_t *soff, uint32_t *vcrc) {
    const uint32_t ntry = totals[1], nfull = totals2[1];
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < ntry + nfull; t += gridDim.x * 256) {
        uint32_t i, c, s, raw;
        uint64_t o;
        if (t < ntry) {
            i = try_idx[t];
            if (!keep[t] || val_len[i] > try_len[t]) continue;
            c = try_csize[t], s = 1, o = try_dst_off[t], raw = ~try_crc[t];
        } else {
            const uint32_t j = t - ntry;
            if (full_status[j] != QLZX_OK) continue;
            i = full_idx[j];
            c = full_csize[j], s = 2, o = full_dst_off[j], raw = ~full_crc[j];
        }
        flag_out[i] += kFlagCompress;  // store/item.go:159
        vsz[i] = c;
        sz[i] = kRpHdr + key_len[i] + c;
        sel[i] = s;
        soff[i] = o;
        vcrc[i] = raw;
    }
}

// One record's image: crc placeholder ‖ ts ‖ flag ‖ ver ‖ ksz ‖ vsz ‖ key ‖ value ‖ zeros.
struct WrRec {
    uint32_t h[5];  // ts, flag, ver, ksz, vsz
    const uint8_t *key, *val;
    uint32_t vstart, end;  // 24 + ksz, 24 + ksz + vsz
    bool vzero;            // the value's CRC comes from the compressor: its bytes count as zeros
    __device__ __forceinline__ uint32_t byte(uint32_t x) const {
        if (x < 4) return 0;
        if (x < kRpHdr) {
            const uint32_t k = x >> 2;
            const uint32_t w = k == 1 ? h[0] : k == 2 ? h[1] : k == 3 ? h[2] : k == 4 ? h[3] : h[4];
            return (w >> (8 * (x & 3))) & 0xffu;
        }
        if (x < vstart) return key[x - kRpHdr];
        if (x < end) return val[x - vstart];
        return 0;
    }
};

// Writes the image bytes [r0, r1) of record R to rec (r0, r1 multiples of 16; the CRC word itself,
// bytes 0..3, is left to the caller) and returns the raw CRC register of image[max(r0, 4), r1)
// from state 0, with the initial state ~0 folded into the span's first dword when r0 == 0.
// The layout is wave_crc's, anchored at the END of the span so that every piece starts on a
// 16-B boundary of the record: lane l owns the 64-B piece l of every 4 KiB stripe of the virtual
// stream zeros ‖ image[r0, r1), keeps one register over its pieces (x^(8*4032) between stripes)
// and the 64 registers merge in a 6-level tree.  A piece that lies inside the value is read as
// dwords at 4-aligned source addresses, byte-aligned with v_alignbyte and stored as four 16-B
// stores; the pieces with header, key, the value's edges or bytes below r0 are composed bytewise.
// With R.vzero the value bytes count as zeros: the result is the prefix register shifted over the
// value, to be XORed with the compressor's raw CRC of it.
__device__ uint32_t wr_span(const uint32_t *lds, const WrRec &R, uint8_t *rec, uint32_t r0, uint32_t r1,
                            uint32_t lane) {
    const uint32_t *t8 = lds, *mul = lds + 8 * 256;
    const uint32_t nst = (r1 - r0 + kStripe - 1) / kStripe;
    const int64_t base = (int64_t)r1 - (int64_t)nst * kStripe;
    uint32_t c = 0;
    for (uint32_t t = 0; t < nst; t++) {
        const int64_t p = base + (int64_t)t * kStripe + kPiece * lane;
        c = crc_mul_tab(mul + 6 * 1024, c);
        if (p + (int64_t)kPiece <= (int64_t)r0) continue;  // all leading zeros
        uint32_t w[17], cw[16];
        const bool inner = p >= (int64_t)r0 && p >= (int64_t)R.vstart && p + kPiece <= (int64_t)R.end;
        if (inner) {
            const uint8_t *s = R.val + ((uint32_t)p - R.vstart);
            const uint32_t m = (uint32_t)((uintptr_t)s & 3u);
            const uint4 *q4 = (const uint4 *)(s - m);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint4 v = q4[k];
                w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
            }
            w[16] = m ? ((const uint32_t *)(s - m))[16] : 0u;
            if (m) {
#pragma unroll
                for (int k = 0; k < 16; k++) w[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], m);
            }
            uint4 *d = (uint4 *)(rec + p);
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
            if (R.vzero) {  // 64 zero bytes: x^(8*64), the tree's first table
                c = crc_mul_tab(mul, c);
                continue;
            }
#pragma unroll
            for (int k = 0; k < 16; k++) cw[k] = w[k];
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                uint32_t word = 0, cword = 0;
                for (int b = 0; b < 4; b++) {
                    const int64_t x = p + 4 * k + b;
                    if (x < (int64_t)r0) continue;
                    const uint32_t v = R.byte((uint32_t)x) << (8 * b);
                    word |= v;
                    if (!(R.vzero && x >= (int64_t)R.vstart)) cword |= v;
                }
                if (p + 4 * k == 4) cword ^= 0xffffffffu;  // the initial state over the span's first dword
                w[k] = word, cw[k] = cword;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t xc = p + 16 * k;
                if (xc < (int64_t)r0) continue;
                store_rec_chunk(rec + xc, make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]), xc == 0);
            }
        }
#pragma unroll
        for (int k = 0; k < 16; k += 2) c = crc_slice8(t8, c, cw[k], cw[k + 1]);
    }
    return crc_lane_merge(mul, c);
}

// The record's last bytes: reg continued over image[e16, end) (fewer than 16 bytes), and the
// 16-B chunks from e16 to the padded end written, the padding zeros included.
__device__ uint32_t wr_tail(const uint32_t *t8, const WrRec &R, uint8_t *rec, uint32_t e16, uint32_t rsz,
                            uint32_t reg, uint32_t lane) {
    for (uint32_t x = e16; x < R.end; x++) reg = crc_byte(t8, reg, R.vzero && x >= R.vstart ? 0u : R.byte(x));
    const uint32_t xc = e16 + 16 * lane;
    if (xc < rsz) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (lane == 0)
            for (uint32_t b = 0; b < 16 && e16 + b < R.end; b++) w[b >> 2] |= R.byte(e16 + b) << (8 * (b & 3));
        *(uint4 *)(rec + xc) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return reg;
}

struct WrIn {
    const uint8_t *values, *keys, *trial_buf, *full_buf;
    const uint64_t *key_off;
    const uint32_t *key_len, *ts;
    const int32_t *ver;
    const uint32_t *flag_out, *vsz, *sel, *vcrc;
    const uint64_t *soff, *rec_off;
    __device__ __forceinline__ WrRec rec(uint32_t i) const {
        WrRec R;
        const uint32_t ksz = key_len[i], v = vsz[i], s = sel[i];
        R.h[0] = ts[i], R.h[1] = flag_out[i], R.h[2] = (uint32_t)ver[i], R.h[3] = ksz, R.h[4] = v;
        R.key = keys + key_off[i];
        R.val = (s == 0 ? values : s == 1 ? trial_buf : full_buf) + soff[i];
        R.vstart = kRpHdr + ksz;
        R.end = kRpHdr + ksz + v;
        R.vzero = s != 0;
        return R;
    }
};

// k_wr_assemble: a wave per record, grid-stride.  Failed records get zeros; a record that would
// end past out_cap gets QLZX_WR_NO_SPACE and writes nothing; one whose CRC span exceeds kRpLong
// goes to the long list (k_rec_long<WrLong>).
__global__ void __launch_bounds__(256) k_wr_assemble(WrIn in, uint32_t n, uint8_t *out, uint64_t out_cap,
                                                     int32_t *wr_status, uint64_t *rec_off, uint32_t *flag_out,
                                                     uint32_t *vsz, uint32_t *crc, WrCounters *cnt, uint32_t *lng,
                                                     uint32_t *lacc, uint32_t *ldone) {
    // the list's arrays one by one, its counter taken from cnt: the kernel sits at the SGPR limit,
    // and a fourth pointer argument costs a VGPR
    const LongList ll{&cnt->nlong, lng, lacc, ldone};
    __shared__ uint32_t tab[kCrcLdsWords];
    load_crc_lds(tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    uint32_t nwritten = 0;
    unsigned long long bytes = 0;
    for (uint32_t i = blockIdx.x * 4 + threadIdx.x / 64; i < n; i += gridDim.x * 4) {
        const uint64_t ro = rec_off[i];
        bool ok = wr_status[i] == QLZX_WR_OK;
        const WrRec R = in.rec(i);
        const uint64_t rsz = pad256(R.end);
        if (ok && (ro > out_cap || out_cap - ro < rsz)) {
            ok = false;
            if (lane == 0) wr_status[i] = QLZX_WR_NO_SPACE;
        }
        if (!ok) {
            if (lane == 0) rec_off[i] = 0, flag_out[i] = 0, vsz[i] = 0, crc[i] = 0;
            continue;
        }
        nwritten++;
        bytes += rsz;
        if (R.end - 4 > kRpLong) {
            if (lane == 0) ll.push(i);
            continue;
        }
        uint8_t *rec = out + ro;
        const uint32_t e16 = R.end & ~15u;
        uint32_t reg = wr_span(tab, R, rec, 0, e16, lane);
        reg = wr_tail(tab, R, rec, e16, (uint32_t)rsz, reg, lane);
        if (lane == 0) {
            if (R.vzero) reg ^= in.vcrc[i];
            *(uint32_t *)rec = ~reg;
            crc[i] = ~reg;
        }
    }
    if (lane == 0 && nwritten) {
        atomicAdd(&cnt->nwritten, nwritten);
        atomicAdd(&cnt->bytes, bytes);
    }
}

// k_rec_long's policy: a long record's segments are spans of its image, the last one with the tail.
struct WrLong {
    WrIn in;
    uint8_t *out;
    uint32_t *crc;
    struct Rec {
        WrRec R;
        uint8_t *dst;
    };
    __device__ Rec rec(uint32_t i) const { return Rec{in.rec(i), out + in.rec_off[i]}; }
    __device__ bool valid(const Rec &) const { return true; }
    __device__ uint32_t end(const Rec &r) const { return r.R.end; }
    __device__ uint32_t segment(const uint32_t *lds, const Rec &r, uint32_t r0, uint32_t r1, bool last,
                                uint32_t lane) const {
        const uint32_t reg = wr_span(lds, r.R, r.dst, r0, r1, lane);
        return last ? wr_tail(lds, r.R, r.dst, r1, (uint32_t)pad256(r.R.end), reg, lane) : reg;
    }
    __device__ void finish(uint32_t i, const Rec &r, uint32_t sum) const {
        if (r.R.vzero) sum ^= in.vcrc[i];
        *(uint32_t *)r.dst = ~sum;
        crc[i] = ~sum;
    }
};

// Getvhash of the ORIGINAL value (CalcValueHash runs before TryCompress in checkAndSet,
// store/item.go:102); zeros for the records not written.
__global__ void __launch_bounds__(256) k_wr_vhash(const uint8_t *values, const uint64_t *val_off,
                                                  const uint32_t *val_len, const int32_t *wr_status, uint32_t n,
                                                  uint16_t *vh) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (wr_status[i] != QLZX_WR_OK) {
            vh[i] = 0;
            continue;
        }
        const uint8_t *v = values + val_off[i];
        const uint32_t l = val_len[i];
        vh[i] = getvhash(v, l);
    }
}
__global__ void k_wr_totals3(uint32_t *totals3, const WrCounters *cnt) {
    totals3[0] = cnt->nwritten;
    totals3[1] = (uint32_t)cnt->bytes;
    totals3[2] = (uint32_t)(cnt->bytes >> 32);
}

// ---- workspace: the counters, per-record scratch, the long list, the scan tiles ----
struct WrWs {
    WrCounters *cnt;
    uint8_t *cand;
    uint32_t *cap, *sz, *sel, *vcrc, *lng, *lacc, *ldone, *tiles;
    uint64_t *soff;
};
inline size_t write_ws_layout(uint32_t n, uint8_t *base, WrWs *w) {
    WsCarver c{base};
    WrWs t;
    t.cnt = c.take<WrCounters>(sizeof(WrCounters));
    t.cand = c.take((size_t)n);
    t.cap = c.take<uint32_t>(4 * (size_t)n);
    t.sz = c.take<uint32_t>(4 * (size_t)n);
    t.sel = c.take<uint32_t>(4 * (size_t)n);
    t.vcrc = c.take<uint32_t>(4 * (size_t)n);
    t.lng = c.take<uint32_t>(4 * (size_t)n);
    t.lacc = c.take<uint32_t>(4 * (size_t)n);
    t.ldone = c.take<uint32_t>(4 * (size_t)n);
    t.soff = c.take<uint64_t>(8 * (size_t)n);
    t.tiles = c.take<uint32_t>(4 * ((size_t)n / kScanTile + 2));
    if (w) *w = t;
    return c.bytes();
}

inline int launch_write_plan(const uint8_t *values, const uint64_t *val_off, const uint32_t *val_len,
                             const uint32_t *key_len, const uint32_t *flag, const int32_t *ver, uint32_t n,
                             uint32_t max_key, uint64_t body_max, uint32_t not_compress, int32_t *wr_status,
                             uint32_t *try_idx, uint64_t *try_off, uint32_t *try_len, uint64_t *try_dst_off,
                             uint32_t *totals, void *ws, hipStream_t s) {
    if (n == 0) return 0;
    WrWs w;
    write_ws_layout(n, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(WrCounters), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wr_plan, dim3(grid_for(n)), dim3(256), 0, s, values, val_off, val_len, key_len, flag, ver, n,
                       max_key, body_max, not_compress, wr_status, w.cand, w.cnt);
    launch_compact(WrCandFlag{w.cand}, ScatterTry{val_off, val_len, try_idx, try_len, w.cap, try_off}, n, w.tiles,
                   &w.cnt->t5[0], s);
    hipLaunchKernelGGL(k_rp_dstoff, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.cap,
                       (const uint32_t *)&w.cnt->t5[0], try_dst_off, totals, (const uint32_t *)&w.cnt->nok);
    hipLaunchKernelGGL(k_wr_totals, dim3(1), dim3(1), 0, s, totals, (const WrCounters *)w.cnt, 1);
    return (int)hipGetLastError();
}

inline int launch_write_decide(const uint64_t *val_off, const uint32_t *val_len, uint32_t n, const uint32_t *totals,
                               const uint32_t *try_idx, const uint32_t *try_len, const uint32_t *try_csize,
                               const int32_t *try_status, uint8_t *keep, uint32_t *full_idx, uint64_t *full_off,
                               uint32_t *full_len, uint64_t *full_dst_off, uint32_t *totals2, void *ws,
                               hipStream_t s) {
    if (n == 0) return 0;
    WrWs w;
    write_ws_layout(n, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(WrCounters), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wr_decide, dim3(grid_for(n)), dim3(256), 0, s, totals, try_len, try_csize, try_status, keep,
                       w.cnt);
    launch_compact(WrFullFlag{totals, try_idx, try_len, val_len, keep},
                   ScatterFull{try_idx, val_len, val_off, full_idx, full_len, w.cap, full_off}, n, w.tiles,
                   &w.cnt->t5[0], s);
    hipLaunchKernelGGL(k_rp_dstoff, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.cap,
                       (const uint32_t *)&w.cnt->t5[0], full_dst_off, totals2, (const uint32_t *)&w.cnt->nkeep);
    hipLaunchKernelGGL(k_wr_totals, dim3(1), dim3(1), 0, s, totals2, (const WrCounters *)w.cnt, 0);
    return (int)hipGetLastError();
}

struct WrFinishArgs {
    const uint8_t *values, *keys, *trial_buf, *full_buf;
    const uint64_t *val_off, *key_off, *try_dst_off, *full_dst_off;
    const uint32_t *val_len, *key_len, *flag, *ts, *totals, *try_idx, *try_len, *try_csize, *try_crc, *totals2,
        *full_idx, *full_csize, *full_crc;
    const int32_t *ver, *full_status;
    const uint8_t *keep;
};

inline int launch_write_finish(const WrFinishArgs &a, uint32_t n, uint8_t *out, uint64_t out_cap, int32_t *wr_status,
                               uint64_t *rec_off, uint32_t *flag_out, uint32_t *vsz, uint32_t *crc, uint16_t *vhash,
                               uint32_t *totals3, void *ws, hipStream_t s) {
    if (n == 0) return 0;
    WrWs w;
    write_ws_layout(n, (uint8_t *)ws, &w);
    const hipError_t e = hipMemsetAsync(w.cnt, 0, sizeof(WrCounters), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wr_sizes, dim3(grid_for(n)), dim3(256), 0, s, a.val_off, a.val_len, a.key_len, a.flag,
                       (const int32_t *)wr_status, n, flag_out, vsz, w.sz, w.sel, w.soff, w.cnt);
    hipLaunchKernelGGL(k_wr_apply, dim3(grid_for(n)), dim3(256), 0, s, a.totals, a.try_idx, a.try_len, a.try_dst_off,
                       a.try_csize, a.try_crc, a.keep, a.totals2, a.full_idx, a.full_dst_off, a.full_csize,
                       a.full_status, a.full_crc, a.val_len, a.key_len, flag_out, vsz, w.sz, w.sel, w.soff, w.vcrc);
    // record offsets: the exclusive scan of the padded sizes (0 for a failed record)
    hipLaunchKernelGGL(k_rp_dstoff, dim3(1), dim3(1024), 0, s, (const uint32_t *)w.sz, (const uint32_t *)&w.cnt->n,
                       rec_off, &w.cnt->t5[0], (const uint32_t *)&w.cnt->zero);
    const WrIn in{a.values, a.keys,  a.trial_buf, a.full_buf, a.key_off, a.key_len, a.ts,
                  a.ver,    flag_out, vsz,         w.sel,      w.vcrc,    w.soff,    rec_off};
    hipLaunchKernelGGL(k_wr_assemble, dim3(grid_for(n, 4, 2048)), dim3(256), 0, s, in, n, out, out_cap, wr_status,
                       rec_off, flag_out, vsz, crc, w.cnt, w.lng, w.lacc, w.ldone);
    hipLaunchKernelGGL(k_rec_long<WrLong>, dim3(2048), dim3(256), 0, s, WrLong{in, out, crc},
                       LongList{&w.cnt->nlong, w.lng, w.lacc, w.ldone});
    if (vhash)
        hipLaunchKernelGGL(k_wr_vhash, dim3(grid_for(n)), dim3(256), 0, s, a.values, a.val_off, a.val_len,
                           (const int32_t *)wr_status, n, vhash);
    hipLaunchKernelGGL(k_wr_totals3, dim3(1), dim3(1), 0, s, totals3, (const WrCounters *)w.cnt);
    return (int)hipGetLastError();
}

}  // namespace qlzx
