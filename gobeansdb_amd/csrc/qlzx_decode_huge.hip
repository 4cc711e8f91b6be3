// qlzx_decode_huge.hip -- level-3 decode of ONE large block (dsize > QLZX_FAST_MAX_DSIZE, up to
// BodyMax = 50 MiB, config/mc_config.go:7) by the whole GPU, every phase data-parallel.
//
// The batch decoder parses with one lane per block (K1); for a 50 MiB value that lane would walk
// ~400 K control-word groups serially.  Here (N = csize, M = dsize, quicklz.c:513-671):
//   1. code[x]  2-bit token length code of every stream byte;
//   2. delta[x] length of the control-word group that WOULD start at x (speculative parse at
//      every byte; 0 = no shortcut: no sentinel (C1) or within 128 B of the end);
//   3. J_k[x]   the stream offset 2^k groups on (k = 1..8, u16, 0 = not all shortcuts), built
//      level by level from J_{k-1};
//   4. one lane walks the chain from the header with the largest valid jump at each step and
//      lists segments {start, first group, 2^k}; groups without a shortcut (the last ones, or a
//      corrupt stream) are parsed byte by byte there, with K1's checks (C1, C2, group bound);
//   5. the segments are expanded into the group list (one lane per segment);
//   6. per group: the output length of its items; 7. exclusive scan over groups;
//   8. per item: checks C3-C5 (oracle/qlz_oracle.c:180-231) and, for every output byte, its
//      source (itself for a literal, p - offset for a match byte) plus the literal bytes;
//   9. pointer jumping s[p] <- s[s[p]] until every byte points at a literal (log2 of the
//      deepest copy chain rounds); 10. gather: out[p] = lit[s[p]].
// The record CRC (store/datafile.go:161-168) is one wave per 16 KiB segment of the stream plus
// a GF(2) shift-combine, verified before decoding as readRecordAt does.
// The host drives the phases (it knows N and M), so a batch holding such values synchronises
// once per value; values over 64 KiB are rare (the batch path owns the 4-64 KiB ones).  The
// drivers are at the end of this file: launch_decode_huge for a batch, huge_one per value.
#include <algorithm>
#include <vector>

#include "qlzx_decode_fmt.h"
#include "qlzx_host.h"

namespace qlzx {

constexpr uint32_t kHugeLevels = 8;            // jump tables J_1 .. J_8 (256 groups per jump)
constexpr uint32_t kHugeSeg = 16u << 10;       // CRC segment
constexpr uint32_t kHugeGrid = 2048, kHugeWG = 256;

struct HugeCtl {
    uint32_t ngroups, nseg, klast, st;
    CheckAcc acc;
    uint32_t crc;
    uint32_t pad[7];
    uint32_t changed[64];  // pointer-jumping rounds
};
struct HugeSeg {
    uint32_t x, g, cnt, pad;
};

__host__ __device__ inline uint64_t huge_nmax(uint64_t m) { return m + m / 2 + 64; }  // csize bound (4 B per 3 + cw)
__host__ __device__ inline uint64_t huge_gmax(uint64_t m) { return m / 31 + 2; }

struct HugeWs {  // carved out of one workspace
    HugeCtl *ctl;
    uint32_t *code;
    uint8_t *delta;
    uint16_t *J;      // kHugeLevels x nmax
    HugeSeg *seg;
    uint32_t *glist, *glen;
    uint32_t *src;    // per output byte
    uint8_t *lit;
    uint32_t *scrc;   // CRC per segment
};

inline size_t huge_ws_layout(uint64_t m, uint8_t *base, HugeWs *w) {
    const uint64_t n = huge_nmax(m), g = huge_gmax(m) + 64;
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + o : nullptr; o += (bytes + 255) & ~(size_t)255; return p; };
    HugeWs h;
    h.ctl = (HugeCtl *)take(sizeof(HugeCtl));
    h.code = (uint32_t *)take((n / 16 + 8) * 4);
    h.delta = take(n + 256);
    h.J = (uint16_t *)take((size_t)kHugeLevels * (n + 256) * 2);
    h.seg = (HugeSeg *)take(g * sizeof(HugeSeg));
    h.glist = (uint32_t *)take(g * 4);
    h.glen = (uint32_t *)take(g * 4);
    h.src = (uint32_t *)take(m * 4 + 64);
    h.lit = take(m + 64);
    h.scrc = (uint32_t *)take((n / kHugeSeg + 8) * 4);
    if (w) *w = h;
    return o;
}

__global__ void __launch_bounds__(kHugeWG) k_h_codes(const uint8_t *src, uint32_t n, uint32_t *code) {
    for (uint32_t w = blockIdx.x * kHugeWG + threadIdx.x; w < (n + 15) / 16; w += gridDim.x * kHugeWG) {
        const uint8_t *p = src + 16 * w;
        code[w] = 16 * w + 16 <= n ? pack_codes16(ld_dword(p), ld_dword(p + 4), ld_dword(p + 8), ld_dword(p + 12))
                                   : pack_codes_tail(p, n - 16 * w);
    }
}

__global__ void __launch_bounds__(kHugeWG) k_h_delta(const uint8_t *src, uint32_t n, uint32_t hdr, const uint32_t *code,
                                                  uint8_t *delta) {
    for (uint32_t x = blockIdx.x * kHugeWG + threadIdx.x; x < n + 256; x += gridDim.x * kHugeWG) {
        const bool in = x >= hdr && x + 128 <= n;  // no shortcut within 128 B of the end
        delta[x] = (uint8_t)(in ? spec_group_len(ld_dword(src + x), CodeWords{code}, x) : 0u);
    }
}

// J_1 from delta, J_k from J_{k-1}: two valid jumps compose, any invalid one gives 0
__global__ void __launch_bounds__(kHugeWG) k_h_jump1(const uint8_t *delta, uint32_t n, uint16_t *J1) {
    for (uint32_t x = blockIdx.x * kHugeWG + threadIdx.x; x < n + 256; x += gridDim.x * kHugeWG) {
        const uint32_t a = delta[x];
        const uint32_t b = a && x + a < n ? delta[x + a] : 0u;
        J1[x] = (uint16_t)(b ? a + b : 0u);
    }
}
__global__ void __launch_bounds__(kHugeWG) k_h_jumpk(const uint16_t *Jp, uint32_t n, uint16_t *Jk) {
    for (uint32_t x = blockIdx.x * kHugeWG + threadIdx.x; x < n + 256; x += gridDim.x * kHugeWG) {
        const uint32_t a = Jp[x];
        const uint32_t b = a && x + a < n ? Jp[x + a] : 0u;
        Jk[x] = (uint16_t)(b ? a + b : 0u);
    }
}

// 4. the chain (one lane).  K1's checks where there is no shortcut.
__global__ void __launch_bounds__(64) k_h_walk(const uint8_t *src, uint32_t n, uint32_t hdr, uint32_t m,
                                               const uint32_t *code, const uint8_t *delta, const uint16_t *J,
                                               uint32_t nmax, HugeSeg *seg, HugeCtl *ctl) {
    if (threadIdx.x != 0 || ctl->st != QLZX_OK) return;  // a record CRC mismatch stops here
    const uint32_t gmax = (uint32_t)huge_gmax(m);
    uint32_t x = hdr, g = 0, ns = 0, klast = 31;
    int st = QLZX_OK;
    while (x + 4 <= n) {  // else: the stream ends at a control word
        int k = (int)kHugeLevels;
        uint32_t j = 0;
        for (; k >= 1; k--) {
            j = J[(size_t)(k - 1) * (nmax + 256) + x];
            if (j && g + (1u << k) <= gmax) break;
        }
        if (k >= 1) {
            seg[ns++] = HugeSeg{x, g, 1u << k, 0};
            g += 1u << k;
            x += j;
            continue;
        }
        if (g >= gmax) { st = QLZX_E_CORRUPT; break; }
        const uint32_t d = delta[x];
        seg[ns++] = HugeSeg{x, g, 1, 0};
        g++;
        if (d) { x += d; continue; }
        uint32_t next = x;
        st = parse_group_bytewise(ld_dword(src + x), x, n, CodeWords{code}, klast, next);
        if (st != QLZX_OK || klast < 31) break;  // corrupt, or the stream ends inside this group
        x = next;
    }
    ctl->ngroups = g;
    ctl->nseg = ns;
    ctl->klast = klast;
    ctl->st = (uint32_t)chain_status(st, g);
    ctl->acc = check_acc_init();
}

__global__ void __launch_bounds__(kHugeWG) k_h_expand(const uint8_t *delta, const HugeSeg *seg, const HugeCtl *ctl,
                                                   uint32_t *glist) {
    const uint32_t ns = ctl->st == QLZX_OK ? ctl->nseg : 0u;
    for (uint32_t s = blockIdx.x * kHugeWG + threadIdx.x; s < ns; s += gridDim.x * kHugeWG) {
        const HugeSeg e = seg[s];
        uint32_t x = e.x;
        for (uint32_t c = 0; c < e.cnt; c++) {
            glist[e.g + c] = x;
            x += delta[x];
        }
    }
}

// Items of group g: calls f(item index k, is match, token, stream position, token bytes, output length).
template <typename F>
__device__ __forceinline__ void hg_items(const uint8_t *src, uint32_t n, const uint32_t *code, uint32_t x, uint32_t nk,
                                         F &&f) {
    const uint32_t cw = ld_dword(src + x);
    uint32_t p = x + 4;
    for (uint32_t k = 0; k < nk; k++) {
        const bool ism = (cw >> k) & 1u;
        const uint32_t t = p + 4 <= n ? ld_dword(src + p) : (ld_dword(src + n - 4) >> (8 * (p + 4 - n)));
        uint32_t off = 0, len = 1, tl = 1;
        if (ism) decode_tok_bf(t, off, len, tl);
        f(k, ism, t, p, tl, off, len);
        p += tl;
    }
}

__global__ void __launch_bounds__(kHugeWG) k_h_glen(const uint8_t *src, uint32_t n, const uint32_t *code,
                                                 const uint32_t *glist, const HugeCtl *ctl, uint32_t *glen) {
    if (ctl->st != QLZX_OK) return;
    const uint32_t ng = ctl->ngroups, klast = ctl->klast;
    for (uint32_t g = blockIdx.x * kHugeWG + threadIdx.x; g < ng; g += gridDim.x * kHugeWG) {
        uint32_t sum = 0;
        hg_items(src, n, code, glist[g], g + 1 == ng ? klast : 31u,
                 [&](uint32_t, bool, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t len) { sum += len; });
        glen[g] = sum;
    }
}

// exclusive scan of glen (in place) by one workgroup of 1024 threads
__global__ void __launch_bounds__(1024) k_h_scan(uint32_t *glen, const HugeCtl *ctl) {
    __shared__ uint32_t wsum[kBlockWaves];
    __shared__ uint32_t carry;
    if (ctl->st != QLZX_OK) return;
    const uint32_t ng = ctl->ngroups, tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < ng; base += 1024 * 8) {
        uint32_t v[8], s = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t g = base + tid * 8 + j;
            v[j] = g < ng ? glen[g] : 0u;
            s += v[j];
        }
        uint32_t total;
        const uint32_t ex = block_excl<false>(s, wsum, total) + carry;
        uint32_t acc = ex;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t g = base + tid * 8 + j;
            if (g < ng) glen[g] = acc;
            acc += v[j];
        }
        __syncthreads();
        if (tid == 0) carry += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kHugeWG) k_h_items(const uint8_t *src, uint32_t n, uint32_t hdr, uint32_t m,
                                                  const uint32_t *code, const uint32_t *glist, const uint32_t *gd,
                                                  HugeCtl *ctl, uint32_t *sp, uint8_t *lit) {
    if (ctl->st != QLZX_OK) return;
    const uint32_t ng = ctl->ngroups, klast = ctl->klast;
    const uint32_t tail_from = tail_start(m);
    CheckAcc acc = check_acc_init();
    for (uint32_t g = blockIdx.x * kHugeWG + threadIdx.x; g < ng; g += gridDim.x * kHugeWG) {
        uint32_t d = gd[g];
        hg_items(src, n, code, glist[g], g + 1 == ng ? klast : 31u,
                 [&](uint32_t k, bool ism, uint32_t t, uint32_t pos, uint32_t tl, uint32_t off, uint32_t len) {
                     if (d < m && check_item(ism, off, len, tl, pos, d, g * 31 + k, m, n, hdr, tail_from, acc)) {
                         if (ism) {
                             for (uint32_t j = 0; j < len; j++) sp[d + j] = d + j - off;
                         } else {
                             sp[d] = d;
                             lit[d] = (uint8_t)t;
                         }
                     }
                     d += len;
                 });
    }
    check_acc_merge(&ctl->acc, acc);
}

// s[p] <- s[s[p]]; a stale read is an earlier link of the same chain, so it costs only a round
__global__ void __launch_bounds__(kHugeWG) k_h_jumpround(uint32_t *sp, uint32_t m, uint32_t *changed) {
    uint32_t ch = 0;
    for (uint32_t p = blockIdx.x * kHugeWG + threadIdx.x; p < m; p += gridDim.x * kHugeWG) {
        const uint32_t s = sp[p];
        const uint32_t t = sp[s];
        if (t != s) {
            sp[p] = t;
            ch = 1;
        }
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}

__global__ void __launch_bounds__(kHugeWG) k_h_gather(const uint32_t *sp, const uint8_t *lit, uint32_t m, uint8_t *dst) {
    for (uint32_t q = blockIdx.x * kHugeWG + threadIdx.x; q < (m + 3) / 4; q += gridDim.x * kHugeWG) {
        const uint32_t p = 4 * q;
        if (p + 4 <= m) {
            const uint4 s = *(const uint4 *)(sp + p);
            const uint32_t w = lit[s.x] | (lit[s.y] << 8) | (lit[s.z] << 16) | ((uint32_t)lit[s.w] << 24);
            if ((((uintptr_t)dst) & 3u) == 0) *(uint32_t *)(dst + p) = w;
            else for (uint32_t j = 0; j < 4; j++) dst[p + j] = (uint8_t)(w >> (8 * j));
        } else {
            for (uint32_t j = 0; p + j < m; j++) dst[p + j] = lit[sp[p + j]];
        }
    }
}

// record CRC: raw CRC (from 0) of every kHugeSeg segment, one wave each; then the combine
__global__ void __launch_bounds__(256) k_h_crcseg(const uint8_t *p, uint64_t len, uint32_t *scrc) {
    __shared__ uint32_t tab[kCrcLdsWords];
    load_crc_lds(tab);
    __syncthreads();
    const uint32_t nseg = (uint32_t)((len + kHugeSeg - 1) / kHugeSeg);
    for (uint32_t s = blockIdx.x * 4 + threadIdx.x / 64; s < nseg; s += gridDim.x * 4) {
        const uint64_t o = (uint64_t)s * kHugeSeg;
        const uint32_t l = (uint32_t)min((uint64_t)kHugeSeg, len - o);
        const uint32_t c = wave_crc(tab, p + o, l, 0u, threadIdx.x & 63);
        if ((threadIdx.x & 63) == 0) scrc[s] = c;
    }
}
__global__ void k_h_crccomb_ctl(const uint32_t *scrc, uint64_t len, HugeCtl *ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t nseg = (uint32_t)((len + kHugeSeg - 1) / kHugeSeg);
    uint32_t acc = ctl->crc;  // the initial state (k_h_crcinit)
    for (uint32_t s = 0; s < nseg; s++) {
        const uint64_t l = min((uint64_t)kHugeSeg, len - (uint64_t)s * kHugeSeg);
        acc = crc_shift(acc, l) ^ scrc[s];
    }
    ctl->crc = acc;
}
// stored values and early verdicts: only while no CRC mismatch was found
__global__ void __launch_bounds__(kHugeWG) k_h_copy_if(const HugeCtl *ctl, const uint8_t *s, uint8_t *d, uint64_t len) {
    if (ctl->st != QLZX_OK) return;
    for (uint64_t p = (uint64_t)(blockIdx.x * kHugeWG + threadIdx.x); p < len; p += (uint64_t)gridDim.x * kHugeWG) d[p] = s[p];
}
__global__ void k_h_setstatus_ok_if(const HugeCtl *ctl, int32_t *status, uint32_t *dsize_out, int32_t st, uint32_t ds) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || ctl->st != QLZX_OK) return;
    *status = st;
    if (dsize_out) *dsize_out = ds;
}

// Pending large blocks of a batch (status kPending after K1): {block, csize, dsize, compressed}
struct HugeItem {
    uint32_t i, csize, dsize, comp;
};
__global__ void __launch_bounds__(256) k_h_pending(qlzx_blocks b, const int32_t *status, uint32_t *count,
                                                   HugeItem *items) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < b.n; i += gridDim.x * 256) {
        if (status[i] != kPending) continue;
        const Header h = parse_header(b.src + b.src_off[i]);
        const uint32_t j = atomicAdd(count, 1u);
        items[j] = HugeItem{i, h.csize, h.dsize, h.compressed ? 1u : 0u};
    }
}

__global__ void k_h_setstatus(int32_t *status, uint32_t *dsize_out, int32_t st, uint32_t ds) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *status = st;
        if (dsize_out) *dsize_out = ds;
    }
}
// record CRC verdict of one large block: crc_out, and QLZX_E_CRC (nothing decoded) on a mismatch
__global__ void k_h_crcverdict(HugeCtl *ctl, const uint32_t *crc_expect, uint32_t *crc_out, int32_t *status,
                               uint32_t *dsize_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t c = ~ctl->crc;
    if (crc_out) *crc_out = c;
    if (crc_expect && c != *crc_expect) {
        ctl->st = QLZX_E_CRC;
        *status = QLZX_E_CRC;
        if (dsize_out) *dsize_out = 0;
    }
}
__global__ void k_h_crcinit(HugeCtl *ctl, const uint32_t *crc_state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctl->crc = crc_state ? *crc_state : 0xffffffffu;
}

// One large block (dsize > QLZX_FAST_MAX_DSIZE) by the whole GPU.  The host knows the sizes from
// the pending list; it synchronises to read the verdict of the parse and the pointer-jumping flags.
inline int huge_one(const uint8_t *src, uint32_t csize, uint8_t *dst, uint32_t dsize, bool comp, uint32_t max_dsize,
                    const uint32_t *crc_state, const uint32_t *crc_expect, uint32_t *crc_out, int32_t *status,
                    uint32_t *dsize_out, uint8_t *ws, hipStream_t s) {
    HugeWs w;
    huge_ws_layout(max_dsize, ws, &w);
    const uint32_t nmax = (uint32_t)huge_nmax(max_dsize);
    const dim3 G(kHugeGrid), B(kHugeWG);
    HIP_OK(hipMemsetAsync(w.ctl, 0, sizeof(HugeCtl), s));
    const bool crc = crc_state || crc_expect || crc_out;
    if (crc) {
        hipLaunchKernelGGL(k_h_crcseg, dim3(std::min<uint32_t>((csize + kHugeSeg * 4 - 1) / (kHugeSeg * 4), 1024)),
                           dim3(256), 0, s, src, (uint64_t)csize, w.scrc);
        hipLaunchKernelGGL(k_h_crcinit, dim3(1), dim3(64), 0, s, w.ctl, crc_state);
        // the combine reads the initial state from ctl->crc
        hipLaunchKernelGGL(k_h_crccomb_ctl, dim3(1), dim3(64), 0, s, w.scrc, (uint64_t)csize, w.ctl);
        hipLaunchKernelGGL(k_h_crcverdict, dim3(1), dim3(64), 0, s, w.ctl, crc_expect, crc_out, status, dsize_out);
    }
    const uint32_t hdr = 9;  // header of a value over 64 KiB: always 9 bytes (quicklz.c:771-772)
    if (!comp) {  // stored (quicklz.c:808-811)
        if ((uint64_t)csize < (uint64_t)hdr + dsize) {
            hipLaunchKernelGGL(k_h_setstatus_ok_if, dim3(1), dim3(64), 0, s, w.ctl, status, dsize_out, QLZX_E_CORRUPT, 0u);
        } else {
            hipLaunchKernelGGL(k_h_copy_if, G, B, 0, s, w.ctl, src + hdr, dst, (uint64_t)dsize);
            hipLaunchKernelGGL(k_h_setstatus_ok_if, dim3(1), dim3(64), 0, s, w.ctl, status, dsize_out, QLZX_OK, dsize);
        }
        HIP_OK(hipGetLastError());
        return QLZX_R_OK;
    }
    if (csize > nmax) {  // longer than any stream of dsize bytes can be: trailing garbage (C5)
        hipLaunchKernelGGL(k_h_setstatus_ok_if, dim3(1), dim3(64), 0, s, w.ctl, status, dsize_out, QLZX_E_CORRUPT, 0u);
        HIP_OK(hipGetLastError());
        return QLZX_R_OK;
    }
    hipLaunchKernelGGL(k_h_codes, G, B, 0, s, src, csize, w.code);
    hipLaunchKernelGGL(k_h_delta, G, B, 0, s, src, csize, hdr, (const uint32_t *)w.code, w.delta);
    hipLaunchKernelGGL(k_h_jump1, G, B, 0, s, (const uint8_t *)w.delta, csize, w.J);
    for (uint32_t k = 2; k <= kHugeLevels; k++)
        hipLaunchKernelGGL(k_h_jumpk, G, B, 0, s, (const uint16_t *)(w.J + (size_t)(k - 2) * (nmax + 256)), csize,
                           w.J + (size_t)(k - 1) * (nmax + 256));
    hipLaunchKernelGGL(k_h_walk, dim3(1), dim3(64), 0, s, src, csize, hdr, dsize, (const uint32_t *)w.code,
                       (const uint8_t *)w.delta, (const uint16_t *)w.J, nmax, w.seg, w.ctl);
    hipLaunchKernelGGL(k_h_expand, G, B, 0, s, (const uint8_t *)w.delta, (const HugeSeg *)w.seg,
                       (const HugeCtl *)w.ctl, w.glist);
    hipLaunchKernelGGL(k_h_glen, G, B, 0, s, src, csize, (const uint32_t *)w.code, (const uint32_t *)w.glist,
                       (const HugeCtl *)w.ctl, w.glen);
    hipLaunchKernelGGL(k_h_scan, dim3(1), dim3(1024), 0, s, w.glen, (const HugeCtl *)w.ctl);
    hipLaunchKernelGGL(k_h_items, G, B, 0, s, src, csize, hdr, dsize, (const uint32_t *)w.code,
                       (const uint32_t *)w.glist, (const uint32_t *)w.glen, w.ctl, w.src, w.lit);
    HIP_OK(hipGetLastError());
    HugeCtl h;
    HIP_OK(hipMemcpyAsync(&h, w.ctl, sizeof(HugeCtl), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (h.st == QLZX_E_CRC) return QLZX_R_OK;  // already reported
    if (h.st != QLZX_OK || verdict_corrupt(h.acc)) {
        hipLaunchKernelGGL(k_h_setstatus, dim3(1), dim3(64), 0, s, status, dsize_out, (int32_t)QLZX_E_CORRUPT, 0u);
        HIP_OK(hipGetLastError());
        return QLZX_R_OK;
    }
    // pointer jumping, four rounds per check of the last round's flag
    for (uint32_t r = 0;; r += 4) {
        if (r + 4 > 64) return fail(QLZX_R_HIP, "huge decode: pointer jumping did not converge");
        for (uint32_t j = 0; j < 4; j++)
            hipLaunchKernelGGL(k_h_jumpround, G, B, 0, s, w.src, dsize, w.ctl->changed + r + j);
        uint32_t ch = 0;
        HIP_OK(hipMemcpyAsync(&ch, w.ctl->changed + r + 3, 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        if (!ch) break;
    }
    hipLaunchKernelGGL(k_h_gather, G, B, 0, s, (const uint32_t *)w.src, (const uint8_t *)w.lit, dsize, dst);
    hipLaunchKernelGGL(k_h_setstatus, dim3(1), dim3(64), 0, s, status, dsize_out, (int32_t)QLZX_OK, dsize);
    HIP_OK(hipGetLastError());
    return QLZX_R_OK;
}

// The pending list of a batch, as k_h_pending / k_he_pending (qlzx_encode_huge.hip) left it on the
// device, read back: the count, then the items, then each item's source and destination offset.
template <typename Item>
struct PendingList {
    std::vector<Item> item;
    std::vector<uint64_t> src_off, dst_off;
};
template <typename Item>
int read_pending(const qlzx_blocks &b, const uint32_t *count, const Item *items, hipStream_t s, PendingList<Item> *p) {
    uint32_t np = 0;
    HIP_OK(hipMemcpyAsync(&np, count, 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    p->item.resize(np), p->src_off.resize(np), p->dst_off.resize(np);
    if (np == 0) return QLZX_R_OK;
    HIP_OK(hipMemcpyAsync(p->item.data(), items, np * sizeof(Item), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < np; j++) {
        HIP_OK(hipMemcpyAsync(&p->src_off[j], b.src_off + p->item[j].i, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(&p->dst_off[j], b.dst_off + p->item[j].i, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipStreamSynchronize(s));
    return QLZX_R_OK;
}

// The pending large blocks of a batch (K1 left them kPending): listed on the device, read back
// once, then decoded one at a time by huge_one.  ws: [count 256 | items | huge_ws_layout].
inline int launch_decode_huge(const qlzx_blocks &b, const uint32_t *crc_state, const uint32_t *crc_expect,
                              uint32_t *crc_out, int32_t *status, uint32_t *dsize_out, uint32_t max_dsize,
                              uint8_t *ws, hipStream_t s) {
    uint32_t *count = (uint32_t *)ws;
    HugeItem *items = (HugeItem *)(ws + 256);
    uint8_t *hws = ws + align_up((size_t)b.n * sizeof(HugeItem) + 256, 256);
    HIP_OK(hipMemsetAsync(count, 0, 4, s));
    hipLaunchKernelGGL(k_h_pending, dim3(std::min<uint32_t>((b.n + 255) / 256, 4096)), dim3(256), 0, s, b,
                       (const int32_t *)status, count, items);
    HIP_OK(hipGetLastError());
    PendingList<HugeItem> p;
    if (int r = read_pending(b, count, items, s, &p)) return r;
    for (size_t j = 0; j < p.item.size(); j++) {
        const HugeItem &it = p.item[j];
        const uint32_t i = it.i;
        if (int r = huge_one(b.src + p.src_off[j], it.csize, b.dst + p.dst_off[j], it.dsize, it.comp != 0, max_dsize,
                             crc_state ? crc_state + i : nullptr, crc_expect ? crc_expect + i : nullptr,
                             crc_out ? crc_out + i : nullptr, status + i, dsize_out ? dsize_out + i : nullptr, hws, s))
            return r;
    }
    return QLZX_R_OK;
}

}  // namespace qlzx
