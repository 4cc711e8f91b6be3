// qlzx_decode_batch.hip -- the host side of the fast batched level-3 decoder (the kernels are in
// qlzx_decode_k1.h and qlzx_decode_k2.h, what they share in qlzx_decode_batch.h): the block order
// of a call, the per-thread side streams and launch_decode_wave, which queues K1 and K2 of every
// chunk.  K1 of chunk c+1 runs on a side stream beside K2 of chunk c.
#include "qlzx_decode_batch.h"
#include "qlzx_decode_k2.h"
#include "qlzx_host.h"

namespace qlzx {

// ---------------------------------------------------------- block order ----
// K1 runs one lane per block, so a wave lasts as long as its longest stream: with mixed
// 4-64 KiB values (c4, c5) most lanes would idle behind one 64 KiB block.  Two small
// kernels list ALL blocks of the call by compressed size, smallest first (counting sort on
// len / 512, 128 classes), and the chunks are cut from that list: K1 and K2 of chunk c take
// blocks list[c * chunk ..] and index their workspace by the place in the chunk.  So a K1
// wave's lanes have similar lengths, and K1(c+1), whose blocks are at most a class longer,
// hides under K2(c), whose chunk has as many blocks; the first, exposed K1 parses the
// smallest blocks.  Order within a class is arbitrary: outputs are indexed by the block.
// aux (zeroed before k_order_count): [0,128) class counts, [128,256) class cursors.
// One-wave workgroups (16 blocks per lane), launched before the first K1: a kernel queued
// between two K1s on the side stream delayed K1(c+1) until K2(c) had filled the CUs, and a
// 1024-thread workgroup waited for a whole CU to drain; both serialised K1 behind K2.
constexpr uint32_t kOrderClasses = 128, kOrderWG = 64, kOrderEPT = 16, kOrderPerWG = kOrderWG * kOrderEPT;
constexpr uint32_t kOrderAux = 2 * kOrderClasses;
__device__ __forceinline__ uint32_t order_class(uint32_t len) {
    const uint32_t c = len >> 9;
    return c < kOrderClasses - 1 ? c : kOrderClasses - 1;
}
__global__ void __launch_bounds__(kOrderWG) k_order_count(const uint32_t *src_len, uint32_t n, uint32_t *aux) {
    __shared__ uint32_t h[kOrderClasses];
    const uint32_t tid = threadIdx.x, i0 = blockIdx.x * kOrderPerWG + tid;
    for (uint32_t k = tid; k < kOrderClasses; k += kOrderWG) h[k] = 0;
    __syncthreads();
    uint32_t len[kOrderEPT];
#pragma unroll
    for (uint32_t e = 0; e < kOrderEPT; e++) {
        const uint32_t i = i0 + e * kOrderWG;
        len[e] = i < n ? src_len[i] : 0u;
    }
#pragma unroll
    for (uint32_t e = 0; e < kOrderEPT; e++)
        if (i0 + e * kOrderWG < n) atomicAdd(&h[order_class(len[e])], 1u);
    __syncthreads();
    for (uint32_t k = tid; k < kOrderClasses; k += kOrderWG)
        if (h[k]) atomicAdd(&aux[k], h[k]);
}
__global__ void __launch_bounds__(kOrderWG) k_order_scatter(const uint32_t *src_len, uint32_t n, uint32_t *aux,
                                                           uint32_t *list) {
    __shared__ uint32_t start[kOrderClasses], lc[kOrderClasses];
    const uint32_t tid = threadIdx.x, i0 = blockIdx.x * kOrderPerWG + tid;
    for (uint32_t k = tid; k < kOrderClasses; k += kOrderWG) start[k] = aux[k], lc[k] = 0;
    __syncthreads();
    if (tid == 0) {  // exclusive scan of the class counts (128 LDS words)
        uint32_t acc = 0;
        for (uint32_t k = 0; k < kOrderClasses; k++) {
            const uint32_t v = start[k];
            start[k] = acc;
            acc += v;
        }
    }
    uint32_t c[kOrderEPT], r[kOrderEPT];
#pragma unroll
    for (uint32_t e = 0; e < kOrderEPT; e++) {
        const uint32_t i = i0 + e * kOrderWG;
        c[e] = i < n ? order_class(src_len[i]) : 0u;
    }
#pragma unroll
    for (uint32_t e = 0; e < kOrderEPT; e++)
        r[e] = (i0 + e * kOrderWG < n) ? atomicAdd(&lc[c[e]], 1u) : 0u;  // rank in this workgroup's class
    __syncthreads();
    for (uint32_t k = tid; k < kOrderClasses; k += kOrderWG)
        if (lc[k]) start[k] += atomicAdd(&aux[kOrderClasses + k], lc[k]);
    __syncthreads();
#pragma unroll
    for (uint32_t e = 0; e < kOrderEPT; e++)
        if (i0 + e * kOrderWG < n) list[start[c[e]] + r[e]] = i0 + e * kOrderWG;
}

// ------------------------------------------------------------ launcher ----
#ifndef QLZX_K1_KMAX_UNI  // K1's step budget per iteration: uniform 16 KiB calls / mixed sizes (16 / 10 with the
                          // default scheduler; 12 / 10 under iterative-ILP: profiles/r05_sched_strategy_ab.txt)
#define QLZX_K1_KMAX_UNI 12
#endif
#ifndef QLZX_K1_KMAX_MIX
#define QLZX_K1_KMAX_MIX 10
#endif
// K1 and K2 without CRC live in qlzx_k2.hip (its own scheduler strategy).  Both return
// hipGetLastError(), which also clears the error: the callers below keep it.
int launch_k1_parse6(uint32_t grid, hipStream_t s, const qlzx_blocks &b, const uint32_t *dst_cap, uint32_t *dsize,
                     int32_t *status, uint32_t first, uint32_t cnt, BlkInfo *info, GroupRec *recs, uint32_t gmax,
                     const uint32_t *order, uint32_t max_dsize, uint32_t kmax);
int launch_k2_nocrc(uint32_t grid, hipStream_t s, const qlzx_blocks &b, uint32_t *dsize, int32_t *status,
                    uint32_t first, uint32_t cnt, const BlkInfo *info, const GroupRec *recs, uint32_t gmax,
                    const uint32_t *order);
// Test hook (qlzx_service_test_fault modes 3 / 4, inert unless QLZX_TEST_HOOKS=1): the next K1 /
// K2 launch of a batch call is replaced by a launch failure, so the caller's error path runs.
inline std::atomic<int> g_batch_fault{0};
inline int batch_fault(int kernel) {
    int k = kernel;
    return g_batch_fault.load(std::memory_order_relaxed) == kernel && g_batch_fault.compare_exchange_strong(k, 0)
               ? (int)hipErrorLaunchFailure
               : 0;
}

// The side streams and events of a call of several chunks, per host thread (the batch API is
// re-entrant like the reference) and per device; destroyed with the thread (Go runs cgo calls on
// many OS threads).
struct Side {
    hipStream_t st = nullptr, st2 = nullptr;
    hipEvent_t k1[2] = {}, k2[2] = {}, order = nullptr, last = nullptr;
    ~Side() {
        if (!st || g_hip_down.load()) return;
        for (int j = 0; j < 2; j++) {
            if (k1[j]) (void)hipEventDestroy(k1[j]);
            if (k2[j]) (void)hipEventDestroy(k2[j]);
        }
        if (order) (void)hipEventDestroy(order);
        if (last) (void)hipEventDestroy(last);
        if (st2) (void)hipStreamDestroy(st2);
        (void)hipStreamDestroy(st);
    }
};
// The calling thread's Side for the device that owns `s`, created there at first use.
inline int batch_side(hipStream_t s, Side *&out) {
    thread_local Side sides[kMaxDevices];
    int dev = 0, cur = 0;
    if (s) {
        hipDevice_t hd;
        if (hipStreamGetDevice(s, &hd) != hipSuccess) return (int)hipErrorInvalidResourceHandle;
        dev = (int)hd;
    } else if (hipGetDevice(&dev) != hipSuccess) {
        return (int)hipErrorNoDevice;
    }
    if (dev < 0 || dev >= (int)kMaxDevices) return (int)hipErrorInvalidDevice;
    Side &sd = sides[dev];
    if (!sd.st) {
        note_hip_up();
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        hipError_t e = hipStreamCreateWithFlags(&sd.st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&sd.st2, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sd.order, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sd.last, hipEventDisableTiming);
        for (int j = 0; j < 2 && e == hipSuccess; j++) {
            e = hipEventCreateWithFlags(&sd.k1[j], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sd.k2[j], hipEventDisableTiming);
        }
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) return (int)e;
    }
    out = &sd;
    return 0;
}

// What every K1 and K2 launch of a call shares.
struct BatchCall {
    const qlzx_blocks &b;
    const uint32_t *dst_cap;
    uint32_t *dsize;
    int32_t *status;
    const uint32_t *crc_state, *crc_expect;
    uint32_t *crc_out;
    uint32_t max_dsize;
    uint8_t *ws;
    BatchLayout L;
    bool sort;  // the chunks are cut from the block order (list) instead of from the call's order

    BlkInfo *info(uint32_t region) const { return (BlkInfo *)(ws + region * L.one); }
    GroupRec *recs(uint32_t region) const { return (GroupRec *)(ws + region * L.one + L.o_rec); }
    uint32_t *order(uint32_t first) const { return sort ? (uint32_t *)(ws + L.o_list) + first : nullptr; }
};
// K1 of blocks [first, first + cnt) into `region`: one wave per 64 blocks (persistent K1 waves,
// 512-2048 of them, made K1 the critical path: c2 24.2-35.7 ms against 23.8, DESIGN.md history,
// round 6).  K1's step budget per iteration: QLZX_K1_KMAX_UNI (12) for uniform 16 KiB calls,
// QLZX_K1_KMAX_MIX (10) for mixed sizes (c4: 377 vs 363 GiB/s; c5 580 vs 560).
inline int batch_k1(const BatchCall &c, hipStream_t st, uint32_t first, uint32_t cnt, uint32_t region) {
    if (const int ef = batch_fault(3)) return ef;
    return launch_k1_parse6((cnt + kParseWG - 1) / kParseWG, st, c.b, c.dst_cap, c.dsize, c.status, first, cnt,
                            c.info(region), c.recs(region), c.L.gmax, c.order(first), c.max_dsize,
                            c.max_dsize > 16384 ? (uint32_t)QLZX_K1_KMAX_MIX : (uint32_t)QLZX_K1_KMAX_UNI);
}
// K2 of the same: one kernel for every block size (the LDS window slides over longer blocks), with
// the CRC prologue when the call asks for a CRC.  That launch's error is left to the caller's
// hipGetLastError().
inline int batch_k2(const BatchCall &c, hipStream_t st, uint32_t first, uint32_t cnt, uint32_t region) {
    if (const int ef = batch_fault(4)) return ef;
    if (!(c.crc_state || c.crc_expect || c.crc_out))
        return launch_k2_nocrc(cnt, st, c.b, c.dsize, c.status, first, cnt, c.info(region), c.recs(region), c.L.gmax,
                               c.order(first));
    hipLaunchKernelGGL(k_dec_chunk4<true>, dim3(cnt), dim3(64), 0, st, c.b, c.dsize, c.status, first, cnt,
                       (const BlkInfo *)c.info(region), (const GroupRec *)c.recs(region), c.L.gmax,
                       (const uint32_t *)c.order(first), c.crc_state, c.crc_expect, c.crc_out);
    return 0;
}

inline int launch_decode_wave(const qlzx_blocks &b, const uint32_t *dst_cap, uint32_t *dsize,
                              int32_t *status, const uint32_t *crc_state, const uint32_t *crc_expect,
                              uint32_t *crc_out, uint32_t max_dsize, void *ws, size_t ws_bytes,
                              hipStream_t s) {
    const BatchLayout L = batch_layout(b.n, max_dsize);
    const BatchCall c{b, dst_cap, dsize, status, crc_state, crc_expect, crc_out, max_dsize, (uint8_t *)ws, L,
                      L.chunk > 64};
    // two workspace regions when the caller gave room for them: K1 of chunk c+1 runs on a side
    // stream while K2 of chunk c runs on `s` (K1 is latency-bound at low occupancy); with one
    // region K1 and K2 of all chunks run on the caller's stream, one after another
    const bool overlap = L.nchunks > 1 && ws_bytes >= 2 * L.one;
    Side *sd = nullptr;
    if (overlap)
        if (const int e = batch_side(s, sd)) return e;
    // A call of two chunks of mixed block sizes (smallest blocks first): K1 of the second chunk
    // runs on a second side stream, so it starts with the first K1 instead of after it.  It holds
    // the longest streams, and its K1 (one lane per block, latency-bound) was the critical path
    // (c4: 15.3 -> 11.7 ms per 4000 MiB chunk with k_rp_scan).  Calls of more chunks (c5's
    // rounds: 560 vs 620 GiB/s) and uniform 16 KiB chunks keep one side stream: there concurrent
    // K1s only compete with the K2s.
    const bool split_k1 = overlap && max_dsize > 16384 && L.nchunks == 2;  // c4's calls
    // Calls of mixed sizes over three chunks or more (c5's rounds): the last chunk holds the
    // longest values, and its K1 (longest per lane, at low occupancy) ran after K2 of the chunk
    // two before had freed a workspace region, in front of its K2 (c5: the last K1 took 7.5 of
    // an 18.7 ms call).  With a region of its own (when the caller gave three), that K1 starts on
    // side stream 2 right after the block order, beside everything else.
    const bool early = overlap && L.regions == 3 && ws_bytes >= 3 * L.one;
    const uint32_t c_early = L.nchunks - (early ? 1 : 0);  // first chunk whose K1 starts early
    if (overlap) (void)hipEventRecord(sd->k2[1], s), (void)hipStreamWaitEvent(sd->st, sd->k2[1], 0);
    if (split_k1 || early) (void)hipStreamWaitEvent(sd->st2, sd->k2[1], 0);
    if (c.sort) {  // block order of the whole call, ahead of the first K1 (workspace region 0)
        hipStream_t s1 = overlap ? sd->st : s;
        uint32_t *aux = (uint32_t *)(c.ws + L.o_aux);
        (void)hipMemsetAsync(aux, 0, kOrderAux * sizeof(uint32_t), s1);
        const dim3 g((b.n + kOrderPerWG - 1) / kOrderPerWG);
        hipLaunchKernelGGL(k_order_count, g, dim3(kOrderWG), 0, s1, b.src_len, b.n, aux);
        hipLaunchKernelGGL(k_order_scatter, g, dim3(kOrderWG), 0, s1, b.src_len, b.n, aux, c.order(0));
        if (split_k1 || early) (void)hipEventRecord(sd->order, sd->st), (void)hipStreamWaitEvent(sd->st2, sd->order, 0);
    }
    if (early) {
        const uint32_t fe = c_early * L.chunk;
        if (const int e1 = batch_k1(c, sd->st2, fe, b.n - fe, 2)) return e1;
        (void)hipEventRecord(sd->last, sd->st2);
    }
    uint32_t ci = 0;
    for (uint32_t first = 0, cnt = 0; first < b.n; first += cnt, ci++) {
        cnt = b.n - first < L.chunk ? b.n - first : L.chunk;
        const bool last_early = ci >= c_early;  // its K1 is already queued on side stream 2
        const uint32_t region = last_early ? 2 : overlap ? ci & 1 : 0;
        if (last_early) {
            (void)hipStreamWaitEvent(s, sd->last, 0);
        } else {
            hipStream_t s1 = overlap ? (split_k1 && (ci & 1) ? sd->st2 : sd->st) : s;
            if (overlap && ci >= 2) (void)hipStreamWaitEvent(s1, sd->k2[ci & 1], 0);  // K2(c-2) freed this half
            if (const int e1 = batch_k1(c, s1, first, cnt, region)) return e1;
            if (overlap) (void)hipEventRecord(sd->k1[ci & 1], s1), (void)hipStreamWaitEvent(s, sd->k1[ci & 1], 0);
        }
        if (const int e2 = batch_k2(c, s, first, cnt, region)) return e2;
        if (overlap) (void)hipEventRecord(sd->k2[ci & 1], s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace qlzx
