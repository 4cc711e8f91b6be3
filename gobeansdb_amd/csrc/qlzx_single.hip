// qlzx_single.hip -- the single-call runtime: the quicklz.h drop-ins (qlz_compress,
// qlz_decompress, crc32_write) and their qlzx_* siblings with an error channel, on the GPU.
// Included by qlzx_api.hip after qlzx_service.hip.  What fits a slot of the request service is
// one request (SvcCall); the rest (large values, the Go-compat and level-1 modes) is a staged
// call (Staged): each calling thread owns a stream, a device buffer and a pinned host buffer, so
// the symbols are re-entrant like the reference (quicklz.h: one scratch per call).  A staged call
// copies the caller's bytes into the pinned buffer, does one H2D, a batch entry point's kernels,
// one D2H of the result and its descriptor, and one stream synchronisation; the caller's
// pageable buffers are touched only by host memcpy.
#include "qlzx_host.h"

namespace {

using qlzx::g_hip_down;

struct Meta {  // one-block batch descriptors, device side
    uint64_t src_off, dst_off;
    uint32_t src_len, dst_cap, out_size, crc_in, crc_out;
    int32_t status;
};

struct Ctx {
    hipStream_t s = nullptr;
    uint8_t *d_buf = nullptr;  // [meta 256 | src | dst | ws]
    size_t d_cap = 0;
    uint8_t *h_buf = nullptr;  // pinned: [meta 256 | staging]
    size_t h_cap = 0;
    bool ok = false;
    ~Ctx() {
        if (g_hip_down.load()) return;
        if (d_buf) (void)hipFree(d_buf);
        if (h_buf) (void)hipHostFree(h_buf);
        if (s) (void)hipStreamDestroy(s);
    }
    int init() {
        if (ok) return 0;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(QLZX_R_NO_DEVICE, "no HIP device");
        qlzx::note_hip_up();
        HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        ok = true;
        return 0;
    }
    // Buffers of a call above kCtxKeep are released after it: a thread keeps at most kCtxKeep
    // of each (the single-call sizes the service does not take are the rare large values).
    static constexpr size_t kCtxKeep = 8u << 20;
    void trim() {
        if (g_hip_down.load()) return;
        if (d_cap > kCtxKeep) (void)hipFree(d_buf), d_buf = nullptr, d_cap = 0;
        if (h_cap > kCtxKeep) (void)hipHostFree(h_buf), h_buf = nullptr, h_cap = 0;
    }
    int reserve(size_t dev_bytes, size_t host_bytes) {
        if (dev_bytes > d_cap) {
            if (d_buf) (void)hipFree(d_buf);
            d_buf = nullptr;
            d_cap = 0;
            const size_t want = align_up(dev_bytes + dev_bytes / 4, 1 << 20);
            HIP_OK(hipMalloc((void **)&d_buf, want));
            d_cap = want;
        }
        if (host_bytes > h_cap) {
            if (h_buf) (void)hipHostFree(h_buf);
            h_buf = nullptr;
            h_cap = 0;
            const size_t want = align_up(host_bytes + host_bytes / 4, 1 << 20);
            HIP_OK(hipHostMalloc((void **)&h_buf, want, hipHostMallocDefault));
            h_cap = want;
        }
        return 0;
    }
};
thread_local Ctx t_ctx;

// One staged call on the calling thread's Ctx.  begin() lays the buffers out and sends the
// descriptor and the input; the caller launches on s with the device pointers; finish() brings
// the descriptor and the result back.  Both return qlzx_return codes.  m and h_data stay valid
// until the destructor, which trims the buffers on every exit path.
struct Staged {
    Ctx &c = t_ctx;
    hipStream_t s = nullptr;
    uint8_t *d_src = nullptr, *d_dst = nullptr, *d_ws = nullptr;
    Meta *dm = nullptr;         // the descriptor on the device: the batch entry points' arrays of one
    Meta *m = nullptr;          // ... and on the host: `fields` before finish(), the device's copy after
    uint8_t *h_data = nullptr;  // pinned staging: the input, then the result
    ~Staged() { c.trim(); }

    // fields.src_len: the input's length; dst_bytes / ws_bytes: device room for result and workspace
    int begin(const Meta &fields, const void *src, size_t dst_bytes, size_t ws_bytes) {
        if (int r = c.init()) return r;
        const size_t len = fields.src_len;
        const size_t src_b = align_up(len, 256), dst_b = align_up(dst_bytes, 256);
        // pinned: [meta | src staging, reused for the result]
        if (int r = c.reserve(256 + src_b + dst_b + ws_bytes, 256 + std::max(src_b, dst_b))) return r;
        s = c.s;
        dm = (Meta *)c.d_buf;
        d_src = c.d_buf + 256, d_dst = d_src + src_b, d_ws = d_dst + dst_b;
        m = (Meta *)c.h_buf;
        h_data = c.h_buf + 256;
        *m = fields;
        memcpy(h_data, src, len);
        // one H2D of descriptor + source (contiguous on both sides)
        HIP_OK(hipMemcpyAsync(c.d_buf, c.h_buf, 256 + len, hipMemcpyHostToDevice, s));
        return QLZX_R_OK;
    }
    qlzx_blocks blocks() const { return qlzx_blocks{d_src, &dm->src_off, &dm->src_len, d_dst, &dm->dst_off, 1}; }
    // D2H of the descriptor and of result_len bytes of the result, then the only synchronisation
    int finish(size_t result_len) {
        HIP_OK(hipMemcpyAsync(m, dm, sizeof(Meta), hipMemcpyDeviceToHost, s));
        if (result_len) HIP_OK(hipMemcpyAsync(h_data, d_dst, result_len, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        return QLZX_R_OK;
    }
};

// One request to the service: the constructor takes a slot and copies the input in; the slot,
// and with it out(), is the caller's until the destructor gives it back.
struct SvcCall {
    Service *S;
    const uint32_t b, len;
    qlzx::SvcDone done{};  // the completion record, after run()
    SvcCall(Service *svc, const void *src, size_t n) : S(svc), b(svc->take_slot()), len((uint32_t)n) {
        memcpy(S->in(b), src, n);
    }
    ~SvcCall() { S->give_slot(b); }
    // r: cap / arg / expect / mode as the op reads them; returns a qlzx_return code
    int run(uint32_t op, qlzx::SvcReq r = {}) {
        r.slot = b, r.len = len;
        const int rc = S->run(op, r);
        done = *(const qlzx::SvcDone *)(S->h_done + b);
        return rc;
    }
    const uint8_t *out() const { return S->out(b); }
};

// The quicklz.h drop-ins have no error channel: cgo's CCompress ignores a 0 return and keeps an
// empty Body (quicklz/cquicklz.go:38-40, then store/item.go:145-159 stores it as "compressed"),
// and crc32_write's result becomes the record CRC (store/crc32.go:81-84).  The reference CPU
// code cannot fail, so a runtime failure here (no device, a HIP error) stops the process with
// the reason instead of returning a plausible wrong value.
[[noreturn]] void die(const char *who) {
    fprintf(stderr, "libqlzx: %s: %s (GPU runtime failure; the drop-in has no error channel)\n", who,
            t_last_error.empty() ? "unknown error" : t_last_error.c_str());
    fflush(stderr);
    abort();
}

// Host CRC-32/IEEE (store/crc32.go:5-59's table, slicing-by-8) for the short slices crc32_write
// receives; the tables are built once from the polynomial.
#ifndef QLZX_CRC_HOST_MAX  // longest crc32_write slice folded on the host (DESIGN.md §3 "Single calls")
#define QLZX_CRC_HOST_MAX 256
#endif
constexpr size_t kCrcHostMax = QLZX_CRC_HOST_MAX;
struct HostCrcTables {
    uint32_t t[8][256];
    HostCrcTables() {
        for (uint32_t b = 0; b < 256; b++) {
            uint32_t c = b;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            t[0][b] = c;
        }
        for (uint32_t b = 0; b < 256; b++)
            for (int j = 1; j < 8; j++) t[j][b] = (t[j - 1][b] >> 8) ^ t[0][t[j - 1][b] & 0xffu];
    }
};
uint32_t host_crc32(uint32_t crc, const unsigned char *p, size_t n) {
    static const HostCrcTables T;
    uint32_t c = crc;  // crc32_write is the raw table update (store/crc32.go:61-68): no inversions
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 0xff] ^ T.t[2][(hi >> 8) & 0xff] ^ T.t[1][(hi >> 16) & 0xff] ^ T.t[0][hi >> 24];
    }
    for (; n; n--, p++) c = T.t[0][(c ^ *p) & 0xffu] ^ (c >> 8);
    return c;
}

thread_local int t_last_status = QLZX_OK;

#ifndef QLZX_SOLO_ENC_CAP
#define QLZX_SOLO_ENC_CAP 65536u
#endif

// One block through the batch encoder.  Returns a qlzx_return code (runtime failure) and sets
// *csize (0 with t_last_status != OK when the kernel rejects the block).
int compress1(const void *source, char *destination, size_t size, uint32_t flags, size_t *csize) {
    *csize = 0;
    t_last_status = QLZX_E_RUNTIME;  // replaced below; never left over from an earlier call
    if (flags == 0 && size <= qlzx::kSvcMaxLen) {  // the request path (qlzx_service.hip)
        Service *S = service();
        if (!S) return QLZX_R_NO_DEVICE;
        SvcCall q(S, source, size);
        qlzx::SvcReq r{};
        r.cap = (uint32_t)size + 400;
        const int rc = q.run(qlzx::kSvcCompress, r);
        if (rc != QLZX_R_OK) return rc;
        t_last_status = q.done.status;
        if (q.done.status != QLZX_OK) return QLZX_R_OK;
        if (q.done.out == 0 || q.done.out > size + 400) return fail(QLZX_R_HIP, "compress1: bad result size");
        memcpy(destination, q.out(), q.done.out);
        *csize = q.done.out;
        return QLZX_R_OK;
    }
    const bool l1 = (flags & QLZX_F_LEVEL1) != 0;
    // a lone block gets the widest encoder workgroup whatever its size (max_len only picks the
    // kernel: a 4 KiB block on the 64-thread k_encode_wg<4096> is one wave walking every phase)
    const uint32_t max_len = size <= QLZX_SOLO_ENC_CAP ? QLZX_SOLO_ENC_CAP : (uint32_t)size;
    const size_t ws_b = l1 ? qlzx_go_l1_workspace_size(1) : qlzx_compress_workspace_size(1, max_len);
    Staged c;
    Meta f{};
    f.src_len = (uint32_t)size;
    if (int r = c.begin(f, source, size + 400, ws_b)) return r;
    const qlzx_blocks b = c.blocks();
    if (int r = l1 ? qlzx_go_l1_compress_batch(&b, &c.dm->out_size, &c.dm->status, c.d_ws, ws_b, c.s)
                   : qlzx_compress_batch(&b, &c.dm->out_size, &c.dm->status, nullptr, nullptr, max_len, flags,
                                         c.d_ws, ws_b, c.s))
        return r;
    if (int r = c.finish(size + 400)) return r;  // the largest possible result
    t_last_status = c.m->status;
    if (c.m->status != QLZX_OK) return QLZX_R_OK;
    if (c.m->out_size == 0 || c.m->out_size > size + 400) return fail(QLZX_R_HIP, "compress1: bad result size");
    memcpy(destination, c.h_data, c.m->out_size);
    *csize = c.m->out_size;
    return QLZX_R_OK;
}

// One level-3 block through the decoder; *dsize = 0 with t_last_status != OK on a corrupt stream.
int decompress1(const char *source, void *destination, size_t *dsize_out) {
    *dsize_out = 0;
    const size_t csize = qlz_size_compressed(source), dsize = qlz_size_decompressed(source);
    t_last_status = QLZX_E_RUNTIME;  // replaced below; never left over from an earlier call
    if (csize < 3) {
        t_last_status = QLZX_E_HEADER;
        return QLZX_R_OK;
    }
    // The service's k_svc_decode runs the one-workgroup decoders (small_decode, solo_decode) on
    // every block they can take, so the staged call below is always the batch decoder.
    static_assert(qlzx::kSvcMaxLen >= QLZX_FAST_MAX_DSIZE, "the request path takes every solo-sized block");
    if (dsize <= qlzx::kSvcMaxLen && csize <= qlzx::kSoloMaxCsize) {  // the request path
        Service *S = service();
        if (!S) return QLZX_R_NO_DEVICE;
        SvcCall q(S, source, csize);
        qlzx::SvcReq r{};
        r.cap = (uint32_t)dsize;
        const int rc = q.run(qlzx::kSvcDecode, r);
        if (rc != QLZX_R_OK) return rc;
        t_last_status = q.done.status;
        if (q.done.status == QLZX_OK) memcpy(destination, q.out(), q.done.out), *dsize_out = q.done.out;
        return QLZX_R_OK;
    }
    const size_t ws_b = align_up(qlzx_decompress_workspace_size(1, (uint32_t)dsize), 256);
    Staged c;
    Meta f{};
    f.src_len = (uint32_t)csize, f.dst_cap = (uint32_t)dsize;
    if (int r = c.begin(f, source, dsize + 1, ws_b)) return r;
    const qlzx_blocks b = c.blocks();
    if (int r = qlzx_decompress_batch(&b, &c.dm->dst_cap, &c.dm->out_size, &c.dm->status, nullptr, nullptr, nullptr,
                                      (uint32_t)dsize, c.d_ws, ws_b, c.s))
        return r;
    if (int r = c.finish(dsize)) return r;
    t_last_status = c.m->status;
    if (c.m->status == QLZX_OK) {
        memcpy(destination, c.h_data, dsize);
        *dsize_out = c.m->out_size;
    }
    return QLZX_R_OK;
}

}  // namespace

extern "C" {

int qlzx_read_record1(const void *value, size_t vlen, uint32_t crc_state, uint32_t crc_expect, int compressed,
                      void *dst, size_t dst_cap, size_t *out_len, int32_t *status) {
    if (!value && vlen) return fail(QLZX_R_BAD_ARG, "qlzx_read_record1: null value");
    if (!out_len || !status) return fail(QLZX_R_BAD_ARG, "qlzx_read_record1: null out_len / status");
    *out_len = 0;
    *status = QLZX_E_RUNTIME;
    const uint8_t *v = (const uint8_t *)value;
    size_t dsize = 0;
    if (compressed) {
        if (vlen < 3 || vlen < (size_t)((v[0] & 2) ? 9 : 3)) {  // Payload.Decompress: CDecompressSafe's panic
            // the CRC is still checked first, as readRecordAt does before the payload is used
            const uint32_t c = vlen ? crc32_write(crc_state, (unsigned char *)value, (int)vlen) : crc_state;
            *status = (~c != crc_expect) ? QLZX_E_CRC : QLZX_E_HEADER;
            return QLZX_R_OK;
        }
        dsize = qlz_size_decompressed((const char *)value);
        if (!dst || dst_cap < dsize) return fail(QLZX_R_BAD_ARG, "qlzx_read_record1: dst_cap below the value's dsize");
    }
    const bool served = vlen <= qlzx::kSvcIn - 64 &&
                        (!compressed || (dsize <= qlzx::kSvcMaxLen && vlen <= qlzx::kSoloMaxCsize));
    if (served) {  // one request: CRC check, then the decode, in one kernel (qlzx_service.hip)
        Service *S = service();
        if (!S) return QLZX_R_NO_DEVICE;
        SvcCall q(S, value, vlen);
        qlzx::SvcReq r{};
        r.cap = (uint32_t)dsize, r.arg = crc_state, r.expect = crc_expect;
        r.mode = qlzx::kSvcVerify | (compressed ? 0u : qlzx::kSvcNoDecode);
        const int rc = q.run(qlzx::kSvcDecode, r);
        if (rc == QLZX_R_OK) {
            *status = q.done.status;
            if (q.done.status == QLZX_OK) {
                if (compressed) memcpy(dst, q.out(), q.done.out), *out_len = q.done.out;
                else *out_len = vlen;
            }
        }
        t_last_status = *status;
        return rc;
    }
    // longer values: the general per-call paths (GPU), CRC first
    const uint32_t c = crc32_write(crc_state, (unsigned char *)value, (int)vlen);
    if (~c != crc_expect) {
        *status = t_last_status = QLZX_E_CRC;
        return QLZX_R_OK;
    }
    if (!compressed) {
        *status = t_last_status = QLZX_OK;
        *out_len = vlen;
        return QLZX_R_OK;
    }
    size_t n = 0;
    const int rc = decompress1((const char *)value, dst, &n);
    *status = t_last_status;
    *out_len = n;
    return rc;
}

int qlzx_last_status(void) { return t_last_status; }

size_t qlz_compress(const void *source, char *destination, size_t size, char *scratch_compress) {
    (void)scratch_compress;
    if (size == 0 || size > 0xffffffffull - 400) return 0;  // quicklz.c:705-706
    size_t n = 0;
    if (compress1(source, destination, size, 0, &n) || n == 0) die("qlz_compress");
    return n;
}

size_t qlzx_compress1(const void *source, char *destination, size_t size, uint32_t flags) {
    t_last_status = QLZX_E_RUNTIME;
    if (size == 0 || size > 0xffffffffull - 400) {  // quicklz.c:705-706
        t_last_status = size ? QLZX_E_TOO_LARGE : QLZX_E_EMPTY;
        return 0;
    }
    size_t n = 0;
    return compress1(source, destination, size, flags, &n) ? 0 : n;
}

size_t qlz_decompress(const char *source, void *destination, char *scratch_decompress) {
    (void)scratch_decompress;
    size_t n = 0;
    if (decompress1(source, destination, &n)) die("qlz_decompress");
    return n;
}

size_t qlzx_go_decompress1(const char *source, size_t source_len, void *destination, size_t dst_cap) {
    t_last_status = QLZX_E_RUNTIME;  // replaced below; never left over from an earlier call
    if (!source || source_len == 0) {
        t_last_status = QLZX_E_HEADER;
        return QLZX_GO_ERROR;
    }
    const size_t hdr = (source[0] & 2) ? 9 : 3;
    const size_t dsize = source_len >= hdr ? qlz_size_decompressed(source) : 0;  // else the kernel: E_HEADER
    const int level = ((unsigned char)source[0] >> 2) & 3;
    if (source_len >= hdr && level != 1 && level != 3) {  // the kernel's order: header, level, then dst_cap
        t_last_status = QLZX_E_LEVEL;
        fail(QLZX_R_OK, "qlzx_go_decompress1: status 3");
        return QLZX_GO_ERROR;
    }
    if (dsize > dst_cap) {
        t_last_status = QLZX_E_DST_CAP;
        fail(QLZX_R_BAD_ARG, "qlzx_go_decompress1: destination too small");
        return QLZX_GO_ERROR;
    }
    const size_t ws_b = qlzx_go_decompress_workspace_size(1);
    Staged c;
    Meta f{};
    f.src_len = (uint32_t)source_len, f.dst_cap = (uint32_t)dsize;
    if (c.begin(f, source, dsize + 1, ws_b)) return QLZX_GO_ERROR;
    const qlzx_blocks b = c.blocks();
    if (qlzx_go_decompress_batch(&b, &c.dm->dst_cap, &c.dm->out_size, &c.dm->status, c.d_ws, ws_b, c.s) ||
        c.finish(dsize))
        return QLZX_GO_ERROR;
    t_last_status = c.m->status;
    if (c.m->status != QLZX_OK) {
        char msg[64];
        snprintf(msg, sizeof msg, "qlzx_go_decompress1: status %d", (int)c.m->status);
        fail(QLZX_R_OK, msg);
        return QLZX_GO_ERROR;
    }
    memcpy(destination, c.h_data, dsize);
    return dsize;
}

uint32_t crc32_write(uint32_t crc, unsigned char *buf, int len) {
    if (len <= 0) return crc;  // store/crc32.go:65 loops zero times
    if ((size_t)len <= kCrcHostMax) {
        // readRecordAt / WriteRecord.getCRC pass header[4:24] and the key as slices of their own
        // (store/datafile.go:66-76); a request round trip (~20 us) costs more than the bytes, so
        // slices up to kCrcHostMax are folded on the calling thread.  The library still requires
        // its device: without one the call stops the process like every drop-in.
        if (!service()) die("crc32_write");
        return host_crc32(crc, buf, (size_t)len);
    }
    if ((size_t)len <= qlzx::kSvcIn - 64) {  // the request path (qlzx_service.hip)
        Service *S = service();
        if (!S) die("crc32_write");
        SvcCall q(S, buf, (size_t)len);
        qlzx::SvcReq r{};
        r.arg = crc;
        if (q.run(qlzx::kSvcCrc, r) != QLZX_R_OK) die("crc32_write");
        return q.done.crc;
    }
    Staged c;
    Meta f{};
    f.src_len = (uint32_t)len, f.crc_in = crc;
    if (c.begin(f, buf, 0, 0) ||
        qlzx_crc32_batch(c.d_src, &c.dm->src_off, &c.dm->src_len, 1, &c.dm->crc_in, 0, &c.dm->crc_out, c.s) ||
        c.finish(0))
        die("crc32_write");
    return c.m->crc_out;
}

}  // extern "C"
