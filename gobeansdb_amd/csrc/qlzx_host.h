// qlzx_host.h -- what the host code of qlzx_api.hip's unit shares: the calling thread's error text
// (qlzx_last_error), the HIP_OK early return, two small helpers and what the per-thread HIP objects
// (the batch launcher's side streams, the single-call contexts) need at process exit.  Included by
// the files that hold host drivers (qlzx_decode_batch.hip, qlzx_decode_huge.hip,
// qlzx_encode_huge.hip, qlzx_service.hip, qlzx_single.hip, qlzx_api.hip); qlzx_k2.hip's unit has
// no use for it.  What the record-file kernels and their launchers share (replay, read, write, gc,
// hint) is qlzx_recfile.h's, not this file's.
#pragma once

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <string>

#include "qlzx_device.h"

namespace qlzx {

constexpr uint32_t kMaxDevices = 64;  // devices with per-thread or per-process state of their own

// Set by an atexit handler registered once the runtime is in use (after HIP registered its own
// teardown; atexit runs in reverse order): per-thread HIP objects destroyed after that (threads
// exiting during process exit) are left to the runtime's teardown.
inline std::atomic<bool> g_hip_down{false};
inline void note_hip_up() {
    static std::once_flag once;
    std::call_once(once, [] { std::atexit([] { g_hip_down.store(true); }); });
}

}  // namespace qlzx

namespace {

thread_local std::string t_last_error;

int fail(int code, const char *what, hipError_t e = hipSuccess) {
    t_last_error = what;
    if (e != hipSuccess) {
        t_last_error += ": ";
        t_last_error += hipGetErrorString(e);
    }
    return code;
}

#define HIP_OK(expr)                                                     \
    do {                                                                 \
        hipError_t _e = (expr);                                          \
        if (_e != hipSuccess) return fail(QLZX_R_HIP, #expr, _e);       \
    } while (0)

inline uint32_t ld32h(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace
