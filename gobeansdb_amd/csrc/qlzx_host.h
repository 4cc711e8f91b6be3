// qlzx_host.h -- what the host code of qlzx_api.hip's unit shares: the calling thread's error text
// (qlzx_last_error), the HIP_OK early return and two small helpers.  Included by the files that
// hold host drivers (qlzx_decode_huge.hip, qlzx_encode_huge.hip, qlzx_service.hip,
// qlzx_single.hip, qlzx_api.hip); qlzx_k2.hip's unit has no use for it.
#pragma once

#include <string>

#include "qlzx_device.h"

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
