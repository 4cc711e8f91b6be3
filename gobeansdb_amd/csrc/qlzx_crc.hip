// qlzx_crc.hip -- k_crc32: batched CRC32 (store/crc32.go:61-68 semantics), one wavefront per
// buffer (wave_crc, qlzx_crc.h).
#include "qlzx_crc.h"

namespace qlzx {
__global__ void __launch_bounds__(256) k_crc32(const uint8_t *src, const uint64_t *off,
                                               const uint32_t *len, uint32_t n,
                                               const uint32_t *init, uint32_t final_xor,
                                               uint32_t *out) {
    __shared__ uint32_t tab[kCrcLdsWords];
    load_crc_lds(tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (i >= n) return;
    const uint32_t reg = wave_crc(tab, src + off[i], len[i], init ? init[i] : 0xffffffffu, lane);
    if (lane == 0) out[i] = reg ^ final_xor;
}

}  // namespace qlzx
