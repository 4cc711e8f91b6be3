// qlzx_synth.hip -- the synthetic workload generator: text and image-like
// blocks from a seed and a block id, one lane per block.
#include "qlzx_device.h"

namespace qlzx {
__device__ __forceinline__ uint64_t sm64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t block_seed(uint64_t seed, uint64_t id) {
    uint64_t s = seed ^ (id * 0xD1B54A32D192ED03ull);
    return sm64(s);
}
__device__ __forceinline__ uint32_t zipf_pick(const uint32_t *cdf, uint32_t nw, uint32_t u) {
    uint32_t lo = 0, hi = nw - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ void gen_text(uint64_t s, const uint8_t *vocab, const uint32_t *voff, const uint32_t *cdf,
                         uint32_t nw, uint8_t *out, uint32_t n) {
    uint32_t p = 0;
    while (p < n) {
        const uint64_t r = sm64(s);
        const uint32_t w = zipf_pick(cdf, nw, (uint32_t)r);
        for (uint32_t i = voff[w]; i < voff[w + 1] && p < n; i++) out[p++] = vocab[i];
        if ((uint32_t)(r >> 32) % 100u < 8u && p < n) out[p++] = '.';
        if (p < n) out[p++] = ' ';
    }
}
__device__ void gen_image(uint64_t s, const uint8_t *vocab, const uint32_t *voff, const uint32_t *cdf,
                          uint32_t nw, uint8_t *out, uint32_t n) {
    const uint64_t kind = sm64(s);
    if ((kind & 3) != 0) {
        for (uint32_t p = 0; p < n; p += 8) {
            const uint64_t r = sm64(s);
            for (uint32_t b = 0; b < 8 && p + b < n; b++) out[p + b] = (uint8_t)(r >> (8 * b));
        }
        return;
    }
    gen_text(sm64(s), vocab, voff, cdf, nw, out, n);
    const uint32_t pct = 40u + (uint32_t)((kind >> 8) % 6u);
    for (uint32_t p = 0; p < n; p++) {
        const uint64_t r = sm64(s);
        if ((uint32_t)r % 100u < pct) out[p] = (uint8_t)(r >> 32);
    }
}

__global__ void __launch_bounds__(64) k_synth(int kind, uint64_t seed, uint64_t first, uint8_t *dst,
                                              const uint64_t *off, const uint32_t *len, uint32_t n,
                                              const uint8_t *vocab, const uint32_t *voff,
                                              const uint32_t *cdf, uint32_t nw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = block_seed(seed, first + i);
    if (kind == 0) gen_text(s, vocab, voff, cdf, nw, dst + off[i], len[i]);
    else gen_image(s, vocab, voff, cdf, nw, dst + off[i], len[i]);
}

}  // namespace qlzx

