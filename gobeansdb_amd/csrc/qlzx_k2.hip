// qlzx_k2.hip -- K1 (k_dec_parse6) and K2 without the CRC prologue (k_dec_chunk4<false>) of the
// batch decoder in a translation unit of their own, compiled with the iterative-ilp machine
// scheduler (-mllvm -amdgpu-sched-strategy=iterative-ilp, gobeansdb_amd/build.py): that strategy
// speeds these two kernels up but slows K2 with its CRC prologue, the encoder and the replay
// kernels, and the strategy is per translation unit (profiles/r05_sched_strategy_ab.txt).  The
// rest of the library is qlzx_api.hip's unit, which launches the two through the functions below.
#include "qlzx_device.h"
#include "qlzx_crc.h"
#include "qlzx_decode_batch.h"
#include "qlzx_decode_k1.h"
#include "qlzx_decode_k2.h"

namespace qlzx {

int launch_k1_parse6(uint32_t grid, hipStream_t s, const qlzx_blocks &b, const uint32_t *dst_cap, uint32_t *dsize,
                     int32_t *status, uint32_t first, uint32_t cnt, BlkInfo *info, GroupRec *recs, uint32_t gmax,
                     const uint32_t *order, uint32_t max_dsize, uint32_t kmax) {
    hipLaunchKernelGGL(k_dec_parse6, dim3(grid), dim3(kParseWG), 0, s, b, dst_cap, dsize, status, first, cnt, info,
                       recs, gmax, order, max_dsize, kmax);
    return (int)hipGetLastError();
}

int launch_k2_nocrc(uint32_t grid, hipStream_t s, const qlzx_blocks &b, uint32_t *dsize, int32_t *status,
                    uint32_t first, uint32_t cnt, const BlkInfo *info, const GroupRec *recs, uint32_t gmax,
                    const uint32_t *order) {
    hipLaunchKernelGGL(k_dec_chunk4<false>, dim3(grid), dim3(64), 0, s, b, dsize, status, first, cnt, info, recs,
                       gmax, order, nullptr, nullptr, nullptr);
    return (int)hipGetLastError();
}

#ifdef QLZX_PROFILE
int k2_profile_set(void *dev_buf) {  // this unit's g_prof (qlzx_profile_set)
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_prof), &dev_buf, sizeof(void *));
}
#endif

}  // namespace qlzx
