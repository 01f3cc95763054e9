// rdb_fused_reg.hip — the fp16 inference chain for REGULAR geometry (csrc/rdb_chain_kernel.h: REG): H a multiple of 16,
// W of 32, no bands, no noise layers, no trace — every tile lies inside the image, so the kernel carries no test for
// ragged tiles and no clamp.  chain_launch (rdb_fused.hip) picks it per launch; ESR_RDB_GENERAL=1 keeps the general one.
#include "rdb_chain_kernel.h"

const void* esr_rdb_fwd_reg_fn() { return (const void*)rdb_chain_kernel<_Float16, 0, false, 0, false, true>; }
int esr_rdb_launch_fwd_reg(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st) {
  hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, false, 0, false, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  return esr_check_launch("rdb_chain_kernel<forward, regular>");
}
