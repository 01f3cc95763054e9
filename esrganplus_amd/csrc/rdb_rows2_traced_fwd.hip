// rdb_rows2_traced_fwd.hip — rdb_rows2_fwd.hip's chain WITH the trace stamps (esr_rdb_chain.trace non-null), 8x32 tiles
// (csrc/rdb_chain_kernel.h: ESR_R, TRC).
#define ESR_R 2
#include "rdb_chain_kernel.h"

int esr_rdb_launch_fwd_r2_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st) {
  hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, false, 0, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  return esr_check_launch("rdb_chain_kernel<fwd, 2 rows, traced>");
}
