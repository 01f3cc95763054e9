// rdb_traced_train.hip — the training-forward chain WITH the trace stamps (esr_rdb_chain.trace non-null:
// tools/chain_trace_train.py), 16-row tiles (csrc/rdb_chain_kernel.h: TRC; rdb_fused_train.hip holds the stamp-free ones).
#include "rdb_chain_kernel.h"

int esr_rdb_launch_train_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st) {
  if (p.noise_mode != ESR_NOISE_OFF)
    hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 1, false, 1, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  else
    hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 1, false, 0, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  return esr_check_launch("rdb_chain_kernel<train, traced>");
}
