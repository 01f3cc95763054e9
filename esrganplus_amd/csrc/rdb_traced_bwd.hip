// rdb_traced_bwd.hip — the backward chain WITH the trace stamps (esr_rdb_chain.trace non-null: tools/chain_trace_bwd.py),
// 16-row tiles (csrc/rdb_chain_kernel.h: TRC; rdb_fused_bwd.hip holds the stamp-free one).
#include "rdb_chain_kernel.h"

int esr_rdb_launch_bwd_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st) {
  hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 2, false, -1, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  return esr_check_launch("rdb_chain_kernel<bwd, traced>");
}
