// rdb_traced_fwd.hip — the fp16 inference chains WITH the trace stamps (esr_rdb_chain.trace non-null: tools/chain_trace.py,
// the ESR_ABL timing builds), 16-row tiles: plain, noisy and banded (csrc/rdb_chain_kernel.h: TRC).  The launches
// without a trace run the stamp-free instantiations of rdb_fused.hip / rdb_fused_noise.hip / rdb_fused_band.hip.
#include "rdb_chain_kernel.h"

const void* esr_rdb_fwd_traced_fn() { return (const void*)rdb_chain_kernel<_Float16, 0, false, 0, true>; }
int esr_rdb_launch_fwd_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st) {
  if (p.band_rows != 0)
    hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, true, 0, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  else if (p.noise_mode != ESR_NOISE_OFF)
    hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, false, 1, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  else
    hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, false, 0, true>), dim3(grid), dim3(NT), 0, st, p, ntiles, tiles_x, tiles_y, host_abort);
  return esr_check_launch("rdb_chain_kernel<forward, traced>");
}
