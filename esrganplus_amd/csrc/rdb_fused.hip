// rdb_fused.hip — host entry points of the fused dense-block chain + the general inference instantiations of its kernel
// (csrc/rdb_chain_kernel.h; the regular-geometry, training-forward, backward and traced instantiations live in
// rdb_fused_reg.hip / rdb_fused_train.hip / rdb_fused_bwd.hip / rdb_traced_*.hip so that they compile in parallel).
#include "rdb_chain_kernel.h"
#include <atomic>
#include <mutex>

int esr_rdb_wgrad_run_follow(const esr_rdb_wgrad* p, esr_stream_t stream, const uint32_t* flags, int tiles_x, int tiles_y, unsigned* host_abort);   // rdb_wgrad.hip
// defined next to their kernels
int esr_rdb_launch_train(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_band(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_noisy(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
// the same chains built for 2 / 1 rows per wave (8x32 / 4x32 tiles): rdb_rows{2,1}_{train,bwd}.hip
int esr_rdb_launch_train_r2(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_train_r1(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd_r2(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd_r1(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_fwd_r2(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_fwd_r1(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
// the fp16 inference chain for regular geometry (rdb_fused_reg.hip)
int esr_rdb_launch_fwd_reg(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
const void* esr_rdb_fwd_reg_fn();
// the fp16 chains with the trace stamps, for launches with esr_rdb_chain.trace set (rdb_traced_*.hip, rdb_rows{1,2}_traced_*.hip)
int esr_rdb_launch_fwd_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
const void* esr_rdb_fwd_traced_fn();
int esr_rdb_launch_train_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_fwd_r2_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_fwd_r1_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_train_r2_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_train_r1_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd_r2_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);
int esr_rdb_launch_bwd_r1_traced(const esr_rdb_chain& p, int grid, int ntiles, int tiles_x, int tiles_y, unsigned* host_abort, hipStream_t st);

// ---- per-device bookkeeping -------------------------------------------------------------------------------------
// Everything the library keeps about launches in flight is keyed by DEVICE: nn.DataParallel (networks.py:105-107) drives
// one replica per device from one thread each inside ONE process, and a chain on device 0 has nothing to do with the
// CUs of device 1 — a process-global table would order them against each other with cross-device event waits, and one
// device's abort would fail the other's next call (VERDICT r04 missing #2).
constexpr int ESR_MAX_DEV = 64;
thread_local int t_dev_alias = -1;               // esr_debug_device_alias: tests on a one-GPU box
int esr_bookkeeping_device() {
  if (t_dev_alias >= 0) return t_dev_alias % ESR_MAX_DEV;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) { (void)hipGetLastError(); dev = 0; }
  return dev % ESR_MAX_DEV;
}
// CUs of the CURRENT device, cached per device (rdb_chain_kernel.h's num_cus() caches the first device's count per
// process; a process may drive several devices)
static int num_cus_dev() {
  static std::atomic<int> cached[ESR_MAX_DEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ESR_MAX_DEV) { (void)hipGetLastError(); return 256; }
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v <= 0) {
    hipDeviceProp_t prop;
    v = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 0;
    if (v <= 0) v = 256;
    cached[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}
extern "C" int esr_debug_device_alias(int32_t alias) {
  const int old = t_dev_alias;
  t_dev_alias = alias;
  return old;
}

namespace {
// pinned host words the kernels raise when a bounded spin times out: one 64-byte line per device in one mapped,
// portable allocation (first use allocates it)
unsigned* abort_words() {
  static unsigned* w = [] {
    unsigned* q = nullptr;
    if (hipHostMalloc((void**)&q, 64 * ESR_MAX_DEV, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return (unsigned*)nullptr; }
    for (int i = 0; i < 16 * ESR_MAX_DEV; ++i) q[i] = 0u;
    return q;
  }();
  return w;
}
unsigned* abort_word(int dev) {
  unsigned* w = abort_words();
  return w ? w + 16 * dev : nullptr;
}
// device-visible alias of a device's word, as seen from the CURRENT device
unsigned* abort_word_dev(int dev) {
  unsigned* w = abort_word(dev);
  void* q = nullptr;
  if (!w || hipHostGetDevicePointer(&q, w, 0) != hipSuccess) { (void)hipGetLastError(); return (unsigned*)nullptr; }
  return (unsigned*)q;
}
bool coop_launch() {
  static const bool v = [] { const char* e = getenv("ESR_RDB_COOP"); return e && atoi(e) != 0; }();
  return v;
}

// Chains on DIFFERENT streams of ONE device.  Every chain launch assumes its whole grid becomes resident (a tile spins
// on the flags of its neighbours); two launches in flight on two streams may each get a part of the CUs and then starve
// each other until the 1 s abort.  So the library keeps, per device, the launches it has not yet seen complete: a launch
// whose grid does not fit next to the ones still in flight on other streams of the same device is ordered after them
// with an event wait on the device (the host never blocks; launches on one stream are ordered anyway; chains that fit
// side by side still overlap).  Streams under graph capture are left alone (their order is the graph's).
struct InFlight { hipEvent_t ev; hipStream_t st; int grid; bool live; };
constexpr int N_INFLIGHT = 8;
struct DevTable { InFlight e[N_INFLIGHT]; std::mutex mu; unsigned next; };
DevTable g_tables[ESR_MAX_DEV];
std::atomic<uint64_t> g_order_waits{0};          // event waits inserted by chain_order_before_launch (esr_debug_chain_order_waits)

bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool c = hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  return c;
}

// ESR_RDB_GENERAL=1 (read once): regular shapes run the general inference chain as well (A/B, tests)
std::atomic<int> g_force_general{-1};             // esr_debug_chain_force_general: 0 / 1 override the environment
bool force_general() {
  static const bool v = [] { const char* e = getenv("ESR_RDB_GENERAL"); return e && atoi(e) != 0; }();
  const int o = g_force_general.load(std::memory_order_relaxed);
  return o >= 0 ? o != 0 : v;
}
std::atomic<int> g_last_variant{0};              // esr_debug_chain_last_variant

bool chain_order_on() {                          // ESR_RDB_ORDER=0: measurement only (tools / experiments)
  static const bool v = [] { const char* e = getenv("ESR_RDB_ORDER"); return !e || atoi(e) != 0; }();
  return v;
}

void chain_order_before_launch(hipStream_t st, int grid, int cus) {
  if (!chain_order_on() || capturing(st)) return;
  DevTable& T = g_tables[esr_bookkeeping_device()];
  std::lock_guard<std::mutex> lk(T.mu);
  int others = 0;
  for (InFlight& e : T.e) {
    if (!e.live) continue;
    if (hipEventQuery(e.ev) == hipSuccess) e.live = false;
    else if (e.st != st) others += e.grid;
  }
  if (others + grid > cus)
    for (InFlight& e : T.e)
      if (e.live && e.st != st) { (void)hipStreamWaitEvent(st, e.ev, 0); g_order_waits.fetch_add(1, std::memory_order_relaxed); }
  (void)hipGetLastError();                       // hipEventQuery's "not ready" is not an error of this launch
}

void chain_record_launch(hipStream_t st, int grid) {
  if (!chain_order_on() || capturing(st)) return;
  DevTable& T = g_tables[esr_bookkeeping_device()];
  std::lock_guard<std::mutex> lk(T.mu);
  // one entry per stream (launches on a stream run one after the other: the newest stands for all of them)
  InFlight* slot = nullptr;
  for (InFlight& e : T.e)
    if (e.ev && e.st == st) { slot = &e; break; }
  if (!slot)
    for (InFlight& e : T.e)
      if (!e.live) { slot = &e; break; }
  if (!slot) {                                   // chains in flight on N_INFLIGHT other streams: let the oldest finish
    slot = &T.e[T.next++ % N_INFLIGHT];
    (void)hipEventSynchronize(slot->ev);
  }
  slot->live = false;
  if (!slot->ev && hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
  if (hipEventRecord(slot->ev, st) != hipSuccess) { (void)hipGetLastError(); return; }
  slot->st = st; slot->grid = grid; slot->live = true;
}
}  // namespace

// Diagnostic (tests/test_gpu_rdb_chain.py): the number of cross-stream event waits the chain ordering has inserted so far.
extern "C" uint64_t esr_debug_chain_order_waits(void) { return g_order_waits.load(std::memory_order_relaxed); }
// Diagnostic (tests/test_gpu_chain_variants.py): the kernel variant the last chain launch of this process ran.
extern "C" int esr_debug_chain_last_variant(void) { return g_last_variant.load(std::memory_order_relaxed); }
// .. and the in-process form of ESR_RDB_GENERAL (which is read once): 1 / 0 = general chain forced / not forced whatever
// the environment says, < 0 = back to the environment.  Returns the previous override.
extern "C" int esr_debug_chain_force_general(int32_t on) { return g_force_general.exchange(on < 0 ? -1 : (on != 0), std::memory_order_relaxed); }

namespace {
// Diagnostic: a workgroup that takes 120 KB of LDS (so that no chain workgroup fits next to it on the CU) and sleeps
// until the host raises *release or max_ms have passed — bounded, it cannot hang the device.
__global__ __launch_bounds__(64) void hold_kernel(const unsigned* release, const unsigned max_ms, unsigned* started, unsigned* sink) {
  __shared__ char pad[120 * 1024];
  pad[threadIdx.x * 64] = (char)threadIdx.x;
  if (started && threadIdx.x == 0) __hip_atomic_fetch_add(started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t lim = (uint64_t)max_ms * 100000ull;                       // 100 MHz counter
  while (__hip_atomic_load(release, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u &&
         __builtin_amdgcn_s_memrealtime() - t0 < lim)
    __builtin_amdgcn_s_sleep(100);
  if (sink && pad[threadIdx.x * 64] == 123) *sink = 1u;                    // keeps the LDS allocation alive
}
}  // namespace

extern "C" int esr_debug_hold_cus(int32_t n_workgroups, const uint32_t* release, uint32_t max_ms, uint32_t* started, esr_stream_t stream) {
  if (n_workgroups <= 0 || !release || max_ms == 0 || max_ms > 10000) {
    esr_set_error("esr_debug_hold_cus: invalid arguments (max_ms in 1..10000)");
    return ESR_ERR_INVALID;
  }
  hipLaunchKernelGGL(hold_kernel, dim3(n_workgroups), dim3(64), 0, (hipStream_t)stream, (const unsigned*)release, max_ms, (unsigned*)started, (unsigned*)nullptr);
  return esr_check_launch("hold_kernel");
}

extern "C" int esr_rdb_check_abort(void) {
  unsigned* w = abort_word(esr_bookkeeping_device());      // the CURRENT device's word: another device's abort is not this caller's
  if (!w) return 0;
  const unsigned v = __atomic_exchange_n(w, 0u, __ATOMIC_RELAXED);
  return v != 0u;
}

extern "C" size_t esr_rdb_weight_stream_bytes(int32_t dtype) {
  return dtype == ESR_F16 ? (size_t)Cfg<_Float16>::STREAM_BYTES : (size_t)Cfg<float>::STREAM_BYTES;
}

// Tile height of a launch: 16 rows (4 per wave) whenever that gives the GPU enough tiles; the training forward /
// backward of small crops (the reference trains on batches of 16 32x32 LR crops = 32 such tiles for 256 CUs) and the inference of small inputs (one 128x128 LR tile: 32 tiles) run
// the 8- or 4-row builds when those still fit one round of workgroups.
// A training forward and its backward get the same answer (same B, H, W): the mask records depend on it.
// ESR_RDB_ROWS = 4 | 2 | 1 forces one (measurement).
static int rows_per_wave(const esr_rdb_chain* p, int cus) {
  // (inference: the short-tile builds exist for fp16 without noise layers; bands, fp32 and the noisy form keep 16 rows)
  if (p->band_rows != 0 || (p->mode == 0 && (p->dtype != ESR_F16 || p->noise_mode != ESR_NOISE_OFF))) return 4;
  const char* const env = getenv("ESR_RDB_ROWS");
  const int ev = env ? atoi(env) : 0, forced = (ev == 1 || ev == 2 || ev == 4) ? ev : 0;
  const int tx = (p->W + TW - 1) / TW;
  auto tiles_per_image = [&](int r) { return ((p->H + 4 * r - 1) / (4 * r)) * tx; };
  if (forced && tiles_per_image(forced) <= cus) return forced;
  // the smallest tile whose launch is still ONE round of workgroups (tools/sweep_rows.py, 128x128 LR, ms per forward
  // with 16- / 8- / 4-row tiles: batch 2: 3.27 / 2.36 / 2.11, batch 4: 3.51 / 2.79 / 4.16, batch 8: 4.46 / 5.31 / 8.13)
  for (int r = 1; r < 4; r <<= 1)
    if ((int64_t)p->B * tiles_per_image(r) <= cus) return r;
  return 4;
}

// sized for the smallest tile (4 rows) any build uses
extern "C" size_t esr_rdb_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t tiles = (size_t)B * ((H + 3) / 4) * ((W + TW - 1) / TW);
  return (WS_HDR + tiles) * sizeof(uint32_t);
}

// LeakyReLU masks of one block: 4 slices x 16 bits per pixel position of a tile = 512 bytes per tile row, whole tiles:
// the 16-row build needs the most (its last tile row is padded to 16 rows)
extern "C" size_t esr_rdb_mask_bytes(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * ((H + 15) / 16) * ((W + TW - 1) / TW) * 8192;
}

extern "C" int esr_rdb_max_tiles_per_image(void) { return num_cus_dev(); }

// The chain kernels reach every channel group of an image through ONE buffer descriptor at the image base (img_view:
// num_records 2^31 - 1) with 32-bit offsets, group * (int)group_stride + the offset inside the plane; a pixel past the
// image is dropped by an offset of 2^31.  So the first ng groups of an image must end below 2^31 bytes from its base:
// beyond that the range check drops the stores and answers the loads with 0 — no fault, a wrong result.
static bool chain_view_ok(const char* name, int blk, const esr_g32& v, int ng, int H) {
  if (!v.ptr) return true;
  if (v.wp > 0 && v.group_stride >= 0 && esr_g32_image_bytes(v, H, ng) < ESR_OFFSET_LIMIT) return true;
  esr_set_error("esr_rdb_chain: %s%s of block %d spans %lld bytes from the base of an image over its %d groups (group_stride %lld, "
                "wp %d): the chain kernels address one image with 32-bit offsets (limit 2^31 bytes)", name, blk < 0 ? " (chain)" : "",
                blk, (long long)esr_g32_image_bytes(v, H, ng), ng, (long long)v.group_stride, v.wp);
  return false;
}
extern "C" int esr_rdb_chain_check(const esr_rdb_chain* p, const esr_rdb_block* blocks_host) {
  if (!p || p->H <= 0 || p->n_blocks < 0) {
    esr_set_error("esr_rdb_chain_check: invalid arguments");
    return ESR_ERR_INVALID;
  }
  const int g32 = p->dtype == ESR_F16 ? 2 : 4;          // groups of 32 channels
  if (p->mode == 0 && !chain_view_ok("dense", -1, p->dense, 4 * g32, p->H)) return ESR_ERR_UNSUPPORTED;
  for (int k = 0; blocks_host && k < p->n_blocks; ++k) {
    const esr_rdb_block& b = blocks_host[k];
    if (!chain_view_ok("x_in", k, b.x_in, 2 * g32, p->H) || !chain_view_ok("x_out", k, b.x_out, 2 * g32, p->H) ||
        !chain_view_ok("res2", k, b.res2, 2 * g32, p->H)) return ESR_ERR_UNSUPPORTED;
    if (p->mode != 0 && !chain_view_ok("dense", k, b.dense, 4 * g32, p->H)) return ESR_ERR_UNSUPPORTED;
    if (p->mode == 2 && (!chain_view_ok("aux", k, b.aux, g32, p->H) || !chain_view_ok("out_a", k, b.out_a, 2 * g32, p->H)))
      return ESR_ERR_UNSUPPORTED;
  }
  return ESR_OK;
}

namespace {
// ChainFollow (api.hip, follower weight gradients): `after_clear` is recorded on the stream between the clearing of the
// workspace and the kernel launch — what polls the launch's flags from another stream waits for it, not for the launch;
// the launch's tile grid and the CUs it leaves free come back.
struct ChainFollow { hipEvent_t after_clear; int tiles_x, tiles_y, rows, grid, cus; };
int chain_launch(const esr_rdb_chain* p, esr_stream_t stream, const char* who, int want_mode, ChainFollow* fol = nullptr) {
  if (!p || !p->blocks || p->n_blocks <= 0 || !p->workspace || p->B <= 0 || p->H <= 0 || p->W <= 0 ||
      (p->mode == 0 && !p->dense.ptr)) {
    esr_set_error("%s: invalid arguments", who);
    return ESR_ERR_INVALID;
  }
  if ((want_mode == 2) != (p->mode == 2) || p->mode < 0 || p->mode > 2) {
    esr_set_error("%s: esr_rdb_chain.mode %d (esr_rdb_forward: 0 / 1, esr_rdb_backward: 2)", who, p->mode);
    return ESR_ERR_INVALID;
  }
  if (p->mode != 0 && p->dtype != ESR_F16) {
    esr_set_error("%s: the training forward / backward chains are fp16 (fp32 training runs the per-conv launches)", who);
    return ESR_ERR_UNSUPPORTED;
  }
  // what this side can see of the views (the block table is device memory: esr_rdb_chain_check on its host copy)
  if (const int rc = esr_rdb_chain_check(p, nullptr)) return rc;
  if (esr_rdb_check_abort()) {
    esr_set_error("%s: an earlier fused-chain launch aborted (a tile waited > 1 s for its neighbours: CUs held by other work?) — its results are invalid", who);
    return ESR_ERR_LAUNCH;
  }
  if (p->noise_mode != ESR_NOISE_OFF && p->noise_mode != ESR_NOISE_PHILOX) {
    esr_set_error("%s: noise_mode must be OFF or PHILOX (explicit z: use the per-conv path)", who);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->band_rows != 0) {
    // row bands: B bands of band_rows + 2 * band_margin rows each (include/esrgan_hip.h)
    if (p->mode != 0 || p->noise_mode != ESR_NOISE_OFF) {
      esr_set_error("%s: row bands are for the inference forward without noise", who);
      return ESR_ERR_UNSUPPORTED;
    }
    if (p->band_rows < 0 || p->band_margin < 5 * p->n_blocks || p->H != p->band_rows + 2 * p->band_margin || p->img_H <= 0 ||
        (int64_t)(p->B - 1) * p->band_rows >= p->img_H) {
      esr_set_error("%s: band geometry: H %d must be band_rows %d + 2 * band_margin %d, band_margin >= 5 * n_blocks (%d), "
                    "and every one of the %d bands must own a row of the %d-row image", who, p->H, p->band_rows, p->band_margin,
                    5 * p->n_blocks, p->B, p->img_H);
      return ESR_ERR_INVALID;
    }
  }
  const int cus = num_cus_dev();
  const int rows = rows_per_wave(p, cus);
  const int tiles_x = (p->W + TW - 1) / TW, tiles_y = (p->H + 4 * rows - 1) / (4 * rows);
  const int tpi = tiles_x * tiles_y, ntiles = tpi * p->B;
  if (tpi > cus) {
    esr_set_error("%s: %d tiles per image > %d CUs (all tiles of an image must be co-resident)", who, tpi, cus);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->workspace_bytes < esr_rdb_workspace_bytes(p->B, p->H, p->W)) {
    esr_set_error("%s: workspace too small", who);
    return ESR_ERR_INVALID;
  }
  const int gpb = p->dtype == ESR_F16 ? 2 : 4;
  if (p->mode == 0 && p->dense.ngroups < 4 * gpb) { esr_set_error("%s: dense scratch needs 128 channels", who); return ESR_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  const int grid = ntiles < cus ? ntiles : cus;
  unsigned* const ha = abort_word_dev(esr_bookkeeping_device());
  chain_order_before_launch(st, grid, cus);
  // flags / ticket / abort word restart at zero on every call (a memset node under graph capture); behind the
  // ordering wait, so that a workspace shared by launches on two streams is not cleared under the running one
  if (hipMemsetAsync(p->workspace, 0, esr_rdb_workspace_bytes(p->B, p->H, p->W), st) != hipSuccess) {
    esr_set_error("%s: hipMemsetAsync failed", who);
    return ESR_ERR_LAUNCH;
  }
  if (fol) {
    fol->tiles_x = tiles_x; fol->tiles_y = tiles_y; fol->rows = rows; fol->grid = grid; fol->cus = cus;
    if (fol->after_clear && hipEventRecord(fol->after_clear, st) != hipSuccess) {
      esr_set_error("%s: hipEventRecord failed", who);
      return ESR_ERR_LAUNCH;
    }
  }
  // fp16 launches run the instantiations without trace stamps unless the launch asks for a trace; the fp16 inference
  // chain of a shape that is a whole number of 16x32 tiles runs the instantiation without ragged-tile handling
  const bool traced = p->trace != nullptr && p->dtype == ESR_F16;
  const bool regular = p->mode == 0 && p->dtype == ESR_F16 && p->band_rows == 0 && p->noise_mode == ESR_NOISE_OFF && rows == 4 &&
                       !traced && p->H % (4 * rows) == 0 && p->W % TW == 0 && !force_general();
  g_last_variant.store((regular ? ESR_CHAIN_VARIANT_REGULAR : 0) | (traced ? ESR_CHAIN_VARIANT_TRACED : 0) | (rows << 8), std::memory_order_relaxed);
  auto dispatch = [&]() -> int {
    if (p->band_rows != 0) {
      if (p->dtype != ESR_F16 && p->dtype != ESR_F32) { esr_set_error("%s: bad dtype %d", who, p->dtype); return ESR_ERR_INVALID; }
      return (traced ? esr_rdb_launch_fwd_traced : esr_rdb_launch_band)(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    }
    if (p->mode == 1)
      return (traced ? (rows == 4 ? esr_rdb_launch_train_traced : rows == 2 ? esr_rdb_launch_train_r2_traced : esr_rdb_launch_train_r1_traced)
                     : (rows == 4 ? esr_rdb_launch_train : rows == 2 ? esr_rdb_launch_train_r2 : esr_rdb_launch_train_r1))(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (p->mode == 2)
      return (traced ? (rows == 4 ? esr_rdb_launch_bwd_traced : rows == 2 ? esr_rdb_launch_bwd_r2_traced : esr_rdb_launch_bwd_r1_traced)
                     : (rows == 4 ? esr_rdb_launch_bwd : rows == 2 ? esr_rdb_launch_bwd_r2 : esr_rdb_launch_bwd_r1))(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (p->dtype != ESR_F16 && p->dtype != ESR_F32) { esr_set_error("%s: bad dtype %d", who, p->dtype); return ESR_ERR_INVALID; }
    // inference with the fused Philox noise layers (a train-mode module under no_grad): its own instantiations
    if (p->noise_mode != ESR_NOISE_OFF) return (traced ? esr_rdb_launch_fwd_traced : esr_rdb_launch_noisy)(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (rows != 4)
      return (traced ? (rows == 2 ? esr_rdb_launch_fwd_r2_traced : esr_rdb_launch_fwd_r1_traced)
                     : (rows == 2 ? esr_rdb_launch_fwd_r2 : esr_rdb_launch_fwd_r1))(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (coop_launch()) {
      // ESR_RDB_COOP=1: the runtime checks the grid against the occupancy query and refuses a grid that cannot be
      // co-resident (a plain launch of the same grid has the same residency, MI355X_MICROARCH.md; the check costs
      // ~17 us per launch)
      esr_rdb_chain arg = *p;
      int a1 = ntiles, a2 = tiles_x, a3 = tiles_y;
      unsigned* a4 = ha;
      void* args[] = {&arg, &a1, &a2, &a3, &a4};
      const void* fn = p->dtype != ESR_F16 ? (const void*)rdb_chain_kernel<float, 0, false, 0>
                       : traced ? esr_rdb_fwd_traced_fn() : regular ? esr_rdb_fwd_reg_fn() : (const void*)rdb_chain_kernel<_Float16, 0, false, 0, false>;
      if (hipLaunchCooperativeKernel(fn, dim3(grid), dim3(NT), args, 0, st) != hipSuccess) {
        esr_set_error("%s: cooperative launch refused: %s", who, hipGetErrorString(hipGetLastError()));
        return ESR_ERR_LAUNCH;
      }
      return ESR_OK;
    }
    if (traced) return esr_rdb_launch_fwd_traced(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (regular) return esr_rdb_launch_fwd_reg(*p, grid, ntiles, tiles_x, tiles_y, ha, st);
    if (p->dtype == ESR_F16) hipLaunchKernelGGL((rdb_chain_kernel<_Float16, 0, false, 0, false>), dim3(grid), dim3(NT), 0, st, *p, ntiles, tiles_x, tiles_y, ha);
    else hipLaunchKernelGGL((rdb_chain_kernel<float, 0, false, 0>), dim3(grid), dim3(NT), 0, st, *p, ntiles, tiles_x, tiles_y, ha);
    return esr_check_launch("rdb_chain_kernel");
  };
  const int rc = dispatch();
  if (rc == ESR_OK) chain_record_launch(st, grid);
  return rc;
}
}  // namespace

// For esr_graph_launch (api.hip): a captured op list with chain nodes replays them outside chain_launch — the replay as
// a whole is ordered like ONE chain launch that needs every CU (before: wait for chains in flight on other streams;
// after: recorded, so that later chain launches on other streams wait for it).
int esr_chain_graph_before(hipStream_t st) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t pr;
    static int cached[64] = {};
    if (dev >= 0 && dev < 64) {
      if (!cached[dev] && hipGetDeviceProperties(&pr, dev) == hipSuccess) cached[dev] = pr.multiProcessorCount;
      if (cached[dev]) cus = cached[dev];
    }
  }
  chain_order_before_launch(st, cus, cus);
  return cus;
}
void esr_chain_graph_after(hipStream_t st, int cus) { chain_record_launch(st, cus); }

extern "C" int esr_rdb_forward(const esr_rdb_chain* p, esr_stream_t stream) { return chain_launch(p, stream, "esr_rdb_forward", 0); }
extern "C" int esr_rdb_backward(const esr_rdb_chain* p, esr_stream_t stream) { return chain_launch(p, stream, "esr_rdb_backward", 2); }

extern "C" int esr_debug_rdb_wgrad_follow(const esr_rdb_wgrad* p, const uint32_t* flags, int32_t tiles_x, int32_t tiles_y, esr_stream_t stream) {
  return esr_rdb_wgrad_run_follow(p, stream, flags, tiles_x, tiles_y, abort_word_dev(esr_bookkeeping_device()));
}

// esr_run_ops (api.hip): the backward chain with a follower pass of weight gradients on `side` (rdb_wgrad.hip:
// esr_rdb_wgrad_run_follow).  Order on the device: [clear of the chain's flags] -> chain kernel (stream) and, behind the
// clear only, the follower (side): it polls the flags of the launch that runs next to it.
int esr_rdb_backward_with_follower(const esr_rdb_chain* ch, const esr_rdb_wgrad* wg, hipStream_t stream, hipStream_t side, hipEvent_t fork) {
  ChainFollow fol{};
  fol.after_clear = fork;
  int rc = chain_launch(ch, (esr_stream_t)stream, "esr_rdb_backward", 2, &fol);
  if (rc != ESR_OK) return rc;
  if (hipStreamWaitEvent(side, fork, 0) != hipSuccess) { esr_set_error("esr_rdb_backward (follower): hipStreamWaitEvent failed"); return ESR_ERR_LAUNCH; }
  esr_rdb_wgrad w = *wg;
  // the follower keeps to the CUs the chain's grid leaves free (a workgroup of either kernel takes a whole CU's LDS)
  const int spare = fol.cus - fol.grid;
  if (spare < 32) { esr_set_error("esr_rdb_backward (follower): the chain launch leaves %d CUs free (< 32): run the weight gradients behind it", spare); return ESR_ERR_UNSUPPORTED; }
  if (w.max_workgroups <= 0 || w.max_workgroups > spare) w.max_workgroups = spare;
  return esr_rdb_wgrad_run_follow(&w, (esr_stream_t)side, (const uint32_t*)ch->workspace + WS_HDR, fol.tiles_x, fol.tiles_y,
                                  abort_word_dev(esr_bookkeeping_device()));
}

// Fused weight stream of a block = 1 KB fragments gathered from the per-conv packed weights
// (esr_pack_conv_weights order [cout_block][cin_group][kh][kw][lane][16 B]).
namespace {
__global__ void frag_gather_kernel(const esr_frag_gather g, const int lanes_per_piece) {
  const int ppb = 256 / lanes_per_piece;                       // pieces per 256-thread block
  const int64_t f = (int64_t)blockIdx.x * ppb + (int)threadIdx.x / lanes_per_piece;
  if (f >= g.n) return;
  const int lane = (int)threadIdx.x % lanes_per_piece;
  const u32x4 v = *(const u32x4*)((const char*)g.src_base + g.src_off[f] + lane * 16);
  *(u32x4*)((char*)g.dst + f * (lanes_per_piece * 16) + lane * 16) = v;
}
}  // namespace

extern "C" int esr_gather_fragments(const esr_frag_gather* g, esr_stream_t stream) {
  const int pb = g ? (g->piece_bytes ? g->piece_bytes : 1024) : 0;
  if (!g || !g->src_off || !g->dst || g->n <= 0 || pb < 16 || pb > 4096 || (pb & (pb - 1))) {
    esr_set_error("esr_gather_fragments: invalid arguments");
    return ESR_ERR_INVALID;
  }
  const int lpp = pb / 16, ppb = 256 / lpp;
  hipLaunchKernelGGL(frag_gather_kernel, dim3((unsigned)((g->n + ppb - 1) / ppb)), dim3(256), 0, (hipStream_t)stream, *g, lpp);
  return esr_check_launch("frag_gather_kernel");
}
