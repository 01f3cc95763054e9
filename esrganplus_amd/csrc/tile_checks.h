// tile_checks.h — what the tiled end entries (tile_io.hip, tile_x8.hip) refuse before they launch anything.  Every
// checker returns 0, or sets the message — `who` is the entry's own name — and returns the status of the C ABI.  An
// entry runs them in the order its refusals have always had; TILE_TRY returns the first that fails.
#pragma once
#include "tile_ends.h"

namespace {

#define TILE_TRY(check) do { if (const int rc_ = (check)) return rc_; } while (0)

// The first block: `ok` is the op's own fields (its struct, image or table pointer, sizes), the rest is every op's.
inline int chk_args(const char* who, bool ok, int to_g32, const esr_g32* g32, const float* slots_nchw, int C, int dtype) {
  if (ok && (to_g32 ? g32->ptr != nullptr : slots_nchw != nullptr) && C > 0 && (dtype == ESR_F16 || dtype == ESR_F32)) return 0;
  esr_set_error("%s: invalid arguments", who);
  return ESR_ERR_INVALID;
}

// per_image: scale must divide the op's H and W (the table ops have none: their items hold LR sizes)
inline int chk_tile_pad_scale(const char* who, int tile, int pad, int scale, bool per_image, int H, int W) {
  if (tile >= 1 && pad >= 0 && (scale == 1 || scale == 4) && !(per_image && (H % scale || W % scale))) return 0;
  esr_set_error("%s: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4%s)", who, tile, pad, scale, per_image ? ", dividing H and W" : "");
  return ESR_ERR_INVALID;
}

inline int chk_channels(const char* who, int C) {
  if (C <= 8) return 0;
  esr_set_error("%s: C = %d does not fit one fp32 channel group", who, C);
  return ESR_ERR_UNSUPPORTED;
}

inline int chk_channels_8bit(const char* who, int C, bool only3) {
  if (C == 3 || (C == 1 && !only3)) return 0;
  esr_set_error("%s: C = %d: 8-bit images have %s channels", who, C, only3 ? "3" : "1 or 3");
  return ESR_ERR_UNSUPPORTED;
}

inline int chk_side_scale(const char* who, int to_g32, int scale) {
  if (scale == (to_g32 ? 1 : 4)) return 0;
  esr_set_error("%s: the gather runs at scale 1 and the stitch at scale 4, got %d", who, scale);
  return ESR_ERR_UNSUPPORTED;
}

inline int chk_k_range(const char* who, int k_begin, int k_count) {
  if (x8_range_error(k_begin, k_count, 0, 0) != 1) return 0;
  esr_set_error("%s: slots [%d, %d + %d) of 8", who, k_begin, k_begin, k_count);
  return ESR_ERR_INVALID;
}

inline int chk_k_square(const char* who, int k_begin, int k_count, int th, int tw) {
  if (x8_range_error(k_begin, k_count, th, tw) != 2) return 0;
  esr_set_error("%s: a range across k = 4 needs square windows, got %d x %d (the transposed slots are %d x %d)", who, th, tw, tw, th);
  return ESR_ERR_INVALID;
}

// The per-image block: the geometry of the image (H x W of this op's side) and the tile range inside it.
struct TileImageGeom { int hl, wl, th, tw, nx, ntiles; };
inline int chk_per_image(const char* who, int H, int W, int tile, int pad, int scale, int t_begin, int t_count, TileImageGeom* g) {
  g->hl = H / scale, g->wl = W / scale;
  g->th = tile_window(g->hl, tile, pad), g->tw = tile_window(g->wl, tile, pad);
  g->nx = tile_count(g->wl, tile);
  const int64_t ntiles = (int64_t)tile_count(g->hl, tile) * g->nx;
  if (ntiles > (1 << 30)) {
    esr_set_error("%s: %lld tiles are more than one image may have", who, (long long)ntiles);
    return ESR_ERR_UNSUPPORTED;
  }
  g->ntiles = (int)ntiles;
  if (t_begin < 0 || t_begin >= ntiles || t_count < 1) {
    esr_set_error("%s: tiles [%d, %d + %d) of %lld", who, t_begin, t_begin, t_count, (long long)ntiles);
    return ESR_ERR_INVALID;
  }
  return 0;
}

// The table block: the window shape every item has, the count, the table's alignment.
inline int chk_window(const char* who, int th, int tw, int tile, int pad) {
  const int64_t win = (int64_t)tile + 2 * (int64_t)pad;
  if (th <= win && tw <= win) return 0;
  esr_set_error("%s: a %d x %d window is larger than tile + 2 pad = %lld", who, th, tw, (long long)win);
  return ESR_ERR_INVALID;
}

inline int chk_count(const char* who, const char* what, int n) {
  if (n >= 1) return 0;
  esr_set_error("%s: %s = %d (>= 1)", who, what, n);
  return ESR_ERR_INVALID;
}

inline int chk_items(const char* who, const void* items) {
  if (!((uintptr_t)items & 7)) return 0;
  esr_set_error("%s: the item table needs 8-byte alignment", who);
  return ESR_ERR_INVALID;
}

// grid.z: `what` names the product that n is
inline int chk_slots(const char* who, const char* what, int64_t n) {
  if (n <= 65535) return 0;
  esr_set_error("%s: %s = %lld slots are too many for one launch", who, what, (long long)n);
  return ESR_ERR_UNSUPPORTED;
}

// grid.y of the gather (rows of th per workgroup) and of the stitch (of the largest owned rectangle, oh LR rows)
inline int chk_window_rows(const char* who, int th, int rows) {
  if ((th + rows - 1) / rows <= 65535) return 0;
  esr_set_error("%s: a window of %d rows is too tall for one launch", who, th);
  return ESR_ERR_UNSUPPORTED;
}

inline int chk_tile_rows(const char* who, int oh, unsigned grid_y) {
  if (grid_y <= 65535) return 0;
  esr_set_error("%s: tiles of %d rows are too tall for one launch", who, oh);
  return ESR_ERR_UNSUPPORTED;
}

// The gather's view: rows of `need` logical pixels and the halo.  slots: " 's slots" for the x8 ops, whose turned slots are tw x th.
inline int chk_g32(const char* who, const esr_g32& g32, int need, int th, int tw, const char* slots) {
  if (g32.wp >= need + 2 && g32.ngroups >= 1) return 0;
  esr_set_error("%s: the G32 view (wp = %d) is narrower than the %d x %d window%s", who, g32.wp, th, tw, slots);
  return ESR_ERR_INVALID;
}

// The stitch's 16-byte accesses: `what` names the pointers the entry can see (and those it cannot)
inline int chk_aligned(const char* who, uintptr_t bits, const char* what) {
  if (!(bits & 15)) return 0;
  esr_set_error("%s: the stitch needs 16-byte aligned %s", who, what);
  return ESR_ERR_INVALID;
}

}  // namespace
