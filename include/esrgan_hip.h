/* esrgan_hip.h — C ABI of libesrgan_hip.so (MI355X / gfx950 only).
 *
 * The reference (ncarraz/ESRGANplus) has no FFI layer: its hot path is expressed as stock
 * torch.nn modules that dispatch to cuDNN/cuBLAS.  This header is the boundary a maintainer binds
 * instead (INTEGRATION.md shows the ctypes stub): every entry point replaces the library call made
 * by the cited reference line.  Plain C types only; all buffers are caller-owned device memory;
 * every launch goes to the caller's hipStream_t; the library never allocates, never synchronises
 * and never changes the current device (graph-capture safe).  Every entry returns 0 on success
 * or a negative esr_status; esr_last_error() gives a per-thread message.
 *
 * ---- activation layout "G32" -----------------------------------------------------------------
 * A tensor of C channels is stored as ngroups = ceil(C / cpg) planes of 32-byte channel groups
 * (cpg = 16 for fp16, 8 for fp32):   [B][ngroups][Hp][Wp][32 bytes]
 * Logical pixel (y,x) lives at padded coordinates (y+1, x+1); row 0 / column 0 and everything at
 * or beyond (H+1, W+1) is ZERO and is never written by any kernel (this is the conv zero padding
 * of block.py:55-58,137 — the halo is physical, so kernels need no bounds checks on loads).
 * Hp >= roundup(H,32)+6, Wp >= roundup(W,32)+2 (see esr_g32_dims).
 */
#ifndef ESRGAN_HIP_H
#define ESRGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* esr_stream_t; /* hipStream_t */

enum esr_status {
  ESR_OK = 0,
  ESR_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
  ESR_ERR_LAUNCH = -2,      /* HIP launch error (message in esr_last_error) */
  ESR_ERR_UNSUPPORTED = -3
};

enum esr_dtype { ESR_F16 = 0, ESR_F32 = 1 };
enum esr_act { ESR_ACT_NONE = 0, ESR_ACT_LRELU = 1 /* slope 0.2, block.py:12 */, ESR_ACT_RELU = 2 };
enum esr_noise { ESR_NOISE_OFF = 0, ESR_NOISE_PHILOX = 1, ESR_NOISE_EXPLICIT = 2 };

/* One G32 tensor view (pointer already offset to the first channel group of interest).
 * Address widths (DESIGN.md "Address widths" has the table).  Every kernel forms b * batch_stride in 64 bits, so
 * batch_stride itself is free except where noted.  With plane(H) = esr_g32_dims(H).Hp * wp * 32 bytes and
 * image(n, H) = (n - 1) * group_stride + plane(H) — the first n groups of one batch entry, from its base — the
 * launchers refuse, with ESR_ERR_UNSUPPORTED and a message naming the limit, before anything runs:
 *   esr_conv_forward             `in`: plane(input rows) < 2^31 (32-bit staging map inside a plane).  Every other view
 *                                of esr_conv is addressed in 64 bits: no limit.  With ksplit > 1 (packed tiles) also
 *                                (images of a tile - 1) * in.batch_stride + plane < 2^31.
 *   esr_conv_wgrad[_multi] fp16  `g` and `in`: image(view.ngroups, rows) < 2^31; packed tiles (maps of <= 16 columns)
 *                                also + (images of a tile - 1) * batch_stride.  The fp32 kernel has no limit.
 *   esr_rdb_forward / _backward  every view: group_stride >= 0 and image(64 / 128 / 32 channels' groups, H) < 2^31
 *                                (one buffer descriptor per image, 32-bit offsets; beyond it the hardware range check
 *                                drops stores and answers loads with 0 — a wrong result, no fault).  The launcher
 *                                checks esr_rdb_chain.dense; the block table is DEVICE memory, so the caller runs
 *                                esr_rdb_chain_check on its host copy (engine.py does before every upload).
 *   esr_rdb_wgrad_run            `in` (12 groups) and `q` (14): image < 2^31 (offsets formed in int), and
 *                                image <= batch_stride <= 2^32 - 16 (it is the descriptor's size).  Device table again: esr_rdb_wgrad_check on the host copy.
 * The BatchNorm / pooling / pixel-shuffle kernels, esr_convert_layout and the image ends (dihedral, tile ops) add
 * 64-bit products only: no limit. */
typedef struct esr_g32 {
  void* ptr;
  int64_t batch_stride; /* bytes */
  int64_t group_stride; /* bytes */
  int32_t wp;           /* row pitch in pixels (32-byte units) */
  int32_t ngroups;      /* groups addressable through this view */
} esr_g32;

/* Fused convolution.  Replaces nn.Conv2d + LeakyReLU/ReLU + the elementwise tail the reference
 * runs as separate kernels (conv_block block.py:125-151; RDB tail block.py:263,266,268; RRDB
 * tail block.py:291 / test_image/block.py:256; ShortcutBlock block.py:84-86; nearest upsample
 * block.py:315-322 folded into the load).  Epilogue, per output element, in this order:
 *     v = acc + bias;  v = act(v);  [aux_out = v];  v += acc_1x1;
 *     v = v*alpha + res1;  v *= (1 + sigma*z1);  v = v*beta + res2;  v *= (1 + sigma*z2);  out = v
 * (each step skipped when its operand is absent, except alpha: without res1, alpha != 1 still
 * scales, v = v*alpha, while beta without res2 is ignored; a residual / z view with fewer channel
 * groups than the output contributes zero to the channels it does not cover).  Backward chains add
 *     out2 = v * act'(mask)      for cout blocks >= mask_cb_begin (act' = 1 if mask>0 else 0.2 / 0)
 *     out3 = v * gamma * (1 + sigma*z3)
 * which is how dgrad launches also apply the LeakyReLU / GaussianNoise / residual-scale backward
 * of block.py:262-268,291 without extra elementwise passes.                                    */
typedef struct esr_conv {
  int32_t dtype;       /* esr_dtype: storage type of every G32 tensor here (accumulate fp32) */
  int32_t ks;          /* 1, 3 or 4 (2: upsample == 3) */
  int32_t stride;      /* 1, or 2 (ks==4) */
  int32_t upsample;    /* 1: input is nearest-x2 upsampled on load (ks==3 only);
                          2: TRANSPOSED 4x4/stride-2 conv (adjoint of ks==4,stride==2): the input is at
                             half the output resolution; weights packed with transpose_flip=2;
                          3: the same function as 1 in its 4-phase 2x2 ("sub-pixel") form, ks == 2, weights
                             packed with esr_pack.ups_fwd (2.25x fewer MACs; results differ from 1 only by the
                             rounding of the pre-summed taps) */
  int32_t B, H, W;     /* OUTPUT logical size */
  int32_t cin_groups;  /* K loop length: input channel groups read from `in` */
  int32_t cout_blocks; /* ceil(Cout/32) */
  esr_g32 in;
  esr_g32 out;         /* out.ngroups bounds the groups actually stored */
  const void* w;       /* packed by esr_pack_conv_weights */
  const float* bias;   /* fp32 [cout_blocks*32] or NULL */
  const void* w1x1;    /* packed 1x1 (bias-free, block.py:153-154,263) or NULL */
  int32_t n1x1_groups; /* input groups the 1x1 reads (prefix of `in`) */
  int32_t act;         /* esr_act */
  esr_g32 aux_out;     /* ptr NULL = off */
  float alpha; esr_g32 res1;
  float beta;  esr_g32 res2;
  int32_t noise_mode;  /* esr_noise */
  float sigma;         /* 0.1, block.py:111 */
  uint64_t seed;       /* philox key */
  uint32_t layer1, layer2; /* philox stream ids of z1 / z2; layer==0xFFFFFFFF = that noise off */
  esr_g32 z1, z2;      /* explicit z (G32, same dtype); ptr NULL = off */
  esr_g32 mask;        /* dgrad: saved activation whose sign gives act' (ptr NULL = off) */
  esr_g32 out2;        /* dgrad: masked output */
  int32_t nchw_out_c;  /* >0: ALSO store the first nchw_out_c channels as fp32 NCHW */
  float* nchw_out;     /* [B][nchw_out_c][H][W] */
  int32_t debug_flags; /* measurement only: 1 = skip epilogue, 2 = skip MFMAs, 4 = skip activation DMA;
                          test hooks (results valid): 64 = force the plain K loop, 128 = force the hand-pipelined
                          K loop of the 32-cout 3x3 conv (default: pipelined up to 256 tiles), 256 = keep 16-row
                          tiles (default: fp16 3x3/s1 convs whose 16-row grid x cout blocks is <= 128 / <= 384
                          workgroups, or whose map has <= 4 / <= 8 rows, run on 4- / 8-row tiles — same results),
                          512 = refuse the call (ESR_ERR_UNSUPPORTED) unless it runs a PLAIN kernel: an fp16 forward
                          layer that is bias + activation into one output, G32 or NCHW (csrc/conv_plain.h; bits 3..4,
                          the store flavours, keep such a layer on the general kernel — same results with flavour 1) */
  int32_t mask_cb_begin; /* mask/out2 apply to cout blocks >= this one, indexed from it */
  float gamma;          /* third stage (backward chains): out3 = v * gamma * (1 + sigma*z3) */
  uint32_t layer3;      /* philox stream id of z3 (0xFFFFFFFF = no noise on out3) */
  esr_g32 z3;           /* explicit z3 */
  esr_g32 out3;         /* ptr NULL = off */
  int32_t mask_act;     /* esr_act whose derivative the mask selects (LRELU: 1 / 0.2, RELU: 1 / 0) */
  int32_t _pad2;
  const uint64_t* seed_dev; /* non-NULL: the Philox seed is read from DEVICE memory at run time (so a
                               captured graph can be replayed with a fresh seed); overrides `seed` */
  /* ---- round 4: the discriminators' deep 4x4/s2 convs (architecture.py:87-129: features.14 / .20 / .26 — fp16, square
   * maps of 4 / 8 / 16 output columns, plain layer: bias [+ act], one G32 output).  ksplit > 1: several images share a
   * tile and the K loop is split over ksplit workgroups per tile; each writes an fp32 slab of split_ws
   * ([ksplit][B][H][W][cout_blocks * 32] floats) and a finishing launch of the same call adds the slabs up in split
   * order (deterministic), applies bias / act and stores `out`.  stat_sums (optional): that pass also accumulates the
   * BatchNorm statistics of the stored output exactly as ESR_BN_STATS would (sums[grp][c] += x, sums[grp][C + c] +=
   * x^2, groups = stat_groups, C = stat_C; the caller zeroes stat_sums), so the BatchNorm that follows starts at
   * ESR_BN_FIN_APPLY.  ksplit <= 1: off. */
  int32_t ksplit, stat_groups, stat_C, _pad3;
  float* split_ws;
  double* stat_sums;
} esr_conv;

/* Weight packing: OIHW fp32 master (the nn.Parameter the reference keeps, e.g. state-dict key
 * model.1.sub.0.RDB1.conv1.0.weight) -> MFMA A-fragment order
 *   [cout_block][cin_group][kh][kw][lane 0..63][16 bytes].
 * transpose_flip=1 packs the dgrad operand (Cin<->Cout swapped, taps rotated 180 degrees). */
typedef struct esr_pack {
  const float* src;    /* OIHW fp32 */
  void* dst;
  int32_t cout, cin, ks;
  int32_t dtype;
  int32_t transpose_flip; /* 1: dgrad operand (Cin<->Cout, taps rotated 180 deg); 2: Cin<->Cout only
                             (operand of the transposed stride-2 conv, upsample==2);
                             `cout`/`cin` below are still the FORWARD conv's */
  int32_t sum_dst;     /* transpose_flip only: dgrad output channels [sum_dst, sum_dst+sum_count) */
  int32_t sum_src;     /*   additionally receive the weights of forward input channels             */
  int32_t sum_count;   /*   [sum_src, sum_src+sum_count) (x4 = lrelu(a4) + x2, block.py:266)      */
  int32_t ups_dgrad;   /* 1 (with transpose_flip, ks==3): emit the 4x4/stride-2 kernel that is the
                          exact adjoint of nearest-x2-upsample + 3x3 conv (block.py:315-322)       */
  /* gather == 1 (with transpose_flip == 1, ks == 3): this entry fills ONE K range of a larger packed
   * operand — the input-gradient conv of a dense-block channel slice in "gather" form:
   *   g_slice = sum over the later convs k of  conv_k^T[slice] (g_ak)
   * is ONE conv whose K dimension concatenates the gradients g_ak (dense connectivity mirrored), so
   * the slice's gradient is written once instead of being accumulated conv by conv.  The piece
   * maps packed row r -> forward input channel src_co0 + r (r < dst_cout) and packed K index c
   * (c < cout, placed at chunks [dst_chunk0, ...) of dst_nchunks) -> forward output channel c;
   * weights are multiplied by `scale`; src_ks == 1 embeds a 1x1 kernel as the centre tap. */
  int32_t gather, dst_cout, dst_chunk0, dst_nchunks, src_co0, src_ks;
  float scale;
  int32_t ups_fwd;     /* 1 (ks == 3, no transpose_flip): emit the 4-phase 2x2 ("sub-pixel") form of
                          nearest-x2-upsample + 3x3 conv (block.py:315-322), the operand of esr_conv.upsample == 3:
                          output pixel (2y+dy, 2x+dx) only ever sees the 2x2 input pixels (y-1+dy .., x-1+dx ..),
                          each weighted by the SUM of the 3x3 taps that land on it — 16 instead of 36 MACs per
                          4 outputs.  Packed as a 2x2 conv with 4*cout_blocks blocks, phase-major:
                          [phase = 2 dy + dx][cout_block][chunk][2 a + b] */
  int32_t fold_co0;    /* gather pieces (3x3): when > 0, the weights of forward input channels fold_co0 + r are ADDED to
                          those of src_co0 + r — the identity path x4 = lrelu(a4) + x2 (block.py:266) folded into conv5's
                          x2 columns, so that the backward chain needs no residual for g_x2.  0: off */
  int32_t one_t;       /* 1: the transposed 1x1 of a dense block (src = conv1x1.weight [32][64]) as the backward chain
                          consumes it: g_x[64] += W^T g_x2[32]; 2 cout blocks x 2 K chunks of 1 KB, chunk c holding the
                          K order k = 8 h + i <-> g_x2 channel 16 h + 8 c + i (the lane's packed epilogue registers
                          are the B fragments).  fp16 only */
} esr_pack;

/* All weight packs of a network in ONE launch: `table` is a DEVICE array of n esr_pack entries,
 * `piece_begin` a DEVICE int64[n+1] prefix sum of their 16-byte piece counts. */
typedef struct esr_pack_batch {
  const esr_pack* table;
  const int64_t* piece_begin;
  int32_t n, _pad;
  int64_t total_pieces;
} esr_pack_batch;
int64_t esr_pack_pieces(const esr_pack* p);   /* host helper: 16-byte pieces one entry produces */

size_t esr_packed_weight_bytes(int32_t cout, int32_t cin, int32_t ks, int32_t dtype);

/* NCHW fp32 <-> G32 (the tensors crossing the nn.Module boundary are NCHW fp32:
 * test_image/test.py:31-37, SRRaGAN_model.py:103-111). */
typedef struct esr_layout {
  int32_t dtype;
  int32_t to_g32;      /* 1: NCHW -> G32 (pads channels with zeros), 0: G32 -> NCHW */
  int32_t B, C, H, W;
  float* nchw;
  esr_g32 g32;
  int32_t use_affine;  /* to_g32 only, C <= 4: v = (v - mean_c[c]) * inv_std_c[c]  (VGG input
                          norm, architecture.py:304-305) */
  float mean_c[4];
  float inv_std_c[4];
  int32_t accumulate;  /* to_g32 == 0 only: nchw += value instead of nchw = value (round 4: the input gradients of netF
                          and netD land in the buffer that already holds the pixel loss's, SRRaGAN_model.py:124-140:
                          dL/d fake_H = d l_pix + d l_fea + d l_gan without add launches) */
  int32_t _pad;
} esr_layout;

/* Geometric self-ensemble ends (the reference's `SRModel.test_x8`, codes/models/SR_model.py:82-120: eight flip /
 * transpose copies of the LR image, eight forwards, each inverse applied to its SR output, mean).  Transform k = 0..7 in
 * the reference's list order, v = k & 1 (flip along W), h = k & 2 (flip along H), t = k & 4 (transpose, applied last):
 *   ys(i) = h ? H-1-i : i,   xs(j) = v ? W-1-j : j                      (H x W = the NCHW side)
 *   slot_k[y][x] = src[ys(y)][xs(x)]   (k < 4, an H x W image)      slot_k[p][q] = src[ys(q)][xs(p)]   (k >= 4, W x H)
 *   R_k(o)[y][x] = o_k[ys(y)][xs(x)]   (k < 4)                      R_k(o)[y][x] = o_k[xs(x)][ys(y)]   (k >= 4)
 * Slot s (0 <= s < k_count, k = k_begin + s) of image b is batch index s * B + b of the G32 view; a range may contain
 * both k < 4 and k >= 4 only when H == W (else ESR_ERR_INVALID).  One channel group: C <= 16 (fp16) / 8 (fp32), else
 * ESR_ERR_UNSUPPORTED.
 *   to_g32 = 1  import: reads nchw [B][C][H][W] once and writes the logical pixels of every slot of the range (channels
 *               padded with zeros to the group; the halo is never touched).
 *   to_g32 = 0  reduce: acc = accumulate ? nchw : 0;  acc += R_k(o_k) for k ascending (one fp32 add per k);
 *               nchw = acc * scale.  scale = 0.125 on the last range gives the reference's cat(...).mean(0); the result
 *               does not depend on how the eight slots are split into ranges (accumulate chains them, scale = 1 before
 *               the last).  slots_nchw (optional, C <= 8): the slots are read from fp32 NCHW [k_count * B][C][h][w]
 *               (h x w = H x W for k < 4, W x H for k >= 4) instead of the G32 view — what a conv's nchw_out leaves,
 *               unrounded in either precision; g32 is then unused.                                                  */
typedef struct esr_dihedral {
  int32_t dtype, to_g32;
  int32_t B, C, H, W;
  float* nchw;
  esr_g32 g32;
  int32_t k_begin, k_count;
  int32_t accumulate;
  float scale;
  const float* slots_nchw;
} esr_dihedral;

/* Tiled inference ends: the gather cuts fixed-size windows out of an NCHW image into G32 slots, the stitch copies every
 * tile's owned rectangle out of the windows' fp32 NCHW outputs into the caller's image.  Geometry, in LR pixels (Hl x Wl
 * = the LR image: H x W of the gather, H / scale x W / scale of the stitch), parameters tile >= 1 and pad >= 0:
 *   window shape  th = min(tile + 2 pad, Hl),  tw = min(tile + 2 pad, Wl)      (one shape for every tile of the image)
 *   tile grid     ny = ceil(Hl / tile) by nx = ceil(Wl / tile), row-major, t = i nx + j
 *   tile (i, j)   owns rows [i tile, min((i + 1) tile, Hl)); its window starts at wy = clamp(i tile - pad, 0, Hl - th);
 *                 columns alike (wx from j, Wl, tw)
 * A window always lies inside the image — at the borders it is shifted inward, never zero-filled — so a window edge
 * either is an image edge (the convs' own zero padding is then the whole-image arithmetic) or lies at least `pad` pixels
 * from every owned pixel.  On the HR side every offset is multiplied by `scale`: the owned pixels of tile (i, j) are
 * copied from offset scale (i tile - wy), scale (j tile - wx) of its window's output.  With pad >= 15 nb + 4 (15 per
 * RRDB, 1 each for fea_conv and LR_conv, 1.25 for the four HR-side convs) the tiled RRDBNet forward is mathematically
 * the whole-image forward; smaller pads approximate it.  The kernels derive all of this from tile, pad and the tile
 * index; there is no table.
 * Slot s (0 <= s < t_count) of image b is batch index s * B + b.  C <= 8, else ESR_ERR_UNSUPPORTED.
 *   to_g32 = 1, scale = 1  gather: slot s holds the th x tw window of tile min(t_begin + s, ny nx - 1) of nchw
 *               [B][C][H][W], converted to dtype, as finished 32-byte channel groups at the logical pixels of the G32
 *               view (channels >= C zero, the halo is never touched).  A tail pass repeats the last tile, so that no slot
 *               holds stale data.
 *   to_g32 = 0, scale = 4  stitch: slots_nchw is fp32 [t_count * B][C][4 th][4 tw] (what a conv's nchw_out leaves); the
 *               owned rectangle of every tile t_begin + s < ny nx is copied, bit for bit, into nchw [B][C][H][W] (H, W
 *               multiples of 4; both pointers 16-byte aligned).  Slots beyond the last tile are not read; g32 and dtype's
 *               storage type are unused.                                                                              */
typedef struct esr_tile {
  int32_t dtype, to_g32;
  int32_t B, C, H, W;      /* the full image on this op's side: LR for the gather, HR for the stitch */
  int32_t tile, pad;       /* LR pixels */
  int32_t scale;           /* 1: gather, 4: stitch */
  int32_t t_begin, t_count;
  float* nchw;
  esr_g32 g32;
  const float* slots_nchw;
} esr_tile;

/* Tiled x8 self-ensemble ends: esr_tile's windows, each turned the eight ways of esr_dihedral — per WINDOW, pad included,
 * not per image.  Geometry is esr_tile's (window shape th x tw, tile grid ny x nx, inward shift, owned rectangles, LR
 * pixels; H x W = the full image of this op's side); transform k = 0..7 is esr_dihedral's with the window in the place of
 * the image, v = k & 1, h = k & 2, t = k & 4:
 *   ys(i) = h ? n-1-i : i over the window's rows,   xs(j) = v ? m-1-j : j over its columns
 *   gather (n x m = th x tw, win = the window of the tile):
 *     slot_k[y][x] = win[ys(y)][xs(x)]   (k < 4, a th x tw slot)      slot_k[p][q] = win[ys(q)][xs(p)]   (k >= 4, tw x th)
 *   stitch (n x m = 4 th x 4 tw, the window's output; (y, x) window-local HR coordinates):
 *     R_k(o)[y][x] = o_k[ys(y)][xs(x)]   (k < 4)                      R_k(o)[y][x] = o_k[xs(x)][ys(y)]   (k >= 4)
 * Slot k of window s (0 <= s < t_count) of image b is batch index ((k - k_begin) t_count + s) B + b: the transforms
 * outermost, then esr_tile's slot-major windows.  A range may contain both k < 4 and k >= 4 only when th == tw (else
 * ESR_ERR_INVALID): a pass cannot mix th x tw and tw x th slots.  C <= 8 and k_count t_count B <= 65535, else
 * ESR_ERR_UNSUPPORTED.
 *   to_g32 = 1, scale = 1  gather-import: every pixel of the window of tile min(t_begin + s, ny nx - 1) of nchw
 *               [B][C][H][W] is read once and written, converted to dtype, as a finished 32-byte channel group to the
 *               logical pixel of every slot of the range in the G32 view (th x tw for k < 4, tw x th for k >= 4; channels
 *               >= C zero, the halo is never touched).  A tail pass repeats the last tile.
 *   to_g32 = 0, scale = 4  stitch-reduce: slots_nchw is fp32 [k_count * t_count * B][C][4 th][4 tw] (k < 4) or
 *               [...][4 tw][4 th] (k >= 4), what a conv's nchw_out leaves.  For every HR pixel of the owned rectangle of
 *               every tile t_begin + s < ny nx:  acc = accumulate ? nchw : 0;  acc += R_k(o_k) for k ascending (one fp32
 *               add per k);  nchw = acc * mean_scale.  mean_scale = 0.125 on the last range gives the mean; accumulate
 *               chains the ranges (mean_scale = 1 before the last) and the result does not depend on how the eight slots
 *               are split.  Nothing is blended and nothing outside the owned rectangles is written; slots beyond the last
 *               tile are neither read nor written.  H, W multiples of 4, both pointers 16-byte aligned (esr_tile's rule);
 *               g32 and dtype's storage type are unused.                                                             */
typedef struct esr_tile_x8 {
  int32_t dtype, to_g32;
  int32_t B, C, H, W;      /* the full image on this op's side: LR for the gather, HR for the stitch */
  int32_t tile, pad;       /* LR pixels */
  int32_t scale;           /* 1: gather, 4: stitch */
  int32_t t_begin, t_count;
  float* nchw;
  esr_g32 g32;
  const float* slots_nchw;
  int32_t k_begin, k_count;
  int32_t accumulate;
  float mean_scale;
} esr_tile_x8;

/* Tiled inference over an image SET: the windows of many images, of any sizes, share one pass.  Geometry is esr_tile's,
 * per image: slot s (0 <= s < n_slots, = batch index s; there is no B) belongs to tile items[s].t of the image
 * items[s].nchw, whose tile grid ny x nx, inward shift and owned rectangle the kernels derive from that image's H, W and
 * this op's tile, pad — the table holds no geometry.  Every item's window, min(tile + 2 pad, H) x min(tile + 2 pad, W),
 * must be the op's th x tw: a pass holds windows of one shape.  The table lives in DEVICE memory (n_slots entries, read
 * by the launch, so it must stay valid until the launch has run); this entry cannot read it, and whoever fills it
 * guarantees per item: nchw a live fp32 image of C x H x W (gather) / C x 4H x 4W (stitch, 16-byte aligned), H, W >= 1,
 * the window shape above, 0 <= t < ny nx, and for the stitch that no two live items name the same tile of one image.
 * functional.run_rrdbnet_tiled_many builds it from validated sizes.  C <= 8 and n_slots <= 65535, else
 * ESR_ERR_UNSUPPORTED.
 *   to_g32 = 1, scale = 1  gather: slot s holds the th x tw window of its item's tile, converted to dtype, as finished
 *               32-byte channel groups at the logical pixels of the G32 view (channels >= C zero, the halo is never
 *               touched) — esr_tile's arithmetic and writes.  `live` is not read: a filler slot is filled like any other,
 *               so that no slot holds stale data.
 *   to_g32 = 0, scale = 4  stitch: slots_nchw is fp32 [n_slots][C][4 th][4 tw] (16-byte aligned); for every item with
 *               live != 0 the owned rectangle of its tile is copied, bit for bit, into ITS image.  Slots with live == 0
 *               are neither read nor written; g32 and dtype's storage type are unused.                                 */
typedef struct esr_tile_item {   /* one slot of one pass; lives in DEVICE memory */
  float*  nchw;                  /* gather: the LR image [C][H][W]; stitch: the HR result [C][4H][4W] */
  int32_t H, W;                  /* LR size of that image (on both sides) */
  int32_t t;                     /* tile index in that image's own ny x nx grid */
  int32_t live;                  /* 0: a filler slot — the gather fills it, the stitch skips it */
} esr_tile_item;

typedef struct esr_tile_many {
  int32_t dtype, to_g32;
  int32_t C;
  int32_t tile, pad;             /* LR pixels */
  int32_t scale;                 /* 1: gather, 4: stitch */
  int32_t th, tw;                /* the window shape every item has */
  int32_t n_slots;               /* batch entries = slots, one image per slot */
  const esr_tile_item* items;    /* n_slots entries, device memory */
  esr_g32 g32;
  const float* slots_nchw;
} esr_tile_many;

/* esr_tile_many with 8-bit ends: the gather reads 8-bit HWC images, the stitch writes them; between the two sits the same
 * plan.  Slots, the device table, its guarantees, th x tw, tile, pad, n_slots and the limits are esr_tile_many's; an item
 * has esr_tile_item's layout with a byte pointer.  C is 1 or 3, else ESR_ERR_UNSUPPORTED.  With (y, x) a logical pixel of
 * slot s, (wy, wx) the start of its window, (oy, ox) the start of its owned rectangle, in LR pixels of ITS image of H x W:
 *   to_g32 = 1, scale = 1  gather: hwc is the LR image uint8 [H][W][C].  Channel c of slot pixel (y, x) is
 *                 float32(hwc[((wy + y) W + wx + x) C + m(c)]) / 255.0f,   m(c) = 2 - c when bgr and C == 3, else c,
 *               one correctly rounded float32 division (NOT a multiplication by 1/255, which differs for 126 of the 256
 *               values from the float64 division the reference's scripts round to float32), then converted to dtype and
 *               written as esr_tile_many's gather writes: finished 32-byte channel groups, channels >= C zero, the halo
 *               never touched, filler slots filled like any other.  slot channel 0 is R whatever the order in memory.
 *   to_g32 = 0, scale = 4  stitch: slots_nchw is fp32 [n_slots][C][4 th][4 tw], 16-byte aligned; hwc is the HR result
 *               uint8 [4H][4W][C], 4-byte aligned.  For every item with live != 0 and every HR pixel (Y, X) of its owned
 *               rectangle [4 oy, 4 (oy + on_y)) x [4 ox, 4 (ox + on_x)):
 *                 hwc[(Y 4W + X) C + m(c)] = uint8(rintf(fminf(fmaxf(v, 0), 1) * 255.0f)),
 *                 v = slots_nchw[s][c][Y - 4 wy][X - 4 wx]
 *               (metrics.hip's quant8(v, 0, 1): the reference's tensor2img rounding, half to even; the result for a
 *               non-finite v is unspecified).  Four HR pixels of a row are written at a time, as C aligned dwords: the byte
 *               offset (Y 4W + 4 x) C is a multiple of 4.  Nothing outside the owned rectangles is written; slots with
 *               live == 0 are neither read nor written; g32 and dtype's storage type are unused.
 * Items live in device memory: this entry cannot check them (pointer alignment included); functional.run_rrdbnet_images
 * builds them from validated sizes and fresh allocations.                                                              */
typedef struct esr_tile_img_item {   /* esr_tile_item's layout; lives in DEVICE memory */
  uint8_t* hwc;                  /* gather: the LR image [H][W][C]; stitch: the HR result [4H][4W][C] */
  int32_t H, W;                  /* LR size of that image (on both sides) */
  int32_t t;                     /* tile index in that image's own ny x nx grid */
  int32_t live;                  /* 0: a filler slot — the gather fills it, the stitch skips it */
} esr_tile_img_item;

typedef struct esr_tile_img {
  int32_t dtype, to_g32;
  int32_t C;                     /* 1 or 3 */
  int32_t tile, pad;             /* LR pixels */
  int32_t scale;                 /* 1: gather, 4: stitch */
  int32_t th, tw;                /* the window shape every item has */
  int32_t n_slots;               /* batch entries = slots, one image per slot */
  const esr_tile_img_item* items;    /* n_slots entries, device memory */
  esr_g32 g32;
  const float* slots_nchw;
  int32_t bgr;                   /* C == 3: the channel order in memory is B, G, R on this op's side (else R, G, B) */
} esr_tile_img;

/* esr_tile_img whose gather makes the LR window itself: every slot's window is cut straight out of the 8-bit HR image
 * through the MATLAB-bicubic tables of the WHOLE image (esr_resample's layout, for (hr_h, 1/4) and (hr_w, 1/4)), so that
 * a generator is scored from ground-truth images alone (LRHR_dataset.py:44-125 with dataroot_LR null: modcrop,
 * imresize_np(HR, 1/4) on the float image, not quantised, not clamped).  x4 only.  Fields, slots, th x tw, tile, pad,
 * n_slots, the limits and the 24-byte table are esr_tile_img's; C is 3, else ESR_ERR_UNSUPPORTED.
 *   to_g32 = 1, scale = 1  gather: an item's pointer names a per-image DESCRIPTOR in device memory (esr_tile_hr_desc,
 *               64 bytes, 8-byte aligned); H, W of the item are the LR size (hr_h / 4, hr_w / 4), t and live as in
 *               esr_tile_img.  A source sample is float32(byte) / 255.0f, one correctly rounded division; slot channel c
 *               reads byte m(c) = 2 - c when bgr, else c, of pixel (Y, X) at hr[(Y pitch + X) 3 + m(c)] — pitch in
 *               PIXELS, so a modcropped view of a larger image needs no copy.  LR pixel (wy + y, wx + x) is the H pass then
 *               the W pass, each an fp32 sum over the taps in ascending order, acc += w * x — the bits of esr_resample_axis
 *               run twice on the float image and of esr_batch_assemble's generated LR.  One workgroup makes one 16 x 16 LR
 *               tile: the H pass of its rows over the source columns its 16 LR columns touch (at most ESR_TILE_HR_SPAN:
 *               15 * 4 + the 17 taps of a x4 table, mirrored taps folding inside) into LDS, the W pass out of it.  Source
 *               rows and columns are clamped into the image and the LDS row whatever the tables hold.  The result is
 *               converted to dtype and written as esr_tile_img's gather writes: finished 32-byte channel groups at the
 *               logical pixels of the G32 view, channels >= 3 zero, the halo never touched, filler slots filled like any
 *               other.
 *   to_g32 = 0, scale = 4  stitch: esr_tile_img's stitch itself (the same kernel): an item's pointer is the uint8 HR
 *               result [4H][4W][3], 4-byte aligned.
 * Items and descriptors live in device memory: this entry cannot check them (pointers, sizes, tables, alignment);
 * functional.run_rrdbnet_hr_images builds them from validated sizes, and keeps the tables referenced until the call's
 * work is queued.                                                                                                      */
#define ESR_TILE_HR_SPAN 77          /* source columns staged per LDS row: 15 * 4 + 17 */
typedef struct esr_tile_hr_desc {    /* one per image; lives in DEVICE memory */
  const uint8_t* hr;                 /* uint8 [>= hr_h][pitch][3] */
  const float* wy; const int32_t* iy;   /* [hr_h / 4][taps_y] weights / source rows */
  const float* wx; const int32_t* ix;   /* [hr_w / 4][taps_x] weights / source columns */
  int32_t pitch;                     /* pixels from one row to the next, >= hr_w */
  int32_t hr_h, hr_w;                /* the modcropped HR size: multiples of 4 */
  int32_t taps_y, taps_x;
  int32_t _pad;
} esr_tile_hr_desc;

typedef struct esr_tile_hr_item {    /* esr_tile_item's layout; lives in DEVICE memory */
  void* ptr;                         /* gather: const esr_tile_hr_desc*; stitch: uint8_t* HR result [4H][4W][3] */
  int32_t H, W;                      /* LR size of that image (on both sides) */
  int32_t t;                         /* tile index in that image's own ny x nx grid */
  int32_t live;                      /* 0: a filler slot — the gather fills it, the stitch skips it */
} esr_tile_hr_item;

typedef struct esr_tile_hr {         /* esr_tile_img's fields */
  int32_t dtype, to_g32;
  int32_t C;                         /* 3 */
  int32_t tile, pad;                 /* LR pixels */
  int32_t scale;                     /* 1: gather, 4: stitch */
  int32_t th, tw;                    /* the window shape every item has */
  int32_t n_slots;                   /* batch entries = slots, one image per slot */
  const esr_tile_hr_item* items;     /* n_slots entries, device memory */
  esr_g32 g32;
  const float* slots_nchw;
  int32_t bgr;                       /* the channel order in memory is B, G, R on this op's side (else R, G, B) */
} esr_tile_hr;

/* The x8 self-ensemble over an image SET: esr_tile_many's table-driven windows, each turned the eight ways of
 * esr_tile_x8, with fp32 NCHW or 8-bit HWC images outside.  Geometry is esr_tile's per image, derived by the kernels from
 * the item's H, W and this op's tile, pad; the table (esr_tile_item / esr_tile_img_item, the same 24 bytes) holds ONE
 * entry per WINDOW p (0 <= p < n_windows), not per slot: the kernels run the k loop.  th x tw is the upright window every
 * item has; the slots of k >= 4 are tw x th.  Transform k, ys, xs, the gather map and R_k are esr_tile_x8's.
 * Batch entry of transform k of window p: (k - k_begin) n_windows + p — esr_tile_x8's index at B = 1.  A range may
 * contain both k < 4 and k >= 4 only when th == tw (else ESR_ERR_INVALID).  C <= 8, with img C is 1 or 3, and
 * k_count n_windows <= 65535, else ESR_ERR_UNSUPPORTED.  The table's guarantees are esr_tile_many's (img = 0) /
 * esr_tile_img's (img = 1); this entry cannot read it.
 *   to_g32 = 1, scale = 1  gather-import: every pixel of window p is read once — img = 0: C strided fp32 reads of
 *               nchw [C][H][W]; img = 1: C bytes of hwc [H][W][C], float32(v) / 255.0f correctly rounded, channel
 *               m(c) = 2 - c when bgr and C == 3 (esr_tile_img's arithmetic) — and written, converted to dtype, as a
 *               finished 32-byte channel group to the logical pixel of every slot of the range in the G32 view (channels
 *               >= C zero, the halo never touched).  `live` is not read: a filler window is gathered for every k.
 *   to_g32 = 0, scale = 4  stitch-reduce: slots_nchw is fp32 [k_count * n_windows][C][4 th][4 tw] (k < 4) or
 *               [...][4 tw][4 th] (k >= 4), 16-byte aligned.  For every HR pixel (Y, X) of the owned rectangle of every
 *               window with live != 0, (y, x) = (Y - 4 wy, X - 4 wx) its window-local position:
 *                 a = accumulate ? PARTIAL : 0;   a += R_k(o_k)[y][x] for k ascending, one fp32 add per k
 *               img = 0: PARTIAL is the result itself, nchw [C][4H][4W] of the item:  nchw = a * mean_scale
 *                        (esr_tile_x8's protocol: mean_scale = 1 before the last range, 0.125 on it).
 *               img = 1: an 8-bit result cannot carry a partial sum.  PARTIAL is acc, fp32 [n_windows][C][4 th][4 tw],
 *                        upright and window-local, element ((p C + c) 4 th + y) 4 tw + x, 16-byte aligned:
 *                        k_begin + k_count < 8:   acc = a * mean_scale   (the result is not touched)
 *                        k_begin + k_count == 8:  hwc[(Y 4W + X) C + m(c)] = uint8(rintf(fminf(fmaxf(a * mean_scale, 0), 1)
 *                                                 * 255.0f))   (esr_tile_img's rounding; acc is not written)
 *                        acc is read only with accumulate and written only before the last range: all eight slots in one
 *                        pass never touch it, and it may then be null; else a null acc is ESR_ERR_INVALID.  The two
 *                        plans of a non-square window shape share one acc.  The bytes of a row of a workgroup's 32
 *                        pixels go out as aligned dwords (three per four pixels for C = 3, one for C = 1).
 *               The result does not depend on how the eight slots are split.  Nothing outside the owned rectangles is
 *               written; windows with live == 0 are neither read nor written (their acc entries included); g32 and
 *               dtype's storage type are unused.                                                                       */
typedef struct esr_tile_set_x8 {
  int32_t dtype, to_g32;
  int32_t C;
  int32_t tile, pad;             /* LR pixels */
  int32_t scale;                 /* 1: gather, 4: stitch */
  int32_t th, tw;                /* the upright window shape every item has */
  int32_t n_windows;             /* P: windows of the pass = table entries; batch entries = k_count * n_windows */
  const esr_tile_item* items;    /* n_windows entries, device memory (img: esr_tile_img_item, the same layout) */
  esr_g32 g32;
  const float* slots_nchw;
  int32_t k_begin, k_count;
  int32_t accumulate;
  float mean_scale;
  int32_t img;                   /* 0: fp32 NCHW images outside, 1: uint8 HWC */
  int32_t bgr;                   /* img, C == 3: B, G, R in memory on this op's side (else R, G, B) */
  float* acc;                    /* img stitch-reduce: the partial sums between the ranges (see above) */
} esr_tile_set_x8;

/* Philox-4x32-7 + Box-Muller N(0,1) fill (csrc/common.h), NCHW fp32 — the exact z the fused noise epilogue uses for
 * (seed, layer); lets tests feed the same z to the oracle (GaussianNoise, block.py:117-122). */
typedef struct esr_noise_fill {
  float* dst; int32_t B, C, H, W; uint64_t seed; uint32_t layer;
} esr_noise_fill;

/* Weight + bias gradient of a fused conv (autograd's conv backward-weight; SRRaGAN_model.py:140).
 * Accumulates with fp32 atomics: the caller zeroes dw / dbias first. */
typedef struct esr_wgrad {
  int32_t dtype, ks, stride, upsample;
  int32_t B, H, W;     /* size of g (= conv OUTPUT) */
  int32_t cout, cin;   /* true channel counts of dw [cout][cin][ks][ks] */
  esr_g32 g;           /* upstream gradient wrt the conv's pre-activation output */
  esr_g32 in;          /* the conv's saved input */
  float* dw;
  float* dbias;        /* may be NULL */
  float scale;
  int32_t tap_major;   /* 1: dw is laid out [tap][cout][cin] (lane-contiguous atomics: 2 cache lines per
                          wave instruction instead of ~36); esr_grad_unpermute restores OIHW */
  /* Deterministic two-stage reduction (ESR_F16 kernels): with `partial` set every workgroup stores its
   * 32x32xtaps partial with plain stores into its own slot of this arena and a second launch of the same
   * call adds the slots of a conv up in a fixed order into dw / dbias (+=, no atomics): bit-identical
   * gradients run to run.  `partial_elems` = floats available; esr_wgrad_workspace_elems() returns what an
   * op list needs (the arena is shared by all wgrad ops of a stream: a slot lives only inside one call).
   * NULL: fp32 atomicAdd (results vary in the last bits with the arrival order). */
  float* partial;
  int64_t partial_elems;
} esr_wgrad;

/* One launch that rewrites every tap-major gradient block into its OIHW slot.  `table` is a DEVICE
 * array of n entries {src_off, dst_off, elem_begin, cout, cin, ntap} (int64 x3, int32 x3, pad);
 * src/dst are fp32 arenas. */
typedef struct esr_unperm_entry {
  int64_t src_off, dst_off, elem_begin;
  int32_t cout, cin, ntap;
  int32_t pair_begin;       /* number of (cout, cin) pairs of the entries before this one (used when n_pairs > 0) */
} esr_unperm_entry;
typedef struct esr_unpermute {
  const esr_unperm_entry* table;
  int32_t n;
  int32_t n_pairs;          /* > 0: the sum of cout * cin over the table; the kernel then runs one thread per pair
                               (ntap coalesced reads, ntap adjacent writes, one table search per pair); 0: per element */
  int64_t total;
  const float* src;
  float* dst;
} esr_unpermute;

/* BatchNorm2d(affine) over a G32 tensor (block.py:28-32; Discriminator_VGG_128,
 * architecture.py:93-118), split in phases so each is one memory pass:
 *   STATS      sums[c] += sum x, sums[C+c] += sum x^2            (fp64 atomics; caller zeroes sums)
 *   FINALIZE   mean/invstd from sums (training: biased var; running stats updated with momentum and
 *              the UNBIASED var) or from running stats (eval)
 *   APPLY      y = act((x-mean)*invstd*gamma + beta)
 *   BWD_REDUCE g' = g*act'(y);  sums[c] += sum g',  sums[C+c] += sum g'*xhat
 *   BWD_FINAL  dgamma += sums[C+c]; dbeta += sums[c]
 *   BWD_APPLY  gx = gamma*invstd*(g' - sum g'/N - xhat*sum(g' xhat)/N)   (eval: gamma*invstd*g') */
enum esr_bn_mode { ESR_BN_STATS = 0, ESR_BN_FINALIZE = 1, ESR_BN_APPLY = 2, ESR_BN_BWD_REDUCE = 3,
                   ESR_BN_BWD_FINAL = 4, ESR_BN_BWD_APPLY = 5,
                   ESR_BN_FIN_APPLY = 7,  /* training: FINALIZE and APPLY as ONE pass (every workgroup forms its channels'
                                          statistics from the sums; mean / invstd / running statistics / num_batches_tracked
                                          are written as FINALIZE would).  BWD_APPLY likewise performs BWD_FINAL when
                                          dgamma is set */
                   ESR_BN_RESTAT = 6   /* training: apply the running-statistics (and num_batches_tracked) updates of
                                          ANOTHER forward call over the same batch from the sums still in place, groups in
                                          REVERSE order — the train step calls netD on (fake, real) and then, weights
                                          unchanged, on (real, fake) (SRRaGAN_model.py:133-134,150-151): the second pair's
                                          activations equal the first's, only the BatchNorm buffers move */ };
typedef struct esr_bn {
  int32_t dtype, mode;
  int32_t B, C, H, W;
  int32_t training, act;
  float momentum, eps;
  esr_g32 x, y, g, gx;
  double* sums;                 /* [2*C] */
  float* mean; float* invstd;   /* [C] batch statistics kept for backward */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  float* dgamma; float* dbeta;
  /* groups > 1: the batch is `groups` independent BatchNorm batches of B/groups images each (the reference's
   * netD(real) and netD(fake) calls, SRRaGAN_model.py:133-134,150-151, as ONE launch per layer): sums is
   * [groups][2*C], mean / invstd are [groups][C]; FINALIZE applies the running-statistics update once per group,
   * in group order; BWD_FINAL adds the groups' sums into dgamma / dbeta.  0 or 1 = one batch. */
  int32_t groups, _pad;
  int64_t* num_batches_tracked; /* FINALIZE (training): += groups (NULL: caller counts) */
} esr_bn;

/* MaxPool2d(2,2) (torchvision VGG19 cfg 'E', architecture.py:287-298).  mode 0: y = pool(x);
 * mode 1: gx = route g to the FIRST maximum of each 2x2 window (torch semantics).
 * Round 5 — the same struct carries nn.PixelShuffle(2) (pixelshuffle_block, block.py:299-312; SRResNet's upsampler):
 * mode 2: y[b][c][2h+i][2w+j] = x[b][4c + 2i + j][h][w]   (C = channels of y, H x W = size of x; C % channel group == 0)
 * mode 3: its adjoint, gx[b][4c + 2i + j][h][w] = g[b][c][2h+i][2w+j], with relu_mask: times ReLU'(x) of the conv that
 *         produced x (the activation behind the shuffle commutes with it, so it rides in the conv's epilogue).
 * Added under ABI 6 (a pure addition) — the 3x pixel shuffle behind the folded nearest-x3 up-conv (esr_fold3):
 * mode 4: y[b][c][3h+i][3w+j] = x[b][(3i + j) C + c][h][w]   (C = channels of y, H x W = size of x; C % channel group == 0;
 *         x has 9 C channels).  Phase-major channel order — not torch's PixelShuffle(3) — so that a thread moves whole
 *         32-byte channel groups in either precision; only image pixels of y are written, never its zero ring.
 * mode 5: its exact adjoint, gx[b][(3i + j) C + c][h][w] = g[b][c][3h+i][3w+j]  (relu_mask is ignored: the activation's
 *         mask is applied at high resolution by the consumer's input-gradient conv). */
typedef struct esr_pool {
  int32_t dtype, mode;
  int32_t B, C, H, W;           /* OUTPUT (pooled) size */
  int32_t relu_mask;            /* mode 1: also apply ReLU' of the pooled tensor's producer (x > 0) */
  int32_t _pad;
  esr_g32 x, y, g, gx;
} esr_pool;

/* nn.Linear on row-major fp32 (Discriminator classifier, architecture.py:121-123).
 * mode 0: y = act(x W^T + b);  mode 1: gx = (g * act'(y_saved)) W ... see fields;  mode 2: dw, db. */
typedef struct esr_linear {
  int32_t mode, B, I, O, act;
  int32_t in_act;               /* mode 1 (input gradient): the activation that PRODUCED x (a conv + LeakyReLU feeding the
                                   head without a norm layer, architecture.py:163-170): gx *= in_act'(x); 0 = none */
  const float* x; const float* w; const float* b; float* y;
  const float* g;               /* dL/dy (already multiplied by act' by the caller kernel: see gmask) */
  const float* ysaved;          /* bwd: saved activation output of THIS layer for act' (may be NULL) */
  float* gx; float* dw; float* db;
} esr_linear;

/* One axis of a separable resampling on fp32 planes (MATLAB-style bicubic `imresize`,
 * codes/data/util.py:221-343: the H pass then the W pass).  out[p][i][j] = sum_t w[o][t] * in[p][..]
 * where o is the output coordinate along `axis` (0 = rows/H, 1 = columns/W) and idx[o][t] the source
 * coordinate of tap t with the symmetric border padding already resolved.  Tables are DEVICE arrays. */
typedef struct esr_resample {
  const float* in; float* out;
  int32_t planes, in_h, in_w, out_len, axis, taps;
  const float* w;        /* [out_len][taps] */
  const int32_t* idx;    /* [out_len][taps] */
} esr_resample;

/* One training batch cut out of a device-resident image pool in ONE launch: B calls of LRHRDataset.__getitem__
 * (codes/data/LRHR_dataset.py:81-121) — per sample the paired crop windows, util.augment's flips (util.py:94-106),
 * uint8 -> float32 (util.py:79) and BGR -> RGB (LRHR_dataset.py:117-119) — and, for a sample without an LR image, the
 * LR window of imresize(hr, 1 / scale) (util.py:276-343) computed from the HR image.  Images may differ in size and
 * kind from sample to sample.  With `crop` a sample's window (LR: lr_size^2 at (y0, x0); HR: (scale lr_size)^2 at
 * (scale y0, scale x0)) and n its side:
 *   out[c][i][j] = t[c][a][b],  (a, b) = (j, i) if transpose else (i, j),
 *   t[c][a][b]   = crop[c'][vflip ? n - 1 - a : a][hflip ? n - 1 - b : b],  c' = swap_rb ? 2 - c : c.
 * A uint8 value v converts as (float)v / 255.0f, a true division.  A generated LR pixel is the H pass then the W pass
 * over the WHOLE image's tables (the mirror border is the image's, not the window's), each a sum over the taps in
 * ascending order, as esr_resample_axis forms it.  The item table is DEVICE memory and the caller's contract: windows
 * inside their images, tables of esr_resample's layout for (hr_h, 1 / scale) and (hr_w, 1 / scale), so that
 * lr_h = hr_h / scale and lr_w = hr_w / scale.  No workspace. */
typedef struct esr_batch_item {
  const void* hr;            /* src_format 0: float32 [3][hr_h][hr_w] in [0,1]; 1: uint8 [hr_h][hr_w][3], rows packed */
  const void* lr;            /* the same format, lr_h x lr_w; NULL: generate the LR window from hr */
  const float* wy; const int32_t* iy;   /* generated LR only: [lr_h][taps_y] weights / source rows */
  const float* wx; const int32_t* ix;   /*                    [lr_w][taps_x] weights / source columns */
  int32_t hr_h, hr_w, lr_h, lr_w;
  int32_t y0, x0;            /* the window's origin on the LR grid */
  int32_t flags;             /* bit 0 hflip, bit 1 vflip, bit 2 transpose, applied in that order */
  int32_t taps_y, taps_x;
  int32_t _pad;
} esr_batch_item;

typedef struct esr_batch {
  int32_t B, C;              /* C = 3, else ESR_ERR_UNSUPPORTED; B <= 65535, else ESR_ERR_UNSUPPORTED */
  int32_t lr_size;           /* s: the LR window's side */
  int32_t scale;             /* 1, 2, 3, 4 or 8 */
  int32_t src_format;        /* 0: float32 CHW planes; 1: uint8 HWC */
  int32_t swap_rb;           /* output channel c reads source channel 2 - c */
  float* lr_out;             /* [B][3][s][s] */
  float* hr_out;             /* [B][3][s scale][s scale] */
  const esr_batch_item* items;   /* DEVICE table of B entries */
} esr_batch;

/* Adam over a whole network in ONE launch (torch.optim.Adam semantics, SRRaGAN_model.py:77-91:
 * amsgrad off; the reference steps ~770 parameter tensors per optimizer).  `entries` / `blocks` are
 * DEVICE tables built once per parameter set: entry e = {param pointer, offset of its gradient /
 * moments in the flat fp32 buffers, element count}; block b = {entry, first element}: each
 * workgroup updates up to ESR_ADAM_BLOCK_ELEMS consecutive elements of one tensor.
 *   g = grad[goff+i]*grad_scale (+ weight_decay*p);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)          bc1 = 1-b1^t, bc2 = 1-b2^t (host). */
#define ESR_ADAM_BLOCK_ELEMS 4096
typedef struct esr_adam_entry { float* p; int64_t goff; int64_t n; } esr_adam_entry;
typedef struct esr_adam_block { int32_t entry; int32_t first; } esr_adam_block;
typedef struct esr_adam {
  const esr_adam_entry* entries;
  const esr_adam_block* blocks;
  int32_t nblocks, _pad;
  const float* grad;      /* flat gradients (loss-scaled; see grad_scale) */
  float* exp_avg;         /* flat first / second moments, same offsets as grad */
  float* exp_avg_sq;
  float lr, beta1, beta2, eps, bc1, bc2, grad_scale, weight_decay;
  const float* amp_state; /* NULL, or the DEVICE state of dynamic loss scaling (esr_amp): gradients are additionally
                             divided by amp_state[0] (the loss scale), and the whole update is skipped — weights and
                             moments untouched — while amp_state[4 + amp_slot] != 0 (a non-finite gradient was found in
                             THIS optimizer's gradients).  No host synchronisation anywhere: the fp16 train path's
                             overflow handling */
  int32_t amp_slot, _pad2;
  const float* step_count; /* NULL: bc1 / bc2 above are used.  Else a DEVICE counter of the steps this optimizer has
                             APPLIED including the current one (ESR_AMP_COUNT advances it only when the step is not
                             skipped): bc = 1 - beta^step_count[0] is formed in the kernel from beta1_d / beta2_d, so a
                             skipped step does not age Adam's bias correction (torch.amp.GradScaler semantics) */
  double beta1_d, beta2_d; /* the betas in fp64: 1 - beta (and the device-side bias correction) come from these, so that
                             fp32 rounding of a beta near 1 does not scale the moments; 0: taken from beta1 / beta2 */
} esr_adam;

/* Dynamic loss scaling for the fp16 training path (new capability; the reference trains in fp32 only).
 * state = DEVICE float[8] {scale, -, good_steps, -, found[0..3]}: one found-a-non-finite-gradient flag per optimizer
 * (slot), as torch.amp.GradScaler tracks found_inf per optimizer — an overflow in G's gradients does not skip D's step.
 *   ESR_AMP_CHECK   found[slot] |= any(!isfinite(grad[0..n)))       (after the backward / gradient exchange)
 *   ESR_AMP_COUNT   if (!found[slot]) step_count[0] += 1            (before esr_adam_step: the step it will apply)
 *   ESR_AMP_UPDATE  any(found) ? (scale *= backoff, good = 0) : (++good == interval ? (scale *= growth, good = 0) : -);
 *                   found[*] = 0                                      (once per iteration, after the optimizers)  */
enum esr_amp_mode { ESR_AMP_CHECK = 0, ESR_AMP_UPDATE = 1, ESR_AMP_COUNT = 2 };
typedef struct esr_amp {
  int32_t mode, interval;
  float* state;
  const float* grad;
  int64_t n;
  float growth, backoff;
  int32_t slot, _pad;         /* 0..3 (CHECK, COUNT) */
  float* step_count;          /* COUNT */
} esr_amp;

/* ---- validation metrics on the device (metrics.hip) -------------------------------------------------
 * tensor2img (codes/utils/util.py:71-95: clamp, scale, x255, round, RGB -> BGR, HWC uint8) of one image or of
 * an (sr, hr) pair, and on the pair, cropped by `crop` pixels per side (codes/train.py:131-148):
 *   out[0] = sum of squared uint8 differences, out[1] unused, out[2] = sum of the SSIM map (util.py:117-158;
 *   over all compared planes), out[3] unused;   PSNR = 20 log10(255 / sqrt(out[0] / n)),  SSIM = out[2] / n_ssim
 * with n = (H-2crop)(W-2crop) planes, n_ssim = (H-2crop-10)(W-2crop-10) planes (the caller divides).
 * y_only (C == 3): compare the MATLAB-style Y planes of the BGR images as codes/test.py:81-90 forms them — bgr2ycbcr on
 * the float images, data/util.py:150-168, i.e. luma NOT rounded to uint8. */
typedef struct esr_l1_loss {
  const float* a; const float* b;
  float* grad_a;               /* may be NULL */
  float* loss;                 /* 1 float */
  double* scratch;             /* 2 doubles, zero */
  int64_t n;
  float weight;
  float grad_scale;            /* round 4: grad_a is additionally multiplied by this (the loss scale of the fp16 path: the
                                  loss itself stays unscaled); 0 = 1 */
  const float* grad_scale_dev; /* non-NULL: multiplied in as well, read on the device (dynamic loss scaling, esr_amp state[0]) */
} esr_l1_loss;

typedef struct esr_ragan_loss {
  const float* x; const float* y;      /* n logits each */
  float* grad_x; float* grad_y;        /* may be NULL */
  float* loss; float* mean_x; float* mean_y;
  float* bce_x; float* bce_y;          /* optional: the two BCE terms, unweighted (the reference logs them) */
  int32_t n;
  float tx, ty, weight;                /* targets (1 = real, 0 = fake) of the x / y terms */
  /* Data-parallel form (round 3): the batch means stay GLOBAL (SRRaGAN_model.py:136-137,151-152) while every
   * launch only sees the rank's own n logits — the two scalar sums cross the ranks (RCCL all-reduce) between launches:
   *   mode 0  everything from the local batch (one GPU)
   *   mode 1  sums[0..1] = {sum x, sum y}
   *   mode 2  means = ext[0]/ext[2], ext[1]/ext[2] (global sums, global count): loss, mean_x/y, bce_x/y and
   *           sums[0..1] = {sum_i sigmoid(x_i - mean y) - tx,  sum_i sigmoid(y_i - mean x) - ty}
   *   mode 3  grad_x / grad_y from the global means and ext[3..4] = those two sums over all ranks         */
  int32_t mode;
  float grad_scale;                    /* round 4: grad_x / grad_y times this (loss scale); 0 = 1 */
  float* sums;                         /* 2 floats (modes 1, 2) */
  const float* ext;                    /* 5 floats (modes 2, 3) */
  const float* grad_scale_dev;         /* non-NULL: multiplied in as well, read on the device */
} esr_ragan_loss;

typedef struct esr_gan_loss {
  const float* x; const float* y;      /* n_x logits; y (n_y logits) may be NULL: one operand */
  float* grad_x; float* grad_y;        /* may be NULL */
  float* loss;                         /* weight * (l(x, tx) [+ l(y, ty)]) */
  float* term_x; float* term_y;        /* optional: the two terms, unweighted (l_d_real / l_d_fake) */
  float* mean_x; float* mean_y;        /* optional: mean(x), mean(y) (D_real / D_fake) */
  const float* grad_scale_dev;         /* non-NULL: multiplied into the gradients as well, read on the device */
  int32_t n_x, n_y;
  float tx, ty;                        /* the label VALUES (GANLoss real_label_val / fake_label_val) */
  int32_t kind;                        /* 0 = vanilla (BCE with logits), 1 = lsgan (MSE) */
  float weight;
  float grad_scale;                    /* grad_x / grad_y times this (loss scale); 0 = 1 */
  int32_t _pad;
} esr_gan_loss;

typedef struct esr_img_metrics {
  const float* sr;           /* [C][H][W] fp32 */
  const float* hr;           /* same shape, or NULL: conversion only */
  int32_t C, H, W, crop;
  int32_t y_only, _pad;
  float lo, hi;              /* tensor2img's min_max */
  uint8_t* img_sr;           /* [H][W][C] uint8 BGR */
  uint8_t* img_hr;
  double* y_sr;              /* [H][W] fp64 (y_only): UNROUNDED luma, codes/test.py:81-86 converts the float images */
  double* y_hr;
  double* out;               /* 4 doubles (device) */
  double win[11];            /* 1-D Gaussian window (cv2.getGaussianKernel(11, 1.5)); the 2-D one is its outer product */
} esr_img_metrics;

/* The four validation sums of an image SET in one launch set (esr_image_set_metrics; csrc/metrics_set.hip): what
 * codes/test.py:69-110 logs per image — PSNR, SSIM, PSNR_Y, SSIM_Y — and the validation loop of codes/train.py:121-159
 * averages, from pairs of 8-bit images on the device (esr_tile_img's stitch results against their ground truth).
 * Pair i is items[i]: sr and hr are uint8 [H][W][3] (HWC, any byte alignment, rows of 3 W bytes without padding).  With
 * (ch, cw) = (H - 2 crop, W - 2 crop) the cropped region, k = win, and a(y, x, c), b(y, x, c) the bytes of sr, hr at
 * cropped position (y, x), out[4 i + 0 .. 3] receives, in fp64:
 *   0  sum over y, x, c of (a - b)^2                                               (util.py:107-114; exact, an integer)
 *   1  sum over y, x of (Y_a - Y_b)^2,  Y = (24.966 B + 128.553 G + 65.481 R) / 255 + 16, NOT rounded (test.py:85-89);
 *      B is byte 0 of a pixel when bgr != 0 (cv2, metrics.hip's images, esr_tile_img with bgr), else byte 2 (PIL)
 *   2  sum over the three channels and the (ch - 10) x (cw - 10) valid positions of the SSIM map of util.py:117-137:
 *      window outer(k, k), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
 *   3  the same sum over the Y plane
 * Sums 2 and 3 are 0 when ch <= 10 or cw <= 10 (no valid position).  The window runs as a row filter and a column filter
 * (22 taps, not 121): against esr_image_metrics the fp64 summation order differs, nothing else.
 * Work units: image i is cut into ceil(ch / ESR_SET_METRICS_TILE_H) x ceil(cw / ESR_SET_METRICS_TILE_W) tiles, one
 * workgroup each; items[i].first is the number of tiles of the images before it (items[0].first = 0) and n_units the
 * number of all tiles.  Every workgroup writes its four partial sums to scratch[4 unit .. 4 unit + 3] (4 n_units doubles,
 * need not be initialised), and a second kernel adds an image's partials in an order that depends on its tile count
 * alone.  No floating-point atomics: two calls on the same bytes give the same bits, and an image's four sums do not
 * depend on the other images of the call or on its place in the table.
 * The table lives in DEVICE memory (read by the launch: it must stay valid until the launch has run) and cannot be
 * checked by this entry.  So the caller repeats the sizes in HOST memory: sizes_host[2 i], sizes_host[2 i + 1] = H, W of
 * pair i, read during the call only.  From them the entry refuses (ESR_ERR_INVALID) a crop that leaves no pixels of some
 * image and an n_units that is not the sum of the tile counts, and sizes the launch; whoever fills the table guarantees
 * that its H, W and first agree with sizes_host and that sr, hr are live images of that size.  (The largest H, W alone
 * would not do: it is the smallest image that a crop empties.)  A workgroup whose unit lies outside its item's tiles
 * reads no image and adds zeros.  The kernel reads whole aligned dwords that contain image bytes.                       */
#define ESR_SET_METRICS_TILE_H 16
#define ESR_SET_METRICS_TILE_W 32
typedef struct esr_set_metrics_item {   /* one image pair, 32 bytes; lives in DEVICE memory */
  const uint8_t* sr;             /* [H][W][3] uint8 */
  const uint8_t* hr;             /* [H][W][3] uint8 */
  int32_t H, W;
  int32_t first;                 /* work units (tiles) of the items before this one */
  int32_t _pad;
} esr_set_metrics_item;

typedef struct esr_set_metrics {
  int32_t n;                     /* image pairs, >= 1 */
  int32_t crop;                  /* pixels cut from every side, >= 0 */
  int32_t bgr;                   /* byte 0 of a pixel is B (else R): matters to the luma only */
  int32_t n_units;               /* tiles of all images */
  const esr_set_metrics_item* items;   /* n entries, device memory, 8-byte aligned */
  const int32_t* sizes_host;     /* n x (H, W), HOST memory */
  double* out;                   /* n x 4 doubles (device) */
  double* scratch;               /* 4 n_units doubles (device) */
  double win[11];                /* 1-D Gaussian window, normalised (esr_img_metrics.win) */
} esr_set_metrics;

/* ---- fused ResidualDenseBlock_5C chain (rdb_fused.hip) -------------------------------------------
 * ONE persistent launch runs n_blocks dense blocks (block.py:260-268) back to back on every 16x32
 * tile, the fp32 accumulators of all 192 output channels of the block in flight held in registers
 * ("input stationary": each input slice x, x1..x4 is staged once and feeds every later conv), with
 * the 1-pixel halos of x1..x4 / the block output exchanged between neighbouring tiles inside the
 * launch.  The RRDB tail (block.py:291: out*0.2 + x_rrdb; test_image/block.py:256 adds a noise
 * layer) is the second residual stage of a block whose res2 is set.
 *   x1 = lrelu(conv1(x));  x2 = lrelu(conv2(x,x1)) + conv1x1(x);  x3 = lrelu(conv3(x..x2));
 *   x4 = lrelu(conv4(x..x3)) + x2;  y = noise1(conv5(x..x4)*0.2 + x);  [y = noise2(y*0.2 + res2)]
 * Weights: one fused stream per block (esr_rdb_weight_stream_bytes), 1 KB MFMA A fragments
 * F(blk, c, kh, kw) = packed(conv)[cout_block][chunk c][kh][kw] (blk 0..3 = conv1..conv4, 4/5 = conv5's
 * two cout blocks) in the order the kernel consumes them.  With c running over the K steps (chunks) of
 * the input slice of phase p = 1..5 (x, x1, x2, x3, x4):
 *   ESR_F32:  for p, c, kw, blk = p-1..5, kh: F;  then the 1x1's chunks.
 *   ESR_F16:  for p = 1..4: [for c, kw, kh: F(p-1)]  [for c, kw, blk = p..5, kh: F]  (after p = 1: the
 *             1x1's chunks);  p = 5: for c, kw, blk = 4..5, kh: F.
 *             (conv_p alone first, so that its epilogue and halo hand-off overlap the remaining convs.)
 * Build it from the per-conv packed weights with esr_gather_fragments.
 * All views share one geometry (same wp / H / W); x_out may alias x_in or res2 (pixel-local). */
typedef struct esr_rdb_block {
  const void* w;            /* fused weight stream of this block */
  const float* bias;        /* fp32 [192]: biases of conv1..conv4 (32 each) then conv5 (64), gathered by the caller
                               (esr_gather_fragments with piece_bytes = 128 does it in one launch for a whole net) */
  esr_g32 x_in;             /* 64-channel block input */
  esr_g32 x_out;            /* 64-channel block output */
  esr_g32 res2;             /* RRDB input of the fused RRDB tail; ptr NULL = plain dense block */
  uint32_t layer1, layer2;  /* Philox stream ids of the block noise / the RRDB-tail noise; 0xFFFFFFFF = off */
  uint32_t flags;           /* ESR_RDB_FULL_OUT: every pixel of x_out must reach memory — the chain's last block, or an
                               output that is read again as a later block's res2.  Otherwise (fp16, no noise) only the
                               tiles' border pixels are stored: the next block takes its input from the LDS and its
                               `+ x` residual from the accumulators this block's epilogue primes with 5 x */
  uint32_t _pad;
  /* ---- training chains (esr_rdb_chain.mode 1 / 2, fp16) ---- */
  esr_g32 dense;            /* this block's own 128 channels: mode 1: x1..x4 (kept for the backward);
                               mode 2: g_a4 | g_a3 | g_a2 | g_a1 (what the weight gradients read) */
  void* mask;               /* LeakyReLU masks of a1..a4, one bit per element: B * tiles records of 8 KB in the chain's
                               16x32 tile order, [slice a1..a4][wave][lane][4 rows x u16] (esr_rdb_mask_bytes); written
                               by mode 1, read by mode 2 of the same geometry */
  esr_g32 aux;              /* mode 2: unmasked g_x2 (32 channels), input of the 1x1's weight gradient */
  esr_g32 out_a;            /* mode 2, blocks with res2 (the RDB1 of an RRDB): A' = (acc + res2) (1 + sigma z[layer2]) is
                               stored here (the skip gradient of the previous RRDB) and x_out = 0.2 A' (1 + sigma z[layer1]);
                               ptr NULL: x_out = (acc [+ res2]) (1 + sigma z[layer1]) */
} esr_rdb_block;
#define ESR_RDB_FULL_OUT 1u
#define ESR_RDB_BAND_OWN 2u  /* banded launch (esr_rdb_chain.band_rows): x_out receives only the band's OWN rows */
/* Backward weight stream of a block (mode 2): the forward's layout over the gather-form operands
 *   blk 0..3 = the x4, x3, x2, x1 slice convs (esr_pack.gather; the x2 one with fold_co0 = the x4 columns of conv5),
 *   blk 4/5 = the x slice conv's two cout blocks (K = 192: g_t, g_a4..g_a1),
 * crit_p / bulk_p as in the forward; the 1x1 unit (esr_pack.one_t: 2 cout blocks x 2 chunks) sits behind crit_3. */

typedef struct esr_rdb_chain {
  int32_t dtype, B, H, W;
  int32_t n_blocks;
  int32_t noise_mode;       /* ESR_NOISE_OFF or ESR_NOISE_PHILOX (explicit z: per-conv path) */
  float sigma;
  int32_t save_dense;       /* 0: fp16 path stores only each tile's border pixels of x1..x4 (all the launch itself
                               re-reads); 1: the whole slices reach `dense` (e.g. to inspect / save activations) */
  uint64_t seed;
  const uint64_t* seed_dev; /* as esr_conv.seed_dev */
  esr_g32 dense;            /* 128-channel scratch: x1..x4 of the block in flight */
  const esr_rdb_block* blocks;  /* DEVICE array of n_blocks entries */
  void* workspace;          /* esr_rdb_workspace_bytes(B,H,W) bytes of device memory; word 1 != 0 after the
                               launch = a bounded spin timed out (results invalid) */
  size_t workspace_bytes;
  uint64_t* trace;          /* measurement only (NULL = off): per tile 64 x uint64 time stamps (100 MHz) */
  int32_t mode;             /* 0: inference forward (esr_rdb_forward);  1: TRAINING forward (esr_rdb_forward, fp16): every
                               block writes x1..x4 to its own `dense`, its output in full and its LeakyReLU masks;
                               2: BACKWARD (esr_rdb_backward, fp16): blocks in backward order, x_in = the block's g_t
                               (dL/d(conv5 * 0.2 + x)), weights = the gather-form streams (below), x_out = the next
                               block's g_t */
  int32_t _pad2;
  /* Row bands (mode 0, noise off): an image with more 16x32 tiles than CUs cannot run as one chain (a tile spins on
   * its neighbours, so all tiles of an image must be resident).  It is cut into bands of `band_rows` rows and the
   * bands take the place of the batch: B = number of bands, H = band_rows + 2 * band_margin.  A view of the IMAGE (the
   * chain's input, its result, a res2 that is the image) has batch_stride = band_rows rows, and its row 0 of band b is
   * image row b * band_rows - band_margin (the caller's buffers carry band_margin rows of zero padding above and
   * below the image).  A view that lives only inside the launch — the outputs of the blocks in between, the dense
   * scratch — is band-local: one entry of H rows per band at any batch_stride (engine.py: a G32 of B = bands); the
   * kernels form b * batch_stride in 64 bits, and an image of many bands takes it past 2^32.  A band recomputes band_margin rows
   * of its neighbours on either side — band_margin >= 5 * n_blocks, the chain's dependency radius — and the kernel
   * writes only rows that exist in the image (0 <= row < img_H), and into an ESR_RDB_BAND_OWN block's x_out only the
   * band's own rows.  band_rows = 0: off. */
  int32_t band_rows, band_margin, img_H, _pad3;
} esr_rdb_chain;

/* Piece gather: dst[f * piece_bytes ..] = src_base[src_off[f] ..] for f < n (src_off: DEVICE int64 byte offsets;
 * src_base may be NULL, then they are absolute addresses).  piece_bytes: power of two in 16..4096, 0 = 1024 (one MFMA
 * A fragment). */
typedef struct esr_frag_gather {
  const int64_t* src_off;
  const void* src_base;
  void* dst;
  int64_t n;
  int32_t piece_bytes, _pad;
} esr_frag_gather;

/* ---- weight / bias gradients of a whole dense block in one pass (rdb_wgrad.hip) --------------------------------
 * Replaces the six esr_conv_wgrad problems of a ResidualDenseBlock_5C (block.py:239-268; autograd's conv
 * backward-weight, SRRaGAN_model.py:140) for n_blocks blocks in ONE launch (+ one deterministic reduce launch):
 *   in = [x (64) | x1 | x2 | x3 | x4] (192 channels),   q = [g_t (64) | g_a4 | g_a3 | g_a2 | g_a1 | g_x2] (224 channels)
 *   dW_convk += g_ak (x) in[0 : 32 (k + 1))  (3x3; conv5: g_a5 = scale5 * g_t),  dW_1x1 += g_x2 (x) x,  db_k += sum g_ak
 * where g_x2 is the gradient of x2 BEFORE its LeakyReLU mask (it feeds the bias-free 1x1, block.py:263).
 * Both views share one geometry (wp, H, W); one image of either must be < 2 GB (see esr_g32).  dw[k]: k = 0..4 conv1..conv5 ([cout][cin][3][3] fp32, or tap-major
 * [tap][cout][cin] when tap_major; accumulated: +=), k = 5 the 1x1 ([32][64]); db[k] k = 0..4 (NULL: skipped). */
typedef struct esr_rdb_wgrad_block {
  esr_g32 in;               /* the block's saved concat buffer (forward) */
  esr_g32 q;                /* the block's gradient concat (backward chain) */
  float* dw[6];
  float* db[6];             /* db[5] unused (the 1x1 has no bias) */
} esr_rdb_wgrad_block;
typedef struct esr_rdb_wgrad {
  int32_t dtype;            /* ESR_F16 */
  int32_t B, H, W;
  int32_t n_blocks, tap_major;
  float scale5;             /* 0.2: g_a5 = 0.2 g_t (block.py:267) */
  float scale;              /* applied to every gradient (1.0) */
  const esr_rdb_wgrad_block* blocks;   /* DEVICE array */
  float* partial;           /* esr_rdb_wgrad_workspace_elems() floats: per-task partial sums, reduced in a fixed order
                               (+ the step counters that keep the four channel sets of a row band in lock step) */
  int64_t partial_elems;
  int32_t max_workgroups;   /* 0 (default): one workgroup per task, a plain non-persistent grid; n > 0: a persistent
                               grid of at most n workgroups striding over the tasks — the caller runs the pass NEXT TO
                               other work (the train plan: a run of RRDBs' weight gradients on the side stream under the
                               next run's backward chain) */
  int32_t _pad;
} esr_rdb_wgrad;

/* Nearest-x3 up-sampling followed by a zero-padded 3x3 conv (upconv_blcok with upscale_factor 3, block.py:315-322) IS a
 * zero-padded 3x3 conv on the low-resolution grid to 9 cout channels followed by the 3x pixel shuffle of esr_pool mode 4:
 * output phase p in {0,1,2} along an axis reads, for tap k in {0,1,2}, the low-resolution offset off(p,k) =
 * floor((p + k - 1) / 3), i.e. (-1,0,0), (0,0,0), (0,0,+1).
 * mode 0 (fold):   wf[(3p+q) cout + co][ci][a][b] = sum of w[co][ci][kh][kw] over the taps with off(p,kh) = a - 1 and
 *                  off(q,kw) = b - 1, added in (kh, kw) order in fp32 (1 to 4 terms; 0 where no tap lands);
 *                  bf[(3p+q) cout + co] = bias[co].
 * mode 1 (unfold): the adjoint, for gradients: w[co][ci][kh][kw] = sum over (p, q) in order of
 *                  wf[(3p+q) cout + co][ci][off(p,kh)+1][off(q,kw)+1];  bias[co] = sum over (p, q) of bf[(3p+q) cout + co].
 * All tensors fp32 OIHW; bias / bf may both be NULL. */
typedef struct esr_fold3 {
  int32_t mode, cout, cin, _pad;
  float* w;      /* [cout][cin][3][3]: read by mode 0, written by mode 1 */
  float* bias;   /* [cout] */
  float* wf;     /* [9 cout][cin][3][3]: written by mode 0, read by mode 1 */
  float* bf;     /* [9 cout] */
} esr_fold3;

enum esr_op_kind { ESR_OP_CONV = 1, ESR_OP_PACK = 2, ESR_OP_LAYOUT = 3, ESR_OP_NOISE_FILL = 4,
                   ESR_OP_WGRAD = 5, ESR_OP_BN = 6, ESR_OP_POOL = 7, ESR_OP_LINEAR = 8,
                   ESR_OP_UNPERMUTE = 9, ESR_OP_PACK_BATCH = 10,
                   ESR_OP_RDB_CHAIN = 11, ESR_OP_FRAG_GATHER = 12, ESR_OP_RDB_WGRAD = 13,
                   ESR_OP_RDB_CHAIN_BWD = 14 /* u.rdb_chain with mode 2 */, ESR_OP_DIHEDRAL = 15,
                   ESR_OP_TILE = 16, ESR_OP_TILE_X8 = 17, ESR_OP_FOLD3 = 18, ESR_OP_TILE_MANY = 19,
                   ESR_OP_TILE_IMG = 20, ESR_OP_TILE_SET_X8 = 21, ESR_OP_TILE_HR = 22 };

/* esr_op.flags */
#define ESR_OPF_SIDE 1   /* on a run of consecutive ESR_OP_WGRAD ops: launch the run on the library's side
                            stream, ordered after every earlier op.  It is complete (a) before any op that
                            follows the NEXT side run, (b) before any ESR_OP_UNPERMUTE op, (c) when the work
                            esr_run_ops enqueued on `stream` completes.  The caller guarantees that nothing
                            up to the end of the next side run writes the run's inputs or reads its outputs
                            (the train plan double-buffers the gradient slices it reads). */
#define ESR_OPF_SIDE_FREE 2   /* with ESR_OPF_SIDE: the run's inputs are never overwritten and its outputs never read
                            inside this list, and its esr_wgrad.partial region belongs to this run alone — it is
                            launched without waiting for earlier side runs, on one of three library-owned streams
                            (round robin), complete before any ESR_OP_UNPERMUTE and when the list's work on `stream`
                            completes.  (The discriminator's backward: ten independent, latency-bound weight
                            gradients next to the dgrad chain.) */

#define ESR_OPF_FOLLOW 4   /* on an ESR_OP_RDB_WGRAD op that stands right behind the ESR_OP_RDB_CHAIN_BWD op whose blocks it
                            lists (same blocks, the chain's order): the pass is launched TOGETHER with the chain, on the
                            library's side stream, as a persistent grid on the CUs the chain's grid leaves free (at least
                            32; esr_rdb_wgrad.max_workgroups caps it further) — a task of block k starts when the chain's
                            tiles it reads have published the end of block k, a block's partial sums are reduced in
                            slices, one slice by each task of the block a whole round of the grid later (the last
                            blocks' reductions by extra tasks at the end of the list).  Results are bit-identical to the pass run behind the chain; completion as for
                            ESR_OPF_SIDE.  For launches that leave CUs free (training crops); refused otherwise. */

typedef struct esr_op {
  int32_t kind;
  int32_t flags;
  union {
    esr_conv conv;
    esr_pack pack;
    esr_layout layout;
    esr_noise_fill noise_fill;
    esr_wgrad wgrad;
    esr_bn bn;
    esr_pool pool;
    esr_linear linear;
    esr_unpermute unpermute;
    esr_pack_batch pack_batch;
    esr_rdb_chain rdb_chain;
    esr_frag_gather frag_gather;
    esr_rdb_wgrad rdb_wgrad;
    esr_dihedral dihedral;
    esr_tile tile;
    esr_tile_x8 tile_x8;
    esr_fold3 fold3;
    esr_tile_many tile_many;
    esr_tile_img tile_img;
    esr_tile_set_x8 tile_set_x8;
    esr_tile_hr tile_hr;
  } u;
} esr_op;

/* Geometry helper: padded plane size for a logical HxW image. */
void esr_g32_dims(int32_t H, int32_t W, int32_t* Hp, int32_t* Wp);

/* Single-op entry points. */
int esr_conv_forward(const esr_conv* p, esr_stream_t stream);
int esr_pack_conv_weights(const esr_pack* p, esr_stream_t stream);
int esr_convert_layout(const esr_layout* p, esr_stream_t stream);
int esr_fill_noise(const esr_noise_fill* p, esr_stream_t stream);
int esr_dihedral_op(const esr_dihedral* p, esr_stream_t stream);   /* added under ABI 6: a pure addition */
int esr_tile_op(const esr_tile* p, esr_stream_t stream);           /* added under ABI 6: a pure addition */
int esr_tile_x8_op(const esr_tile_x8* p, esr_stream_t stream);     /* added under ABI 6: a pure addition */
int esr_fold3_op(const esr_fold3* p, esr_stream_t stream);         /* added under ABI 6: a pure addition */
int esr_tile_many_op(const esr_tile_many* p, esr_stream_t stream); /* added under ABI 6: a pure addition */
int esr_tile_img_op(const esr_tile_img* p, esr_stream_t stream);   /* added under ABI 6: a pure addition */
int esr_tile_set_x8_op(const esr_tile_set_x8* p, esr_stream_t stream);   /* added under ABI 6: a pure addition */
int esr_tile_hr_op(const esr_tile_hr* p, esr_stream_t stream);     /* added under ABI 6: a pure addition */
int esr_conv_wgrad(const esr_wgrad* p, esr_stream_t stream);
/* n independent weight-gradient problems (disjoint dw/dbias blocks).  fp16 3x3/s1 and 1x1 entries are
 * packed, up to 8 at a time, into ONE launch (at training sizes a single conv's wgrad is ~64
 * mostly-idle workgroups); anything else falls back to esr_conv_wgrad.  esr_run_ops routes every run
 * of consecutive ESR_OP_WGRAD ops through this entry. */
int esr_conv_wgrad_multi(const esr_wgrad* items, int32_t n, esr_stream_t stream);
int esr_batchnorm(const esr_bn* p, esr_stream_t stream);
int esr_maxpool2(const esr_pool* p, esr_stream_t stream);
int esr_linear_op(const esr_linear* p, esr_stream_t stream);
int esr_grad_unpermute(const esr_unpermute* p, esr_stream_t stream);
int esr_adam_step(const esr_adam* p, esr_stream_t stream);
int esr_amp_step(const esr_amp* p, esr_stream_t stream);
int esr_resample_axis(const esr_resample* p, esr_stream_t stream);
int esr_batch_assemble(const esr_batch* p, esr_stream_t stream);   /* added under ABI 6: a pure addition, not an op of esr_run_ops */
int esr_pack_conv_weights_batch(const esr_pack_batch* p, esr_stream_t stream);
/* Fused dense-block chain (replaces 5 x n_blocks esr_conv_forward launches; block.py:260-268,287-291).
 * Every launch assumes its whole grid resident.  Launches on one stream are ordered by the stream; a launch whose
 * grid does not fit next to the chain launches still in flight on OTHER streams is made to wait for them on the
 * device (event wait; the call itself never blocks).  Streams under graph capture are not tracked. */
int esr_rdb_forward(const esr_rdb_chain* p, esr_stream_t stream);
/* Fused dense-block BACKWARD chain (mode 2): the input gradients of n_blocks dense blocks (autograd backward of
 * block.py:260-268,287-291, triggered at SRRaGAN_model.py:140) in one persistent launch — replaces 5 x n_blocks dgrad
 * launches; the weight gradients follow with esr_rdb_wgrad_run over the Q buffers this launch leaves complete. */
int esr_rdb_backward(const esr_rdb_chain* p, esr_stream_t stream);
/* Host-side address check of a chain launch (see esr_g32): every view the kernels would reach must keep the groups of
 * one image below 2^31 bytes from the image base.  blocks_host: a HOST copy of the n_blocks entries p->blocks names on
 * the device, or NULL to check esr_rdb_chain's own views only (what esr_rdb_forward / esr_rdb_backward do themselves).
 * Launches nothing.  ESR_OK, or ESR_ERR_UNSUPPORTED with the view and the limit in esr_last_error(). */
int esr_rdb_chain_check(const esr_rdb_chain* p, const esr_rdb_block* blocks_host);
size_t esr_rdb_mask_bytes(int32_t B, int32_t H, int32_t W);   /* esr_rdb_block.mask of one block */
/* Sticky abort report: 1 if a chain launch — or a follower pass of weight gradients (ESR_OPF_FOLLOW) waiting for one —
 * since the last call gave up on a bounded spin (its results are invalid; e.g. another kernel held CUs for > 1 s), else 0.  Reads a pinned host word: no synchronisation, but only meaningful
 * for launches that have completed.  esr_run_ops / esr_rdb_forward / esr_rdb_backward check it on entry and fail with
 * ESR_ERR_LAUNCH, so an aborted launch cannot go unnoticed past the next call. */
int esr_rdb_check_abort(void);
/* Diagnostic (tests/test_gpu_rdb_chain.py: starved launch): n_workgroups workgroups that each take a CU's LDS and
 * sleep until *release (device-visible memory) becomes non-zero or max_ms (<= 10000) have passed; every workgroup
 * that has started adds 1 to *started (optional). */
int esr_debug_hold_cus(int32_t n_workgroups, const uint32_t* release, uint32_t max_ms, uint32_t* started, esr_stream_t stream);
/* Diagnostic (bench.py `mfma_sustained_probe`; tools/experiments/mfma_power_probe.hip is the stand-alone form): what the
 * matrix pipe sustains under the package power limit.  n_workgroups workgroups of four waves (one per SIMD; one workgroup
 * per CU) each issue iters x 16 independent v_mfma_f32_32x32x16_f16 from registers; operands: 8 x 256 x 16 bytes of fp16
 * (four A and four B fragments per lane: zeros reach the quoted 2.5 PFLOP/s, random values ~1.65 on MI355X).  clk2[0] /
 * clk2[1] = shader-clock / 100 MHz ticks the loop took on workgroup 0; sink: 4 bytes nothing is written to. */
int esr_debug_mfma_probe(const void* operands, int32_t iters, uint64_t* clk2, float* sink, int32_t n_workgroups, esr_stream_t stream);
/* Diagnostic (tests/test_gpu_train_chain.py: a follower without its chain): the follower form of esr_rdb_wgrad_run
 * (ESR_OPF_FOLLOW) against `flags` — tiles_x * tiles_y words per image that the caller controls instead of a chain
 * launch.  A follower whose flags never rise gives up after 2 s, raises the abort word (esr_rdb_check_abort) and runs
 * to its end on whatever is in its inputs. */
int esr_debug_rdb_wgrad_follow(const struct esr_rdb_wgrad* p, const uint32_t* flags, int32_t tiles_x, int32_t tiles_y, esr_stream_t stream);
/* Library state and devices.  What the library keeps between calls — the chain launches in flight (the ordering above),
 * the abort word, the side streams of ESR_OPF_SIDE runs — is keyed by the CURRENT DEVICE of the calling thread:
 * nn.DataParallel's one-thread-per-device replicas (networks.py:105-107) never wait for, or report the aborts of, each
 * other's devices.  Callers on several threads / streams of ONE device share that device's side streams; their fork
 * (event record + wait) is atomic under a per-device mutex, so the sharing is safe (ESR_SIDE_PER_STREAM=1: one set of
 * side streams per caller stream instead — measured slower).
 * Diagnostics for tests on a one-GPU box: esr_debug_device_alias makes the CALLING THREAD's bookkeeping use `alias` in
 * place of hipGetDevice() (alias < 0: back to the real device; returns the previous alias); launches still go to the
 * real device.  esr_debug_chain_order_waits: cross-stream event waits the chain ordering has inserted so far. */
int esr_debug_device_alias(int32_t alias);
uint64_t esr_debug_chain_order_waits(void);
/* The kernel variant the last chain launch of this process ran (tests): ESR_CHAIN_VARIANT_* | rows per wave << 8.
 * REGULAR: the fp16 inference chain built for shapes that are a whole number of 16x32 tiles (H % 16 == 0, W % 32 == 0,
 * no bands, no noise layers; ESR_RDB_GENERAL=1 in the environment keeps the general one).  TRACED: esr_rdb_chain.trace
 * was set — only then do the fp16 chains run the instantiations that carry the trace stamps.
 * This query and esr_debug_chain_force_general are for tests only: ONE process-wide word each (not per device like the
 * rest of the launch bookkeeping), so they mean nothing while several devices or threads launch chains. */
#define ESR_CHAIN_VARIANT_REGULAR 1
#define ESR_CHAIN_VARIANT_TRACED 2
int esr_debug_chain_last_variant(void);
/* In-process form of ESR_RDB_GENERAL (the environment is read once): on = 1 / 0 forces / does not force the general
 * chain whatever the environment says, on < 0 goes back to the environment; returns the previous override (-1: none). */
int esr_debug_chain_force_general(int32_t on);
size_t esr_rdb_workspace_bytes(int32_t B, int32_t H, int32_t W);
size_t esr_rdb_weight_stream_bytes(int32_t dtype);
int esr_rdb_max_tiles_per_image(void);   /* 16x32 tiles of ONE image must not exceed this (= CUs) */
int esr_gather_fragments(const esr_frag_gather* g, esr_stream_t stream);
/* Dense-block weight gradients (replaces 6 x n_blocks esr_conv_wgrad calls). */
int esr_rdb_wgrad_run(const esr_rdb_wgrad* p, esr_stream_t stream);
/* Host-side address check of esr_rdb_wgrad_run on a HOST copy of its block table (see esr_g32): one image of `in` / `q`
 * must end below 2^31 bytes from its base and inside batch_stride, which is at most 2^32 - 16.  Launches nothing. */
int esr_rdb_wgrad_check(const esr_rdb_wgrad* p, const esr_rdb_wgrad_block* blocks_host);
int64_t esr_rdb_wgrad_workspace_elems(int32_t B, int32_t H, int32_t W, int32_t n_blocks);
int esr_image_metrics(const esr_img_metrics* p, esr_stream_t stream);   /* replaces util.py:71-158 on the device */
int esr_image_set_metrics(const esr_set_metrics* p, esr_stream_t stream);   /* added under ABI 6: a pure addition; test.py:69-110 over an image set */

/* The train step's losses with their gradients, one launch each (SRRaGAN_model.py:124-137,150-156).
 * esr_l1_loss_forward: *loss = weight * mean|a - b| (nn.L1Loss, loss.py cri_pix / cri_fea);
 *   grad_a (optional) = weight * sign(a - b) / n.  scratch: 2 doubles of device memory, zero before the first
 *   call (the kernel leaves them zero).
 * esr_l2_loss_forward: *loss = weight * mean (a - b)^2 (nn.MSELoss, cri_pix / cri_fea 'l2': SR_model.py:28-34,
 *   SRRaGAN_model.py:31-53); grad_a (optional) = weight * 2 (a - b) / n.  The same argument struct, the same scratch
 *   (shared with esr_l1_loss_forward: either kernel leaves it zero) and the same meaning of grad_scale /
 *   grad_scale_dev; a - b is formed in fp32, squared and summed in fp64.
 * esr_ragan_loss_forward: *loss = weight/2 * ( BCEWithLogits(x - mean(y), tx) + BCEWithLogits(y - mean(x), ty) )
 *   (GANLoss 'vanilla' on the relativistic-average logits, loss.py:6-38); grad_x / grad_y optional (the means'
 *   dependence on the other side included); mean_x / mean_y optional outputs (the D_real / D_fake log values). */
int esr_l1_loss_forward(const esr_l1_loss* p, esr_stream_t stream);
int esr_l2_loss_forward(const esr_l1_loss* p, esr_stream_t stream);
int esr_ragan_loss_forward(const esr_ragan_loss* p, esr_stream_t stream);
/* esr_gan_loss_forward: GANLoss.forward (loss.py:6-38) of the standard-GAN step (SRGAN_model.py:129-146) on one or two
 *   operands: l(x, t) = mean BCEWithLogits(x, t) (kind 0, 'vanilla') or mean (x - t)^2 (kind 1, 'lsgan') against the
 *   constant label t; *loss = weight * (l(x, tx) [+ l(y, ty)]); grad_x = weight * grad_scale [* grad_scale_dev[0]] *
 *   (sigmoid(x) - tx) / n_x  resp.  ... * 2 (x - tx) / n_x, grad_y alike.  One launch, no scratch. */
int esr_gan_loss_forward(const esr_gan_loss* p, esr_stream_t stream);

/* Run a recorded list of ops back to back on `stream` (one host call per network pass; this is
 * what RRDBNet.forward — architecture.py:76-78 — becomes). */
int esr_run_ops(const esr_op* ops, int32_t n, esr_stream_t stream);
/* floats of esr_wgrad.partial arena the wgrad ops of an op list need (max over the launches esr_run_ops forms) */
int64_t esr_wgrad_workspace_elems(const esr_op* ops, int32_t n);

/* hipGraph replay of an op list (training plans are ~1 000 launches of 10-100 us: per-launch host cost
 * is what bounds the step).  esr_graph_create captures `esr_run_ops(ops, n)` — including its
 * ESR_OPF_SIDE fork/joins — on a library-owned capture stream and instantiates it; every pointer and
 * scalar inside the ops is baked in, so callers keep their I/O in fixed buffers and pass per-step
 * scalars through device memory (esr_conv.seed_dev).  esr_graph_launch enqueues the whole list on
 * `stream` with one host call. */
typedef struct esr_graph_s* esr_graph_t;
int esr_graph_create(const esr_op* ops, int32_t n, esr_graph_t* out);
int esr_graph_launch(esr_graph_t g, esr_stream_t stream);
int esr_graph_destroy(esr_graph_t g);

/* Measurement-only variant (bench.py): brackets every op with hipEvents on `stream`, waits for the
 * stream, and writes each op's elapsed milliseconds to ms_out[n].  This is the one entry point that
 * creates events and synchronises; never call it under graph capture. */
int esr_run_ops_timed(const esr_op* ops, int32_t n, esr_stream_t stream, float* ms_out);

const char* esr_last_error(void);
int esr_abi_version(void);   /* 6 (round 6: ESR_OPF_FOLLOW, esr_debug_rdb_wgrad_follow; esr_dihedral / esr_dihedral_op / ESR_OP_DIHEDRAL, esr_tile / esr_tile_op / ESR_OP_TILE esr_tile_x8 / esr_tile_x8_op / ESR_OP_TILE_X8, esr_fold3 / esr_fold3_op / ESR_OP_FOLD3 with esr_pool modes 4 / 5, esr_batch / esr_batch_item / esr_batch_assemble, esr_tile_many / esr_tile_item / esr_tile_many_op / ESR_OP_TILE_MANY, esr_tile_img / esr_tile_img_item / esr_tile_img_op / ESR_OP_TILE_IMG, esr_tile_hr / esr_tile_hr_item / esr_tile_hr_desc / esr_tile_hr_op / ESR_OP_TILE_HR, and esr_set_metrics / esr_set_metrics_item / esr_image_set_metrics were added later under 6: no existing struct or entry changed); 5 (round 5: esr_rdb_wgrad.max_workgroups, esr_debug_device_alias / esr_debug_chain_order_waits); 4 (round 4: esr_conv.ksplit / split_ws / stat_sums, ESR_BN_FIN_APPLY / ESR_BN_RESTAT); 3 (round 3: esr_ragan_loss.mode / sums / ext, ...; 2 = round 2: esr_bn.groups / num_batches_tracked,
                                esr_l1_loss, esr_ragan_loss, ESR_OPF_SIDE_FREE) */
size_t esr_sizeof_op(void);

#ifdef __cplusplus
}
#endif
#endif /* ESRGAN_HIP_H */
