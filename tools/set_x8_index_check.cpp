// set_x8_index_check.cpp — a host program over csrc/tile_geom.h and csrc/tile_x8_index.h, the geometry, the window
// resolvers and the index and accumulator arithmetic of the x8 ends (esr_dihedral, esr_tile_x8, esr_tile_set_x8): it
// walks the two kernel bodies' workgroups and lanes on the CPU for each of the three resolvers — by table, per image
// (B = 2, tail passes included) and the whole image — in exactly sized heap buffers, with a nearest-neighbour "net"
// between them (equivariant under the eight transforms, so every R_k(o_k) is the upsampled window), and checks that every
// slot pixel is written once with the transform's value, that every result pixel of every image is written once with the
// right value and nothing else is, that the result does not depend on how the eight slots are split, and that acc is
// touched only when the protocol says so (a null acc where it must not be).  The 8-bit result form is walked by table
// only: esr_tile_set_x8 is the one op that has it.
// Built and run by hand, on the CPU, with the sanitizers that find an index out of bounds:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/set_x8_index_check.cpp -o set_x8_index_check
//   ./set_x8_index_check
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../esrganplus_amd/csrc/tile_geom.h"
#include "../esrganplus_amd/csrc/tile_x8_index.h"

namespace {

int imin(int a, int b) { return a < b ? a : b; }

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the byte a pixel of an image holds in channel c: the images are bytes so that the 8-bit form is exact too
int pixel(int image, int c, int y, int x) { return (image * 53 + c * 101 + y * 37 + x * 11) % 256; }
float unit(int b) { return (float)b / 255.0f; }
unsigned quant8(float v) { return (unsigned)(int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// One pass as the walk sees it: a resolver R of tile_geom.h over P windows (the grid's z), and which image of the case a
// window's base pointer names (the resolvers' pointers go into exactly sized arrays, one element or one image each).
template <typename R>
struct Pass {
  R r;
  int P, C;
  int goh, gow;                                  // the largest owned rectangle, LR pixels: what the entry sizes the grid by
  int (*image_of)(const Pass&, const TileWin&);
  const float* base;                             // of the array the pointers go into
  int64_t stride;                                // elements of one image in it
};
template <typename R>
int image_of_base(const Pass<R>& ps, const TileWin& w) {
  const int64_t d = (const float*)w.img - ps.base;
  CHECK(d >= 0 && d % ps.stride == 0, "an image base %lld elements in, images of %lld", (long long)d, (long long)ps.stride);
  return (int)(d / ps.stride);
}

// The gather-import of one pass: slots[i][p] is a [C][sh][sw] plane set, exactly sized; counts the writes per pixel.
template <typename R>
void gather(const Pass<R>& ps, int k_begin, int k_count, std::vector<std::vector<float>>& slots, std::vector<std::vector<int>>& hits) {
  const int P = ps.P, C = ps.C, th = ps.r.th, tw = ps.r.tw;
  slots.assign((size_t)k_count * P, std::vector<float>((size_t)C * th * tw, -1.f));
  hits.assign((size_t)k_count * P, std::vector<int>((size_t)th * tw, 0));
  for (int z = 0; z < P; ++z) {
    const TileWin w = R::gather(ps.r, z);              // fillers and repeated windows are gathered like any other
    const int image = ps.image_of(ps, w);
    CHECK(w.ay.w0 >= 0 && w.ay.w0 + th <= w.H && w.ax.w0 >= 0 && w.ax.w0 + tw <= w.W, "window %d at (%d, %d) of a %d x %d image", z, w.ay.w0, w.ax.w0, w.H, w.W);
    for (int by = 0; by < (th + X8_TILE - 1) / X8_TILE; ++by)
      for (int bx = 0; bx < (tw + X8_TILE - 1) / X8_TILE; ++bx)
        for (int i = 0; i < k_count; ++i)
          for (int lane = 0; lane < X8_TILE * X8_TILE; ++lane) {
            const int k = k_begin + i, lx = lane & 31, ly = lane >> 5;
            const bool tr = (k & 4) != 0;
            const int sy = by * X8_TILE + (tr ? lx : ly), sx = bx * X8_TILE + (tr ? ly : lx);
            if (sy >= th || sx >= tw) continue;
            const X8Pos at = x8_gather_pos(k, th, tw, sy, sx);
            const int sh = tr ? tw : th, sw = tr ? th : tw;
            CHECK(at.row >= 0 && at.row < sh && at.col >= 0 && at.col < sw, "slot pixel (%d, %d) of a %d x %d slot", at.row, at.col, sh, sw);
            const int64_t e = x8_entry(i, P, z);
            for (int c = 0; c < C; ++c)
              slots.at(e).at(((size_t)c * sh + at.row) * sw + at.col) = unit(pixel(image, c, w.ay.w0 + sy, w.ax.w0 + sx));
            ++hits.at(e).at((size_t)at.row * sw + at.col);
          }
    // every pixel of every slot once, and slot_k = the transform of the window by its definition
    for (int i = 0; i < k_count; ++i) {
      const int k = k_begin + i;
      const bool tr = (k & 4) != 0;
      const int sh = tr ? tw : th, sw = tr ? th : tw;
      for (int r = 0; r < sh; ++r)
        for (int q = 0; q < sw; ++q) {
          CHECK(hits[x8_entry(i, P, z)][(size_t)r * sw + q] == 1, "k %d window %d pixel (%d, %d) written %d times", k, z, r, q,
                hits[x8_entry(i, P, z)][(size_t)r * sw + q]);
          // x8_transform: flip along W (bit 0), along H (bit 1), then transpose (bit 2)
          const int y = tr ? q : r, x = tr ? r : q;
          const int wy = (k & 2) ? th - 1 - y : y, wx = (k & 1) ? tw - 1 - x : x;
          for (int c = 0; c < C; ++c)
            CHECK(slots[x8_entry(i, P, z)][((size_t)c * sh + r) * sw + q] == unit(pixel(image, c, w.ay.w0 + wy, w.ax.w0 + wx)),
                  "k %d window %d pixel (%d, %d) channel %d", k, z, r, q, c);
        }
    }
  }
}

// nearest xS of every slot: [C][S sh][S sw]
std::vector<float> upsample(const std::vector<float>& s, int C, int sh, int sw, int S) {
  std::vector<float> o((size_t)C * S * S * sh * sw);
  for (int c = 0; c < C; ++c)
    for (int y = 0; y < S * sh; ++y)
      for (int x = 0; x < S * sw; ++x) o[((size_t)c * S * sh + y) * S * sw + x] = s[((size_t)c * sh + y / S) * sw + x / S];
  return o;
}

struct Results {
  std::vector<std::vector<float>> f;            // img = 0: [C][SH][SW] per image
  std::vector<std::vector<unsigned char>> u;    // img = 1: [SH][SW][C]
  std::vector<std::vector<int>> hits;           // writes per result pixel
};

// The stitch-reduce of one range of one pass, lane by lane; acc may be null.  S = R::SCALE: the result's side.
template <typename R>
void reduce(const Pass<R>& ps, int k_begin, int k_count, int accumulate, float mean_scale, int img, int bgr,
            const std::vector<std::vector<float>>& outs, float* acc, size_t acc_elems, Results& res) {
  constexpr int S = R::SCALE;
  const int P = ps.P, C = ps.C, th = ps.r.th, tw = ps.r.tw, hh = S * th, hw = S * tw;
  for (int z = 0; z < P; ++z) {
    const TileWin w = R::stitch(ps.r, z);
    if (!w.live) continue;
    const int image = ps.image_of(ps, w);
    const TileAxis ay = w.ay, ax = w.ax;
    const int oh = S * ay.on, ow = S * ax.on, wy = S * (ay.o0 - ay.w0), wx = S * (ax.o0 - ax.w0);
    CHECK(ay.on <= ps.goh && ax.on <= ps.gow, "an owned rectangle %d x %d larger than the grid's %d x %d", ay.on, ax.on, ps.goh, ps.gow);
    for (int by = 0; by < (S * ps.goh + X8_TILE - 1) / X8_TILE; ++by)
      for (int bx = 0; bx < (S * ps.gow + X8_TILE - 1) / X8_TILE; ++bx) {
        const int x0 = bx * X8_TILE, y0 = by * X8_TILE;
        if (x0 >= ow || y0 >= oh) continue;
        std::vector<unsigned char> bytes((size_t)X8_TILE * X8_TILE * C, 0xEE);     // the workgroup's LDS rows
        for (int lane = 0; lane < X8_TILE * X8_TILE; ++lane) {
          const int lx = lane & 31, ly = lane >> 5;
          if (!(y0 + ly < oh && x0 + lx < ow)) continue;
          const int y = wy + y0 + ly, x = wx + x0 + lx;        // window-local result pixel
          const int Y = S * ay.o0 + y0 + ly, X = S * ax.o0 + x0 + lx;
          for (int c = 0; c < C; ++c) {
            float a = 0.f;
            if (accumulate) {
              if (img) {
                const int64_t o = x8_acc_offset(z, c, C, hh, hw, y, x);
                CHECK(x8_acc_read(img, accumulate) && acc && o >= 0 && (size_t)o < acc_elems, "acc read at %lld of %zu", (long long)o, acc_elems);
                a = acc[o];
              } else {
                a = res.f.at(image).at(((size_t)c * S * w.H + Y) * S * w.W + X);
              }
            }
            for (int i = 0; i < k_count; ++i) {
              const int64_t o = x8_reduce_src(k_begin + i, hh, hw, y, x);
              CHECK(o >= 0 && o < (int64_t)hh * hw, "slot offset %lld of %d", (long long)o, hh * hw);
              const X8Pos at = x8_reduce_pos(k_begin + i, hh, hw, y, x);     // what a G32 slot is read at
              const bool tr = ((k_begin + i) & 4) != 0;
              CHECK(at.row >= 0 && at.row < (tr ? hw : hh) && at.col >= 0 && at.col < (tr ? hh : hw) && o == (int64_t)at.row * (tr ? hh : hw) + at.col,
                    "slot pixel (%d, %d) at offset %lld", at.row, at.col, (long long)o);
              const float v = outs.at(x8_entry(i, P, z)).at((size_t)c * hh * hw + o);
              a = (i == 0 && !accumulate) ? v : a + v;
            }
            a *= mean_scale;
            if (!img) {
              res.f.at(image).at(((size_t)c * S * w.H + Y) * S * w.W + X) = a;
            } else if (x8_acc_write(img, k_begin, k_count)) {
              const int64_t o = x8_acc_offset(z, c, C, hh, hw, y, x);
              CHECK(acc && o >= 0 && (size_t)o < acc_elems, "acc write at %lld of %zu", (long long)o, acc_elems);
              acc[o] = a;
            } else {
              bytes.at(((size_t)ly * X8_TILE + lx) * C + ((bgr && C == 3) ? 2 - c : c)) = (unsigned char)quant8(a);
            }
          }
          if (x8_last_range(k_begin, k_count)) ++res.hits.at(image).at((size_t)Y * S * w.W + X);
        }
        if (img && x8_last_range(k_begin, k_count)) {
          const int n = ow - x0 < X8_TILE ? ow - x0 : X8_TILE;
          CHECK(n % 4 == 0 && (n * C) % 4 == 0, "%d owned pixels of a row", n);
          for (int lane = 0; lane < X8_TILE * X8_TILE; ++lane) {
            const int lx = lane & 31, ly = lane >> 5;
            if (!(y0 + ly < oh && lx < x8_row_dwords(n, C))) continue;
            const int64_t row = ((int64_t)(S * ay.o0 + y0 + ly) * (S * w.W) + S * ax.o0 + x0) * C;
            CHECK(row % 4 == 0, "a row of dwords at byte %lld", (long long)row);
            for (int b = 0; b < 4; ++b)      // one aligned dword
              res.u.at(image).at((size_t)row + 4 * lx + b) = bytes.at(((size_t)ly * (X8_TILE * C / 4) + lx) * 4 + b);
          }
        }
      }
  }
}

// All eight transforms of one pass, `slots` at a time: gather, the net, reduce.  ps: the gather's side, st: the stitch's
// (the same resolver, except per image, where each launch has the image of its own side).
template <typename R>
void run_pass(const Pass<R>& ps, const Pass<R>& st, int slots, int img, int bgr, float* acc, size_t acc_elems, Results& res) {
  const int th = ps.r.th, tw = ps.r.tw;
  for (int k0 = 0; k0 < 8; k0 += slots) {
    CHECK(x8_range_error(k0, slots, th, tw) == 0, "range [%d, %d) of a %d x %d window", k0, k0 + slots, th, tw);
    CHECK(x8_acc_needed(img, k0 > 0, k0, slots) == (acc != nullptr), "acc needed at [%d, %d)", k0, k0 + slots);
    std::vector<std::vector<float>> sl, outs;
    std::vector<std::vector<int>> hits;
    gather(ps, k0, slots, sl, hits);
    for (int i = 0; i < slots; ++i)
      for (int z = 0; z < ps.P; ++z) {
        const bool tr = ((k0 + i) & 4) != 0;
        outs.push_back(upsample(sl[x8_entry(i, ps.P, z)], ps.C, tr ? tw : th, tr ? th : tw, R::SCALE));
      }
    reduce(st, k0, slots, k0 > 0, k0 + slots == 8 ? 0.125f : 1.0f, img, bgr, outs, acc, acc_elems, res);
  }
}

// every result pixel of image j (H x W on the LR side, S the result's scale) once, with the upsampled pixel if the image
// is `mine`; everything else untouched
void check_image(const Results& res, size_t j, int H, int W, int S, int C, bool mine, int img, int bgr) {
  for (int Y = 0; Y < S * H; ++Y)
    for (int X = 0; X < S * W; ++X) {
      CHECK(res.hits[j][(size_t)Y * S * W + X] == (mine ? 1 : 0), "image %zu result pixel (%d, %d) written %d times", j, Y, X, res.hits[j][(size_t)Y * S * W + X]);
      for (int c = 0; c < C; ++c) {
        const float v = unit(pixel((int)j, c, Y / S, X / S));
        float mean = v;                                   // eight equal terms, summed as the kernel sums them
        for (int k = 1; k < 8; ++k) mean += v;
        mean *= 0.125f;
        if (img) CHECK(res.u[j][((size_t)Y * S * W + X) * C + ((bgr && C == 3) ? 2 - c : c)] == (mine ? quant8(mean) : 0xAB), "image %zu byte (%d, %d, %d)", j, Y, X, c);
        else CHECK(res.f[j][((size_t)c * S * H + Y) * S * W + X] == (mine ? mean : -7.f), "image %zu value (%d, %d, %d)", j, Y, X, c);
      }
    }
}

void add_image(Results& res, int H, int W, int S, int C) {
  res.f.emplace_back((size_t)C * S * S * H * W, -7.f);
  res.u.emplace_back((size_t)C * S * S * H * W, 0xAB);
  res.hits.emplace_back((size_t)S * S * H * W, 0);
}

// The table resolver (esr_tile_set_x8): images of several sizes, passes of P windows, fillers in the last.
void run_table(const std::vector<std::pair<int, int>>& sizes, int C, int tile, int pad, int P, int split, int img, int bgr) {
  std::vector<float> tags(sizes.size());         // an item's pointer names its image: one element each
  // group by window shape, as functional.tiled_many_x8_passes does
  for (size_t first = 0; first < sizes.size(); ++first) {
    const int th = tile_window(sizes[first].first, tile, pad), tw = tile_window(sizes[first].second, tile, pad);
    bool seen = false;
    for (size_t j = 0; j < first; ++j)
      seen = seen || (tile_window(sizes[j].first, tile, pad) == th && tile_window(sizes[j].second, tile, pad) == tw);
    if (seen) continue;
    std::vector<esr_tile_item> wins;
    for (size_t j = first; j < sizes.size(); ++j) {
      const int H = sizes[j].first, W = sizes[j].second;
      if (tile_window(H, tile, pad) != th || tile_window(W, tile, pad) != tw) continue;
      for (int t = 0; t < tile_count(H, tile) * tile_count(W, tile); ++t) wins.push_back({&tags[j], H, W, t, 1});
    }
    const int slots = (th != tw && split > 4) ? 4 : split;
    Results res;
    for (auto& s : sizes) add_image(res, s.first, s.second, 4, C);
    const size_t acc_elems = (size_t)P * C * 16 * th * tw;
    float* const acc = (img && slots < 8) ? (float*)malloc(acc_elems * sizeof(float)) : nullptr;   // exactly sized, or none
    for (size_t at = 0; at < wins.size(); at += P) {
      std::vector<esr_tile_item> pass(wins.begin() + at, wins.begin() + imin((int)wins.size(), (int)at + P));
      while ((int)pass.size() < P) { pass.push_back(wins.back()); pass.back().live = 0; }
      const Pass<TileTable> ps{TileTable{pass.data(), tile, pad, th, tw}, P, C, imin(tile, th), imin(tile, tw), image_of_base<TileTable>, tags.data(), 1};
      run_pass(ps, ps, slots, img, bgr, acc, acc_elems, res);
    }
    free(acc);
    for (size_t j = 0; j < sizes.size(); ++j) {
      const int H = sizes[j].first, W = sizes[j].second;
      check_image(res, j, H, W, 4, C, tile_window(H, tile, pad) == th && tile_window(W, tile, pad) == tw, img, bgr);
    }
  }
}

// The per-image resolver (esr_tile_x8): B images of one size, passes of t_count tiles; the last pass runs beyond the
// last tile when t_count does not divide the tile count: its repeated windows are gathered and not stitched.
void run_per_image(int H, int W, int B, int C, int tile, int pad, int t_count, int split) {
  const int th = tile_window(H, tile, pad), tw = tile_window(W, tile, pad), nx = tile_count(W, tile), ntiles = tile_count(H, tile) * nx;
  const int slots = (th != tw && split > 4) ? 4 : split;
  std::vector<float> lr((size_t)B * C * H * W), hr((size_t)B * C * 16 * H * W);   // what nchw names on each side
  Results res;
  for (int b = 0; b < B; ++b) add_image(res, H, W, 4, C);
  bool tail = false;
  for (int t_begin = 0; t_begin < ntiles; t_begin += t_count) {
    tail = tail || t_begin + t_count > ntiles;
    // the gather's op has the LR image, the stitch's the HR one: two resolvers, as the two launches have
    const Pass<TilePerImage> g{TilePerImage{lr.data(), B, C, H, W, tile, pad, t_begin, th, tw, nx, ntiles}, t_count * B, C,
                               imin(tile, H), imin(tile, W), image_of_base<TilePerImage>, lr.data(), (int64_t)C * H * W};
    const Pass<TilePerImage> s{TilePerImage{hr.data(), B, C, 4 * H, 4 * W, tile, pad, t_begin, th, tw, nx, ntiles}, t_count * B, C,
                               imin(tile, H), imin(tile, W), image_of_base<TilePerImage>, hr.data(), (int64_t)C * 16 * H * W};
    for (int z = 0; z < t_count * B; ++z) {
      const TileWin wg = TilePerImage::gather(g.r, z), ws = TilePerImage::stitch(s.r, z);
      const int t = t_begin + z / B;
      CHECK(wg.t == imin(t, ntiles - 1) && ws.live == (t < ntiles) && (!ws.live || ws.t == t) && ws.H == H && ws.W == W,
            "tile %d of %d: gathered as %d, stitched as %d (live %d) of a %d x %d image", t, ntiles, wg.t, ws.t, ws.live, ws.H, ws.W);
    }
    run_pass(g, s, slots, 0, 0, nullptr, 0, res);
  }
  CHECK(tail == (ntiles % t_count != 0), "a tail pass of %d tiles in passes of %d", ntiles, t_count);
  for (int b = 0; b < B; ++b) check_image(res, b, H, W, 4, C, true, 0, 0);
}

// The whole-image resolver (esr_dihedral): B images, no tiles, the result at the scale of the op's own H x W.
void run_whole(int H, int W, int B, int C, int split) {
  const int slots = (H != W && split > 4) ? 4 : split;
  std::vector<float> io((size_t)B * C * H * W);
  Results res;
  for (int b = 0; b < B; ++b) add_image(res, H, W, 1, C);
  const Pass<TileWhole> ps{TileWhole{io.data(), C, H, W}, B, C, H, W, image_of_base<TileWhole>, io.data(), (int64_t)C * H * W};
  run_pass(ps, ps, slots, 0, 0, nullptr, 0, res);
  for (int b = 0; b < B; ++b) check_image(res, b, H, W, 1, C, true, 0, 0);
}

}  // namespace

int main() {
  const std::vector<std::pair<int, int>> sizes = {{24, 24}, {40, 52}, {33, 70}, {21, 37}, {24, 24}, {1, 1}, {5, 3}};
  int cases = 0;
  for (int img = 0; img < 2; ++img)
    for (int C : {1, 3, 8})
      for (auto tp : {std::pair<int, int>{16, 4}, {32, 8}, {7, 0}, {96, 16}})
        for (int split : {8, 4, 2, 1})
          for (int P : {1, 3}) {
            if ((img && C == 8) || (P == 1 && split != 8)) continue;
            run_table(sizes, C, tp.first, tp.second, P, split, img, img && C == 3 && split != 4);
            ++cases;
          }
  // per image: 13 x 21 at tile 8 has 2 x 3 tiles, 20 x 26 has 3 x 4: passes of 4 leave a tail in the first, of 5 in both
  for (auto hw : {std::pair<int, int>{13, 21}, {20, 26}, {12, 12}, {5, 40}})
    for (int B : {1, 2})
      for (int C : {1, 3})
        for (auto tp : {std::pair<int, int>{8, 2}, {16, 4}})
          for (int t_count : {1, 4, 5})
            for (int split : {8, 2}) {
              run_per_image(hw.first, hw.second, B, C, tp.first, tp.second, t_count, split);
              ++cases;
            }
  // the whole image: square ones take all eight at once, the others k 0..3 and 4..7 (split 8 becomes 4) or less
  for (auto hw : {std::pair<int, int>{13, 21}, {20, 26}, {40, 33}, {24, 24}, {35, 35}, {1, 1}})
    for (int B : {1, 2})
      for (int C : {3, 8})
        for (int split : {8, 4, 2, 1}) {
          run_whole(hw.first, hw.second, B, C, split);
          ++cases;
        }
  // the refusals of a k range
  if (x8_range_error(-1, 2, 8, 8) != 1 || x8_range_error(0, 0, 8, 8) != 1 || x8_range_error(7, 2, 8, 8) != 1 ||
      x8_range_error(0, 8, 8, 9) != 2 || x8_range_error(2, 4, 9, 8) != 2 || x8_range_error(0, 8, 8, 8) != 0 ||
      x8_range_error(0, 4, 8, 9) != 0 || x8_range_error(4, 4, 8, 9) != 0 || x8_range_error(2147483647, 2147483647, 8, 8) != 1)
    ++failures, printf("FAILED: x8_range_error\n");
  if (x8_acc_needed(0, 1, 4, 4) || x8_acc_needed(1, 0, 0, 8) || !x8_acc_needed(1, 0, 0, 4) || !x8_acc_needed(1, 1, 4, 4))
    ++failures, printf("FAILED: x8_acc_needed\n");
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
