// set_x8_index_check.cpp — a host program over csrc/tile_set_x8_index.h, the index and accumulator arithmetic of
// esr_tile_set_x8: it walks the two kernels' workgroups and lanes on the CPU, in exactly sized heap buffers, with a
// nearest-x4 "net" between them (equivariant under the eight transforms, so every R_k(o_k) is the upsampled window),
// and checks that every slot pixel is written once with the transform's value, that every HR pixel
// of every image is written once with the right value and nothing else is, that the result does not depend on how the
// eight slots are split, and that acc is touched only when the protocol says so (a null acc where it must not be).
// Built and run by hand, on the CPU, with the sanitizers that find an index out of bounds:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/set_x8_index_check.cpp -o set_x8_index_check
//   ./set_x8_index_check
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../esrganplus_amd/csrc/tile_set_x8_index.h"

namespace {

// include/esrgan_hip.h (esr_tile), restated: one axis of tile i of an image of n, window of `win`
struct Axis { int o0, on, w0; };
Axis axis(int n, int tile, int pad, int win, int i) {
  Axis a;
  a.o0 = i * tile;
  a.on = n - a.o0 < tile ? n - a.o0 : tile;
  const int w = a.o0 - pad;
  a.w0 = w < 0 ? 0 : (w > n - win ? n - win : w);
  return a;
}
int imin(int a, int b) { return a < b ? a : b; }

struct Item { int image, H, W, t, live; };

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the byte a pixel of an image holds in channel c: the images are bytes so that the 8-bit form is exact too
int pixel(int image, int c, int y, int x) { return (image * 53 + c * 101 + y * 37 + x * 11) % 256; }
float unit(int b) { return (float)b / 255.0f; }
unsigned quant8(float v) { return (unsigned)(int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// The gather-import of one pass: slots[i][p] is a [C][sh][sw] plane set, exactly sized; counts the writes per pixel.
void gather(const std::vector<Item>& items, int C, int tile, int pad, int th, int tw, int k_begin, int k_count,
            std::vector<std::vector<float>>& slots, std::vector<std::vector<int>>& hits) {
  const int P = (int)items.size();
  slots.assign((size_t)k_count * P, std::vector<float>((size_t)C * th * tw, -1.f));
  hits.assign((size_t)k_count * P, std::vector<int>((size_t)th * tw, 0));
  for (int w = 0; w < P; ++w) {
    const Item& it = items[w];
    const int nx = (it.W - 1) / tile + 1;
    const Axis ay = axis(it.H, tile, pad, th, it.t / nx), ax = axis(it.W, tile, pad, tw, it.t % nx);
    for (int by = 0; by < (th + SX8_TILE - 1) / SX8_TILE; ++by)
      for (int bx = 0; bx < (tw + SX8_TILE - 1) / SX8_TILE; ++bx)
        for (int i = 0; i < k_count; ++i)
          for (int lane = 0; lane < SX8_TILE * SX8_TILE; ++lane) {
            const int k = k_begin + i, lx = lane & 31, ly = lane >> 5;
            const bool tr = (k & 4) != 0;
            const int sy = by * SX8_TILE + (tr ? lx : ly), sx = bx * SX8_TILE + (tr ? ly : lx);
            if (sy >= th || sx >= tw) continue;
            const SX8Pos at = sx8_gather_pos(k, th, tw, sy, sx);
            const int sh = tr ? tw : th, sw = tr ? th : tw;
            CHECK(at.row >= 0 && at.row < sh && at.col >= 0 && at.col < sw, "slot pixel (%d, %d) of a %d x %d slot", at.row, at.col, sh, sw);
            const int64_t e = sx8_entry(i, P, w);
            for (int c = 0; c < C; ++c)
              slots.at(e).at(((size_t)c * sh + at.row) * sw + at.col) = unit(pixel(it.image, c, ay.w0 + sy, ax.w0 + sx));
            ++hits.at(e).at((size_t)at.row * sw + at.col);
          }
  }
  // every pixel of every slot once, and slot_k = the transform of the window by its definition
  for (int i = 0; i < k_count; ++i)
    for (int w = 0; w < P; ++w) {
      const int k = k_begin + i;
      const bool tr = (k & 4) != 0;
      const int sh = tr ? tw : th, sw = tr ? th : tw;
      const Item& it = items[w];
      const int nx = (it.W - 1) / tile + 1;
      const Axis ay = axis(it.H, tile, pad, th, it.t / nx), ax = axis(it.W, tile, pad, tw, it.t % nx);
      for (int r = 0; r < sh; ++r)
        for (int q = 0; q < sw; ++q) {
          CHECK(hits[sx8_entry(i, P, w)][(size_t)r * sw + q] == 1, "k %d window %d pixel (%d, %d) written %d times", k, w, r, q,
                hits[sx8_entry(i, P, w)][(size_t)r * sw + q]);
          // x8_transform: flip along W (bit 0), along H (bit 1), then transpose (bit 2)
          const int y = tr ? q : r, x = tr ? r : q;
          const int wy = (k & 2) ? th - 1 - y : y, wx = (k & 1) ? tw - 1 - x : x;
          for (int c = 0; c < C; ++c)
            CHECK(slots[sx8_entry(i, P, w)][((size_t)c * sh + r) * sw + q] == unit(pixel(it.image, c, ay.w0 + wy, ax.w0 + wx)),
                  "k %d window %d pixel (%d, %d) channel %d", k, w, r, q, c);
        }
    }
}

// nearest x4 of every slot: [C][4 sh][4 sw]
std::vector<float> upsample(const std::vector<float>& s, int C, int sh, int sw) {
  std::vector<float> o((size_t)C * 16 * sh * sw);
  for (int c = 0; c < C; ++c)
    for (int y = 0; y < 4 * sh; ++y)
      for (int x = 0; x < 4 * sw; ++x) o[((size_t)c * 4 * sh + y) * 4 * sw + x] = s[((size_t)c * sh + y / 4) * sw + x / 4];
  return o;
}

struct Results {
  std::vector<std::vector<float>> f;            // img = 0: [C][4H][4W] per image
  std::vector<std::vector<unsigned char>> u;    // img = 1: [4H][4W][C]
  std::vector<std::vector<int>> hits;           // writes per HR pixel
};

// The stitch-reduce of one range of one pass, lane by lane; acc may be null.
void reduce(const std::vector<Item>& items, int C, int tile, int pad, int th, int tw, int k_begin, int k_count, int accumulate,
            float mean_scale, int img, int bgr, const std::vector<std::vector<float>>& outs, float* acc, size_t acc_elems, Results& res) {
  const int P = (int)items.size(), hh = 4 * th, hw = 4 * tw;
  const int gow = imin(tile, tw), goh = imin(tile, th);
  for (int w = 0; w < P; ++w) {
    const Item& it = items[w];
    if (!it.live) continue;
    const int nx = (it.W - 1) / tile + 1;
    const Axis ay = axis(it.H, tile, pad, th, it.t / nx), ax = axis(it.W, tile, pad, tw, it.t % nx);
    const int oh = 4 * ay.on, ow = 4 * ax.on, wy = 4 * (ay.o0 - ay.w0), wx = 4 * (ax.o0 - ax.w0);
    CHECK(ay.on <= goh && ax.on <= gow, "an owned rectangle %d x %d larger than the grid's %d x %d", ay.on, ax.on, goh, gow);
    for (int by = 0; by < (4 * goh + SX8_TILE - 1) / SX8_TILE; ++by)
      for (int bx = 0; bx < (4 * gow + SX8_TILE - 1) / SX8_TILE; ++bx) {
        const int x0 = bx * SX8_TILE, y0 = by * SX8_TILE;
        if (x0 >= ow || y0 >= oh) continue;
        std::vector<unsigned char> bytes((size_t)SX8_TILE * SX8_TILE * C, 0xEE);     // the workgroup's LDS rows
        for (int lane = 0; lane < SX8_TILE * SX8_TILE; ++lane) {
          const int lx = lane & 31, ly = lane >> 5;
          if (!(y0 + ly < oh && x0 + lx < ow)) continue;
          const int y = wy + y0 + ly, x = wx + x0 + lx;        // window-local HR pixel
          const int Y = 4 * ay.o0 + y0 + ly, X = 4 * ax.o0 + x0 + lx;
          for (int c = 0; c < C; ++c) {
            float a = 0.f;
            if (accumulate) {
              if (img) {
                const int64_t o = sx8_acc_offset(w, c, C, hh, hw, y, x);
                CHECK(sx8_acc_read(img, accumulate) && acc && o >= 0 && (size_t)o < acc_elems, "acc read at %lld of %zu", (long long)o, acc_elems);
                a = acc[o];
              } else {
                a = res.f.at(it.image).at(((size_t)c * 4 * it.H + Y) * 4 * it.W + X);
              }
            }
            for (int i = 0; i < k_count; ++i) {
              const int64_t o = sx8_reduce_src(k_begin + i, hh, hw, y, x);
              CHECK(o >= 0 && o < (int64_t)hh * hw, "slot offset %lld of %d", (long long)o, hh * hw);
              const float v = outs.at(sx8_entry(i, P, w)).at((size_t)c * hh * hw + o);
              a = (i == 0 && !accumulate) ? v : a + v;
            }
            a *= mean_scale;
            if (!img) {
              res.f.at(it.image).at(((size_t)c * 4 * it.H + Y) * 4 * it.W + X) = a;
            } else if (sx8_acc_write(img, k_begin, k_count)) {
              const int64_t o = sx8_acc_offset(w, c, C, hh, hw, y, x);
              CHECK(acc && o >= 0 && (size_t)o < acc_elems, "acc write at %lld of %zu", (long long)o, acc_elems);
              acc[o] = a;
            } else {
              bytes.at(((size_t)ly * SX8_TILE + lx) * C + ((bgr && C == 3) ? 2 - c : c)) = (unsigned char)quant8(a);
            }
          }
          if (sx8_last_range(k_begin, k_count)) ++res.hits.at(it.image).at((size_t)Y * 4 * it.W + X);
        }
        if (img && sx8_last_range(k_begin, k_count)) {
          const int n = ow - x0 < SX8_TILE ? ow - x0 : SX8_TILE;
          CHECK(n % 4 == 0 && (n * C) % 4 == 0, "%d owned pixels of a row", n);
          for (int lane = 0; lane < SX8_TILE * SX8_TILE; ++lane) {
            const int lx = lane & 31, ly = lane >> 5;
            if (!(y0 + ly < oh && lx < sx8_row_dwords(n, C))) continue;
            const int64_t row = ((int64_t)(4 * ay.o0 + y0 + ly) * (4 * it.W) + 4 * ax.o0 + x0) * C;
            CHECK(row % 4 == 0, "a row of dwords at byte %lld", (long long)row);
            for (int b = 0; b < 4; ++b)      // one aligned dword
              res.u.at(it.image).at((size_t)row + 4 * lx + b) = bytes.at(((size_t)ly * (SX8_TILE * C / 4) + lx) * 4 + b);
          }
        }
      }
  }
}

void run_case(const std::vector<std::pair<int, int>>& sizes, int C, int tile, int pad, int P, int split, int img, int bgr) {
  // group by window shape, as functional.tiled_many_x8_passes does
  for (size_t first = 0; first < sizes.size(); ++first) {
    const int th = imin(tile + 2 * pad, sizes[first].first), tw = imin(tile + 2 * pad, sizes[first].second);
    bool seen = false;
    for (size_t j = 0; j < first; ++j)
      seen = seen || (imin(tile + 2 * pad, sizes[j].first) == th && imin(tile + 2 * pad, sizes[j].second) == tw);
    if (seen) continue;
    std::vector<Item> wins;
    for (size_t j = first; j < sizes.size(); ++j) {
      const int H = sizes[j].first, W = sizes[j].second;
      if (imin(tile + 2 * pad, H) != th || imin(tile + 2 * pad, W) != tw) continue;
      for (int t = 0; t < ((H - 1) / tile + 1) * ((W - 1) / tile + 1); ++t) wins.push_back({(int)j, H, W, t, 1});
    }
    const int slots = (th != tw && split > 4) ? 4 : split;
    Results res;
    for (auto& s : sizes) {
      res.f.emplace_back((size_t)C * 16 * s.first * s.second, -7.f);
      res.u.emplace_back((size_t)C * 16 * s.first * s.second, 0xAB);
      res.hits.emplace_back((size_t)16 * s.first * s.second, 0);
    }
    const size_t acc_elems = (size_t)P * C * 16 * th * tw;
    float* const acc = (img && slots < 8) ? (float*)malloc(acc_elems * sizeof(float)) : nullptr;   // exactly sized, or none
    for (size_t at = 0; at < wins.size(); at += P) {
      std::vector<Item> pass(wins.begin() + at, wins.begin() + imin((int)wins.size(), (int)at + P));
      while ((int)pass.size() < P) { pass.push_back(wins.back()); pass.back().live = 0; }
      for (int k0 = 0; k0 < 8; k0 += slots) {
        CHECK(sx8_range_error(k0, slots, th, tw) == 0, "range [%d, %d) of a %d x %d window", k0, k0 + slots, th, tw);
        CHECK(sx8_acc_needed(img, k0 > 0, k0, slots) == (acc != nullptr), "acc needed at [%d, %d)", k0, k0 + slots);
        std::vector<std::vector<float>> sl, outs;
        std::vector<std::vector<int>> hits;
        gather(pass, C, tile, pad, th, tw, k0, slots, sl, hits);
        for (int i = 0; i < slots; ++i)
          for (int w = 0; w < P; ++w) {
            const bool tr = ((k0 + i) & 4) != 0;
            outs.push_back(upsample(sl[sx8_entry(i, P, w)], C, tr ? tw : th, tr ? th : tw));
          }
        reduce(pass, C, tile, pad, th, tw, k0, slots, k0 > 0, k0 + slots == 8 ? 0.125f : 1.0f, img, bgr, outs, acc, acc_elems, res);
      }
    }
    free(acc);
    // every HR pixel of every image of the group once, with the upsampled pixel; everything else untouched
    for (size_t j = 0; j < sizes.size(); ++j) {
      const int H = sizes[j].first, W = sizes[j].second;
      const bool mine = imin(tile + 2 * pad, H) == th && imin(tile + 2 * pad, W) == tw;
      for (int Y = 0; Y < 4 * H; ++Y)
        for (int X = 0; X < 4 * W; ++X) {
          CHECK(res.hits[j][(size_t)Y * 4 * W + X] == (mine ? 1 : 0), "image %zu HR pixel (%d, %d) written %d times", j, Y, X, res.hits[j][(size_t)Y * 4 * W + X]);
          for (int c = 0; c < C; ++c) {
            const float v = unit(pixel((int)j, c, Y / 4, X / 4));
            float mean = v;                                   // eight equal terms, summed as the kernel sums them
            for (int k = 1; k < 8; ++k) mean += v;
            mean *= 0.125f;
            if (img) CHECK(res.u[j][((size_t)Y * 4 * W + X) * C + ((bgr && C == 3) ? 2 - c : c)] == (mine ? quant8(mean) : 0xAB), "image %zu byte (%d, %d, %d)", j, Y, X, c);
            else CHECK(res.f[j][((size_t)c * 4 * H + Y) * 4 * W + X] == (mine ? mean : -7.f), "image %zu value (%d, %d, %d)", j, Y, X, c);
          }
        }
    }
  }
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
            if (img && C == 8) continue;
            run_case(sizes, C, tp.first, tp.second, P, split, img, img && C == 3 && split != 4);
            ++cases;
          }
  // the refusals of a k range
  if (sx8_range_error(-1, 2, 8, 8) != 1 || sx8_range_error(0, 0, 8, 8) != 1 || sx8_range_error(7, 2, 8, 8) != 1 ||
      sx8_range_error(0, 8, 8, 9) != 2 || sx8_range_error(2, 4, 9, 8) != 2 || sx8_range_error(0, 8, 8, 8) != 0 ||
      sx8_range_error(0, 4, 8, 9) != 0 || sx8_range_error(4, 4, 8, 9) != 0 || sx8_range_error(2147483647, 2147483647, 8, 8) != 1)
    ++failures, printf("FAILED: sx8_range_error\n");
  if (sx8_acc_needed(0, 1, 4, 4) || sx8_acc_needed(1, 0, 0, 8) || !sx8_acc_needed(1, 0, 0, 4) || !sx8_acc_needed(1, 1, 4, 4))
    ++failures, printf("FAILED: sx8_acc_needed\n");
  printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
