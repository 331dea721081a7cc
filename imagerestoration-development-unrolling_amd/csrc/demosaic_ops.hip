// Bayer mosaicking of uint8 pictures and the initial fill of the missing channels (include/grr.h has the
// definition: four patterns, three fills, reflection without the edge sample, integer sixteenths), gfx950.
//
//   grr_u8_demosaic          one HWC uint8 image (any byte address), 1 or 3 channels -> H x W x 3
//   grr_u8_demosaic_images   every image of an RGB arena into the same place of a second arena, one pattern per image
//
// One launch.  A 256-thread workgroup owns a kRows x kCols tile of the picture and keeps the tile's part of the
// mosaic plane, with a 2-sample halo, as bytes in LDS:
//
//   fill     a task is 4 adjacent bytes of one LDS row: four byte loads from global memory -- only the site's
//            channel of each source pixel -- packed into one dword write.  The reflection is applied here, so
//            every byte of the region holds the sample the formulas expect
//   compute  a lane owns 4 adjacent pixels of one row.  The LDS column of a sample is its tile column plus 2, so the
//            lane's 8-sample window of each of the 5 rows starts at a dword: 10 dword reads, no bounds tests.  The
//            four sums of every pixel are formed and chosen by the site's parities with selects; the fill mode is a
//            template argument
//   output   the lane's 12 bytes as three dword stores where the address is 4-byte aligned and all 4 pixels exist,
//            else byte stores (ragged ends, odd bases, rows of odd-width pictures)
//
// LDS rows are kStride bytes apart: 48 dwords, so that the two rows of a 32-lane group (16 lanes each, 17 dwords
// touched) fall on disjoint banks.  The region is 20 x 192 bytes: occupancy is bounded by the waves, not by LDS.
// All arithmetic is int32 (|s| <= 2 * 20 * 255); no float, no atomics, each output byte is written once.
//
// The image table and the pattern list of the arena form are device data: every value read from them is clamped,
// every element index read is kept inside [0, elems) and a write at or past elems is dropped, so a bad table
// gives wrong pixels, never an access outside the two arenas.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 16, kCols = 64;     // a workgroup's tile; kernels.DEMOSAIC_TILE
constexpr int kHalo = 2;
constexpr int kLdsRows = kRows + 2 * kHalo;
constexpr int kLdsWords = (kCols + 2 * kHalo) / 4;     // dwords filled per row
constexpr int kStride = 192;              // bytes between two LDS rows
constexpr int kMaxImages = 65535;         // one grid row (blockIdx.y) per image
constexpr int64_t kMaxElems = (1ll << 31) - 1;
static_assert(kRows * (kCols / 4) == kThreads, "a lane owns 4 pixels of the tile");
static_assert(kLdsWords * 4 <= kStride && kStride % 4 == 0, "LDS row");

struct DemosaicArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_elems;            // one image: H W src_c; arena: the elements of either arena
  int64_t dst_elems;            // one image: 3 H W
  const int64_t* table;         // [n_img, 3] (element offset, H, W) on the device; null: the one image below
  const int32_t* patterns;      // [n_img] on the device; null: pattern
  int H, W;                     // one image: its sides; arena: they bound every image's
  int src_c;                    // 1: src is the mosaic plane; 3: R, G, B
  int pattern;
  int tiles_x;                  // tiles per row of the largest image
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index i of [-2, n + 1] reflected about the edge samples of a side n: i mod 2(n - 1) folded, without the division
__device__ __forceinline__ int reflect(int i, int n) {
  if (n == 1) return 0;
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return i < 0 ? -i : i;          // n = 2 folds twice
}

__device__ __forceinline__ int u8_round(int s) {
  const int v = (s + 8) >> 4;     // arithmetic shift
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// kFill: 0 zero, 1 bilinear, 2 malvar
template <int kFill>
__global__ __launch_bounds__(kThreads) void demosaic_kernel(DemosaicArgs a) {
  __shared__ uint32_t plane[kLdsRows * kStride / 4];
  int64_t off = 0;
  int H = a.H, W = a.W, pat = a.pattern;
  if (a.table) {
    const int64_t* it = a.table + (int64_t)blockIdx.y * 3;
    off = clamp64(it[0], 0, a.src_elems - 1);
    H = (int)clamp64(it[1], 1, a.H);
    W = (int)clamp64(it[2], 1, a.W);
    pat = a.patterns[blockIdx.y];
  }
  pat = clampi(pat, 0, 3);
  const int ry = pat >> 1, rx = pat & 1;              // the parities of the R site
  const int ty0 = (int)(blockIdx.x / (uint32_t)a.tiles_x) * kRows, tx0 = (int)(blockIdx.x % (uint32_t)a.tiles_x) * kCols;
  if (ty0 >= H || tx0 >= W) return;                   // the whole workgroup: a smaller image of the arena
  const int t = (int)threadIdx.x;
  const int C = a.src_c;

  // fill: LDS byte (ly, lx) is m[reflect(ty0 + ly - 2), reflect(tx0 + lx - 2)]; beyond the picture's own halo the
  // index is held at the halo's end, whose value no output uses
  for (int idx = t; idx < kLdsRows * kLdsWords; idx += kThreads) {
    const int ly = idx / kLdsWords, lw = idx % kLdsWords;
    const int y = reflect(min(ty0 + ly - kHalo, H + 1), H);
    const int64_t row = (int64_t)y * W;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = reflect(min(tx0 + 4 * lw + k - kHalo, W + 1), W);
      const int ch = C == 3 ? ((y ^ ry) & 1) + ((x ^ rx) & 1) : 0;      // R 0 at (0, 0), B 2 at (1, 1), else G 1
      const int64_t el = min(off + (row + x) * C + ch, a.src_elems - 1);
      word |= (uint32_t)a.src[el] << (8 * k);
    }
    plane[ly * (kStride / 4) + lw] = word;
  }
  __syncthreads();

  const int r = t / (kCols / 4), k = t % (kCols / 4);
  const int y = ty0 + r, x0 = tx0 + 4 * k;
  if (y >= H || x0 >= W) return;
  // the 8-sample windows of the 5 rows: byte c of row j is the sample at (y + j - 2, x0 + c - 2)
  uint32_t lo[5], hi[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    lo[j] = plane[(r + j) * (kStride / 4) + k];
    hi[j] = plane[(r + j) * (kStride / 4) + k + 1];
  }
  auto at = [&](int j, int c) { return (int)(((c < 4 ? lo[j] : hi[j]) >> (8 * (c & 3))) & 255u); };
  const int py = (y ^ ry) & 1;
  uint32_t out[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i + 2;
    const int px = (i ^ rx) & 1;                      // x0 is a multiple of 4
    const int ctr = at(2, c);
    int rgb[3];
    if constexpr (kFill == 0) {
      rgb[0] = rgb[1] = rgb[2] = 0;
    } else {
      const int h1 = at(2, c - 1) + at(2, c + 1), v1 = at(1, c) + at(3, c);
      const int diag = at(1, c - 1) + at(1, c + 1) + at(3, c - 1) + at(3, c + 1);
      int green, other, inrow, incol;               // G at R / B; R at B and B at R; at G: the row's and the column's colour
      if constexpr (kFill == 1) {
        green = 4 * (h1 + v1);
        other = 4 * diag;
        inrow = 8 * h1;
        incol = 8 * v1;
      } else {
        const int h2 = at(2, c - 2) + at(2, c + 2), v2 = at(0, c) + at(4, c);
        green = 8 * ctr + 4 * (h1 + v1) - 2 * (h2 + v2);
        other = 12 * ctr + 4 * diag - 3 * (h2 + v2);
        inrow = 10 * ctr + 8 * h1 - 2 * diag - 2 * h2 + v2;
        incol = 10 * ctr + 8 * v1 - 2 * diag - 2 * v2 + h2;
      }
      // at a G site the row's colour is R in an R row (py = 0) and B in a B row
      const bool site_g = py != px;
      rgb[0] = u8_round(site_g ? (py ? incol : inrow) : other);
      rgb[1] = u8_round(green);
      rgb[2] = u8_round(site_g ? (py ? inrow : incol) : other);
    }
    const int site = py + px;                       // R 0, G 1, B 2: a measured sample passes through
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int b = 3 * i + ch;
      out[b >> 2] |= (uint32_t)(ch == site ? ctr : rgb[ch]) << (8 * (b & 3));
    }
  }
  const int64_t el = off + ((int64_t)y * W + x0) * 3;
  uint8_t* p = a.dst + el;
  if (x0 + 4 <= W && el + 12 <= a.dst_elems && ((uintptr_t)p & 3) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = out[0];
    q[1] = out[1];
    q[2] = out[2];
  } else {
    const int n = min(4, W - x0) * 3;
#pragma unroll
    for (int b = 0; b < 12; ++b)
      if (b < n && el + b < a.dst_elems) p[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
  }
}

void launch(int fill, dim3 grid, hipStream_t s, const DemosaicArgs& a) {
  if (fill == 0) {
    hipLaunchKernelGGL((demosaic_kernel<0>), grid, dim3(kThreads), 0, s, a);
  } else if (fill == 1) {
    hipLaunchKernelGGL((demosaic_kernel<1>), grid, dim3(kThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((demosaic_kernel<2>), grid, dim3(kThreads), 0, s, a);
  }
}

int tiles(int n, int side) { return (n + side - 1) / side; }

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_u8_demosaic_supported(int src_c, int H, int W) {
  if ((src_c != 1 && src_c != 3) || H < 1 || W < 1) return 0;
  return (int64_t)H * W <= kMaxElems / 3 ? 1 : 0;
}

grr_status grr_u8_demosaic(const uint8_t* src, int H, int W, int src_c, uint8_t* dst, int pattern, int fill,
                           void* stream) {
  clear_error();
  const char* what = "grr_u8_demosaic";
  GRR_REQUIRE(src && dst && H > 0 && W > 0 && src_c > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(pattern >= 0 && pattern <= 3, GRR_ERR_INVALID_ARG,
              "%s: the pattern is 0 (rggb), 1 (grbg), 2 (gbrg) or 3 (bggr) (got %d)", what, pattern);
  GRR_REQUIRE(fill >= 0 && fill <= 2, GRR_ERR_INVALID_ARG, "%s: the fill is 0 (zero), 1 (bilinear) or 2 (malvar) (got %d)",
              what, fill);
  GRR_REQUIRE(grr_u8_demosaic_supported(src_c, H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs a source of 1 or 3 channels and 3 H W < 2^31 (got %d x %d x %d)", what, H, W, src_c);
  DemosaicArgs a{};
  a.src = src;
  a.dst = dst;
  a.src_elems = (int64_t)H * W * src_c;
  a.dst_elems = (int64_t)H * W * 3;
  a.H = H;
  a.W = W;
  a.src_c = src_c;
  a.pattern = pattern;
  a.tiles_x = tiles(W, kCols);
  launch(fill, dim3((uint32_t)(a.tiles_x * tiles(H, kRows))), (hipStream_t)stream, a);      // < 2^20 tiles
  return launch_status(what);
}

grr_status grr_u8_demosaic_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, int max_h,
                                  int max_w, uint8_t* dst_arena, const int32_t* patterns, int fill, void* stream) {
  clear_error();
  const char* what = "grr_u8_demosaic_images";
  GRR_REQUIRE(arena && dst_arena && table && patterns && elems > 0 && n_img > 0 && max_h > 0 && max_w > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE((uintptr_t)table % 8 == 0 && (uintptr_t)patterns % 4 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image table must be 8-byte and the pattern list 4-byte aligned", what);
  GRR_REQUIRE(fill >= 0 && fill <= 2, GRR_ERR_INVALID_ARG, "%s: the fill is 0 (zero), 1 (bilinear) or 2 (malvar) (got %d)",
              what, fill);
  GRR_REQUIRE(grr_u8_demosaic_supported(3, max_h, max_w), GRR_ERR_UNSUPPORTED,
              "%s: needs 3 max_h max_w < 2^31 (got %d x %d)", what, max_h, max_w);
  GRR_REQUIRE(grr_image_arena_supported(3, n_img, elems) && elems >= 3, GRR_ERR_UNSUPPORTED,
              "%s: needs 3 <= 3 n_img <= arena elements < 2^62 (got %d images, %lld elements)", what, n_img,
              (long long)elems);
  GRR_REQUIRE(n_img <= kMaxImages, GRR_ERR_UNSUPPORTED, "%s: at most %d images per call (got %d)", what, kMaxImages,
              n_img);
  DemosaicArgs a{};
  a.src = arena;
  a.dst = dst_arena;
  a.src_elems = elems;
  a.dst_elems = elems;
  a.table = table;
  a.patterns = patterns;
  a.H = max_h;
  a.W = max_w;
  a.src_c = 3;
  a.tiles_x = tiles(max_w, kCols);
  launch(fill, dim3((uint32_t)(a.tiles_x * tiles(max_h, kRows)), (uint32_t)n_img), (hipStream_t)stream, a);
  return launch_status(what);
}

}  // extern "C"
