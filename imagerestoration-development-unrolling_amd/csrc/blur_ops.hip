// 2-D blur of uint8 pictures by an integer point-spread function (include/grr.h has the definition: a kh x kw table of
// non-negative int32 weights that sum to 65536, a true convolution, three boundary rules, (32768 + sum) >> 16), gfx950.
//
//   grr_u8_blur          one HWC uint8 image (any byte address), 1..4 channels
//   grr_u8_blur_images   every image of an arena into the same place of a second arena, one kernel per image
//
// One launch.  A 256-thread workgroup owns a kRows x kCols tile of the picture:
//
//   pack     the kernel's weights, flipped (so the loop below is a correlation), clamped into [0, 65536] and split into
//            three byte planes W = 65536 top + 256 hi + lo, four taps of a row to a dword, go to LDS: one thread per
//            group of four.  top is non-zero only for a lone tap of 65536 (the identity, or a shift); whether any is
//            set is voted once and chooses the loop without or with the third plane
//   maps     the source row of every LDS row and the source column of every LDS column under the boundary rule, with
//            the divisions it takes, once per workgroup: kRows + kh - 1 and kCols + kw - 1 values
//   fill     the tile and a halo of the kernel's own radius, de-interleaved into one byte plane per channel; a task is 4
//            adjacent bytes of one LDS row of every channel.  The boundary is applied here, so the loop has no branches
//   compute  a lane owns 4 adjacent pixels of one row.  The LDS column of a sample is its tile column plus kw / 2, so
//            the window of tap group g of pixel p is bytes 4 (k + g) + p .. + 3 of the row: dword k + g for p = 0,
//            v_alignbyte_b32 of dwords k + g and k + g + 1 otherwise.  Two v_dot4_u32_u8 per four taps and pixel (lo
//            and hi plane), accumulated in uint32: sum lo <= 961 * 255 * 255 < 2^26, sum hi <= 255 * 256.  The loop
//            bounds are the kernel's own kh and ceil(kw / 4), wave-uniform
//   output   the lane's 4 C bytes as C dword stores where the address is 4-byte aligned and all 4 pixels exist, else
//            byte stores (ragged ends, odd bases, rows whose width in bytes is no multiple of 4)
//
// LDS rows are kStride bytes apart: 48 dwords, so that the two rows of a 32-lane group (16 lanes each) fall on disjoint
// banks.  All arithmetic is unsigned 32-bit and exact; no float, no atomics, each output byte is written once.
//
// The image table, the kernel list, the kernels' sides and the weights of the arena form are device data: every value
// read from them is clamped, every element index read is kept inside [0, elems) and a write at or past elems is
// dropped, so a bad table gives wrong pixels, never an access outside the two arenas.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 16, kCols = 64;     // a workgroup's tile; kernels.BLUR_TILE
constexpr int kMaxSide = 31;              // GRR_BLUR_MAX_SIDE
constexpr int kOne = 65536;               // GRR_BLUR_ONE
constexpr int kGroups = (kMaxSide + 3) / 4;               // tap groups of a kernel row
constexpr int kLdsRows = kRows + kMaxSide - 1;
constexpr int kLdsWords = (kCols + kMaxSide - 1 + 3) / 4;  // dwords filled per row, at most
constexpr int kStride = 192;              // bytes between two LDS rows
constexpr int kPlane = kLdsRows * kStride / 4;            // dwords of one channel's plane
constexpr int kMaxImages = 65535;         // one grid row (blockIdx.y) per image
constexpr int kMaxKernels = 16;
constexpr int64_t kMaxElems = (1ll << 31) - 1;
static_assert(kRows * (kCols / 4) == kThreads, "a lane owns 4 pixels of the tile");
static_assert(kMaxSide * kGroups <= kThreads, "one thread packs one group of four taps");
static_assert(kLdsRows + kLdsWords * 4 <= kThreads, "one thread per entry of the two index maps");
static_assert((kCols / 4 + kGroups) * 4 <= kStride && kStride % 4 == 0, "LDS row: the last group's second dword");

struct BlurArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t elems;                // one image: H W C; arena: the elements of either arena
  const int64_t* table;         // [n_img, 3] (element offset, H, W) on the device; null: the one image below
  const int32_t* weights;       // one image: [kh * kw]; arena: [n_kernels, 31 * 31], a kernel in the top-left kh x kw
  const int32_t* sizes;         // arena: [n_kernels, 2]
  const int32_t* kernel_of;     // arena: [n_img]
  int n_kernels;
  int H, W;                     // one image: its sides; arena: they bound every image's
  int C;
  int kh, kw;                   // one image
  int boundary;
  int tiles_x;                  // tiles per row of the largest image
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// b(t, n) of the definition for any int t: 0 wrap, 1 replicate, 2 reflect without the edge sample
__device__ __forceinline__ int bound(int t, int n, int mode) {
  if (mode == 1) return clampi(t, 0, n - 1);
  if (mode == 0) {
    const int m = t % n;
    return m < 0 ? m + n : m;
  }
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int m = t % p;
  m = m < 0 ? m + p : m;
  return m < n ? m : p - m;
}

// the sums of pixel channel ch over the kernel: kTop adds the third weight plane
template <bool kTop>
__device__ __forceinline__ void accumulate(const uint32_t* __restrict__ plane, const uint2* __restrict__ wts,
                                           const uint32_t* __restrict__ wtop, int r, int k, int kh, int groups,
                                           uint32_t (&sum)[4]) {
  uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, top[4] = {0, 0, 0, 0};
  for (int i = 0; i < kh; ++i) {
    const uint32_t* row = plane + (r + i) * (kStride / 4) + k;
    uint32_t d0 = row[0];
    for (int g = 0; g < groups; ++g) {
      const uint32_t d1 = row[g + 1];
      const uint2 w = wts[i * kGroups + g];
      uint32_t win[4];
      win[0] = d0;
      win[1] = __builtin_amdgcn_alignbyte(d1, d0, 1);
      win[2] = __builtin_amdgcn_alignbyte(d1, d0, 2);
      win[3] = __builtin_amdgcn_alignbyte(d1, d0, 3);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        lo[p] = __builtin_amdgcn_udot4(win[p], w.x, lo[p], false);
        hi[p] = __builtin_amdgcn_udot4(win[p], w.y, hi[p], false);
      }
      if constexpr (kTop) {
        const uint32_t wt = wtop[i * kGroups + g];
#pragma unroll
        for (int p = 0; p < 4; ++p) top[p] = __builtin_amdgcn_udot4(win[p], wt, top[p], false);
      }
      d0 = d1;
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) sum[p] = lo[p] + (hi[p] << 8) + (top[p] << 16);
}

__global__ __launch_bounds__(kThreads) void blur_kernel(BlurArgs a) {
  extern __shared__ uint32_t planes[];            // C planes of kPlane dwords
  __shared__ uint2 wts[kMaxSide * kGroups];       // (lo, hi) of four flipped taps
  __shared__ uint32_t wtop[kMaxSide * kGroups];
  __shared__ int rowmap[kLdsRows], colmap[kLdsWords * 4];
  int64_t off = 0;
  int H = a.H, W = a.W, kh = a.kh, kw = a.kw, wstride = a.kw;
  const int32_t* wsrc = a.weights;
  if (a.table) {
    const int64_t* it = a.table + (int64_t)blockIdx.y * 3;
    off = clamp64(it[0], 0, a.elems - 1);
    H = (int)clamp64(it[1], 1, a.H);
    W = (int)clamp64(it[2], 1, a.W);
    const int ki = clampi(a.kernel_of[blockIdx.y], 0, a.n_kernels - 1);
    kh = a.sizes[2 * ki];
    kw = a.sizes[2 * ki + 1];
    wsrc = a.weights + ki * (kMaxSide * kMaxSide);
    wstride = kMaxSide;
  }
  kh = clampi(kh, 1, kMaxSide) | 1;               // odd, still at most 31
  kw = clampi(kw, 1, kMaxSide) | 1;
  const int ry = kh >> 1, rx = kw >> 1;
  const int groups = (kw + 3) >> 2;
  const int ty0 = (int)(blockIdx.x / (uint32_t)a.tiles_x) * kRows, tx0 = (int)(blockIdx.x % (uint32_t)a.tiles_x) * kCols;
  if (ty0 >= H || tx0 >= W) return;               // the whole workgroup: a smaller image of the arena
  const int t = (int)threadIdx.x;
  const int C = a.C;
  const int lds_rows = kRows + 2 * ry, lds_words = (kCols + 2 * rx + 3) >> 2;

  // pack: group g of flipped row i holds the taps W[kh - 1 - i][kw - 1 - (4 g + q)], q = 0..3; beyond kw they are 0
  int any_top = 0;
  if (t < kh * kGroups) {
    const int i = t / kGroups, g = t % kGroups;
    uint32_t lo = 0, hi = 0, top = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * g + q;
      const int w = j < kw ? clampi(wsrc[(kh - 1 - i) * wstride + (kw - 1 - j)], 0, kOne) : 0;
      lo |= (uint32_t)(w & 255) << (8 * q);
      hi |= (uint32_t)((w >> 8) & 255) << (8 * q);
      top |= (uint32_t)(w >> 16) << (8 * q);
    }
    wts[t] = make_uint2(lo, hi);
    wtop[t] = top;
    any_top = top != 0;
  }
  // maps: LDS row ly is source row b(ty0 + ly - ry, H), LDS column lx source column b(tx0 + lx - rx, W)
  if (t < kLdsRows) {
    rowmap[t] = bound(ty0 + t - ry, H, a.boundary);
  } else if (t - kLdsRows < kLdsWords * 4) {
    colmap[t - kLdsRows] = bound(tx0 + (t - kLdsRows) - rx, W, a.boundary);
  }
  any_top = __syncthreads_or(any_top);

  // fill: one task is the dword (ly, lw) of every channel's plane
  for (int idx = t; idx < lds_rows * lds_words; idx += kThreads) {
    const int ly = idx / lds_words, lw = idx % lds_words;
    const int64_t row = (int64_t)rowmap[ly] * W;
    uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t px = off + (row + colmap[4 * lw + q]) * C;
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < C) word[ch] |= (uint32_t)a.src[min(px + ch, a.elems - 1)] << (8 * q);
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < C) planes[ch * kPlane + ly * (kStride / 4) + lw] = word[ch];
  }
  __syncthreads();

  const int r = t / (kCols / 4), k = t % (kCols / 4);
  const int y = ty0 + r, x0 = tx0 + 4 * k;
  if (y >= H || x0 >= W) return;
  uint32_t px[4] = {0, 0, 0, 0};                  // byte ch of px[p] is channel ch of pixel x0 + p
  for (int ch = 0; ch < C; ++ch) {
    uint32_t sum[4];
    if (any_top) {
      accumulate<true>(planes + ch * kPlane, wts, wtop, r, k, kh, groups, sum);
    } else {
      accumulate<false>(planes + ch * kPlane, wts, wtop, r, k, kh, groups, sum);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) px[p] |= min((sum[p] + 32768u) >> 16, 255u) << (8 * ch);
  }
  // the lane's 4 C bytes in memory order
  uint32_t out[4] = {px[0], px[1], px[2], px[3]};
  if (C == 1) {
    out[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else if (C == 2) {
    out[0] = px[0] | (px[1] << 16);
    out[1] = px[2] | (px[3] << 16);
  } else if (C == 3) {
    out[0] = px[0] | (px[1] << 24);
    out[1] = (px[1] >> 8) | (px[2] << 16);
    out[2] = (px[2] >> 16) | (px[3] << 8);
  }
  const int64_t el = off + ((int64_t)y * W + x0) * C;
  uint8_t* p = a.dst + el;
  if (x0 + 4 <= W && el + 4 * C <= a.elems && ((uintptr_t)p & 3) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < C) q[d] = out[d];
  } else {
    const int n = min(4, W - x0) * C;
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (b < n && el + b < a.elems) p[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
  }
}

int tiles(int n, int side) { return (n + side - 1) / side; }

void launch(dim3 grid, hipStream_t s, const BlurArgs& a) {
  hipLaunchKernelGGL(blur_kernel, grid, dim3(kThreads), (size_t)a.C * kPlane * 4, s, a);
}

bool side_ok(int n) { return n >= 1 && n <= kMaxSide && (n & 1); }

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_u8_blur_supported(int C, int H, int W) {
  if (C < 1 || C > 4 || H < 1 || W < 1) return 0;
  return (int64_t)H * W <= kMaxElems / C ? 1 : 0;
}

grr_status grr_u8_blur(const uint8_t* src, int H, int W, int C, uint8_t* dst, const int32_t* weights, int kh, int kw,
                       int boundary, void* stream) {
  clear_error();
  const char* what = "grr_u8_blur";
  GRR_REQUIRE(src && dst && weights && H > 0 && W > 0 && C > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE((uintptr_t)weights % 4 == 0, GRR_ERR_INVALID_ARG, "%s: the weights must be 4-byte aligned", what);
  GRR_REQUIRE(side_ok(kh) && side_ok(kw), GRR_ERR_INVALID_ARG,
              "%s: the kernel's sides are odd and in 1..%d (got %d x %d)", what, kMaxSide, kh, kw);
  GRR_REQUIRE(boundary >= 0 && boundary <= 2, GRR_ERR_INVALID_ARG,
              "%s: the boundary is 0 (wrap), 1 (replicate) or 2 (reflect) (got %d)", what, boundary);
  GRR_REQUIRE(grr_u8_blur_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs 1..4 channels and H W C < 2^31 (got %d x %d x %d)", what, H, W, C);
  BlurArgs a{};
  a.src = src;
  a.dst = dst;
  a.elems = (int64_t)H * W * C;
  a.weights = weights;
  a.n_kernels = 1;
  a.H = H;
  a.W = W;
  a.C = C;
  a.kh = kh;
  a.kw = kw;
  a.boundary = boundary;
  a.tiles_x = tiles(W, kCols);
  launch(dim3((uint32_t)(a.tiles_x * tiles(H, kRows))), (hipStream_t)stream, a);      // < 2^21 tiles
  return launch_status(what);
}

grr_status grr_u8_blur_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, int max_h, int max_w,
                              int C, uint8_t* dst_arena, const int32_t* weights, const int32_t* sizes, int n_kernels,
                              const int32_t* kernel_of, int boundary, void* stream) {
  clear_error();
  const char* what = "grr_u8_blur_images";
  GRR_REQUIRE(arena && dst_arena && table && weights && sizes && kernel_of && elems > 0 && n_img > 0 && max_h > 0 &&
                  max_w > 0 && C > 0 && n_kernels > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE((uintptr_t)table % 8 == 0 && (uintptr_t)weights % 4 == 0 && (uintptr_t)sizes % 4 == 0 &&
                  (uintptr_t)kernel_of % 4 == 0,
              GRR_ERR_INVALID_ARG, "%s: the image table must be 8-byte, the kernel tables and the kernel list 4-byte aligned",
              what);
  GRR_REQUIRE(boundary >= 0 && boundary <= 2, GRR_ERR_INVALID_ARG,
              "%s: the boundary is 0 (wrap), 1 (replicate) or 2 (reflect) (got %d)", what, boundary);
  GRR_REQUIRE(grr_u8_blur_supported(C, max_h, max_w), GRR_ERR_UNSUPPORTED,
              "%s: needs 1..4 channels and max_h max_w C < 2^31 (got %d x %d x %d)", what, max_h, max_w, C);
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, elems), GRR_ERR_UNSUPPORTED,
              "%s: needs C n_img <= arena elements < 2^62 (got %d images, %lld elements)", what, n_img, (long long)elems);
  GRR_REQUIRE(n_img <= kMaxImages, GRR_ERR_UNSUPPORTED, "%s: at most %d images per call (got %d)", what, kMaxImages,
              n_img);
  GRR_REQUIRE(n_kernels <= kMaxKernels, GRR_ERR_UNSUPPORTED, "%s: at most %d kernels per call (got %d)", what,
              kMaxKernels, n_kernels);
  BlurArgs a{};
  a.src = arena;
  a.dst = dst_arena;
  a.elems = elems;
  a.table = table;
  a.weights = weights;
  a.sizes = sizes;
  a.kernel_of = kernel_of;
  a.n_kernels = n_kernels;
  a.H = max_h;
  a.W = max_w;
  a.C = C;
  a.boundary = boundary;
  a.tiles_x = tiles(max_w, kCols);
  launch(dim3((uint32_t)(a.tiles_x * tiles(max_h, kRows)), (uint32_t)n_img), (hipStream_t)stream, a);
  return launch_status(what);
}

}  // extern "C"
