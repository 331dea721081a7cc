// Image metrics beside the PSNR's grr_u8_sse (image_ops.hip), gfx950.
//
//   grr_u8_ssim         sum over the valid pixels and channels of rint(2^32 s), s the Gaussian-window SSIM of
//                       two uint8 H x W x C images, as an exact signed 64-bit integer
//   grr_u8_ssim_images  the same for every image of two arenas that share one image table, in one launch
//
// Definition (Wang et al.; skimage's structural_similarity with gaussian_weights, sigma 1.5,
// use_sample_covariance=False, data_range 255): an 11 x 11 separable Gaussian window, taps
// g[k] = exp(-(k - 5)^2 / 4.5) / sum; per channel the five filtered moments mx, my, E[x^2], E[y^2], E[xy] at the
// (H - 10) x (W - 10) pixels whose window lies inside the image; vx = E[x^2] - mx^2, vy likewise,
// vxy = E[xy] - mx my; s = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), C1 = 6.5025,
// C2 = 58.5225.  SSIM is the mean of s over the N = (H - 10)(W - 10) C values: sum / (2^32 N).
//
// Every s is float64 from the bytes, in one fixed order -- the horizontal taps k = 0..10 ascending (fma), then
// the vertical taps ascending (fma), then the formula above with every product and sum rounded on its own (no
// contraction in this file) -- so a pixel's value does not depend on the tile, the lane or the image's place in
// an arena.  It is quantised to q = rint(2^32 s) and the q are added as integers (lane, wave, one 64-bit vector
// atomic per wave): the sum is the same whatever order the atomics land in and whatever the grid is.  |s| <= 1,
// so |q| <= 2^32 and N < 2^31 values stay below 2^63.  Equal images give num == den bit for bit, s = 1 and
// q = 2^32 at every pixel.
//
// An image is H rows of W C interleaved bytes; output byte column j < (W - 10) C of output row i reads the bytes
// j + k C, k = 0..10, of the rows i..i + 10.  A 256-thread workgroup owns kSsimCols = 256 output byte columns by
// kSsimRows = 32 output rows.  Per input row it stages the 256 + 10 C bytes of a and of b as float64 in LDS (one
// conversion per byte, two buffers, one barrier per row; the next row's bytes are in flight meanwhile), each lane
// forms its five horizontal sums and keeps the last 11 rows of them in a register ring whose slots are
// compile-time (the row loop is unrolled by 11), and from the 11th row of the tile on it emits one output row per
// input row.  Both images are read (32 + 10) / 32 times.  Images start at any byte: all global reads are single
// bytes, adjacent lanes adjacent bytes.
//
// The arena's image table is device data: the offset is clamped into [0, arena_elems), H and W into
// [1, max_h] x [1, max_w], and every byte index into [0, arena_elems), so a bad table gives a wrong number,
// never an access outside the arenas.  An image with a side below 11 contributes nothing.
//
// Luma (Y of ITU-R BT.601 "studio range" YCbCr: MATLAB's rgb2ycbcr, BasicSR's to_y_channel, not rounded to uint8)
// of two uint8 H x W x 3 images, channels R, G, B interleaved:
//
//   grr_u8_luma_sse, grr_u8_luma_sse_images    sum D^2 as two exact 64-bit words
//   grr_u8_luma_ssim, grr_u8_luma_ssim_images  the sum q above of the single plane Y
//
// Y = Ny / 255000 with the integer Ny = 4080000 + 65481 R + 128553 G + 24966 B <= 59 925 000.  The SSE is the
// integer sum of D^2, D = Ny(a) - Ny(b) = 65481 dR + 128553 dG + 24966 dB, |D| <= 55 845 000 < 2^26: D^2 < 2^52,
// and the sum over fewer than 2^30 pixels can reach 2^82, so the kernel adds D^2 mod 2^32 and D^2 >> 32 apart
// (below 2^62 and 2^50) and the caller joins them: out[0] + (out[1] << 32).  The SSIM stages one float64
// Y = double(Ny) / 255000.0 per pixel -- the integer is exact and the division rounds once, so the device and
// every host form the same bits -- and runs the body above over pixel columns: u8_ssim_kernel takes what a staged
// column is (BytePx<C>: one interleaved byte; LumaPx: the luma of three) as a template parameter.
//
// The blocking sums of PSNR-B of one uint8 H x W x C image (include/grr.h has the definition):
//
//   grr_u8_blocking, grr_u8_blocking_images    S_b, N_b, S_n, N_n as four exact 64-bit words per image
#include <algorithm>

#include "grr_common.h"
#include "ssim_window.h"

#pragma clang fp contract(off)

namespace grr {
namespace {

// the tile, the taps and C1, C2 are ssim_window.h's, shared with the training loss (ssim_loss_ops.hip)
constexpr int kSsimMaxImages = 65535;   // one grid row (blockIdx.y) per image

struct SsimImage {
  int64_t off;   // first byte of the image in a and in b
  int H, W;
};

// grr_u8_ssim: one H x W image at a and b; the caller sized both from (H, W, C).
struct SsimOne {
  int H, W;
  __device__ __forceinline__ SsimImage image(int) const { return SsimImage{0, H, W}; }
  __device__ __forceinline__ int64_t clamped(int64_t e) const { return e; }
};

// grr_u8_ssim_images: image blockIdx.y of the device image table [n_img, 3] (element offset, H, W), clamped.
struct SsimArena {
  const int64_t* img_table;
  int64_t elems;
  int max_h, max_w;
  __device__ __forceinline__ SsimImage image(int i) const {
    const int64_t* it = img_table + (int64_t)i * 3;
    const int64_t off = it[0], h = it[1], w = it[2];
    return SsimImage{off < 0 ? 0 : (off > elems - 1 ? elems - 1 : off), (int)(h < 1 ? 1 : (h > max_h ? max_h : h)),
                     (int)(w < 1 ? 1 : (w > max_w ? max_w : w))};
  }
  __device__ __forceinline__ int64_t clamped(int64_t e) const { return e < elems - 1 ? e : elems - 1; }   // e >= 0
};

// What a staged column of a row is.  kStep: the columns between two taps of one output column; kBytes: the bytes a
// column is made of; cols(W): the columns of a row; load: the column's integer, which is in flight while the row
// before it is filtered; value: its float64, formed once per column when it is staged.

// every interleaved byte of an H x W x C image: the SSIM of each channel
template <int C>
struct BytePx {
  static constexpr int kStep = C, kBytes = 1;
  static __host__ __device__ __forceinline__ int64_t cols(int W) { return (int64_t)W * C; }
  template <typename Src>
  static __device__ __forceinline__ uint32_t load(const uint8_t* __restrict__ p, const Src& src, int64_t e) {
    return (uint32_t)p[src.clamped(e)];
  }
  static __device__ __forceinline__ double value(uint32_t v) { return (double)v; }
};

// the luma of every pixel of an H x W x 3 image: Ny <= 59 925 000 in flight, double(Ny) / 255000.0 staged
constexpr uint32_t kLumaBase = 4080000u, kLumaR = 65481u, kLumaG = 128553u, kLumaB = 24966u;
struct LumaPx {
  static constexpr int kStep = 1, kBytes = 3;
  static __host__ __device__ __forceinline__ int64_t cols(int W) { return W; }
  template <typename Src>
  static __device__ __forceinline__ uint32_t load(const uint8_t* __restrict__ p, const Src& src, int64_t e) {
    return kLumaBase + kLumaR * p[src.clamped(e)] + kLumaG * p[src.clamped(e + 1)] + kLumaB * p[src.clamped(e + 2)];
  }
  static __device__ __forceinline__ double value(uint32_t v) { return (double)v / 255000.0; }
};

// column col of a row that starts at byte row0 and has ncols columns; 0 beyond the row (no valid column reads it)
template <typename Px, typename Src>
__device__ __forceinline__ uint32_t ssim_col(const uint8_t* __restrict__ p, const Src& src, int64_t row0, int64_t col,
                                             int64_t ncols) {
  return col < ncols ? Px::load(p, src, row0 + col * Px::kBytes) : 0u;
}

template <typename Px, typename Src>
__global__ __launch_bounds__(kSsimThreads) void u8_ssim_kernel(const uint8_t* __restrict__ a,
                                                               const uint8_t* __restrict__ b, Src src, SsimTaps taps,
                                                               unsigned long long* out) {
  constexpr int kExtra = (kSsimTaps - 1) * Px::kStep;     // columns a tile's row needs beyond its 256
  __shared__ double lds[2][2][kSsimCols + kExtra];        // [buffer][a, b][column of the tile]
  const SsimImage im = src.image(blockIdx.y);
  if (im.H < kSsimTaps || im.W < kSsimTaps) return;       // whole block: before any barrier
  const int64_t ncols = Px::cols(im.W), rowlen = ncols * Px::kBytes, vcols = ncols - kExtra;
  const int vrows = im.H - (kSsimTaps - 1);
  const int64_t tcols = (vcols + kSsimCols - 1) / kSsimCols, trows = (vrows + kSsimRows - 1) / kSsimRows;
  if ((int64_t)blockIdx.x >= tcols * trows) return;       // the grid is the largest image's
  const int64_t j0 = ((int64_t)blockIdx.x % tcols) * kSsimCols;
  const int r0 = (int)((int64_t)blockIdx.x / tcols) * kSsimRows;
  const int rin_end = min(r0 + kSsimRows, vrows) + (kSsimTaps - 1);   // input rows [r0, rin_end), rin_end <= H
  const int t = threadIdx.x;
  const bool active = j0 + t < vcols;
  const bool extra = t < kExtra;

  // what this lane stages for the row in flight: column j0 + t and, for the first kExtra lanes, j0 + 256 + t
  uint32_t pa0, pb0, pa1 = 0, pb1 = 0;
  {
    const int64_t row0 = im.off + (int64_t)r0 * rowlen;
    pa0 = ssim_col<Px>(a, src, row0, j0 + t, ncols);
    pb0 = ssim_col<Px>(b, src, row0, j0 + t, ncols);
    if (extra) {
      pa1 = ssim_col<Px>(a, src, row0, j0 + kSsimCols + t, ncols);
      pb1 = ssim_col<Px>(b, src, row0, j0 + kSsimCols + t, ncols);
    }
  }

  double ring[kSsimTaps][5];     // horizontal sums (x, y, x^2, y^2, xy) of the last 11 input rows; slot = (r - r0) % 11
#pragma unroll
  for (int p = 0; p < kSsimTaps; ++p)
#pragma unroll
    for (int m = 0; m < 5; ++m) ring[p][m] = 0.0;
  long long acc = 0;

  for (int base = r0; base < rin_end; base += kSsimTaps) {
#pragma unroll
    for (int p = 0; p < kSsimTaps; ++p) {
      const int r = base + p;                  // input row; block-uniform
      if (r < rin_end) {
        double* la = lds[(r - r0) & 1][0];
        double* lb = lds[(r - r0) & 1][1];
        la[t] = Px::value(pa0);
        lb[t] = Px::value(pb0);
        if (extra) {
          la[kSsimCols + t] = Px::value(pa1);
          lb[kSsimCols + t] = Px::value(pb1);
        }
        if (r + 1 < rin_end) {
          const int64_t row0 = im.off + (int64_t)(r + 1) * rowlen;
          pa0 = ssim_col<Px>(a, src, row0, j0 + t, ncols);
          pb0 = ssim_col<Px>(b, src, row0, j0 + t, ncols);
          if (extra) {
            pa1 = ssim_col<Px>(a, src, row0, j0 + kSsimCols + t, ncols);
            pb1 = ssim_col<Px>(b, src, row0, j0 + kSsimCols + t, ncols);
          }
        }
        // this buffer was last read two rows ago, before the previous row's barrier
        __syncthreads();
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < kSsimTaps; ++k) {
          const double x = la[t + k * Px::kStep], y = lb[t + k * Px::kStep], g = taps.g[k];
          hx = __builtin_fma(g, x, hx);
          hy = __builtin_fma(g, y, hy);
          hxx = __builtin_fma(g, x * x, hxx);      // a product of two bytes is exact, of two lumas rounded once
          hyy = __builtin_fma(g, y * y, hyy);
          hxy = __builtin_fma(g, x * y, hxy);
        }
        ring[p][0] = hx;
        ring[p][1] = hy;
        ring[p][2] = hxx;
        ring[p][3] = hyy;
        ring[p][4] = hxy;
        if (r - r0 >= kSsimTaps - 1) {           // output row r - 10: input rows r - 10..r = slots p + 1..p + 11
          double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = __builtin_fma(taps.g[k], ring[(p + 1 + k) % kSsimTaps][m], v[m]);
          const double mx = v[0], my = v[1];
          const double mxx = mx * mx, myy = my * my, mxy = mx * my;
          const double vx = v[2] - mxx, vy = v[3] - myy, vxy = v[4] - mxy;
          const double num = (2.0 * mxy + kSsimC1) * (2.0 * vxy + kSsimC2);
          const double den = (mxx + myy + kSsimC1) * (vx + vy + kSsimC2);
          const double s = num / den;
          if (active) acc += __double2ll_rn(s * 4294967296.0);
        }
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(out + blockIdx.y, (unsigned long long)acc);
}

template <typename Src>
void ssim_launch(int C, dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, const Src& src,
                 unsigned long long* out) {
  switch (C) {
    case 1: hipLaunchKernelGGL((u8_ssim_kernel<BytePx<1>, Src>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out); break;
    case 2: hipLaunchKernelGGL((u8_ssim_kernel<BytePx<2>, Src>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out); break;
    case 3: hipLaunchKernelGGL((u8_ssim_kernel<BytePx<3>, Src>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out); break;
    default: hipLaunchKernelGGL((u8_ssim_kernel<BytePx<4>, Src>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out); break;
  }
}

void luma_ssim_launch(dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, const SsimOne& src,
                      unsigned long long* out) {
  hipLaunchKernelGGL((u8_ssim_kernel<LumaPx, SsimOne>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out);
}
void luma_ssim_launch(dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, const SsimArena& src,
                      unsigned long long* out) {
  hipLaunchKernelGGL((u8_ssim_kernel<LumaPx, SsimArena>), grid, dim3(kSsimThreads), 0, s, a, b, src, kTaps, out);
}

// tiles of an h x w image with both sides >= 11 and C columns per pixel (the luma: 1)
int64_t ssim_tiles(int h, int w, int C) {
  const int64_t vcols = (int64_t)(w - (kSsimTaps - 1)) * C, vrows = h - (kSsimTaps - 1);
  return ((vcols + kSsimCols - 1) / kSsimCols) * ((vrows + kSsimRows - 1) / kSsimRows);
}

// ---------------------------------------------------------------------------
// Luma SSE.  A 256-thread workgroup takes kLumaSsePx consecutive pixels per step, lane t the pixels
// t + 256 k, k < kLumaSseLanePx, so adjacent lanes read adjacent pixels; gridDim.x workgroups stride over the
// image.  Six single-byte loads per pixel: an image starts at any byte.  D in 32 bits, D^2 in 64, the two halves
// added apart: per lane, per wave (shuffles), per workgroup (LDS), then one 64-bit vector atomic per workgroup and
// half.  All integer adds: the same sums whatever the grid and whatever order the atomics land in.
constexpr int kLumaSseThreads = 256;
constexpr int kLumaSseLanePx = 8;                                   // kernels.LUMA_SSE_BLOCK[1]
constexpr int kLumaSsePx = kLumaSseThreads * kLumaSseLanePx;        // kernels.LUMA_SSE_BLOCK[0]
constexpr int kLumaSseMaxBlocks = 1024;                             // kernels.LUMA_SSE_MAX_BLOCKS: stride beyond

struct LumaSpan {
  int64_t off;   // first byte of the image in a and in b
  int64_t n;     // pixels
};

// grr_u8_luma_sse: one image of n pixels at a and b
struct LumaSseOne {
  int64_t n;
  __device__ __forceinline__ LumaSpan image(int) const { return LumaSpan{0, n}; }
};

// grr_u8_luma_sse_images: image blockIdx.y of the device image table [n_img, 3] (element offset, H, W).  The
// offset is clamped into [0, elems), H and W into [1, 2^31) and the pixel count to what the arena holds from the
// offset on, so every byte read lies inside the arenas and the loop ends with the arena.
struct LumaSseArena {
  const int64_t* img_table;
  int64_t elems;
  __device__ __forceinline__ LumaSpan image(int i) const {
    const int64_t* it = img_table + (int64_t)i * 3;
    const int64_t lim = (1ll << 31) - 1;
    const int64_t off = it[0] < 0 ? 0 : (it[0] > elems - 1 ? elems - 1 : it[0]);
    const int64_t h = it[1] < 1 ? 1 : (it[1] > lim ? lim : it[1]), w = it[2] < 1 ? 1 : (it[2] > lim ? lim : it[2]);
    const int64_t fit = (elems - off) / 3, n = h * w;
    return LumaSpan{off, n < fit ? n : fit};
  }
};

template <typename Src>
__global__ __launch_bounds__(kLumaSseThreads) void u8_luma_sse_kernel(const uint8_t* __restrict__ a,
                                                                      const uint8_t* __restrict__ b, Src src,
                                                                      unsigned long long* out) {
  const LumaSpan im = src.image(blockIdx.y);
  const uint8_t* __restrict__ pa = a + im.off;
  const uint8_t* __restrict__ pb = b + im.off;
  unsigned long long lo = 0, hi = 0;      // sum (D^2 mod 2^32) < 2^62, sum (D^2 >> 32) < 2^50 over n < 2^30 pixels
  for (int64_t base = (int64_t)blockIdx.x * kLumaSsePx; base < im.n; base += (int64_t)gridDim.x * kLumaSsePx) {
#pragma unroll
    for (int k = 0; k < kLumaSseLanePx; ++k) {
      const int64_t px = base + k * kLumaSseThreads + threadIdx.x;
      if (px < im.n) {
        const uint8_t* x = pa + 3 * px;
        const uint8_t* y = pb + 3 * px;
        const int d = (int)kLumaR * ((int)x[0] - (int)y[0]) + (int)kLumaG * ((int)x[1] - (int)y[1]) +
                      (int)kLumaB * ((int)x[2] - (int)y[2]);                       // |d| <= 55 845 000
        const unsigned long long d2 = (unsigned long long)((long long)d * (long long)d);
        lo += d2 & 0xffffffffull;
        hi += d2 >> 32;
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    lo += __shfl_down(lo, off, kWave);
    hi += __shfl_down(hi, off, kWave);
  }
  // the waves' sums through LDS: both words of an image share a cache line, and atomics on one line run one after
  // another chip-wide, so a workgroup sends one pair, not one per wave
  __shared__ unsigned long long part[2][kLumaSseThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[0][threadIdx.x / kWave] = lo;
    part[1][threadIdx.x / kWave] = hi;
  }
  __syncthreads();      // every lane arrives: nothing above returns
  if (threadIdx.x == 0) {
    lo = hi = 0;
#pragma unroll
    for (int w = 0; w < kLumaSseThreads / kWave; ++w) {
      lo += part[0][w];
      hi += part[1][w];
    }
    if (lo) atomicAdd(out + 2 * (int64_t)blockIdx.y, lo);
    if (hi) atomicAdd(out + 2 * (int64_t)blockIdx.y + 1, hi);
  }
}

// ---------------------------------------------------------------------------
// The blocking sums of PSNR-B (include/grr.h): over the horizontally and vertically adjacent pairs of one channel,
// the squared differences and the counts of the pairs that straddle a multiple-of-8 line (S_b, N_b) and of the rest
// (S_n, N_n).  The workgroup and lane shape is the luma SSE's: 2048 consecutive bytes per step, lane t the bytes
// t + 256 k; a byte owns its pair to the right (the same channel of the next pixel) and its pair below.  Integer
// adds per lane, per wave, per workgroup, then one 64-bit vector atomic per workgroup and word.
constexpr int kBlockingThreads = 256;
constexpr int kBlockingLaneBytes = 8;
constexpr int kBlockingBytes = kBlockingThreads * kBlockingLaneBytes;   // kernels.BLOCKING_BLOCK
constexpr int kBlockingMaxBlocks = 1024;                                // kernels.BLOCKING_MAX_BLOCKS: stride beyond

template <typename Src>
__global__ __launch_bounds__(kBlockingThreads) void u8_blocking_kernel(const uint8_t* __restrict__ p, Src src, int C,
                                                                       unsigned long long* out) {
  const SsimImage im = src.image(blockIdx.y);
  const uint32_t rowlen = (uint32_t)im.W * (uint32_t)C;           // H W C < 2^31: a byte's index fits 32 bits
  const int64_t n = (int64_t)im.H * rowlen;
  unsigned long long v[4] = {0, 0, 0, 0};                         // S_b, N_b, S_n, N_n
  for (int64_t base = (int64_t)blockIdx.x * kBlockingBytes; base < n; base += (int64_t)gridDim.x * kBlockingBytes) {
#pragma unroll
    for (int k = 0; k < kBlockingLaneBytes; ++k) {
      const int64_t e = base + k * kBlockingThreads + threadIdx.x;
      if (e < n) {
        const uint32_t y = (uint32_t)e / rowlen, x = ((uint32_t)e - y * rowlen) / (uint32_t)C;
        const int here = p[src.clamped(im.off + e)];
        if (x + 1 < (uint32_t)im.W) {
          const int d = here - (int)p[src.clamped(im.off + e + C)];
          const bool edge = (x & 7) == 7;
          v[0] += edge ? (unsigned long long)(d * d) : 0ull;
          v[1] += edge ? 1 : 0;
          v[2] += edge ? 0ull : (unsigned long long)(d * d);
          v[3] += edge ? 0 : 1;
        }
        if (y + 1 < (uint32_t)im.H) {
          const int d = here - (int)p[src.clamped(im.off + e + rowlen)];
          const bool edge = (y & 7) == 7;
          v[0] += edge ? (unsigned long long)(d * d) : 0ull;
          v[1] += edge ? 1 : 0;
          v[2] += edge ? 0ull : (unsigned long long)(d * d);
          v[3] += edge ? 0 : 1;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[j] += __shfl_down(v[j], off, kWave);
  __shared__ unsigned long long part[4][kBlockingThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) part[j][threadIdx.x / kWave] = v[j];
  }
  __syncthreads();      // every lane arrives: nothing above returns
  if (threadIdx.x < 4) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kBlockingThreads / kWave; ++w) s += part[threadIdx.x][w];
    if (s) atomicAdd(out + 4 * (int64_t)blockIdx.y + threadIdx.x, s);
  }
}

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_u8_ssim_supported(int C, int H, int W) {
  return C >= 1 && C <= 4 && H >= kSsimTaps && W >= kSsimTaps && (int64_t)H * W * C < (1ll << 31) ? 1 : 0;
}

grr_status grr_u8_ssim(const uint8_t* a, const uint8_t* b, int H, int W, int C, int64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && out && H > 0 && W > 0 && C > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG,
              "grr_u8_ssim: bad args");
  GRR_REQUIRE(grr_u8_ssim_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "grr_u8_ssim: needs C <= 4, H and W >= 11 and H W C < 2^31 (got %d x %d x %d)", H, W, C);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(int64_t), s) == hipSuccess, GRR_ERR_HIP, "grr_u8_ssim: zeroing the sum failed");
  // tiles <= H W C < 2^31
  ssim_launch(C, dim3((uint32_t)ssim_tiles(H, W, C)), s, a, b, SsimOne{H, W}, reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_ssim");
}

grr_status grr_u8_ssim_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, int C, const int64_t* img_table,
                              int n_img, int max_h, int max_w, int64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && img_table && out && arena_elems > 0 && C > 0 && n_img > 0 && max_h > 0 && max_w > 0 &&
                  (uintptr_t)out % 8 == 0 && (uintptr_t)img_table % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_u8_ssim_images: bad args");
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "grr_u8_ssim_images: needs C <= 4, n_img <= arena_elems < 2^62 (got C %d, %d images, %lld elements)", C,
              n_img, (long long)arena_elems);
  GRR_REQUIRE(n_img <= kSsimMaxImages, GRR_ERR_UNSUPPORTED,
              "grr_u8_ssim_images: at most %d images per call, one grid row each (got %d)", kSsimMaxImages, n_img);
  const bool any = max_h >= kSsimTaps && max_w >= kSsimTaps;      // else no image has a valid pixel: all sums are 0
  const int64_t tiles = any ? ssim_tiles(max_h, max_w, C) : 0;
  GRR_REQUIRE(tiles < (1ll << 31), GRR_ERR_UNSUPPORTED,
              "grr_u8_ssim_images: max_h x max_w x C must be below 2^31 tiles of %d x %d (got %d x %d x %d)", kSsimRows,
              kSsimCols, max_h, max_w, C);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(int64_t) * n_img, s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_ssim_images: zeroing the sums failed");
  if (!any) return GRR_OK;
  ssim_launch(C, dim3((uint32_t)tiles, (uint32_t)n_img), s, a, b, SsimArena{img_table, arena_elems, max_h, max_w},
              reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_ssim_images");
}

int grr_u8_luma_supported(int H, int W, int need_window) {
  const int least = need_window ? kSsimTaps : 1;
  return H >= least && W >= least && (int64_t)H * W * 3 < (1ll << 31) ? 1 : 0;
}

grr_status grr_u8_luma_sse(const uint8_t* a, const uint8_t* b, int H, int W, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && out && H > 0 && W > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG,
              "grr_u8_luma_sse: bad args");
  GRR_REQUIRE(grr_u8_luma_supported(H, W, 0), GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_sse: needs H W 3 < 2^31 (got %d x %d x 3)", H, W);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, 2 * sizeof(uint64_t), s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_luma_sse: zeroing the sums failed");
  const int64_t n = (int64_t)H * W;
  const int blocks = (int)std::min<int64_t>((n + kLumaSsePx - 1) / kLumaSsePx, kLumaSseMaxBlocks);
  hipLaunchKernelGGL((u8_luma_sse_kernel<LumaSseOne>), dim3(blocks), dim3(kLumaSseThreads), 0, s, a, b, LumaSseOne{n},
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_luma_sse");
}

grr_status grr_u8_luma_sse_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, const int64_t* img_table,
                                  int n_img, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && img_table && out && arena_elems > 0 && n_img > 0 && (uintptr_t)out % 8 == 0 &&
                  (uintptr_t)img_table % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_u8_luma_sse_images: bad args");
  GRR_REQUIRE(grr_image_arena_supported(3, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_sse_images: needs n_img <= arena_elems < 2^62 (got %d images, %lld elements)", n_img,
              (long long)arena_elems);
  GRR_REQUIRE(n_img <= kSsimMaxImages, GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_sse_images: at most %d images per call, one grid row each (got %d)", kSsimMaxImages, n_img);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, 2 * sizeof(uint64_t) * n_img, s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_luma_sse_images: zeroing the sums failed");
  // workgroups per image from the mean image: one step each, at most 256
  const int64_t px = arena_elems / 3 / n_img;
  const int bx = (int)std::min<int64_t>(std::max<int64_t>((px + kLumaSsePx - 1) / kLumaSsePx, 1), 256);
  hipLaunchKernelGGL((u8_luma_sse_kernel<LumaSseArena>), dim3(bx, n_img), dim3(kLumaSseThreads), 0, s, a, b,
                     LumaSseArena{img_table, arena_elems}, reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_luma_sse_images");
}

grr_status grr_u8_luma_ssim(const uint8_t* a, const uint8_t* b, int H, int W, int64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && out && H > 0 && W > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG,
              "grr_u8_luma_ssim: bad args");
  GRR_REQUIRE(grr_u8_luma_supported(H, W, 1), GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_ssim: needs H and W >= 11 and H W 3 < 2^31 (got %d x %d x 3)", H, W);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(int64_t), s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_luma_ssim: zeroing the sum failed");
  luma_ssim_launch(dim3((uint32_t)ssim_tiles(H, W, 1)), s, a, b, SsimOne{H, W}, reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_luma_ssim");
}

grr_status grr_u8_luma_ssim_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, const int64_t* img_table,
                                   int n_img, int max_h, int max_w, int64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && img_table && out && arena_elems > 0 && n_img > 0 && max_h > 0 && max_w > 0 &&
                  (uintptr_t)out % 8 == 0 && (uintptr_t)img_table % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_u8_luma_ssim_images: bad args");
  GRR_REQUIRE(grr_image_arena_supported(3, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_ssim_images: needs n_img <= arena_elems < 2^62 (got %d images, %lld elements)", n_img,
              (long long)arena_elems);
  GRR_REQUIRE(n_img <= kSsimMaxImages, GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_ssim_images: at most %d images per call, one grid row each (got %d)", kSsimMaxImages, n_img);
  const bool any = max_h >= kSsimTaps && max_w >= kSsimTaps;      // else no image has a valid pixel: all sums are 0
  const int64_t tiles = any ? ssim_tiles(max_h, max_w, 1) : 0;
  GRR_REQUIRE(tiles < (1ll << 31), GRR_ERR_UNSUPPORTED,
              "grr_u8_luma_ssim_images: max_h x max_w must be below 2^31 tiles of %d x %d (got %d x %d)", kSsimRows,
              kSsimCols, max_h, max_w);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(int64_t) * n_img, s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_luma_ssim_images: zeroing the sums failed");
  if (!any) return GRR_OK;
  luma_ssim_launch(dim3((uint32_t)tiles, (uint32_t)n_img), s, a, b, SsimArena{img_table, arena_elems, max_h, max_w},
                   reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_luma_ssim_images");
}

grr_status grr_u8_blocking(const uint8_t* est, int H, int W, int C, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(est && out && H > 0 && W > 0 && C > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG,
              "grr_u8_blocking: bad args");
  GRR_REQUIRE(grr_image_io_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "grr_u8_blocking: needs C <= 4 and H W C < 2^31 (got %d x %d x %d)", H, W, C);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, 4 * sizeof(uint64_t), s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_blocking: zeroing the sums failed");
  const int64_t n = (int64_t)H * W * C;
  const int blocks = (int)std::min<int64_t>((n + kBlockingBytes - 1) / kBlockingBytes, kBlockingMaxBlocks);
  hipLaunchKernelGGL((u8_blocking_kernel<SsimOne>), dim3(blocks), dim3(kBlockingThreads), 0, s, est, SsimOne{H, W}, C,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_blocking");
}

grr_status grr_u8_blocking_images(const uint8_t* est, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                                  int max_h, int max_w, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(est && img_table && out && arena_elems > 0 && C > 0 && n_img > 0 && max_h > 0 && max_w > 0 &&
                  (uintptr_t)out % 8 == 0 && (uintptr_t)img_table % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_u8_blocking_images: bad args");
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "grr_u8_blocking_images: needs C <= 4, n_img <= arena_elems < 2^62 (got C %d, %d images, %lld elements)", C,
              n_img, (long long)arena_elems);
  GRR_REQUIRE(n_img <= kSsimMaxImages, GRR_ERR_UNSUPPORTED,
              "grr_u8_blocking_images: at most %d images per call, one grid row each (got %d)", kSsimMaxImages, n_img);
  GRR_REQUIRE(grr_image_io_supported(C, max_h, max_w), GRR_ERR_UNSUPPORTED,
              "grr_u8_blocking_images: max_h x max_w x C must be below 2^31 (got %d x %d x %d)", max_h, max_w, C);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, 4 * sizeof(uint64_t) * n_img, s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_blocking_images: zeroing the sums failed");
  // workgroups per image from the mean image: one step each, at most 256
  const int64_t bytes = arena_elems / n_img;
  const int bx = (int)std::min<int64_t>(std::max<int64_t>((bytes + kBlockingBytes - 1) / kBlockingBytes, 1), 256);
  hipLaunchKernelGGL((u8_blocking_kernel<SsimArena>), dim3(bx, n_img), dim3(kBlockingThreads), 0, s, est,
                     SsimArena{img_table, arena_elems, max_h, max_w}, C, reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_blocking_images");
}

}  // extern "C"
