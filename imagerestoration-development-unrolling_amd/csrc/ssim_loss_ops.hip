// The SSIM training loss on float32 planar batches, forward and reverse, gfx950.
//
//   grr_ssim_loss_forward   per batch item the exact integer sum of rint(2^32 s) over its C (H - 10)(W - 10) valid
//                           positions and, on request, the three float64 coefficient planes the reverse needs
//   grr_ssim_loss_backward  the gradient of loss = 1 - (sum s) / N with respect to the prediction x
//
// Definition (include/grr.h has it in full): the index of metric_ops.hip -- the window, the tile, the order of every
// float64 operation and the quantisation are the same, the taps and the tile constants are ssim_window.h's -- on
// float planes of data range 1 (C1 = 1e-4, C2 = 9e-4), x the prediction and y the target, neither clamped.
// With A1 = 2 mx my + C1, A2 = 2 vxy + C2, B1 = mx^2 + my^2 + C1, B2 = vx + vy + C2 and s = A1 A2 / (B1 B2):
//
//   c0 = ds/dmx     = 2 my (A2 - A1) / (B1 B2) - 2 mx s / B1 + 2 mx s / B2
//   c1 = ds/dE[x^2] = -s / B2
//   c2 = ds/dE[xy]  = 2 A1 / (B1 B2)
//
//   dloss/dx = -(1 / N) (F*(c0) + 2 x F*(c1) + y F*(c2)),   N = B C (H - 10)(W - 10)
//
// F* the window's adjoint: F*(c)[i, j] = sum over k, l of g[k] g[l] c[i - k, j - l], c zero outside its
// (H - 10) x (W - 10) positions.  Where x is close to y the three terms are of size 1 / C2 and cancel, so the
// coefficient planes are float64 and so is everything up to the one rounding of the gradient to float32.
//
// Forward: u8_ssim_kernel's body over one (b, c) plane per blockIdx.y.  A 256-thread workgroup owns 256 valid
// columns by 32 valid rows; per input row it stages 266 floats of x and of y as float64 in LDS (two buffers, one
// barrier per row, the next row in flight), each lane forms its five horizontal sums into an 11-slot register ring
// with compile-time slots, and from the tile's 11th row on it emits one valid row per input row: s, q added per
// lane, wave, then one 64-bit vector atomic per wave into the item's sum; and the three coefficients, stored as they
// are formed.  The integer sum does not depend on the grid or on the order the atomics land in.
//
// Reverse: a gather, no atomics.  The same body over the coefficient planes with 10 zero rows and columns implied
// on every side: a workgroup owns 256 x 32 pixels of a plane, stages per padded row 266 float64 of each of the three
// planes, keeps three horizontal sums in the ring, and emits F*(c0), F*(c1), F*(c2) of one pixel row per padded
// row; these are combined with x and y, scaled by -1 / N and by the incoming gradient (one float read from the
// device) and rounded once.  Every pixel's value is formed in one fixed order: run-to-run identical.
#include "grr_common.h"
#include "ssim_window.h"

#pragma clang fp contract(off)

namespace grr {
namespace {

constexpr int kLossMaxPlanes = 65535;       // one grid row (blockIdx.y) per (b, c) plane; kernels.MAX_SSIM_LOSS_PLANES
constexpr int kExtra = kSsimTaps - 1;       // columns a tile's row needs beyond its 256

__device__ __forceinline__ float plane_col(const float* __restrict__ p, int64_t row0, int col, int W) {
  return col < W ? p[row0 + col] : 0.0f;    // 0 beyond the row: no valid column reads it
}

template <bool kCoef>
__global__ __launch_bounds__(kSsimThreads) void ssim_loss_fwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ y, int C, int H, int W,
                                                                     SsimTaps taps, unsigned long long* qsum,
                                                                     double* __restrict__ coef) {
  __shared__ double lds[2][2][kSsimCols + kExtra];        // [buffer][x, y][column of the tile]
  const int vcols = W - kExtra, vrows = H - kExtra;
  const int tcols = (vcols + kSsimCols - 1) / kSsimCols;
  const int j0 = (int)(blockIdx.x % tcols) * kSsimCols;
  const int r0 = (int)(blockIdx.x / tcols) * kSsimRows;
  const int rin_end = min(r0 + kSsimRows, vrows) + kExtra;            // input rows [r0, rin_end), rin_end <= H
  const int64_t plane = blockIdx.y, base = plane * H * W;            // B C H W < 2^31
  const int t = threadIdx.x;
  const bool active = j0 + t < vcols;
  const bool extra = t < kExtra;

  // what this lane stages for the row in flight: column j0 + t and, for the first 10 lanes, j0 + 256 + t
  float px0, py0, px1 = 0.0f, py1 = 0.0f;
  {
    const int64_t row0 = base + (int64_t)r0 * W;
    px0 = plane_col(x, row0, j0 + t, W);
    py0 = plane_col(y, row0, j0 + t, W);
    if (extra) {
      px1 = plane_col(x, row0, j0 + kSsimCols + t, W);
      py1 = plane_col(y, row0, j0 + kSsimCols + t, W);
    }
  }

  double ring[kSsimTaps][5];     // horizontal sums (x, y, x^2, y^2, xy) of the last 11 input rows; slot = (r - r0) % 11
#pragma unroll
  for (int p = 0; p < kSsimTaps; ++p)
#pragma unroll
    for (int m = 0; m < 5; ++m) ring[p][m] = 0.0;
  long long acc = 0;
  const int64_t cplane = (int64_t)vrows * vcols, cstride = (int64_t)gridDim.y * cplane;   // [3, B C, vrows, vcols]

  for (int rb = r0; rb < rin_end; rb += kSsimTaps) {
#pragma unroll
    for (int p = 0; p < kSsimTaps; ++p) {
      const int r = rb + p;                    // input row; block-uniform
      if (r < rin_end) {
        double* lx = lds[(r - r0) & 1][0];
        double* ly = lds[(r - r0) & 1][1];
        lx[t] = (double)px0;
        ly[t] = (double)py0;
        if (extra) {
          lx[kSsimCols + t] = (double)px1;
          ly[kSsimCols + t] = (double)py1;
        }
        if (r + 1 < rin_end) {
          const int64_t row0 = base + (int64_t)(r + 1) * W;
          px0 = plane_col(x, row0, j0 + t, W);
          py0 = plane_col(y, row0, j0 + t, W);
          if (extra) {
            px1 = plane_col(x, row0, j0 + kSsimCols + t, W);
            py1 = plane_col(y, row0, j0 + kSsimCols + t, W);
          }
        }
        // this buffer was last read two rows ago, before the previous row's barrier
        __syncthreads();
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < kSsimTaps; ++k) {
          const double a = lx[t + k], b = ly[t + k], g = taps.g[k];
          hx = __builtin_fma(g, a, hx);
          hy = __builtin_fma(g, b, hy);
          hxx = __builtin_fma(g, a * a, hxx);      // a product of two float32 values is exact in float64
          hyy = __builtin_fma(g, b * b, hyy);
          hxy = __builtin_fma(g, a * b, hxy);
        }
        ring[p][0] = hx;
        ring[p][1] = hy;
        ring[p][2] = hxx;
        ring[p][3] = hyy;
        ring[p][4] = hxy;
        if (r - r0 >= kSsimTaps - 1) {           // valid row r - 10: input rows r - 10..r = slots p + 1..p + 11
          double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = __builtin_fma(taps.g[k], ring[(p + 1 + k) % kSsimTaps][m], v[m]);
          const double mx = v[0], my = v[1];
          const double mxx = mx * mx, myy = my * my, mxy = mx * my;
          const double vx = v[2] - mxx, vy = v[3] - myy, vxy = v[4] - mxy;
          const double a1 = 2.0 * mxy + kSsimUnitC1, a2 = 2.0 * vxy + kSsimUnitC2;
          const double b1 = mxx + myy + kSsimUnitC1, b2 = vx + vy + kSsimUnitC2;
          const double num = a1 * a2, den = b1 * b2;
          const double s = num / den;
          if (active) {
            acc += __double2ll_rn(s * 4294967296.0);
            if (kCoef) {
              const double c0 = (2.0 * my) * (a2 - a1) / den - (2.0 * mx) * s / b1 + (2.0 * mx) * s / b2;
              double* out = coef + plane * cplane + (int64_t)(r - kExtra) * vcols + (j0 + t);
              out[0] = c0;
              out[cstride] = -s / b2;
              out[2 * cstride] = (2.0 * a1) / den;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(qsum + plane / C, (unsigned long long)acc);
}

// coefficient (cr, cc) of a plane, 0 in the implied border
__device__ __forceinline__ double coef_at(const double* __restrict__ p, int cr, int cc, int vrows, int vcols) {
  return cr >= 0 && cr < vrows && cc >= 0 && cc < vcols ? p[(int64_t)cr * vcols + cc] : 0.0;
}

__global__ __launch_bounds__(kSsimThreads) void ssim_loss_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ y,
                                                                     const double* __restrict__ coef,
                                                                     const float* __restrict__ gout,
                                                                     float* __restrict__ gx, int H, int W,
                                                                     double neg_inv_n, SsimTaps taps) {
  __shared__ double lds[2][3][kSsimCols + kExtra];        // [buffer][c0, c1, c2][padded column of the tile]
  const int vcols = W - kExtra, vrows = H - kExtra;
  const int tcols = (W + kSsimCols - 1) / kSsimCols;
  const int j0 = (int)(blockIdx.x % tcols) * kSsimCols;   // pixel (i, j) reads the padded rows i..i + 10 and columns
  const int r0 = (int)(blockIdx.x / tcols) * kSsimRows;   // j..j + 10; padded (pr, pc) is coefficient (pr - 10, pc - 10)
  const int rin_end = min(r0 + kSsimRows, H) + kExtra;    // padded rows [r0, rin_end)
  const int64_t plane = blockIdx.y, cplane = (int64_t)vrows * vcols, cstride = (int64_t)gridDim.y * cplane;
  const double* __restrict__ cp = coef + plane * cplane;
  const int t = threadIdx.x;
  const bool active = j0 + t < W;
  const bool extra = t < kExtra;
  const int cc0 = j0 + t - kExtra, cc1 = j0 + kSsimCols + t - kExtra;

  double p0[3], p1[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    p0[m] = coef_at(cp + m * cstride, r0 - kExtra, cc0, vrows, vcols);
    if (extra) p1[m] = coef_at(cp + m * cstride, r0 - kExtra, cc1, vrows, vcols);
  }

  double ring[kSsimTaps][3];     // horizontal sums of c0, c1, c2 of the last 11 padded rows; slot = (pr - r0) % 11
#pragma unroll
  for (int p = 0; p < kSsimTaps; ++p)
#pragma unroll
    for (int m = 0; m < 3; ++m) ring[p][m] = 0.0;
  const double scale = (double)gout[0];
  const int64_t base = plane * H * W;

  for (int rb = r0; rb < rin_end; rb += kSsimTaps) {
#pragma unroll
    for (int p = 0; p < kSsimTaps; ++p) {
      const int pr = rb + p;                   // padded row; block-uniform
      if (pr < rin_end) {
        double(*l)[kSsimCols + kExtra] = lds[(pr - r0) & 1];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          l[m][t] = p0[m];
          if (extra) l[m][kSsimCols + t] = p1[m];
        }
        if (pr + 1 < rin_end) {
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            p0[m] = coef_at(cp + m * cstride, pr + 1 - kExtra, cc0, vrows, vcols);
            if (extra) p1[m] = coef_at(cp + m * cstride, pr + 1 - kExtra, cc1, vrows, vcols);
          }
        }
        // this buffer was last read two rows ago, before the previous row's barrier
        __syncthreads();
        double h[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
          for (int m = 0; m < 3; ++m) h[m] = __builtin_fma(taps.g[k], l[m][t + k], h[m]);   // g[10 - k] == g[k]
#pragma unroll
        for (int m = 0; m < 3; ++m) ring[p][m] = h[m];
        if (pr - r0 >= kSsimTaps - 1) {          // pixel row pr - 10: padded rows pr - 10..pr = slots p + 1..p + 11
          double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
            for (int m = 0; m < 3; ++m) v[m] = __builtin_fma(taps.g[k], ring[(p + 1 + k) % kSsimTaps][m], v[m]);
          if (active) {
            const int64_t e = base + (int64_t)(pr - kExtra) * W + (j0 + t);
            const double xv = (double)x[e], yv = (double)y[e];
            const double d = v[0] + (2.0 * xv) * v[1] + yv * v[2];
            gx[e] = (float)(d * neg_inv_n * scale);
          }
        }
      }
    }
  }
}

int64_t tiles(int rows, int cols) {
  return (int64_t)((cols + kSsimCols - 1) / kSsimCols) * ((rows + kSsimRows - 1) / kSsimRows);
}

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_ssim_loss_supported(int B, int C, int H, int W) {
  return B >= 1 && C >= 1 && H >= kSsimTaps && W >= kSsimTaps && (int64_t)B * C <= kLossMaxPlanes &&
                 (int64_t)B * C * H * W < (1ll << 31)
             ? 1
             : 0;
}

grr_status grr_ssim_loss_forward(const float* x, const float* y, int B, int C, int H, int W, int64_t* qsum, double* coef,
                                 void* stream) {
  clear_error();
  GRR_REQUIRE(x && y && qsum && B > 0 && C > 0 && H > 0 && W > 0 && (uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 &&
                  (uintptr_t)qsum % 8 == 0 && (uintptr_t)coef % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_ssim_loss_forward: bad args");
  GRR_REQUIRE(grr_ssim_loss_supported(B, C, H, W), GRR_ERR_UNSUPPORTED,
              "grr_ssim_loss_forward: needs H and W >= 11, B C <= %d and B C H W < 2^31 (got %d x %d x %d x %d)",
              kLossMaxPlanes, B, C, H, W);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(qsum, 0, sizeof(int64_t) * B, s) == hipSuccess, GRR_ERR_HIP,
              "grr_ssim_loss_forward: zeroing the sums failed");
  const dim3 grid((uint32_t)tiles(H - kExtra, W - kExtra), (uint32_t)(B * C));      // tiles <= H W < 2^31
  unsigned long long* out = reinterpret_cast<unsigned long long*>(qsum);
  if (coef)
    hipLaunchKernelGGL(ssim_loss_fwd_kernel<true>, grid, dim3(kSsimThreads), 0, s, x, y, C, H, W, kTaps, out, coef);
  else
    hipLaunchKernelGGL(ssim_loss_fwd_kernel<false>, grid, dim3(kSsimThreads), 0, s, x, y, C, H, W, kTaps, out, coef);
  return launch_status("grr_ssim_loss_forward");
}

grr_status grr_ssim_loss_backward(const float* x, const float* y, const double* coef, const float* gout, float* gx,
                                  int B, int C, int H, int W, void* stream) {
  clear_error();
  GRR_REQUIRE(x && y && coef && gout && gx && B > 0 && C > 0 && H > 0 && W > 0 && (uintptr_t)x % 4 == 0 &&
                  (uintptr_t)y % 4 == 0 && (uintptr_t)gout % 4 == 0 && (uintptr_t)gx % 4 == 0 && (uintptr_t)coef % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_ssim_loss_backward: bad args");
  GRR_REQUIRE(grr_ssim_loss_supported(B, C, H, W), GRR_ERR_UNSUPPORTED,
              "grr_ssim_loss_backward: needs H and W >= 11, B C <= %d and B C H W < 2^31 (got %d x %d x %d x %d)",
              kLossMaxPlanes, B, C, H, W);
  const double n = (double)((int64_t)B * C * (H - kExtra) * (W - kExtra));          // < 2^31: exact
  hipLaunchKernelGGL(ssim_loss_bwd_kernel, dim3((uint32_t)tiles(H, W), (uint32_t)(B * C)), dim3(kSsimThreads), 0,
                     (hipStream_t)stream, x, y, coef, gout, gx, H, W, -1.0 / n, kTaps);
  return launch_status("grr_ssim_loss_backward");
}

}  // extern "C"
