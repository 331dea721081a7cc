// Encoder / decoder convolutions of the v1.0 model (AbtractMultiScaleGraphFilter, REF:991-1174) as gfx950
// kernels, so that a forward and a training step of that model issue no library convolution or GEMM:
//   ReginalPixelEmbeding   REF:991-1009    3x3, replicate padding   grr_conv3x3_embed (+ _bwd_w, _bwd_x)
//   Upsampling             REF:1019-1025   ConvTranspose2d 2x2 / 2  grr_convt2x2s2
// (Downsampling, the combines and linear_output run on grr_conv2x2s2 / grr_conv1x1_ws, feature_ops.hip.)
//
// grr_conv3x3_embed is store bound (K = 9 Cin <= 36: 4 M bytes written per pixel against 4 Cin read).  A
// lane owns 4 consecutive pixels of a row, keeps their 3 x 6 clamped inputs per channel in registers, reads
// the weights from LDS (wave-uniform addresses: broadcast reads) and walks the M output channels with one
// 16-byte store each.  Every output is ONE fmaf chain over (c, ky, kx) in ascending order, so a value does
// not depend on the tiling, the batch or the pixel's position in the lane.
//
// Its weight gradient gathers the 9 Cin clamped taps of every pixel into a [B, 9 Cin, P] patch tensor and
// reduces it against g on grr_wgrad (split-bf16 MFMA, partial tiles added in a fixed order); the data
// gradient is the adjoint of the clamped gather written as a gather (border pixels collect the taps that
// were clamped onto them) -- a training step never asks for it, it only has to be right.
//
// grr_convt2x2s2 is a 1x1 GEMM with the 4 M rows (m, di, dj) on the split-bf16 kernels of grr_conv1x1_ws
// (gemm_x3 up to K = 128, gemm_x3k above) into a workspace tensor, then a 2x2 interleave whose lanes
// read the two dj rows of a pixel and write them as one 8-byte store (512 contiguous bytes per wave).
#include "grr_common.h"

#include <algorithm>

namespace grr {

namespace {

constexpr int CD_NT = 256;
constexpr int EMB_MAX_CIN = 4, EMB_MAX_M = 128;

inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }
unsigned cd_grid(int64_t n, int64_t cap = 1 << 14) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + CD_NT - 1) / CD_NT, cap));
}

// ---- 3x3 embedding, forward ------------------------------------------------------------------
// item = (b, y, quad of 4 pixels); vec: W % 4 == 0 and 16-byte aligned x / out (16-byte loads and stores)
template <int CIN>
__global__ __launch_bounds__(CD_NT) void embed_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                          float* __restrict__ out, int M, int H, int W, int nq,
                                                          int64_t items, int vec) {
  extern __shared__ __attribute__((aligned(16))) float emb_w[];   // [M][CIN * 9]
  for (int i = threadIdx.x; i < M * CIN * 9; i += CD_NT) emb_w[i] = wt[i];
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  for (int64_t it = blockIdx.x * (int64_t)CD_NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * CD_NT) {
    const int q = (int)(it % nq);
    const int64_t r = it / nq;
    const int y = (int)(r % H);
    const int64_t b = r / H;
    const int x0 = 4 * q;
    const bool quad = vec && x0 + 3 < W;
    const float* xb = x + b * CIN * HW;
    float v[CIN][3][6];
#pragma unroll
    for (int c = 0; c < CIN; ++c)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* row = xb + c * HW + (int64_t)clampi(y + ky - 1, 0, H - 1) * W;
        v[c][ky][0] = row[max(x0 - 1, 0)];
        if (quad) {
          const float4 f = *reinterpret_cast<const float4*>(row + x0);
          v[c][ky][1] = f.x; v[c][ky][2] = f.y; v[c][ky][3] = f.z; v[c][ky][4] = f.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c][ky][1 + j] = row[min(x0 + j, W - 1)];
        }
        v[c][ky][5] = row[min(x0 + 4, W - 1)];
      }
    float* ob = out + b * M * HW + (int64_t)y * W + x0;
    for (int m = 0; m < M; ++m) {
      const float* wm = emb_w + m * (CIN * 9);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int c = 0; c < CIN; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float w = wm[(c * 3 + ky) * 3 + kx];
            a0 = __builtin_fmaf(w, v[c][ky][kx], a0);
            a1 = __builtin_fmaf(w, v[c][ky][kx + 1], a1);
            a2 = __builtin_fmaf(w, v[c][ky][kx + 2], a2);
            a3 = __builtin_fmaf(w, v[c][ky][kx + 3], a3);
          }
      float* o = ob + m * HW;
      if (quad) {
        *reinterpret_cast<float4*>(o) = make_float4(a0, a1, a2, a3);
      } else {
        o[0] = a0;                       // x0 < W for every item
        if (x0 + 1 < W) o[1] = a1;
        if (x0 + 2 < W) o[2] = a2;
        if (x0 + 3 < W) o[3] = a3;
      }
    }
  }
}

// ---- 3x3 embedding, reverse ------------------------------------------------------------------
// patches[b][(c, ky, kx)][p] = x[b][c][clamp(p + (ky - 1, kx - 1))]: the B operand of grr_wgrad
__global__ __launch_bounds__(CD_NT) void embed_patches_kernel(const float* __restrict__ x, float* __restrict__ pt,
                                                              int Cin, int H, int W, int64_t n) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = blockIdx.x * (int64_t)CD_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CD_NT) {
    const int64_t b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), xx = (int)(p - (int64_t)y * W);
    const int xl = max(xx - 1, 0), xr = min(xx + 1, W - 1);
    for (int c = 0; c < Cin; ++c) {
      const float* pl = x + (b * Cin + c) * HW;
      float* o = pt + (b * Cin + c) * 9 * HW + p;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* row = pl + (int64_t)clampi(y + ky - 1, 0, H - 1) * W;
        o[(ky * 3 + 0) * HW] = row[xl];
        o[(ky * 3 + 1) * HW] = row[xx];
        o[(ky * 3 + 2) * HW] = row[xr];
      }
    }
  }
}

// gx[b][c][q] = sum_m sum_(ky,kx) sum_{p : clamp(p + (ky - 1, kx - 1)) = q} g[b][m][p] wt[m][c][ky][kx].
// The candidates p lie in q's 3x3 neighbourhood; bit j of ym[ky] says that row qy - 1 + j reaches row qy
// through tap row ky (xm likewise); one fma chain in (m, ky, kx, j, i) order, accumulated in fp64 (each
// product of two floats is exact there) and rounded once: a single fp32 accumulator over the up to 81 M
// terms of a small image drifted past the fp32-class bound of a blocked CPU reduction (1.18e-6 against
// 1.02e-6 at M = 128 on a 2 x 2 image, tests/test_gpu_gemm_class.py).  Off the training path, so the fp64
// rate does not matter.
__global__ __launch_bounds__(CD_NT) void embed_bwd_x_kernel(const float* __restrict__ g, const float* __restrict__ wt,
                                                            float* __restrict__ gx, int Cin, int M, int H, int W,
                                                            int64_t n) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = blockIdx.x * (int64_t)CD_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CD_NT) {
    const int64_t pl = i / HW, q = i - pl * HW;
    const int64_t b = pl / Cin;
    const int c = (int)(pl - b * Cin);
    const int qy = (int)(q / W), qx = (int)(q - (int64_t)qy * W);
    int ym[3], xm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ym[k] = xm[k] = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int py = qy - 1 + j, px = qx - 1 + j;
        if (py >= 0 && py < H && clampi(py + k - 1, 0, H - 1) == qy) ym[k] |= 1 << j;
        if (px >= 0 && px < W && clampi(px + k - 1, 0, W - 1) == qx) xm[k] |= 1 << j;
      }
    }
    double acc = 0.0;
    for (int m = 0; m < M; ++m) {
      const float* gp = g + (b * M + m) * HW;
      const float* wm = wt + ((int64_t)m * Cin + c) * 9;
      float nb[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          nb[j][k] = gp[(int64_t)clampi(qy - 1 + j, 0, H - 1) * W + clampi(qx - 1 + k, 0, W - 1)];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float w = wm[ky * 3 + kx];
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              if ((ym[ky] >> j & 1) && (xm[kx] >> k & 1)) acc = __builtin_fma((double)nb[j][k], (double)w, acc);
        }
    }
    gx[i] = (float)acc;
  }
}

// ---- transposed 2x2 / stride 2 ---------------------------------------------------------------
// w4[(m, di, dj)][k] = wt[k][m][di][dj]: the [4M, K] matrix of the 1x1 GEMM
__global__ __launch_bounds__(CD_NT) void convt_pack_kernel(const float* __restrict__ wt, float* __restrict__ w4, int K,
                                                           int M4) {
  const int n = K * M4;
  for (int i = blockIdx.x * CD_NT + threadIdx.x; i < n; i += gridDim.x * CD_NT) {
    const int r = i / K, k = i - r * K;
    w4[i] = wt[(int64_t)k * M4 + r];
  }
}

// t [B, 4M, H, W] with rows (m, di, dj) -> out [B, M, 2H, 2W].  Item = (row pair r = (b, m, di), pixel):
// rows 2r and 2r + 1 are the two dj of one output row; lanes run along x.
__global__ __launch_bounds__(CD_NT) void convt_interleave_kernel(const float* __restrict__ t, float* __restrict__ out,
                                                                 int H, int W, int64_t n) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = blockIdx.x * (int64_t)CD_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CD_NT) {
    const int64_t r = i / HW, p = i - r * HW;
    const int y = (int)(p / W), xx = (int)(p - (int64_t)y * W);
    const float2 v = make_float2(t[2 * r * HW + p], t[(2 * r + 1) * HW + p]);
    const int64_t bm = r >> 1;
    const int di = (int)(r & 1);
    *reinterpret_cast<float2*>(out + (bm * 2 * H + 2 * y + di) * (2 * (int64_t)W) + 2 * xx) = v;
  }
}

bool embed_ok(int Cin, int M) { return Cin >= 1 && Cin <= EMB_MAX_CIN && M >= 1 && M <= EMB_MAX_M; }

}  // namespace

}  // namespace grr

using namespace grr;

extern "C" {

int grr_conv3x3_embed_supported(int Cin, int M) { return embed_ok(Cin, M) ? 1 : 0; }

grr_status grr_conv3x3_embed(const float* x, const float* wt, float* out, int B, int Cin, int M, int H, int W,
                             void* stream) {
  clear_error();
  GRR_REQUIRE(x && wt && out && B > 0 && Cin > 0 && M > 0 && H > 0 && W > 0, GRR_ERR_INVALID_ARG,
              "grr_conv3x3_embed: bad args");
  GRR_REQUIRE(out != x, GRR_ERR_INVALID_ARG, "grr_conv3x3_embed: out aliases x");
  GRR_REQUIRE(embed_ok(Cin, M), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed: Cin=%d, M=%d outside [1, %d] x [1, %d]", Cin,
              M, EMB_MAX_CIN, EMB_MAX_M);
  GRR_REQUIRE((int64_t)H * W < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed: H*W too large");
  const int nq = (W + 3) / 4;
  const int64_t items = (int64_t)B * H * nq;
  const int vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const dim3 g(cd_grid(items, 1 << 12)), t(CD_NT);
  const size_t lds = (size_t)M * Cin * 9 * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  switch (Cin) {
    case 1: hipLaunchKernelGGL(embed_fwd_kernel<1>, g, t, lds, s, x, wt, out, M, H, W, nq, items, vec); break;
    case 2: hipLaunchKernelGGL(embed_fwd_kernel<2>, g, t, lds, s, x, wt, out, M, H, W, nq, items, vec); break;
    case 3: hipLaunchKernelGGL(embed_fwd_kernel<3>, g, t, lds, s, x, wt, out, M, H, W, nq, items, vec); break;
    default: hipLaunchKernelGGL(embed_fwd_kernel<4>, g, t, lds, s, x, wt, out, M, H, W, nq, items, vec); break;
  }
  return launch_status("grr_conv3x3_embed");
}

int64_t grr_conv3x3_embed_bwd_w_workspace_bytes(int B, int Cin, int M, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || !embed_ok(Cin, M)) return 0;
  const int64_t P = (int64_t)H * W;
  return align256((int64_t)B * 9 * Cin * P * (int64_t)sizeof(float)) + grr_wgrad_workspace_bytes(B, M, 9 * Cin, P);
}

grr_status grr_conv3x3_embed_bwd_w(const float* g, const float* x, float* gw, void* workspace, int B, int Cin, int M,
                                   int H, int W, void* stream) {
  clear_error();
  GRR_REQUIRE(g && x && gw && workspace && B > 0 && Cin > 0 && M > 0 && H > 0 && W > 0, GRR_ERR_INVALID_ARG,
              "grr_conv3x3_embed_bwd_w: bad args");
  GRR_REQUIRE(embed_ok(Cin, M), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed_bwd_w: Cin=%d, M=%d outside [1, %d] x [1, %d]",
              Cin, M, EMB_MAX_CIN, EMB_MAX_M);
  GRR_REQUIRE(((uintptr_t)workspace & 255) == 0, GRR_ERR_INVALID_ARG,
              "grr_conv3x3_embed_bwd_w: workspace not 256-B aligned");
  GRR_REQUIRE(((uintptr_t)g & 15) == 0, GRR_ERR_INVALID_ARG, "grr_conv3x3_embed_bwd_w: g not 16-B aligned");
  GRR_REQUIRE((int64_t)H * W < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed_bwd_w: H*W too large");
  const int64_t P = (int64_t)H * W;
  float* pt = (float*)workspace;
  char* wws = (char*)workspace + align256((int64_t)B * 9 * Cin * P * (int64_t)sizeof(float));
  hipLaunchKernelGGL(embed_patches_kernel, dim3(cd_grid((int64_t)B * P)), dim3(CD_NT), 0, (hipStream_t)stream, x, pt,
                     Cin, H, W, (int64_t)B * P);
  grr_status st = launch_status("grr_conv3x3_embed_bwd_w/patches");
  if (st != GRR_OK) return st;
  return grr_wgrad(g, pt, gw, wws, B, M, 9 * Cin, P, stream);
}

grr_status grr_conv3x3_embed_bwd_x(const float* g, const float* wt, float* gx, int B, int Cin, int M, int H, int W,
                                   void* stream) {
  clear_error();
  GRR_REQUIRE(g && wt && gx && B > 0 && Cin > 0 && M > 0 && H > 0 && W > 0, GRR_ERR_INVALID_ARG,
              "grr_conv3x3_embed_bwd_x: bad args");
  GRR_REQUIRE(gx != g, GRR_ERR_INVALID_ARG, "grr_conv3x3_embed_bwd_x: gx aliases g");
  GRR_REQUIRE(embed_ok(Cin, M), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed_bwd_x: Cin=%d, M=%d outside [1, %d] x [1, %d]",
              Cin, M, EMB_MAX_CIN, EMB_MAX_M);
  GRR_REQUIRE((int64_t)H * W < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_conv3x3_embed_bwd_x: H*W too large");
  const int64_t n = (int64_t)B * Cin * H * W;
  hipLaunchKernelGGL(embed_bwd_x_kernel, dim3(cd_grid(n)), dim3(CD_NT), 0, (hipStream_t)stream, g, wt, gx, Cin, M, H,
                     W, n);
  return launch_status("grr_conv3x3_embed_bwd_x");
}

int64_t grr_convt2x2s2_workspace_bytes(int B, int K, int M, int H, int W) {
  if (B <= 0 || K <= 0 || K > 4096 || M <= 0 || M > (1 << 20) || H <= 0 || W <= 0) return 0;
  const int64_t P = (int64_t)H * W;
  return align256((int64_t)4 * M * K * (int64_t)sizeof(float)) + align256(grr_conv1x1_workspace_bytes(K, 4 * M)) +
         (int64_t)B * 4 * M * P * (int64_t)sizeof(float);
}

grr_status grr_convt2x2s2(const float* x, const float* wt, float* out, void* workspace, int B, int K, int M, int H,
                          int W, void* stream) {
  clear_error();
  GRR_REQUIRE(x && wt && out && workspace && B > 0 && K > 0 && M > 0 && H > 0 && W > 0, GRR_ERR_INVALID_ARG,
              "grr_convt2x2s2: bad args");
  GRR_REQUIRE(out != x, GRR_ERR_INVALID_ARG, "grr_convt2x2s2: out aliases x");
  GRR_REQUIRE(K <= 4096 && M <= (1 << 20), GRR_ERR_UNSUPPORTED, "grr_convt2x2s2: K=%d > 4096 or M=%d too large", K, M);
  GRR_REQUIRE(((uintptr_t)workspace & 255) == 0, GRR_ERR_INVALID_ARG, "grr_convt2x2s2: workspace not 256-B aligned");
  GRR_REQUIRE(((uintptr_t)out & 7) == 0, GRR_ERR_INVALID_ARG, "grr_convt2x2s2: out not 8-B aligned");
  GRR_REQUIRE((int64_t)K * 4 * M < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_convt2x2s2: weight too large");
  const int64_t P = (int64_t)H * W;
  GRR_REQUIRE(P * 16 < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_convt2x2s2: H*W too large");
  hipStream_t s = (hipStream_t)stream;
  float* w4 = (float*)workspace;
  char* frag = (char*)workspace + align256((int64_t)4 * M * K * (int64_t)sizeof(float));
  float* t = (float*)(frag + align256(grr_conv1x1_workspace_bytes(K, 4 * M)));
  hipLaunchKernelGGL(convt_pack_kernel, dim3(cd_grid((int64_t)K * 4 * M)), dim3(CD_NT), 0, s, wt, w4, K, 4 * M);
  grr_status st = launch_status("grr_convt2x2s2/pack");
  if (st != GRR_OK) return st;
  st = grr_conv1x1_ws(x, w4, t, frag, B, K, 4 * M, P, stream);
  if (st != GRR_OK) return st;
  const int64_t n = (int64_t)B * M * 2 * P;
  hipLaunchKernelGGL(convt_interleave_kernel, dim3(cd_grid(n, 1 << 16)), dim3(CD_NT), 0, s, t, out, H, W, n);
  return launch_status("grr_convt2x2s2/interleave");
}

}  // extern "C"
