// Whole-image restoration I/O (restore.py): the data movement around the model, gfx950.
//
//   grr_tile_gather   HWC image (uint8 or float32, any byte address) -> planar float32 windows [n,C,th,tw],
//                     the bottom / right reflect padding folded into the read
//   grr_tile_scatter  planar float32 windows [n,C,th,tw] -> each window's core box, cut to the unpadded
//                     H x W, into the HWC image (uint8: clamp, x255, round half to even; float32: copy)
//   grr_u8_sse        sum (a - b)^2 of two uint8 arrays as an exact 64-bit integer
//
// A lane owns 4 consecutive pixels of one window row for all C channels (quad = 4 window columns, so the
// planar float side is one 16-byte access per channel when tw % 4 == 0 and the batch is 16-byte aligned).
// The image side is addressed by element: the image may start at any byte and 3 W is rarely a multiple of
// 4, and adjacent lanes touch adjacent bytes, so every cache line that is fetched is used whole.  The
// result does not depend on any alignment.  Window tables are device data the host cannot see: every
// index derived from them is clamped into the image / the window, so a bad table cannot address outside
// the buffers the caller sized from (H, W, C) and (n, th, tw).
#include <algorithm>

#include "grr_common.h"

namespace grr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIoThreads = 256;
constexpr int kTableCols = 6;   // (wr, wc, r0, r1, c0, c1), tiling.Window

// row r of the bottom/right reflect-padded image: r >= n reads 2(n-1) - r (torch's "reflect"); clamped
__device__ __forceinline__ int reflect_hi(int r, int n) { return clampi(r < n ? r : 2 * (n - 1) - r, 0, n - 1); }

__device__ __forceinline__ float load_px(const uint8_t* p) { return __fdiv_rn((float)*p, 255.0f); }
__device__ __forceinline__ float load_px(const float* p) { return *p; }

// img_as_ubyte(clip(v, 0, 1)): float32 product, round half to even, clip, cast.  fmaxf drops a NaN -> 0.
__device__ __forceinline__ void store_px(uint8_t* p, float v) {
  const float c = fminf(fmaxf(v, 0.0f), 1.0f);
  const float r = fminf(fmaxf(__builtin_rintf(c * 255.0f), 0.0f), 255.0f);
  *p = (uint8_t)(int)r;
}
__device__ __forceinline__ void store_px(float* p, float v) { *p = v; }

struct IoArgs {
  void* img;            // HWC
  float* win;           // [n, C, th, tw]
  const int32_t* table; // [n, 6]
  int H, W, n, th, tw, quads;   // quads = ceil(tw / 4)
  int vec;              // tw % 4 == 0 and win 16-byte aligned
  uint32_t total;       // n * th * quads
};

template <typename T, int C>
__global__ __launch_bounds__(kIoThreads) void tile_gather_kernel(IoArgs a) {
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int wr = a.table[win * kTableCols + 0], wc = a.table[win * kTableCols + 1];
  const T* img = static_cast<const T*>(a.img);
  const int sr = reflect_hi(wr + row, a.H);
  const int x0 = 4 * quad, col0 = wc + x0;
  float v[C][4];
  if (col0 >= 0 && col0 + 3 < a.W) {   // 4 C contiguous elements of one image row
    const T* p = img + ((int64_t)sr * a.W + col0) * C;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(p + j * C + c);
  } else {                             // a reflected column (or a table column outside the image)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T* p = img + ((int64_t)sr * a.W + reflect_hi(col0 + j, a.W)) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(p + c);
    }
  }
  float* o = a.win + (((int64_t)win * C) * a.th + row) * a.tw + x0;
  const int64_t plane = (int64_t)a.th * a.tw;
  if (a.vec) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
      *reinterpret_cast<f32x4*>(o + c * plane) = q;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < a.tw) o[c * plane + j] = v[c][j];
  }
}

template <typename T, int C>
__global__ __launch_bounds__(kIoThreads) void tile_scatter_kernel(IoArgs a) {
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int32_t* e = a.table + win * kTableCols;
  const int wr = e[0], wc = e[1];
  // the core box, cut to the window and to the unpadded image
  const int r0 = max(max(e[2], wr), 0), r1 = min(min(e[3], wr + a.th), a.H);
  const int c0 = max(max(e[4], wc), 0), c1 = min(min(e[5], wc + a.tw), a.W);
  const int r = wr + row, x0 = 4 * quad, col0 = wc + x0;
  if (r < r0 || r >= r1 || col0 + 3 < c0 || col0 >= c1) return;
  const float* y = a.win + (((int64_t)win * C) * a.th + row) * a.tw + x0;
  const int64_t plane = (int64_t)a.th * a.tw;
  float v[C][4];
  if (a.vec) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(y + c * plane);
      v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = x0 + j < a.tw ? y[c * plane + j] : 0.0f;
  }
  T* p = static_cast<T*>(a.img) + ((int64_t)r * a.W + col0) * C;
  if (col0 >= c0 && col0 + 3 < c1) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) store_px(p + j * C + c, v[c][j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col0 + j >= c0 && col0 + j < c1) {
#pragma unroll
        for (int c = 0; c < C; ++c) store_px(p + j * C + c, v[c][j]);
      }
  }
}

__device__ __forceinline__ uint32_t sq_diff(uint32_t x, uint32_t y) {
  const int d = (int)x - (int)y;
  return (uint32_t)(d * d);
}

// Integer sum: exact and the same on every run whatever order the waves' atomics land in.  A lane adds at
// most 16 x 65025 per step into a 64-bit register sum; one 64-bit vector atomic per wave.
__global__ __launch_bounds__(kIoThreads) void u8_sse_kernel(const uint8_t* __restrict__ a,
                                                            const uint8_t* __restrict__ b, int64_t n, int vec,
                                                            unsigned long long* out) {
  const int64_t tid = (int64_t)blockIdx.x * kIoThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kIoThreads;
  unsigned long long acc = 0;
  int64_t done = 0;
  if (vec) {   // both arrays 16-byte aligned: 16 bytes of each per step
    const int64_t n16 = n / 16;
    const u32x4* a4 = reinterpret_cast<const u32x4*>(a);
    const u32x4* b4 = reinterpret_cast<const u32x4*>(b);
    for (int64_t i = tid; i < n16; i += nthr) {
      const u32x4 x = a4[i], y = b4[i];
      uint32_t s = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int sh = 0; sh < 32; sh += 8) s += sq_diff((x[k] >> sh) & 255u, (y[k] >> sh) & 255u);
      acc += s;
    }
    done = n16 * 16;
  }
  for (int64_t i = done + tid; i < n; i += nthr) acc += sq_diff(a[i], b[i]);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(out, acc);
}

#define GRR_IO_DISPATCH(kernel, f32, C, grid, s, args)                                                            \
  do {                                                                                                             \
    switch ((f32 ? 4 : 0) + C - 1) {                                                                               \
      case 0: hipLaunchKernelGGL((kernel<uint8_t, 1>), grid, dim3(kIoThreads), 0, s, args); break;                 \
      case 1: hipLaunchKernelGGL((kernel<uint8_t, 2>), grid, dim3(kIoThreads), 0, s, args); break;                 \
      case 2: hipLaunchKernelGGL((kernel<uint8_t, 3>), grid, dim3(kIoThreads), 0, s, args); break;                 \
      case 3: hipLaunchKernelGGL((kernel<uint8_t, 4>), grid, dim3(kIoThreads), 0, s, args); break;                 \
      case 4: hipLaunchKernelGGL((kernel<float, 1>), grid, dim3(kIoThreads), 0, s, args); break;                   \
      case 5: hipLaunchKernelGGL((kernel<float, 2>), grid, dim3(kIoThreads), 0, s, args); break;                   \
      case 6: hipLaunchKernelGGL((kernel<float, 3>), grid, dim3(kIoThreads), 0, s, args); break;                   \
      default: hipLaunchKernelGGL((kernel<float, 4>), grid, dim3(kIoThreads), 0, s, args); break;                  \
    }                                                                                                              \
  } while (0)

// The checks grr_tile_gather and grr_tile_scatter share; fills a.
grr_status io_args(const char* what, const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n,
                   int th, int tw, const float* win, IoArgs* a) {
  GRR_REQUIRE(img && table && win && (img_f32 == 0 || img_f32 == 1) && H > 0 && W > 0 && C > 0 && n > 0 && th > 0 &&
                  tw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(grr_image_io_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4 and H W C < 2^31 (got %d x %d x %d)", what, H, W, C);
  GRR_REQUIRE((int64_t)n * th < (1ll << 31) && grr_image_io_supported(C, (int)((int64_t)n * th), tw), GRR_ERR_UNSUPPORTED,
              "%s: window batch n th tw C must be below 2^31 (got %d x %d x %d x %d)", what, n, C, th, tw);
  GRR_REQUIRE((uintptr_t)win % 4 == 0 && (uintptr_t)table % 4 == 0 && (!img_f32 || (uintptr_t)img % 4 == 0),
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
  a->img = const_cast<void*>(img);
  a->win = const_cast<float*>(win);
  a->table = table;
  a->H = H;
  a->W = W;
  a->n = n;
  a->th = th;
  a->tw = tw;
  a->quads = (tw + 3) / 4;
  a->vec = tw % 4 == 0 && (uintptr_t)win % 16 == 0;
  a->total = (uint32_t)((int64_t)n * th * a->quads);   // <= n th tw < 2^31
  return GRR_OK;
}

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_image_io_supported(int C, int H, int W) {
  return C >= 1 && C <= 4 && H >= 1 && W >= 1 && (int64_t)H * W * C < (1ll << 31) ? 1 : 0;
}

grr_status grr_tile_gather(const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n, int th,
                           int tw, float* out, void* stream) {
  clear_error();
  IoArgs a{};
  grr_status st = io_args("grr_tile_gather", img, img_f32, H, W, C, table, n, th, tw, out, &a);
  if (st != GRR_OK) return st;
  const dim3 grid((a.total + kIoThreads - 1) / kIoThreads);
  GRR_IO_DISPATCH(tile_gather_kernel, img_f32, C, grid, (hipStream_t)stream, a);
  return launch_status("grr_tile_gather");
}

grr_status grr_tile_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* img, int img_f32, int H,
                            int W, int C, void* stream) {
  clear_error();
  IoArgs a{};
  grr_status st = io_args("grr_tile_scatter", img, img_f32, H, W, C, table, n, th, tw, y, &a);
  if (st != GRR_OK) return st;
  const dim3 grid((a.total + kIoThreads - 1) / kIoThreads);
  GRR_IO_DISPATCH(tile_scatter_kernel, img_f32, C, grid, (hipStream_t)stream, a);
  return launch_status("grr_tile_scatter");
}

grr_status grr_u8_sse(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && out && n > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG, "grr_u8_sse: bad args");
  GRR_REQUIRE(n < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_u8_sse: n must be below 2^31 (got %lld)", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(uint64_t), s) == hipSuccess, GRR_ERR_HIP, "grr_u8_sse: zeroing the sum failed");
  const int vec = ((uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0) ? 1 : 0;
  const int64_t items = vec ? (n + 15) / 16 : n;
  const int blocks = (int)std::min<int64_t>((items + kIoThreads - 1) / kIoThreads, 2048);
  hipLaunchKernelGGL(u8_sse_kernel, dim3(blocks), dim3(kIoThreads), 0, s, a, b, n, vec,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_sse");
}

}  // extern "C"
