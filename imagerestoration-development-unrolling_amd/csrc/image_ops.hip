// Whole-image restoration I/O (restore.py): the data movement around the model, gfx950.
//
//   grr_tile_gather   HWC image (uint8 or float32, any byte address) -> planar float32 windows [n,C,th,tw],
//                     the bottom / right reflect padding folded into the read
//   grr_tile_scatter  planar float32 windows [n,C,th,tw] -> each window's core box, cut to the unpadded
//                     H x W, into the HWC image (uint8: clamp, x255, round half to even; float32: copy)
//   grr_u8_sse        sum (a - b)^2 of two uint8 arrays as an exact 64-bit integer
//
// and the same three for a list of images that share window batches (restore_images): the images lie back to
// back in one arena, an int64 image table [n_img, 3] of (element offset, H, W) describes it, and window rows
// carry their image's index in front:
//   grr_tiles_gather / grr_tiles_scatter / grr_u8_sse_segments
//
// A lane owns 4 consecutive pixels of one window row for all C channels (quad = 4 window columns, so the
// planar float side is one 16-byte access per channel when tw % 4 == 0 and the batch is 16-byte aligned).
// The image side is addressed by element: the image may start at any byte and 3 W is rarely a multiple of
// 4, and adjacent lanes touch adjacent bytes, so every cache line that is fetched is used whole.  The
// result does not depend on any alignment.  Window tables are device data the host cannot see: every
// index derived from them is clamped into the image / the window, so a bad table cannot address outside
// the buffers the caller sized from (H, W, C) and (n, th, tw).  The arena kernels read the image table per
// lane too (a wave straddles windows, hence images), clamp the image index, and keep every element index
// inside [0, arena_elems): reads are clamped, writes outside are dropped.
#include <algorithm>

#include "grr_common.h"

namespace grr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIoThreads = 256;
constexpr int kTableCols = 6;   // (wr, wc, r0, r1, c0, c1), tiling.Window

// row r of the bottom/right reflect-padded image: r >= n reads 2(n-1) - r (torch's "reflect"); clamped
// (int for the single-image kernels; int64_t for the arena kernels, whose H and W are device data)
template <typename I>
__device__ __forceinline__ I reflect_hi(I r, I n) {
  const I m = r < n ? r : 2 * (n - 1) - r;
  return m < 0 ? 0 : (m > n - 1 ? n - 1 : m);
}

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

// ---- a list of images in one arena
constexpr int kArenaCols = 7;                        // (img, wr, wc, r0, r1, c0, c1)
constexpr int kMaxSegments = 65535;                  // grr_u8_sse_segments: one grid row (blockIdx.y) per segment
constexpr int64_t kMaxPixels = (1ll << 31) - 1;      // a legal image has H W C < 2^31

struct ArenaArgs {
  void* arena;               // the images back to back, HWC each
  int64_t arena_elems;
  const int64_t* img_table;  // [n_img, 3] (element offset, H, W)
  int n_img;
  float* win;                // [n, C, th, tw]
  const int32_t* table;      // [n, 7]
  int n, th, tw, quads, vec;
  uint32_t total;            // n * th * quads
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One image-table row as a lane sees it: offset in [0, arena_elems), H and W in [1, 2^31).
struct ArenaImage {
  int64_t off, H, W;
};
__device__ __forceinline__ ArenaImage arena_image(const ArenaArgs& a, int img) {
  const int64_t* it = a.img_table + (int64_t)clampi(img, 0, a.n_img - 1) * 3;
  return ArenaImage{clamp64(it[0], 0, a.arena_elems - 1), clamp64(it[1], 1, kMaxPixels), clamp64(it[2], 1, kMaxPixels)};
}
// Element index of channel 0 of pixel (r, col), 0 <= r < H, 0 <= col < W: r W + col < 2^62, and the pixel index
// is cut at 2^31 - 1 (no legal image reaches it), so the sum stays far below 2^63 (arena_elems < 2^62).
__device__ __forceinline__ int64_t arena_px(const ArenaImage& im, int64_t r, int64_t col, int C) {
  return im.off + min(r * im.W + col, kMaxPixels) * C;
}

template <typename T, int C>
__global__ __launch_bounds__(kIoThreads) void tiles_gather_kernel(ArenaArgs a) {
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int32_t* e = a.table + (int64_t)win * kArenaCols;
  const ArenaImage im = arena_image(a, e[0]);
  const T* arena = static_cast<const T*>(a.arena);
  const int64_t sr = reflect_hi((int64_t)e[1] + row, im.H);
  const int x0 = 4 * quad;
  const int64_t col0 = (int64_t)e[2] + x0, last = a.arena_elems - 1;
  const int64_t base = arena_px(im, sr, col0, C);
  float v[C][4];
  if (col0 >= 0 && col0 + 3 < im.W && base + 4 * C - 1 <= last) {   // 4 C contiguous elements of one image row
    const T* p = arena + base;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(p + j * C + c);
  } else {                             // a reflected column, or a table that points past the arena: clamped
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t b = arena_px(im, sr, reflect_hi(col0 + j, im.W), C);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(arena + min(b + c, last));
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
__global__ __launch_bounds__(kIoThreads) void tiles_scatter_kernel(ArenaArgs a) {
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int32_t* e = a.table + (int64_t)win * kArenaCols;
  const ArenaImage im = arena_image(a, e[0]);
  const int64_t wr = e[1], wc = e[2];
  // the core box, cut to the window and to the window's own unpadded image
  const int64_t r0 = max(max((int64_t)e[3], wr), (int64_t)0), r1 = min(min((int64_t)e[4], wr + a.th), im.H);
  const int64_t c0 = max(max((int64_t)e[5], wc), (int64_t)0), c1 = min(min((int64_t)e[6], wc + a.tw), im.W);
  const int x0 = 4 * quad;
  const int64_t r = wr + row, col0 = wc + x0;
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
  T* arena = static_cast<T*>(a.arena);
  // 0 <= r < H, so r W + col0 + j >= 0 for every column kept below; a pixel index a legal image cannot have is dropped
  const int64_t px0 = r * im.W + col0;
  if (px0 > kMaxPixels) return;
  const int64_t base = im.off + px0 * C;
  if (col0 >= c0 && col0 + 3 < c1 && base + 4 * C <= a.arena_elems) {
    T* p = arena + base;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) store_px(p + j * C + c, v[c][j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col0 + j >= c0 && col0 + j < c1) {
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (base + j * C + c < a.arena_elems) store_px(arena + base + j * C + c, v[c][j]);
      }
  }
}

__device__ __forceinline__ uint32_t sq_diff(uint32_t x, uint32_t y) {
  const int d = (int)x - (int)y;
  return (uint32_t)(d * d);
}

// sum of the 16 squared byte differences of two 16-byte words: at most 16 x 65025
__device__ __forceinline__ uint32_t sq_diff16(const u32x4& x, const u32x4& y) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int sh = 0; sh < 32; sh += 8) s += sq_diff((x[k] >> sh) & 255u, (y[k] >> sh) & 255u);
  return s;
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
      acc += sq_diff16(a4[i], b4[i]);
    }
    done = n16 * 16;
  }
  for (int64_t i = done + tid; i < n; i += nthr) acc += sq_diff(a[i], b[i]);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(out, acc);
}

// Segment blockIdx.y of [offsets[s], offsets[s + 1]), the offsets clamped into [0, total] and made monotone;
// gridDim.x blocks stride over it.  A segment starts at any byte: when a and b share their phase modulo 16
// (vec) the bytes up to the first 16-byte boundary and after the last are added one by one and the middle in
// 16-byte words; otherwise all of it byte by byte.  One 64-bit vector atomic per wave into out[s].
__global__ __launch_bounds__(kIoThreads) void u8_sse_segments_kernel(const uint8_t* __restrict__ a,
                                                                     const uint8_t* __restrict__ b, int64_t total,
                                                                     const int64_t* __restrict__ offsets, int vec,
                                                                     unsigned long long* out) {
  const int seg = blockIdx.y;
  const int64_t lo = clamp64(offsets[seg], 0, total), hi = clamp64(offsets[seg + 1], lo, total);
  const int64_t tid = (int64_t)blockIdx.x * kIoThreads + threadIdx.x, nthr = (int64_t)gridDim.x * kIoThreads;
  unsigned long long acc = 0;
  int64_t head_end = lo, body_end = lo;     // [lo, head_end) bytes, [head_end, body_end) words, [body_end, hi) bytes
  if (vec) {
    head_end = min(hi, lo + (int64_t)((16 - (reinterpret_cast<uintptr_t>(a) + (uint64_t)lo) % 16) % 16));
    const int64_t n16 = (hi - head_end) / 16;
    body_end = head_end + n16 * 16;
    const u32x4* a4 = reinterpret_cast<const u32x4*>(a + head_end);
    const u32x4* b4 = reinterpret_cast<const u32x4*>(b + head_end);
    for (int64_t i = tid; i < n16; i += nthr) acc += sq_diff16(a4[i], b4[i]);
    for (int64_t i = lo + tid; i < head_end; i += nthr) acc += sq_diff(a[i], b[i]);
  }
  for (int64_t i = body_end + tid; i < hi; i += nthr) acc += sq_diff(a[i], b[i]);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(out + seg, acc);
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

// The checks grr_tiles_gather and grr_tiles_scatter share; fills a.
grr_status arena_args(const char* what, const void* arena, int64_t arena_elems, int img_f32, int C,
                      const int64_t* img_table, int n_img, const int32_t* table, int n, int th, int tw, const float* win,
                      ArenaArgs* a) {
  GRR_REQUIRE(arena && img_table && table && win && (img_f32 == 0 || img_f32 == 1) && arena_elems > 0 && n_img > 0 &&
                  C > 0 && n > 0 && th > 0 && tw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4, n_img <= arena_elems < 2^62 (got C %d, %d images, %lld elements)", what, C, n_img,
              (long long)arena_elems);
  GRR_REQUIRE((int64_t)n * th < (1ll << 31) && grr_image_io_supported(C, (int)((int64_t)n * th), tw), GRR_ERR_UNSUPPORTED,
              "%s: window batch n th tw C must be below 2^31 (got %d x %d x %d x %d)", what, n, C, th, tw);
  GRR_REQUIRE((uintptr_t)win % 4 == 0 && (uintptr_t)table % 4 == 0 && (uintptr_t)img_table % 8 == 0 &&
                  (!img_f32 || (uintptr_t)arena % 4 == 0),
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte, the image table 8-byte aligned", what);
  a->arena = const_cast<void*>(arena);
  a->arena_elems = arena_elems;
  a->img_table = img_table;
  a->n_img = n_img;
  a->win = const_cast<float*>(win);
  a->table = table;
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

int grr_image_arena_supported(int C, int n_img, int64_t arena_elems) {
  return C >= 1 && C <= 4 && n_img >= 1 && arena_elems >= n_img && arena_elems < (1ll << 62) ? 1 : 0;
}

grr_status grr_tiles_gather(const void* arena, int64_t arena_elems, int img_f32, int C, const int64_t* img_table,
                            int n_img, const int32_t* table, int n, int th, int tw, float* out, void* stream) {
  clear_error();
  ArenaArgs a{};
  grr_status st = arena_args("grr_tiles_gather", arena, arena_elems, img_f32, C, img_table, n_img, table, n, th, tw, out, &a);
  if (st != GRR_OK) return st;
  const dim3 grid((a.total + kIoThreads - 1) / kIoThreads);
  GRR_IO_DISPATCH(tiles_gather_kernel, img_f32, C, grid, (hipStream_t)stream, a);
  return launch_status("grr_tiles_gather");
}

grr_status grr_tiles_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* arena, int64_t arena_elems,
                             int img_f32, int C, const int64_t* img_table, int n_img, void* stream) {
  clear_error();
  ArenaArgs a{};
  grr_status st = arena_args("grr_tiles_scatter", arena, arena_elems, img_f32, C, img_table, n_img, table, n, th, tw, y, &a);
  if (st != GRR_OK) return st;
  const dim3 grid((a.total + kIoThreads - 1) / kIoThreads);
  GRR_IO_DISPATCH(tiles_scatter_kernel, img_f32, C, grid, (hipStream_t)stream, a);
  return launch_status("grr_tiles_scatter");
}

grr_status grr_u8_sse_segments(const uint8_t* a, const uint8_t* b, int64_t total, const int64_t* offsets, int n_seg,
                               uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && offsets && out && total > 0 && n_seg > 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)offsets % 8 == 0,
              GRR_ERR_INVALID_ARG, "grr_u8_sse_segments: bad args");
  GRR_REQUIRE(n_seg <= kMaxSegments, GRR_ERR_UNSUPPORTED,
              "grr_u8_sse_segments: at most %d segments per call, one grid row each (got %d)", kMaxSegments, n_seg);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(uint64_t) * n_seg, s) == hipSuccess, GRR_ERR_HIP,
              "grr_u8_sse_segments: zeroing the sums failed");
  const int vec = ((uintptr_t)a % 16 == (uintptr_t)b % 16) ? 1 : 0;
  // blocks per segment from the mean segment length: one pass of 16-byte words, at most 256 blocks
  const int64_t items = (total / n_seg + 15) / 16;
  const int bx = (int)std::min<int64_t>(std::max<int64_t>((items + kIoThreads - 1) / kIoThreads, 1), 256);
  hipLaunchKernelGGL(u8_sse_segments_kernel, dim3(bx, n_seg), dim3(kIoThreads), 0, s, a, b, total, offsets, vec,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_sse_segments");
}

}  // extern "C"
