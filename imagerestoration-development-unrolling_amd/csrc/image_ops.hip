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
// Both families are instances of one gather body, one scatter body and one SSE kernel.  gather_kernel and
// scatter_kernel are written against an image source (OneImage or Arena below), which says where a window's
// image is, how wide coordinates and table rows are, and which element indices may be touched.
//
// A lane owns 4 consecutive pixels of one window row for all C channels (quad = 4 window columns, so the
// planar float side is one 16-byte access per channel when tw % 4 == 0 and the batch is 16-byte aligned).
// The image side is addressed by element: the image may start at any byte and 3 W is rarely a multiple of
// 4, and adjacent lanes touch adjacent bytes, so every cache line that is fetched is used whole.  The
// result does not depend on any alignment.  Window tables are device data the host cannot see: every
// index derived from them is clamped into the image / the window, so a bad table cannot address outside
// the buffers the caller sized from (H, W, C) and (n, th, tw).  The arena's image table is device data too:
// Arena reads it per lane (a wave straddles windows, hence images), clamps it, and keeps every element index
// inside [0, arena_elems): reads are clamped, writes outside are dropped.
#include <algorithm>

#include "grr_common.h"

namespace grr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIoThreads = 256;
constexpr int kMaxSegments = 65535;                  // grr_u8_sse_segments: one grid row (blockIdx.y) per segment
constexpr int64_t kMaxPixels = (1ll << 31) - 1;      // a legal image has H W C < 2^31

// row r of the bottom/right reflect-padded image: r >= n reads 2(n-1) - r (torch's "reflect"); clamped
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

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct WinArgs {
  float* win;           // [n, C, th, tw]
  const int32_t* table; // [n, Src::cols]; the last 6 columns are (wr, wc, r0, r1, c0, c1), tiling.Window
  int n, th, tw, quads; // quads = ceil(tw / 4)
  int vec;              // tw % 4 == 0 and win 16-byte aligned
  uint32_t total;       // n * th * quads
};

// The image a window belongs to, as a lane sees it: 1 <= H, W, and its elements start at base[off].
template <typename I>
struct Image {
  int64_t off;
  I H, W;
};

// Image source of grr_tile_*: one H x W image at base.  H and W are host arguments, so coordinates are int,
// and the caller sized the buffer from (H, W, C): every pixel of the image may be touched.
struct OneImage {
  typedef int idx;
  static constexpr int cols = 6;
  void* base;
  int H, W;
  __device__ __forceinline__ Image<int> image(const int32_t*) const { return Image<int>{0, H, W}; }
  __device__ __forceinline__ bool has_px(int64_t) const { return true; }
  __device__ __forceinline__ int64_t elem(const Image<int>&, int64_t px, int C) const { return px * C; }
  __device__ __forceinline__ bool inside(int64_t, int) const { return true; }
  __device__ __forceinline__ int64_t clamped(int64_t e) const { return e; }
};

// Image source of grr_tiles_*: image row[0] of the device image table [n_img, 3] (element offset, H, W), read
// per lane and clamped -- index into [0, n_img), offset into [0, elems), H and W into [1, 2^31) -- so
// coordinates are int64_t.  With 0 <= r < H and 0 <= col < W the pixel index r W + col is below 2^62; it is cut
// at 2^31 - 1 (no legal image reaches it), so an element index stays far below 2^63 (elems < 2^62).
struct Arena {
  typedef int64_t idx;
  static constexpr int cols = 7;
  void* base;                // the images back to back, HWC each
  int64_t elems;
  const int64_t* img_table;
  int n_img;
  __device__ __forceinline__ Image<int64_t> image(const int32_t* row) const {
    const int64_t* it = img_table + (int64_t)clampi(row[0], 0, n_img - 1) * 3;
    return Image<int64_t>{clamp64(it[0], 0, elems - 1), clamp64(it[1], 1, kMaxPixels), clamp64(it[2], 1, kMaxPixels)};
  }
  __device__ __forceinline__ bool has_px(int64_t px) const { return px <= kMaxPixels; }
  __device__ __forceinline__ int64_t elem(const Image<int64_t>& im, int64_t px, int C) const {
    return im.off + min(px, kMaxPixels) * C;
  }
  __device__ __forceinline__ bool inside(int64_t e, int count) const { return e + count <= elems; }
  __device__ __forceinline__ int64_t clamped(int64_t e) const { return min(e, elems - 1); }
};

// What gather_kernel and scatter_kernel ask of an image source Src:
//   idx, cols        the coordinate type and the table row width (the window's 6 columns come last)
//   base             the buffer the element indices below address
//   image(row)       the image of the window with this table row
//   elem(im, px, C)  element index of channel 0 of pixel px = r W + col of im, 0 <= r < H, 0 <= col < W
//   has_px(px)       false for a pixel index no legal image has (a write there is dropped)
//   inside(e, k)     elements [e, e + k), e >= 0, may all be touched
//   clamped(e)       e >= 0 moved to an element that may be read

template <typename T, int C, typename Src>
__global__ __launch_bounds__(kIoThreads) void gather_kernel(Src src, WinArgs a) {
  typedef typename Src::idx I;
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int32_t* e = a.table + (I)win * Src::cols;
  const Image<I> im = src.image(e);
  const int32_t* w = e + (Src::cols - 6);
  const T* img = static_cast<const T*>(src.base);
  const I sr = reflect_hi((I)w[0] + row, im.H);
  const int x0 = 4 * quad;
  const I col0 = (I)w[1] + x0;
  const int64_t base = src.elem(im, (int64_t)sr * im.W + col0, C);
  float v[C][4];
  if (col0 >= 0 && col0 + 3 < im.W && src.inside(base, 4 * C)) {   // 4 C contiguous elements of one image row
    const T* p = img + base;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(p + j * C + c);
  } else {                             // a reflected column, or a table that points outside: clamped
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t b = src.elem(im, (int64_t)sr * im.W + reflect_hi(col0 + j, im.W), C);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = load_px(img + src.clamped(b + c));
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

template <typename T, int C, typename Src>
__global__ __launch_bounds__(kIoThreads) void scatter_kernel(Src src, WinArgs a) {
  typedef typename Src::idx I;
  const uint32_t idx = blockIdx.x * (uint32_t)kIoThreads + threadIdx.x;
  if (idx >= a.total) return;
  const int quad = (int)(idx % (uint32_t)a.quads);
  const uint32_t t = idx / (uint32_t)a.quads;
  const int row = (int)(t % (uint32_t)a.th), win = (int)(t / (uint32_t)a.th);
  const int32_t* e = a.table + (I)win * Src::cols;
  const Image<I> im = src.image(e);
  const int32_t* w = e + (Src::cols - 6);
  const I wr = w[0], wc = w[1];
  // the core box, cut to the window and to the window's own unpadded image
  const I r0 = max(max((I)w[2], wr), (I)0), r1 = min(min((I)w[3], wr + a.th), im.H);
  const I c0 = max(max((I)w[4], wc), (I)0), c1 = min(min((I)w[5], wc + a.tw), im.W);
  const int x0 = 4 * quad;
  const I r = wr + row, col0 = wc + x0;
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
  // 0 <= r < H, so r W + col0 + j >= 0 for every column kept below
  const int64_t px0 = (int64_t)r * im.W + col0;
  if (!src.has_px(px0)) return;
  const int64_t base = src.elem(im, px0, C);
  T* img = static_cast<T*>(src.base);
  if (col0 >= c0 && col0 + 3 < c1 && src.inside(base, 4 * C)) {
    T* p = img + base;
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
          if (src.inside(base + j * C + c, 1)) store_px(img + base + j * C + c, v[c][j]);
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

// Segment blockIdx.y of [offsets[s], offsets[s + 1]), the offsets clamped into [0, total] and made monotone
// (offsets == nullptr: the one segment [0, total)); gridDim.x blocks stride over it.  A segment starts at any
// byte: when a and b share their phase modulo 16 (vec) the bytes up to the first 16-byte boundary and after the
// last are added one by one and the middle in 16-byte words; otherwise all of it byte by byte.  Integer sum:
// exact and the same on every run whatever order the waves' atomics land in.  A lane adds at most 16 x 65025
// per step into a 64-bit register sum; one 64-bit vector atomic per wave into out[s].
__global__ __launch_bounds__(kIoThreads) void u8_sse_kernel(const uint8_t* __restrict__ a,
                                                            const uint8_t* __restrict__ b, int64_t total,
                                                            const int64_t* __restrict__ offsets, int vec,
                                                            unsigned long long* out) {
  const int seg = blockIdx.y;
  const int64_t lo = offsets ? clamp64(offsets[seg], 0, total) : 0;
  const int64_t hi = offsets ? clamp64(offsets[seg + 1], lo, total) : total;
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

// The one place that picks <T, C>; the arguments after s are the kernel's.
#define GRR_IO_DISPATCH(kernel, Src, f32, C, grid, s, ...)                                                         \
  do {                                                                                                             \
    switch ((f32 ? 4 : 0) + C - 1) {                                                                               \
      case 0: hipLaunchKernelGGL((kernel<uint8_t, 1, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;     \
      case 1: hipLaunchKernelGGL((kernel<uint8_t, 2, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;     \
      case 2: hipLaunchKernelGGL((kernel<uint8_t, 3, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;     \
      case 3: hipLaunchKernelGGL((kernel<uint8_t, 4, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;     \
      case 4: hipLaunchKernelGGL((kernel<float, 1, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;       \
      case 5: hipLaunchKernelGGL((kernel<float, 2, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;       \
      case 6: hipLaunchKernelGGL((kernel<float, 3, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;       \
      default: hipLaunchKernelGGL((kernel<float, 4, Src>), grid, dim3(kIoThreads), 0, s, __VA_ARGS__); break;      \
    }                                                                                                              \
  } while (0)

// The checks all four gather / scatter entry points share, after their own; fills a.  base: the image or arena.
grr_status win_args(const char* what, const void* base, int img_f32, int C, const int32_t* table, int n, int th, int tw,
                    const float* win, WinArgs* a) {
  GRR_REQUIRE((int64_t)n * th < (1ll << 31) && grr_image_io_supported(C, (int)((int64_t)n * th), tw), GRR_ERR_UNSUPPORTED,
              "%s: window batch n th tw C must be below 2^31 (got %d x %d x %d x %d)", what, n, C, th, tw);
  GRR_REQUIRE((uintptr_t)win % 4 == 0 && (uintptr_t)table % 4 == 0 && (!img_f32 || (uintptr_t)base % 4 == 0),
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
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

dim3 io_grid(const WinArgs& a) { return dim3((a.total + kIoThreads - 1) / kIoThreads); }

// The checks grr_tile_gather and grr_tile_scatter share; fills src and a.
grr_status image_args(const char* what, const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n,
                      int th, int tw, const float* win, OneImage* src, WinArgs* a) {
  GRR_REQUIRE(img && table && win && (img_f32 == 0 || img_f32 == 1) && H > 0 && W > 0 && C > 0 && n > 0 && th > 0 &&
                  tw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(grr_image_io_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4 and H W C < 2^31 (got %d x %d x %d)", what, H, W, C);
  *src = OneImage{const_cast<void*>(img), H, W};
  return win_args(what, img, img_f32, C, table, n, th, tw, win, a);
}

// The checks grr_tiles_gather and grr_tiles_scatter share; fills src and a.
grr_status arena_args(const char* what, const void* arena, int64_t arena_elems, int img_f32, int C,
                      const int64_t* img_table, int n_img, const int32_t* table, int n, int th, int tw, const float* win,
                      Arena* src, WinArgs* a) {
  GRR_REQUIRE(arena && img_table && table && win && (img_f32 == 0 || img_f32 == 1) && arena_elems > 0 && n_img > 0 &&
                  C > 0 && n > 0 && th > 0 && tw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4, n_img <= arena_elems < 2^62 (got C %d, %d images, %lld elements)", what, C, n_img,
              (long long)arena_elems);
  grr_status st = win_args(what, arena, img_f32, C, table, n, th, tw, win, a);
  if (st != GRR_OK) return st;
  GRR_REQUIRE((uintptr_t)img_table % 8 == 0, GRR_ERR_INVALID_ARG, "%s: the image table must be 8-byte aligned", what);
  *src = Arena{const_cast<void*>(arena), arena_elems, img_table, n_img};
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
  OneImage src{};
  WinArgs a{};
  grr_status st = image_args("grr_tile_gather", img, img_f32, H, W, C, table, n, th, tw, out, &src, &a);
  if (st != GRR_OK) return st;
  GRR_IO_DISPATCH(gather_kernel, OneImage, img_f32, C, io_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tile_gather");
}

grr_status grr_tile_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* img, int img_f32, int H,
                            int W, int C, void* stream) {
  clear_error();
  OneImage src{};
  WinArgs a{};
  grr_status st = image_args("grr_tile_scatter", img, img_f32, H, W, C, table, n, th, tw, y, &src, &a);
  if (st != GRR_OK) return st;
  GRR_IO_DISPATCH(scatter_kernel, OneImage, img_f32, C, io_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tile_scatter");
}

grr_status grr_u8_sse(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out, void* stream) {
  clear_error();
  GRR_REQUIRE(a && b && out && n > 0 && (uintptr_t)out % 8 == 0, GRR_ERR_INVALID_ARG, "grr_u8_sse: bad args");
  GRR_REQUIRE(n < (1ll << 31), GRR_ERR_UNSUPPORTED, "grr_u8_sse: n must be below 2^31 (got %lld)", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  GRR_REQUIRE(hipMemsetAsync(out, 0, sizeof(uint64_t), s) == hipSuccess, GRR_ERR_HIP, "grr_u8_sse: zeroing the sum failed");
  const int vec = ((uintptr_t)a % 16 == (uintptr_t)b % 16) ? 1 : 0;
  const int64_t items = vec ? (n + 15) / 16 : n;
  const int blocks = (int)std::min<int64_t>((items + kIoThreads - 1) / kIoThreads, 2048);
  hipLaunchKernelGGL(u8_sse_kernel, dim3(blocks), dim3(kIoThreads), 0, s, a, b, n, (const int64_t*)nullptr, vec,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_sse");
}

int grr_image_arena_supported(int C, int n_img, int64_t arena_elems) {
  return C >= 1 && C <= 4 && n_img >= 1 && arena_elems >= n_img && arena_elems < (1ll << 62) ? 1 : 0;
}

grr_status grr_tiles_gather(const void* arena, int64_t arena_elems, int img_f32, int C, const int64_t* img_table,
                            int n_img, const int32_t* table, int n, int th, int tw, float* out, void* stream) {
  clear_error();
  Arena src{};
  WinArgs a{};
  grr_status st = arena_args("grr_tiles_gather", arena, arena_elems, img_f32, C, img_table, n_img, table, n, th, tw, out,
                             &src, &a);
  if (st != GRR_OK) return st;
  GRR_IO_DISPATCH(gather_kernel, Arena, img_f32, C, io_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tiles_gather");
}

grr_status grr_tiles_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* arena, int64_t arena_elems,
                             int img_f32, int C, const int64_t* img_table, int n_img, void* stream) {
  clear_error();
  Arena src{};
  WinArgs a{};
  grr_status st = arena_args("grr_tiles_scatter", arena, arena_elems, img_f32, C, img_table, n_img, table, n, th, tw, y,
                             &src, &a);
  if (st != GRR_OK) return st;
  GRR_IO_DISPATCH(scatter_kernel, Arena, img_f32, C, io_grid(a), (hipStream_t)stream, src, a);
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
  hipLaunchKernelGGL(u8_sse_kernel, dim3(bx, n_seg), dim3(kIoThreads), 0, s, a, b, total, offsets, vec,
                     reinterpret_cast<unsigned long long*>(out));
  return launch_status("grr_u8_sse_segments");
}

}  // extern "C"
