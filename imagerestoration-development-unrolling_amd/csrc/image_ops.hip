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
// and, for the geometric self-ensemble (restore_image(ensemble=...)), the gather under up to 4 of the 8 flips
// and quarter turns of a window at once and the scatter of the fixed-order mean of the members turned back:
//   grr_tile_gather_d8 / grr_tile_scatter_mean / grr_tiles_gather_d8 / grr_tiles_scatter_mean
// one gather body and one scatter body again, block per (window, tile), the odd quarter turns through LDS.
//
// and, for training on real images (training.DevicePatchLoader), the model's clean and noisy planar batches cut
// from the arena by a device table of (image, row, col, mode), the noise a counter-based function of
// (seed, sample id, element):
//   grr_patch_batch
// and the same batch for degraded / clean picture pairs, two arenas under one image table (one kernel body):
//   grr_patch_pair_batch
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

#include "grr_device.h"

namespace grr {
namespace {

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

// ---------------------------------------------------------------------------
// The 8 flips and quarter turns of a window (geometric self-ensemble), m = 2k + f: np.rot90(a, k), then
// np.flipud if f.  Pixel (i, j) of a th x tw window with i' = flip_i ? th-1-i : i, j' = flip_j ? tw-1-j : j
// lands at (i', j') of T_m (th x tw) for even k and at (j', i') of T_m (tw x th) for odd k:
//   m        0  1  2  3  4  5  6  7
//   flip_i   .  x  .  .  x  .  x  x     0xD2
//   flip_j   .  .  x  .  x  x  .  x     0xB4
//   odd k    .  .  x  x  .  .  x  x     bit 1 of m
// A mode list travels in the kernel arguments, 4 bits a member (at most 8 members), not in a device table.
constexpr int kTileI = 32;       // window rows of a block's tile: a transposed run of 32 floats is 128 bytes
constexpr int kMeanTileJ = 32;   // window columns of a scatter_mean tile

__device__ __forceinline__ int d8_mode(uint32_t modes, int j) { return (int)((modes >> (4 * j)) & 7u); }
__device__ __forceinline__ bool d8_flip_i(int m) { return (0xD2u >> m) & 1u; }
__device__ __forceinline__ bool d8_flip_j(int m) { return (0xB4u >> m) & 1u; }
__device__ __forceinline__ bool d8_odd(int m) { return (m & 2) != 0; }

// window columns of a gather_d8 tile: an image row of the tile is at least 128 bytes (uint8 C = 1: 128 pixels)
template <typename T, int C>
constexpr int d8_tile_j() { return sizeof(T) * C >= 2 ? 64 : 128; }

struct D8Args {
  float* win;            // [n M, C, th, tw] (even k) or [n M, C, tw, th] (odd k), window-major
  const int32_t* table;  // as WinArgs
  int n, th, tw;         // th x tw: the window in the picture's frame
  int tiles_i, tiles_j;  // tiles of kTileI x d8_tile_j per window
  int M;                 // modes of this call, all of one orientation
  uint32_t modes;
};

// One block per (window, tile).  A lane reads one pixel (all C channels, adjacent lanes adjacent elements of an
// image row) through the reflect rule.  Even k: the value goes straight to (i', j') of each mode's plane, a row
// walk, forward or reversed.  Odd k: the tile goes through LDS with a row stride of TJ + 1 floats; it is read
// back down its columns (lanes 32 rows apart in steps of TJ + 1 words: 32 distinct banks), so the planar side
// is written in runs of 32 consecutive floats along the transformed row.
template <typename T, int C, typename Src, bool Odd>
__device__ __forceinline__ void gather_d8_body(const Src& src, const D8Args& a) {
  typedef typename Src::idx I;
  constexpr int TJ = d8_tile_j<T, C>();
  constexpr int PX = kTileI * TJ / kIoThreads;
  __shared__ float tile[Odd ? C * kTileI * (TJ + 1) : 1];
  const uint32_t b = blockIdx.x;
  const int tj = (int)(b % (uint32_t)a.tiles_j);
  const uint32_t t = b / (uint32_t)a.tiles_j;
  const int ti = (int)(t % (uint32_t)a.tiles_i), win = (int)(t / (uint32_t)a.tiles_i);
  const int i0 = ti * kTileI, j0 = tj * TJ;
  const int32_t* e = a.table + (I)win * Src::cols;
  const Image<I> im = src.image(e);
  const int32_t* w = e + (Src::cols - 6);
  const T* img = static_cast<const T*>(src.base);
  const int64_t plane = (int64_t)a.th * a.tw;
  float* out = a.win + (int64_t)win * a.M * C * plane;
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int px = (int)threadIdx.x + k * kIoThreads;
    const int il = px / TJ, jl = px % TJ, i = i0 + il, j = j0 + jl;
    if (i >= a.th || j >= a.tw) continue;
    const I sr = reflect_hi((I)w[0] + i, im.H), sc = reflect_hi((I)w[1] + j, im.W);
    const int64_t base = src.elem(im, (int64_t)sr * im.W + sc, C);
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = load_px(img + src.clamped(base + c));
    if (Odd) {
#pragma unroll
      for (int c = 0; c < C; ++c) tile[(c * kTileI + il) * (TJ + 1) + jl] = v[c];
    } else {
      for (int m = 0; m < a.M; ++m) {
        const int mode = d8_mode(a.modes, m);
        const int p = d8_flip_i(mode) ? a.th - 1 - i : i, q = d8_flip_j(mode) ? a.tw - 1 - j : j;
        float* o = out + (int64_t)m * C * plane + (int64_t)p * a.tw + q;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c * plane] = v[c];
      }
    }
  }
  if (!Odd) return;
  __syncthreads();
  for (int m = 0; m < a.M; ++m) {
    const int mode = d8_mode(a.modes, m);
    const bool fi = d8_flip_i(mode), fj = d8_flip_j(mode);
    float* o = out + (int64_t)m * C * plane;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int px = (int)threadIdx.x + k * kIoThreads;
      const int il = px % kTileI, jl = px / kTileI, i = i0 + il, j = j0 + jl;
      if (i >= a.th || j >= a.tw) continue;
      const int64_t at = (int64_t)(fj ? a.tw - 1 - j : j) * a.th + (fi ? a.th - 1 - i : i);   // plane is tw x th
#pragma unroll
      for (int c = 0; c < C; ++c) o[c * plane + at] = tile[(c * kTileI + il) * (TJ + 1) + jl];
    }
  }
}

template <typename T, int C, typename Src>
__global__ __launch_bounds__(kIoThreads) void gather_d8_even_kernel(Src src, D8Args a) {
  gather_d8_body<T, C, Src, false>(src, a);
}
template <typename T, int C, typename Src>
__global__ __launch_bounds__(kIoThreads) void gather_d8_odd_kernel(Src src, D8Args a) {
  gather_d8_body<T, C, Src, true>(src, a);
}

struct MeanArgs {
  const float* y0;       // [n M0, C, th, tw]: the even-k members, window-major; unused when M0 == 0
  const float* y1;       // [n M1, C, tw, th]: the odd-k members
  const int32_t* table;
  int n, th, tw, tiles_i, tiles_j;
  int M, M0, M1;         // M = M0 + M1 members, in the listed (ascending) order in modes
  uint32_t modes;
};

// float32 pairwise tree over z[0 .. cnt) in the listed order, the odd one carried: [z0+z1, z2+z3, ...] until
// one is left.  Static indices only, so z stays in registers; slots at and past cnt are never read into a sum.
__device__ __forceinline__ float tree_sum8(float (&z)[8], int cnt) {
#pragma unroll
  for (int width = 4; width >= 1; width >>= 1) {
#pragma unroll
    for (int k = 0; k < width; ++k) z[k] = 2 * k + 1 < cnt ? z[2 * k] + z[2 * k + 1] : z[2 * k];
    cnt = (cnt + 1) >> 1;
  }
  return z[0];
}

// One block per (window, tile of kTileI x kMeanTileJ); a tile outside the window's core box ends at once.  Per
// channel: the odd-k members' tile is read from y1 along their own rows (runs of 32 floats) into LDS, row
// stride kMeanTileJ + 1 words (the transposing write meets 32 distinct banks), and read back along the
// picture's rows; the even-k members are read from y0 along their rows, forward or reversed.  A lane owns
// PX pixels of the tile for all channels: it forms the tree mean of the M members in registers and writes the
// pixel's C elements once (adjacent lanes adjacent elements).  No atomics, no canvas, no second pass.
template <typename T, int C, typename Src>
__global__ __launch_bounds__(kIoThreads) void scatter_mean_kernel(Src src, MeanArgs a) {
  typedef typename Src::idx I;
  constexpr int TJ = kMeanTileJ;
  constexpr int PX = kTileI * TJ / kIoThreads;
  constexpr int kSlot = kTileI * (TJ + 1);
  __shared__ float tile[4 * kSlot];
  const uint32_t b = blockIdx.x;
  const int tj = (int)(b % (uint32_t)a.tiles_j);
  const uint32_t t = b / (uint32_t)a.tiles_j;
  const int ti = (int)(t % (uint32_t)a.tiles_i), win = (int)(t / (uint32_t)a.tiles_i);
  const int i0 = ti * kTileI, j0 = tj * TJ;
  const int32_t* e = a.table + (I)win * Src::cols;
  const Image<I> im = src.image(e);
  const int32_t* w = e + (Src::cols - 6);
  const I wr = w[0], wc = w[1];
  // the core box, cut to the window and to the window's own unpadded image
  const I r0 = max(max((I)w[2], wr), (I)0), r1 = min(min((I)w[3], wr + a.th), im.H);
  const I c0 = max(max((I)w[4], wc), (I)0), c1 = min(min((I)w[5], wc + a.tw), im.W);
  if (wr + i0 >= r1 || wr + i0 + kTileI <= r0 || wc + j0 >= c1 || wc + j0 + TJ <= c0) return;   // the whole block
  const int64_t plane = (int64_t)a.th * a.tw;
  const float* y0 = a.y0 + (int64_t)win * a.M0 * C * plane;
  const float* y1 = a.y1 + (int64_t)win * a.M1 * C * plane;
  const float scale = (float)a.M;
  float res[C][PX];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (a.M1 > 0) {
      if (c > 0) __syncthreads();       // the previous channel has been read
      int slot = 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int mode = d8_mode(a.modes, m);
        if (m >= a.M || !d8_odd(mode)) continue;
        const bool fi = d8_flip_i(mode), fj = d8_flip_j(mode);
        const float* y = y1 + ((int64_t)slot * C + c) * plane;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          const int px = (int)threadIdx.x + k * kIoThreads;
          const int il = px % kTileI, jl = px / kTileI, i = i0 + il, j = j0 + jl;
          if (i < a.th && j < a.tw)
            tile[slot * kSlot + il * (TJ + 1) + jl] = y[(int64_t)(fj ? a.tw - 1 - j : j) * a.th + (fi ? a.th - 1 - i : i)];
        }
        ++slot;
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int px = (int)threadIdx.x + k * kIoThreads;
      const int il = px / TJ, jl = px % TJ, i = i0 + il, j = j0 + jl;
      float z[8];
      int even = 0, odd = 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        z[m] = 0.0f;
        if (m >= a.M || i >= a.th || j >= a.tw) continue;
        const int mode = d8_mode(a.modes, m);
        if (d8_odd(mode)) {
          z[m] = tile[odd * kSlot + il * (TJ + 1) + jl];
          ++odd;
        } else {
          const int p = d8_flip_i(mode) ? a.th - 1 - i : i, q = d8_flip_j(mode) ? a.tw - 1 - j : j;
          z[m] = y0[((int64_t)even * C + c) * plane + (int64_t)p * a.tw + q];
          ++even;
        }
      }
      res[c][k] = __fdiv_rn(tree_sum8(z, a.M), scale);
    }
  }
  T* img = static_cast<T*>(src.base);
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int px = (int)threadIdx.x + k * kIoThreads;
    const int i = i0 + px / TJ, j = j0 + px % TJ;
    if (i >= a.th || j >= a.tw) continue;
    const I r = wr + i, col = wc + j;
    if (r < r0 || r >= r1 || col < c0 || col >= c1) continue;
    const int64_t at = (int64_t)r * im.W + col;     // 0 <= r < H and 0 <= col < W
    if (!src.has_px(at)) continue;
    const int64_t base = src.elem(im, at, C);
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (src.inside(base + c, 1)) store_px(img + base + c, res[c][k]);
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

// ---------------------------------------------------------------------------
// Training batches (grr_patch_batch): sample s is the ph x pw patch of image table[s][0] at (row, col), the
// bottom / right filled by the edge-repeating mirror (np.pad "symmetric", OpenCV's BORDER_REFLECT), moved by
// T_mode, plus Gaussian noise that is a function of (seed, sample id, element) alone.  grr_patch_pair_batch
// cuts the same patch from two arenas that share the image table -- the ground truth and its degraded version --
// and adds the noise, if any, to the degraded one.
constexpr int kPatchTile = 32;   // a block's tile of the output patch: 32 rows of 32 floats

struct PatchArgs {
  float* clean;           // [n, C, ph, pw]; the pair's target
  float* noisy;           // the pair's input
  const int32_t* table;   // [n, 4] (img, row, col, mode)
  const int64_t* ids;     // [n]
  const float* sigma;     // [n]; Pair only: may be null (no noise)
  uint64_t seed;
  int n, ph, pw;
  int tiles_y, tiles_x;   // tiles of kPatchTile x kPatchTile per output patch
  int vec;                // pw % 4 == 0 and both outputs 16-byte aligned
  const uint8_t* pair;    // Pair only: the input (degraded) arena, element for element the layout of src
};

// index r >= 0 of the mirror ...cba|abc...|cba... of n >= 1 samples: t = r mod 2n; t < n ? t : 2n - 1 - t
__device__ __forceinline__ int64_t sym_index(int64_t r, int64_t n) {
  if (r < n) return r;
  const int64_t t = r < 2 * n ? r : (int64_t)((uint64_t)r % (uint64_t)(2 * n));
  return t < n ? t : 2 * n - 1 - t;
}

// One block per (sample, 32 x 32 tile of the OUTPUT patch).  Pass 1: a lane reads one source pixel (all C
// channels) through the mirror rule, adjacent lanes adjacent elements of an image row -- for the odd quarter
// turns that walks down the tile's columns -- and puts it at its output place in LDS (row stride 33 floats:
// consecutive words for even k, 32 distinct banks for odd k).  Pass 2: a lane owns 4 consecutive output pixels
// of a row for all C channels; their 4 C noise elements (HWC order) are C whole Philox blocks when they start
// on one (pw C % 4 == 0, every training shape), else one block per element.  Plain and 16-byte vector stores
// only.  Table entries are clamped, element reads go through Arena::clamped.
// Pair: pass 1 reads the same clamped element of a.pair as well into a second tile (2 C 32 33 floats of LDS in
// all), pass 2 writes the first tile to a.clean and the second, plus the noise, to a.noisy; a block whose sigma
// is absent or 0 skips the noise (adding (float)(0 z) = +-0 to a value >= +0 leaves its bits).
template <int C, bool Pair>
__global__ __launch_bounds__(kIoThreads) void patch_batch_kernel(Arena src, PatchArgs a) {
  constexpr int LD = kPatchTile + 1;
  constexpr int kTile = C * kPatchTile * LD;
  __shared__ float tile[(Pair ? 2 : 1) * kTile];
  const uint32_t b = blockIdx.x;
  const int tx = (int)(b % (uint32_t)a.tiles_x);
  const uint32_t t = b / (uint32_t)a.tiles_x;
  const int ty = (int)(t % (uint32_t)a.tiles_y), s = (int)(t / (uint32_t)a.tiles_y);
  const int y0 = ty * kPatchTile, x0 = tx * kPatchTile;
  const int32_t* e = a.table + (int64_t)s * 4;
  const Image<int64_t> im = src.image(e);
  const int64_t row0 = clamp64(e[1], 0, im.H - 1), col0 = clamp64(e[2], 0, im.W - 1);
  int mode = e[3] & 7;
  if (d8_odd(mode) && a.ph != a.pw) mode &= 5;        // an odd turn of a non-square patch has no place
  const bool fi = d8_flip_i(mode), fj = d8_flip_j(mode), odd = d8_odd(mode);
  const uint8_t* img = static_cast<const uint8_t*>(src.base);
#pragma unroll
  for (int k = 0; k < kPatchTile * kPatchTile / kIoThreads; ++k) {
    const int px = (int)threadIdx.x + k * kIoThreads;
    const int fast = px % kPatchTile, slow = px / kPatchTile;
    const int pl = odd ? fast : slow, ql = odd ? slow : fast;
    const int p = y0 + pl, q = x0 + ql;
    if (p >= a.ph || q >= a.pw) continue;
    // (i, j) of the patch lands at (i', j') for even k and at (j', i') for odd k (ph == pw there)
    const int ip = odd ? q : p, jp = odd ? p : q;
    const int i = fi ? a.ph - 1 - ip : ip, j = fj ? a.pw - 1 - jp : jp;
    const int64_t sr = sym_index(row0 + i, im.H), sc = sym_index(col0 + j, im.W);
    const int64_t base = src.elem(im, sr * im.W + sc, C);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int64_t el = src.clamped(base + c);
      tile[(c * kPatchTile + pl) * LD + ql] = load_px(img + el);
      if (Pair) tile[kTile + (c * kPatchTile + pl) * LD + ql] = load_px(a.pair + el);
    }
  }
  __syncthreads();
  const int pl = (int)threadIdx.x / (kPatchTile / 4), quad = (int)threadIdx.x % (kPatchTile / 4);
  const int p = y0 + pl, q = x0 + 4 * quad;
  if (p >= a.ph || q >= a.pw) return;
  float v[C][4], u[C][4], w[C][4];      // u: what the noise is added to
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[c][k] = tile[(c * kPatchTile + pl) * LD + 4 * quad + k];   // past pw: unused
      u[c][k] = Pair ? tile[kTile + (c * kPatchTile + pl) * LD + 4 * quad + k] : v[c][k];
    }
  const double sg = Pair && !a.sigma ? 0.0 : (double)a.sigma[s];
  const uint64_t id = (uint64_t)a.ids[s];
  const NoiseKey key{(uint32_t)id, (uint32_t)(id >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
  const uint32_t e0 = (uint32_t)(((int64_t)p * a.pw + q) * C);      // < ph pw C < 2^31
  if (Pair && sg == 0.0) {              // uniform over the block
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) w[c][k] = u[c][k];
  } else if ((e0 & 3u) == 0) {
#pragma unroll
    for (int blk = 0; blk < C; ++blk) {
      double z[4];
      normals4((e0 >> 2) + blk, key, z);
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int el = 4 * blk + l;           // element k C + c of the lane
        w[el % C][el / C] = u[el % C][el / C] + (float)(sg * z[l]);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < C; ++c)
        w[c][k] = q + k < a.pw ? u[c][k] + (float)(sg * normal_at(e0 + k * C + c, key)) : 0.0f;
  }
  const int64_t plane = (int64_t)a.ph * a.pw;
  const int64_t at = (int64_t)s * C * plane + (int64_t)p * a.pw + q;
  if (a.vec) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 vc = {v[c][0], v[c][1], v[c][2], v[c][3]}, wc = {w[c][0], w[c][1], w[c][2], w[c][3]};
      *reinterpret_cast<f32x4*>(a.clean + at + c * plane) = vc;
      *reinterpret_cast<f32x4*>(a.noisy + at + c * plane) = wc;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q + k < a.pw) {
          a.clean[at + c * plane + k] = v[c][k];
          a.noisy[at + c * plane + k] = w[c][k];
        }
  }
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

// A host mode list, checked: 1..8 modes of 0..7, strictly ascending.  packed as D8Args / MeanArgs carry it.
struct ModeList {
  uint32_t packed;
  int M, M0, M1;      // all, even-k, odd-k
};

grr_status mode_list(const char* what, const int32_t* modes, int n_modes, ModeList* l) {
  GRR_REQUIRE(modes, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(n_modes >= 1 && n_modes <= 8, GRR_ERR_INVALID_ARG, "%s: needs 1..8 modes (got %d)", what, n_modes);
  *l = ModeList{0u, n_modes, 0, 0};
  for (int j = 0; j < n_modes; ++j) {
    const int m = modes[j];
    GRR_REQUIRE(m >= 0 && m <= 7, GRR_ERR_INVALID_ARG, "%s: mode %d is outside 0..7", what, m);
    GRR_REQUIRE(j == 0 || m > modes[j - 1], GRR_ERR_INVALID_ARG, "%s: modes must be strictly ascending (%d after %d)",
                what, m, j ? modes[j - 1] : 0);
    l->packed |= (uint32_t)m << (4 * j);
    ++(m & 2 ? l->M1 : l->M0);
  }
  return GRR_OK;
}

// The mode checks of the two gathers: one orientation.  rows: n M, the rows of the batch, or n where n <= 0.
grr_status gather_d8_modes(const char* what, const int32_t* modes, int n_modes, int n, ModeList* l, int* rows) {
  grr_status st = mode_list(what, modes, n_modes, l);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(l->M0 == 0 || l->M1 == 0, GRR_ERR_INVALID_ARG,
              "%s: the modes of one call share an orientation (got %d of even k and %d of odd k)", what, l->M0, l->M1);
  const int64_t r = n > 0 ? (int64_t)n * l->M : n;
  GRR_REQUIRE(r < (1ll << 31), GRR_ERR_UNSUPPORTED, "%s: window batch n M must be below 2^31 (got %d x %d)", what, n, l->M);
  *rows = (int)r;
  return GRR_OK;
}

D8Args d8_args(const WinArgs& wa, const ModeList& l, int n, int bh, int bw, int tile_j) {
  D8Args a{};
  a.win = wa.win;
  a.table = wa.table;
  a.n = n;
  a.th = l.M1 ? bw : bh;      // odd k: the batch holds the window turned
  a.tw = l.M1 ? bh : bw;
  a.tiles_i = (a.th + kTileI - 1) / kTileI;
  a.tiles_j = (a.tw + tile_j - 1) / tile_j;
  a.M = l.M;
  a.modes = l.packed;
  return a;
}

int gather_tile_j(int img_f32, int C) { return img_f32 || C >= 2 ? 64 : 128; }   // d8_tile_j<T, C>()

// The mode and operand checks of the two scatter_means, before image_args / arena_args: fills l; *y and *rows
// are the larger of the two batches, which those check (NULL, alignment, the 2^31 bound).
grr_status mean_modes(const char* what, const float* y0, const float* y1, const int32_t* modes, int n_modes, int n_even,
                      int n_odd, int n, ModeList* l, const float** y, int* rows) {
  grr_status st = mode_list(what, modes, n_modes, l);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(n_even + n_odd == n_modes && n_even == l->M0 && n_odd == l->M1, GRR_ERR_INVALID_ARG,
              "%s: M0 + M1 must be the list's %d modes, %d of even k and %d of odd k (got %d and %d)", what, l->M, l->M0,
              l->M1, n_even, n_odd);
  GRR_REQUIRE((l->M0 == 0 || y0) && (l->M1 == 0 || y1), GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE((uintptr_t)y0 % 4 == 0 && (uintptr_t)y1 % 4 == 0, GRR_ERR_INVALID_ARG,
              "%s: float32 and int32 operands must be 4-byte aligned", what);
  const int most = std::max(l->M0, l->M1);
  const int64_t r = n > 0 ? (int64_t)n * most : n;
  GRR_REQUIRE(r < (1ll << 31), GRR_ERR_UNSUPPORTED, "%s: window batch n M must be below 2^31 (got %d x %d)", what, n, most);
  *y = l->M0 >= l->M1 ? y0 : y1;
  *rows = (int)r;
  return GRR_OK;
}

MeanArgs mean_args(const float* y0, const float* y1, const WinArgs& wa, const ModeList& l, int n, int th, int tw) {
  MeanArgs a{};
  a.y0 = y0;
  a.y1 = y1;
  a.table = wa.table;
  a.n = n;
  a.th = th;
  a.tw = tw;
  a.tiles_i = (th + kTileI - 1) / kTileI;
  a.tiles_j = (tw + kMeanTileJ - 1) / kMeanTileJ;
  a.M = l.M;
  a.M0 = l.M0;
  a.M1 = l.M1;
  a.modes = l.packed;
  return a;
}

// n tiles_i tiles_j <= n th tw < 2^31
template <typename A>
dim3 tile_grid(const A& a) { return dim3((uint32_t)((int64_t)a.n * a.tiles_i * a.tiles_j)); }

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

grr_status grr_tile_gather_d8(const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n,
                              const int32_t* modes, int n_modes, int bh, int bw, float* out, void* stream) {
  clear_error();
  ModeList l{};
  int rows = 0;
  grr_status st = gather_d8_modes("grr_tile_gather_d8", modes, n_modes, n, &l, &rows);
  if (st != GRR_OK) return st;
  OneImage src{};
  WinArgs wa{};
  st = image_args("grr_tile_gather_d8", img, img_f32, H, W, C, table, rows, bh, bw, out, &src, &wa);
  if (st != GRR_OK) return st;
  const D8Args a = d8_args(wa, l, n, bh, bw, gather_tile_j(img_f32, C));
  if (l.M1)
    GRR_IO_DISPATCH(gather_d8_odd_kernel, OneImage, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  else
    GRR_IO_DISPATCH(gather_d8_even_kernel, OneImage, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tile_gather_d8");
}

grr_status grr_tile_scatter_mean(const float* y0, const float* y1, const int32_t* table, int n, const int32_t* modes,
                                 int n_modes, int n_even, int n_odd, int th, int tw, void* img, int img_f32, int H, int W,
                                 int C, void* stream) {
  clear_error();
  ModeList l{};
  const float* y = nullptr;
  int rows = 0;
  grr_status st = mean_modes("grr_tile_scatter_mean", y0, y1, modes, n_modes, n_even, n_odd, n, &l, &y, &rows);
  if (st != GRR_OK) return st;
  OneImage src{};
  WinArgs wa{};
  st = image_args("grr_tile_scatter_mean", img, img_f32, H, W, C, table, rows, th, tw, y, &src, &wa);
  if (st != GRR_OK) return st;
  const MeanArgs a = mean_args(y0, y1, wa, l, n, th, tw);
  GRR_IO_DISPATCH(scatter_mean_kernel, OneImage, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tile_scatter_mean");
}

grr_status grr_tiles_gather_d8(const void* arena, int64_t arena_elems, int img_f32, int C, const int64_t* img_table,
                               int n_img, const int32_t* table, int n, const int32_t* modes, int n_modes, int bh, int bw,
                               float* out, void* stream) {
  clear_error();
  ModeList l{};
  int rows = 0;
  grr_status st = gather_d8_modes("grr_tiles_gather_d8", modes, n_modes, n, &l, &rows);
  if (st != GRR_OK) return st;
  Arena src{};
  WinArgs wa{};
  st = arena_args("grr_tiles_gather_d8", arena, arena_elems, img_f32, C, img_table, n_img, table, rows, bh, bw, out, &src,
                  &wa);
  if (st != GRR_OK) return st;
  const D8Args a = d8_args(wa, l, n, bh, bw, gather_tile_j(img_f32, C));
  if (l.M1)
    GRR_IO_DISPATCH(gather_d8_odd_kernel, Arena, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  else
    GRR_IO_DISPATCH(gather_d8_even_kernel, Arena, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tiles_gather_d8");
}

grr_status grr_tiles_scatter_mean(const float* y0, const float* y1, const int32_t* table, int n, const int32_t* modes,
                                  int n_modes, int n_even, int n_odd, int th, int tw, void* arena, int64_t arena_elems,
                                  int img_f32, int C, const int64_t* img_table, int n_img, void* stream) {
  clear_error();
  ModeList l{};
  const float* y = nullptr;
  int rows = 0;
  grr_status st = mean_modes("grr_tiles_scatter_mean", y0, y1, modes, n_modes, n_even, n_odd, n, &l, &y, &rows);
  if (st != GRR_OK) return st;
  Arena src{};
  WinArgs wa{};
  st = arena_args("grr_tiles_scatter_mean", arena, arena_elems, img_f32, C, img_table, n_img, table, rows, th, tw, y, &src,
                  &wa);
  if (st != GRR_OK) return st;
  const MeanArgs a = mean_args(y0, y1, wa, l, n, th, tw);
  GRR_IO_DISPATCH(scatter_mean_kernel, Arena, img_f32, C, tile_grid(a), (hipStream_t)stream, src, a);
  return launch_status("grr_tiles_scatter_mean");
}

int grr_patch_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw) {
  if (!grr_image_arena_supported(C, n_img, arena_elems) || n < 1 || ph < 1 || pw < 1) return 0;
  const int64_t rows = (int64_t)n * ph;                                       // < 2^62
  return rows < (1ll << 31) && rows * pw <= ((1ll << 31) - 1) / C ? 1 : 0;    // n C ph pw < 2^31
}

// grr_patch_batch (input_arena null) and grr_patch_pair_batch after clear_error: the checks, then the launch.
static grr_status patch_launch(const char* what, bool pair, const uint8_t* arena, const uint8_t* input_arena,
                               int64_t arena_elems, int C, const int64_t* img_table, int n_img, const int32_t* table,
                               const int64_t* sample_ids, const float* sigma, int n, uint64_t seed, int ph, int pw,
                               float* clean, float* noisy, void* stream) {
  GRR_REQUIRE(arena && (input_arena || !pair) && img_table && table && sample_ids && (sigma || pair) && clean && noisy &&
                  arena_elems > 0 && n_img > 0 && C > 0 && n > 0 && ph > 0 && pw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4, n_img <= arena_elems < 2^62 (got C %d, %d images, %lld elements)", what, C, n_img,
              (long long)arena_elems);
  GRR_REQUIRE(grr_patch_batch_supported(C, n_img, arena_elems, n, ph, pw), GRR_ERR_UNSUPPORTED,
              "%s: patch batch n C ph pw must be below 2^31 (got %d x %d x %d x %d)", what, n, C, ph, pw);
  GRR_REQUIRE((uintptr_t)clean % 4 == 0 && (uintptr_t)noisy % 4 == 0 && (uintptr_t)table % 4 == 0 &&
                  (uintptr_t)sigma % 4 == 0,
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
  GRR_REQUIRE((uintptr_t)img_table % 8 == 0 && (uintptr_t)sample_ids % 8 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image table and the sample ids must be 8-byte aligned", what);
  const Arena src{const_cast<uint8_t*>(arena), arena_elems, img_table, n_img};
  PatchArgs a{};
  a.clean = clean;
  a.noisy = noisy;
  a.pair = input_arena;
  a.table = table;
  a.ids = sample_ids;
  a.sigma = sigma;
  a.seed = seed;
  a.n = n;
  a.ph = ph;
  a.pw = pw;
  a.tiles_y = (ph + kPatchTile - 1) / kPatchTile;
  a.tiles_x = (pw + kPatchTile - 1) / kPatchTile;
  a.vec = pw % 4 == 0 && (uintptr_t)clean % 16 == 0 && (uintptr_t)noisy % 16 == 0;
  const dim3 grid((uint32_t)((int64_t)n * a.tiles_y * a.tiles_x));   // <= n ph pw < 2^31
  hipStream_t s = (hipStream_t)stream;
  switch ((pair ? 4 : 0) + C - 1) {
    case 0: hipLaunchKernelGGL((patch_batch_kernel<1, false>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 1: hipLaunchKernelGGL((patch_batch_kernel<2, false>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 2: hipLaunchKernelGGL((patch_batch_kernel<3, false>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 3: hipLaunchKernelGGL((patch_batch_kernel<4, false>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 4: hipLaunchKernelGGL((patch_batch_kernel<1, true>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 5: hipLaunchKernelGGL((patch_batch_kernel<2, true>), grid, dim3(kIoThreads), 0, s, src, a); break;
    case 6: hipLaunchKernelGGL((patch_batch_kernel<3, true>), grid, dim3(kIoThreads), 0, s, src, a); break;
    default: hipLaunchKernelGGL((patch_batch_kernel<4, true>), grid, dim3(kIoThreads), 0, s, src, a); break;
  }
  return launch_status(what);
}

grr_status grr_patch_batch(const uint8_t* arena, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                           const int32_t* table, const int64_t* sample_ids, const float* sigma, int n, uint64_t seed,
                           int ph, int pw, float* clean, float* noisy, void* stream) {
  clear_error();
  return patch_launch("grr_patch_batch", false, arena, nullptr, arena_elems, C, img_table, n_img, table, sample_ids,
                      sigma, n, seed, ph, pw, clean, noisy, stream);
}

int grr_patch_pair_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw) {
  return grr_patch_batch_supported(C, n_img, arena_elems, n, ph, pw);     // two tiles of LDS fit at every C <= 4
}

grr_status grr_patch_pair_batch(const uint8_t* input_arena, const uint8_t* target_arena, int64_t arena_elems, int C,
                                const int64_t* img_table, int n_img, const int32_t* table, const int64_t* sample_ids,
                                const float* sigma, int n, uint64_t seed, int ph, int pw, float* target, float* input,
                                void* stream) {
  clear_error();
  return patch_launch("grr_patch_pair_batch", true, target_arena, input_arena, arena_elems, C, img_table, n_img, table,
                      sample_ids, sigma, n, seed, ph, pw, target, input, stream);
}

}  // extern "C"
