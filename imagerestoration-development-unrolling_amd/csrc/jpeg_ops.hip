// The JPEG round trip decode(encode(x)) of uint8 pictures in libjpeg's integer ("islow") arithmetic, without a
// bitstream (include/grr.h has the definition), gfx950.
//
//   grr_u8_jpeg          one HWC uint8 image (any byte address), C = 1 or 3 -> the decoded image, same size
//   grr_u8_jpeg_images   every image of an arena into the same place of a second arena, one quality per image
//
// One launch.  A 256-thread workgroup owns a 32 x 32 tile of the picture (kTile: a multiple of the 16 x 16 MCU of
// 4:2:0, so blocks and chroma cells never straddle two tiles) and keeps every plane of it in LDS as 8 x 8 blocks of
// int32, a block's rows 9 words apart so that neither a lane per row nor a lane per column meets a bank conflict:
//
//   fill     colour transform (and, for 4:2:0, the 2 x 2 chroma mean) from global memory, edge-replicated, minus 128
//   pass 1   a lane owns one row of one block: the forward DCT's row pass, 8 values in registers
//   pass 2   a lane owns one column: forward column pass, quantise, dequantise, inverse column pass -- the three
//            are one step because the quantiser is elementwise
//   pass 3   a lane owns one row: the inverse row pass, + 128, clamp
//   output   chroma up-sampling (4:2:0), colour transform back, one byte store per sample
//
// so the int intermediates never reach HBM.  4:2:0 needs decoded chroma one sample beyond the tile for the triangle
// filter: the workgroup recomputes the halo -- it codes the 4 x 4 chroma blocks around its 16 x 16 chroma samples
// (those that exist) rather than 2 x 2.  No scratch, no second launch, and a tile's bytes depend on nothing another
// workgroup wrote (DESIGN.md 5k weighs this against half-resolution planes in scratch).
//
// Width of the arithmetic: every intermediate of the four passes stays inside int32 for every input (DESIGN.md 5k has
// the bound, at most 1.88 x 10^9 < 2^31 in the inverse row pass; tests/test_jpeg_ref.py recomputes it).  The
// quantiser divides unsigned 32-bit integers: an exact quotient.  The tables are made from the quality by the
// workgroup.  No atomics, no float.
//
// The image table and the quality list of the arena form are device data: every value read from them is clamped,
// every element index read is kept inside [0, elems) and a write at or past elems is dropped, so a bad table
// gives wrong pixels, never an access outside the two arenas.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                 // rows and columns of a workgroup's tile; kernels.JPEG_TILE
constexpr int kSide = kTile / 8;          // blocks along a side of a plane's region
constexpr int kBlocks = kSide * kSide;    // blocks of one plane
constexpr int kRow = 9;                   // words between two rows of a block
constexpr int kBlk = 8 * kRow;            // words of a block
constexpr int kMaxImages = 65535;         // one grid row (blockIdx.y) per image
constexpr int64_t kMaxPixels = (1ll << 31) - 1;

// Annex K, natural order
__device__ const uint8_t kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                      14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__device__ const uint8_t kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                        24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

constexpr int C0_298 = 2446, C0_390 = 3196, C0_541 = 4433, C0_765 = 6270, C0_899 = 7373, C1_175 = 9633;
constexpr int C1_501 = 12299, C1_847 = 15137, C1_961 = 16069, C2_053 = 16819, C2_562 = 20995, C3_072 = 25172;

constexpr int fix(double x) { return (int)(x * 65536.0 + 0.5); }

struct JpegArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t elems;                // one image: H W C; arena: the elements of either arena
  const int64_t* table;         // [n_img, 3] (element offset, H, W) on the device; null: the one image below
  const int32_t* qualities;     // [n_img] on the device; null: quality
  int H, W;                     // one image: its sides; arena: they bound every image's
  int quality;
  int tiles_x;                  // tiles per row of the largest image
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }     // arithmetic shift

// the odd part both transforms share: t[0..3] -> the four sums before the final shift
__device__ __forceinline__ void odd_part(int& t4, int& t5, int& t6, int& t7) {
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * C1_175;
  t4 *= C0_298;
  t5 *= C2_053;
  t6 *= C3_072;
  t7 *= C1_501;
  z1 *= -C0_899;
  z2 *= -C2_562;
  z3 = z3 * -C1_961 + z5;
  z4 = z4 * -C0_390 + z5;
  t4 += z1 + z3;
  t5 += z2 + z4;
  t6 += z2 + z3;
  t7 += z1 + z4;
}

// jfdctint, one pass over 8 values in place; kFirst: the row pass
template <bool kFirst>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = kFirst ? 11 : 15;
  d[0] = kFirst ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = kFirst ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int z1 = (t12 + t13) * C0_541;
  d[2] = descale(z1 + t13 * C0_765, n);
  d[6] = descale(z1 - t12 * C1_847, n);
  int o4 = t4, o5 = t5, o6 = t6, o7 = t7;
  odd_part(o4, o5, o6, o7);
  d[7] = descale(o4, n);
  d[5] = descale(o5, n);
  d[3] = descale(o6, n);
  d[1] = descale(o7, n);
}

// jidctint, one pass over 8 values in place; shift 11 for the column pass, 18 for the row pass
template <int kShift>
__device__ __forceinline__ void idct8(int (&c)[8]) {
  const int z1 = (c[2] + c[6]) * C0_541;
  const int t2 = z1 - c[6] * C1_847, t3 = z1 + c[2] * C0_765;
  const int t0 = (c[0] + c[4]) * 8192, t1 = (c[0] - c[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = c[7], o1 = c[5], o2 = c[3], o3 = c[1];
  odd_part(o0, o1, o2, o3);
  c[0] = descale(t10 + o3, kShift);
  c[7] = descale(t10 - o3, kShift);
  c[1] = descale(t11 + o2, kShift);
  c[6] = descale(t11 - o2, kShift);
  c[2] = descale(t12 + o1, kShift);
  c[5] = descale(t12 - o1, kShift);
  c[3] = descale(t13 + o0, kShift);
  c[4] = descale(t13 - o0, kShift);
}

__device__ __forceinline__ int u8_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// word of sample (ly, lx), both in [0, kTile), of plane p's region
__device__ __forceinline__ int word_of(int p, int ly, int lx) {
  return (p * kBlocks + (ly >> 3) * kSide + (lx >> 3)) * kBlk + (ly & 7) * kRow + (lx & 7);
}

__device__ __forceinline__ void ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  *y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16;
  *cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16;
  *cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16;
}

// C: channels (1 or 3); kSub: 4:2:0 (C = 3 only)
template <int C, bool kSub>
__global__ __launch_bounds__(kThreads) void jpeg_kernel(JpegArgs a) {
  constexpr int kPlanes = C;
  __shared__ int32_t blk[kPlanes * kBlocks * kBlk];
  __shared__ int32_t tab[2][64];
  // this workgroup's image and tile
  int64_t off = 0;
  int H = a.H, W = a.W, q = a.quality;
  if (a.table) {
    const int64_t* it = a.table + (int64_t)blockIdx.y * 3;
    off = clamp64(it[0], 0, a.elems - 1);
    H = (int)clamp64(it[1], 1, a.H);
    W = (int)clamp64(it[2], 1, a.W);
    q = a.qualities[blockIdx.y];
  }
  q = clampi(q, 1, 100);
  const int ty0 = (int)(blockIdx.x / (uint32_t)a.tiles_x) * kTile, tx0 = (int)(blockIdx.x % (uint32_t)a.tiles_x) * kTile;
  if (ty0 >= H || tx0 >= W) return;                   // the whole workgroup: a smaller image of the arena
  const int t = (int)threadIdx.x;
  if (t < 128) {
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    const int base = t < 64 ? kLuma[t] : kChroma[t - 64];
    tab[t >> 6][t & 63] = clampi((base * scale + 50) / 100, 1, 255);
  }
  // the chroma planes: their sides, and where this workgroup's 4 x 4 blocks of them start
  const int ch = kSub ? (H + 1) / 2 : H, cw = kSub ? (W + 1) / 2 : W;
  const int oy = kSub ? ty0 / 2 - 8 : ty0, ox = kSub ? tx0 / 2 - 8 : tx0;
  // a block is coded where it holds a sample of its plane
  auto coded = [&](int b) {
    const int p = b / kBlocks, by = (b % kBlocks) / kSide, bx = b % kSide;
    const int y0 = (p ? oy : ty0) + 8 * by, x0 = (p ? ox : tx0) + 8 * bx;
    return y0 >= 0 && x0 >= 0 && y0 < (p ? ch : H) && x0 < (p ? cw : W);
  };
  auto pixel = [&](int y, int x) {                    // element of channel 0 of pixel (y, x), inside the arena
    const int64_t px = (int64_t)y * W + x;
    return min(off + px * C, a.elems - C);
  };

  // fill: samples minus 128, the last row and column replicated
  for (int idx = t; idx < kTile * kTile; idx += kThreads) {
    const int yy = idx / kTile, xx = idx % kTile;
    if (ty0 + (yy & ~7) >= H || tx0 + (xx & ~7) >= W) continue;
    const uint8_t* px = a.src + pixel(min(ty0 + yy, H - 1), min(tx0 + xx, W - 1));
    if constexpr (C == 1) {
      blk[word_of(0, yy, xx)] = (int)px[0] - 128;
    } else {
      int y, cb, cr;
      ycc(px[0], px[1], px[2], &y, &cb, &cr);
      blk[word_of(0, yy, xx)] = y - 128;
      if constexpr (!kSub) {
        blk[word_of(1, yy, xx)] = cb - 128;
        blk[word_of(2, yy, xx)] = cr - 128;
      }
    }
  }
  if constexpr (kSub) {
    for (int idx = t; idx < kTile * kTile; idx += kThreads) {
      const int yy = idx / kTile, xx = idx % kTile;
      const int by = oy + (yy & ~7), bx = ox + (xx & ~7);
      if (by < 0 || bx < 0 || by >= ch || bx >= cw) continue;
      // the padding rows hold the last chroma row; the padding columns the mean of the last full-resolution column
      const int cy = min(oy + yy, ch - 1), cx = ox + xx;
      const int r0 = min(2 * cy, H - 1), r1 = min(2 * cy + 1, H - 1);
      const int c0 = min(2 * cx, W - 1), c1 = min(2 * cx + 1, W - 1);
      int sb = 0, sr = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint8_t* px = a.src + pixel(k < 2 ? r0 : r1, (k & 1) ? c1 : c0);
        int y, cb, cr;
        ycc(px[0], px[1], px[2], &y, &cb, &cr);
        sb += cb;
        sr += cr;
      }
      const int bias = (cx & 1) ? 2 : 1;
      blk[word_of(1, yy, xx)] = ((sb + bias) >> 2) - 128;
      blk[word_of(2, yy, xx)] = ((sr + bias) >> 2) - 128;
    }
  }
  __syncthreads();

  // pass 1: forward rows.  Task k is row k % 8 of block k / 8, at word 9 k.
  for (int k = t; k < kPlanes * kBlocks * 8; k += kThreads) {
    if (!coded(k >> 3)) continue;
    int32_t* p = blk + k * kRow;
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j];
    fdct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = d[j];
  }
  __syncthreads();

  // pass 2: forward columns, quantise, dequantise, inverse columns.  Task k is column k % 8 of block k / 8.
  for (int k = t; k < kPlanes * kBlocks * 8; k += kThreads) {
    const int b = k >> 3, col = k & 7;
    if (!coded(b)) continue;
    int32_t* p = blk + b * kBlk + col;
    const int32_t* tb = tab[b >= kBlocks ? 1 : 0] + col;
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j * kRow];
    fdct8<false>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t e = (uint32_t)tb[j * 8], v = 8u * e;
      const uint32_t mag = (uint32_t)(d[j] < 0 ? -d[j] : d[j]);
      const int level = (int)((mag + (v >> 1)) / v);              // an exact integer quotient
      d[j] = (d[j] < 0 ? -level : level) * (int)e;
    }
    idct8<11>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j * kRow] = d[j];
  }
  __syncthreads();

  // pass 3: inverse rows, + 128, the plain clamp
  for (int k = t; k < kPlanes * kBlocks * 8; k += kThreads) {
    if (!coded(k >> 3)) continue;
    int32_t* p = blk + k * kRow;
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j];
    idct8<18>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = u8_clamp(d[j] + 128);
  }
  __syncthreads();

  // output
  for (int idx = t; idx < kTile * kTile; idx += kThreads) {
    const int yy = idx / kTile, xx = idx % kTile;
    const int y = ty0 + yy, x = tx0 + xx;
    if (y >= H || x >= W) continue;
    const int64_t el = off + ((int64_t)y * W + x) * C;
    const int lum = blk[word_of(0, yy, xx)];
    if constexpr (C == 1) {
      if (el < a.elems) a.dst[el] = (uint8_t)lum;
    } else {
      int cbr[2];
#pragma unroll
      for (int p = 1; p <= 2; ++p) {
        int v;
        if constexpr (!kSub) {
          v = blk[word_of(p, yy, xx)];
        } else {
          const int cy = y >> 1, cx = x >> 1;
          auto at = [&](int sy, int sx) { return blk[word_of(p, sy - oy, sx - ox)]; };      // sy - oy, sx - ox in 7..24
          if (cw <= 2) {
            v = at(cy, cx);                            // the triangle filter is off: replication
          } else {
            const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
            const int s = 3 * at(cy, cx) + at(fy, cx);
            if (x & 1) {
              v = cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * at(cy, cx + 1) + at(fy, cx + 1) + 7) >> 4;
            } else {
              v = cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * at(cy, cx - 1) + at(fy, cx - 1) + 8) >> 4;
            }
          }
        }
        cbr[p - 1] = v - 128;
      }
      const int cb = cbr[0], cr = cbr[1];
      const int r = u8_clamp(lum + ((fix(1.402) * cr + 32768) >> 16));
      const int g = u8_clamp(lum + ((-fix(.34414) * cb - fix(.71414) * cr + 32768) >> 16));
      const int bl = u8_clamp(lum + ((fix(1.772) * cb + 32768) >> 16));
      if (el + 2 < a.elems) {
        a.dst[el] = (uint8_t)r;
        a.dst[el + 1] = (uint8_t)g;
        a.dst[el + 2] = (uint8_t)bl;
      }
    }
  }
}

void launch(int C, int sub, dim3 grid, hipStream_t s, const JpegArgs& a) {
  if (C == 1) {
    hipLaunchKernelGGL((jpeg_kernel<1, false>), grid, dim3(kThreads), 0, s, a);
  } else if (sub == 0) {
    hipLaunchKernelGGL((jpeg_kernel<3, false>), grid, dim3(kThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((jpeg_kernel<3, true>), grid, dim3(kThreads), 0, s, a);
  }
}

int tiles(int n) { return (n + kTile - 1) / kTile; }

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_u8_jpeg_supported(int C, int H, int W, int sub) {
  if ((C != 1 && C != 3) || (sub != 0 && sub != 2) || H < 1 || W < 1) return 0;
  return (int64_t)H * W <= kMaxPixels / C ? 1 : 0;
}

grr_status grr_u8_jpeg(const uint8_t* src, int H, int W, int C, uint8_t* dst, int quality, int sub, void* stream) {
  clear_error();
  const char* what = "grr_u8_jpeg";
  GRR_REQUIRE(src && dst && H > 0 && W > 0 && C > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(quality >= 1 && quality <= 100, GRR_ERR_INVALID_ARG, "%s: the quality is 1..100 (got %d)", what, quality);
  GRR_REQUIRE(grr_u8_jpeg_supported(C, H, W, sub), GRR_ERR_UNSUPPORTED,
              "%s: needs C of 1 or 3, a subsampling of 0 (4:4:4) or 2 (4:2:0) and H W C < 2^31 (got %d x %d x %d, "
              "subsampling %d)", what, H, W, C, sub);
  JpegArgs a{};
  a.src = src;
  a.dst = dst;
  a.elems = (int64_t)H * W * C;
  a.H = H;
  a.W = W;
  a.quality = quality;
  a.tiles_x = tiles(W);
  launch(C, sub, dim3((uint32_t)(a.tiles_x * tiles(H))), (hipStream_t)stream, a);      // < 2^21 tiles
  return launch_status(what);
}

grr_status grr_u8_jpeg_images(const uint8_t* arena, int64_t elems, int C, const int64_t* table, int n_img, int max_h,
                              int max_w, uint8_t* dst_arena, const int32_t* qualities, int sub, void* stream) {
  clear_error();
  const char* what = "grr_u8_jpeg_images";
  GRR_REQUIRE(arena && dst_arena && table && qualities && elems > 0 && C > 0 && n_img > 0 && max_h > 0 && max_w > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE((uintptr_t)table % 8 == 0 && (uintptr_t)qualities % 4 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image table must be 8-byte and the quality list 4-byte aligned", what);
  GRR_REQUIRE(grr_u8_jpeg_supported(C, max_h, max_w, sub), GRR_ERR_UNSUPPORTED,
              "%s: needs C of 1 or 3, a subsampling of 0 (4:4:4) or 2 (4:2:0) and max_h max_w C < 2^31 (got %d x %d x "
              "%d, subsampling %d)", what, max_h, max_w, C, sub);
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, elems) && elems >= C, GRR_ERR_UNSUPPORTED,
              "%s: needs C <= n_img C <= arena elements < 2^62 (got C %d, %d images, %lld elements)", what, C, n_img,
              (long long)elems);
  GRR_REQUIRE(n_img <= kMaxImages, GRR_ERR_UNSUPPORTED, "%s: at most %d images per call (got %d)", what, kMaxImages,
              n_img);
  JpegArgs a{};
  a.src = arena;
  a.dst = dst_arena;
  a.elems = elems;
  a.table = table;
  a.qualities = qualities;
  a.H = max_h;
  a.W = max_w;
  a.tiles_x = tiles(max_w);
  launch(C, sub, dim3((uint32_t)(a.tiles_x * tiles(max_h)), (uint32_t)n_img), (hipStream_t)stream, a);
  return launch_status(what);
}

}  // extern "C"
