// Bicubic resize of uint8 pictures by an integer scale, exact (include/grr.h has the definition), gfx950.
//
//   grr_u8_resize          one HWC uint8 image (any byte address) -> the image s times smaller or larger
//   grr_u8_resize_images   every image of an arena into its place in a second arena, one launch
//
// The weights are fixed-point integers that the caller quantised (a tap set sums to 2^30); they travel in the
// kernel arguments.  The operator is separable with a rounding to uint8 between its two passes, rows (axis 0)
// first: one kernel does both.  A block owns a 32 x 32 tile of the OUTPUT.  Pass 1 computes, for the tile's 32
// output rows, the row-resized picture at every input column the tile's 32 output columns read -- their taps'
// span, at most 289 columns, walked unmirrored so that pass 2 indexes it without the mirror rule -- straight from
// global memory (adjacent lanes adjacent bytes of an image row) into LDS as uint8: the intermediate never reaches
// HBM.  Pass 2 resizes those rows along the columns out of LDS and writes each output byte once, adjacent lanes
// adjacent bytes.  Both passes accumulate q * v in 64-bit integers, so no order of the sum can change a bit.
// No atomics, no float.
//
// The image tables of the arena form are device data: every value read from them is clamped, every element
// index read is kept inside [0, src_elems) and a write at or past dst_elems is dropped, so a bad table gives
// wrong pixels, never an access outside the two arenas.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                 // output rows and columns of a block
constexpr int kMinScale = 2, kMaxScale = 8;
constexpr int kMaxPhases = kMaxScale;     // up: one tap set per output position modulo s; down: one
constexpr int kMaxTaps = 64;              // all phases together: down <= 4 s = 32, up <= 5 s = 40
constexpr int kShift = 30;                // a tap set sums to 2^30
// input columns a tile's output columns read: down, offsets within [-2 s, 3 s]: 31 s + 5 s + 1; up: far fewer
constexpr int kMaxSpan = (kTile - 1) * kMaxScale + 5 * kMaxScale + 1;
constexpr int kMaxImages = 65535;                    // one grid row (blockIdx.y) per image
constexpr int64_t kMaxPixels = (1ll << 31) - 1;      // a legal image has H W C < 2^31

// A checked host tap table as the kernel takes it: phase p has count[p] weights w[start[p] ..] at the
// offsets first[p], first[p] + 1, ... (zero weights inside the run are kept, they add nothing).
struct Taps {
  int n_phase;
  int lo, hi;                   // the smallest first offset and the largest last offset of all phases
  int first[kMaxPhases], count[kMaxPhases], start[kMaxPhases];
  int32_t w[kMaxTaps];
};

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_elems, dst_elems;
  const int64_t* src_table;     // [n_img, 3] (element offset, H, W) on the device; null: the one image below
  const int64_t* dst_table;     // [n_img, 3] (element offset, Ho, Wo)
  int H, W, Ho, Wo;             // one image: its sizes; arena: Ho, Wo bound every image's output
  int s, up;
  int tiles_x;                  // tiles per row of the largest output
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index r (any sign) of the mirror ...cba|abc...|cba... of n >= 1 samples: t = r mod 2n; t < n ? t : 2n - 1 - t
__device__ __forceinline__ int64_t sym_any(int64_t r, int64_t n) {
  if (r >= 0 && r < n) return r;
  int64_t t = r % (2 * n);
  if (t < 0) t += 2 * n;
  return t < n ? t : 2 * n - 1 - t;
}

// output position y of a pass: the phase of its tap set and the input position its offsets count from
__device__ __forceinline__ void tap_origin(int64_t y, int s, int up, int* phase, int64_t* base) {
  *phase = up ? (int)(y % s) : 0;
  *base = up ? y / s : y * s;
}

__device__ __forceinline__ uint8_t round_u8(int64_t acc) {
  const int64_t v = (acc + (1ll << (kShift - 1))) >> kShift;      // arithmetic shift
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int C>
__global__ __launch_bounds__(kThreads) void resize_kernel(ResizeArgs a, Taps taps) {
  __shared__ uint8_t inter[kTile * kMaxSpan * C];     // [row of the tile][unmirrored input column - c_lo][channel]
  __shared__ int32_t tw[kMaxTaps];
  __shared__ int tfirst[kMaxPhases], tcount[kMaxPhases], tstart[kMaxPhases];
  // this block's image and tile
  int64_t soff = 0, doff = 0, H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo;
  if (a.src_table) {
    const int64_t* st = a.src_table + (int64_t)blockIdx.y * 3;
    const int64_t* dt = a.dst_table + (int64_t)blockIdx.y * 3;
    soff = clamp64(st[0], 0, a.src_elems - 1);
    H = clamp64(st[1], 1, kMaxPixels);
    W = clamp64(st[2], 1, kMaxPixels);
    doff = clamp64(dt[0], 0, a.dst_elems);
    Ho = clamp64(dt[1], 1, a.Ho);
    Wo = clamp64(dt[2], 1, a.Wo);
  }
  const int ty0 = (int)(blockIdx.x / (uint32_t)a.tiles_x) * kTile, tx0 = (int)(blockIdx.x % (uint32_t)a.tiles_x) * kTile;
  if (ty0 >= Ho || tx0 >= Wo) return;                 // the whole block: a smaller image of the arena
  if (threadIdx.x < kMaxTaps) tw[threadIdx.x] = taps.w[threadIdx.x];
  if (threadIdx.x < kMaxPhases) {
    tfirst[threadIdx.x] = taps.first[threadIdx.x];
    tcount[threadIdx.x] = taps.count[threadIdx.x];
    tstart[threadIdx.x] = taps.start[threadIdx.x];
  }
  const int th = (int)min((int64_t)kTile, Ho - ty0), twid = (int)min((int64_t)kTile, Wo - tx0);
  int ph;
  int64_t b_lo, b_hi;
  tap_origin(tx0, a.s, a.up, &ph, &b_lo);
  tap_origin(tx0 + twid - 1, a.s, a.up, &ph, &b_hi);
  const int64_t c_lo = b_lo + taps.lo;
  const int span = (int)min((int64_t)kMaxSpan, b_hi + taps.hi - c_lo + 1);    // <= kMaxSpan for a checked table
  const int row_bytes = span * C;
  __syncthreads();
  // pass 1, rows: inter[r][col - c_lo][ch] = the row-resized picture at (ty0 + r, sym(col), ch)
  for (int idx = (int)threadIdx.x; idx < th * row_bytes; idx += kThreads) {
    const int r = idx / row_bytes, e = idx - r * row_bytes;
    const int cpos = e / C, ch = e - cpos * C;
    const int64_t col = sym_any(c_lo + cpos, W);
    int phase;
    int64_t base;
    tap_origin(ty0 + r, a.s, a.up, &phase, &base);
    const int n = tcount[phase], w0 = tstart[phase];
    base += tfirst[phase];
    int64_t acc = 0;
    for (int k = 0; k < n; ++k) {
      const int64_t px = min(sym_any(base + k, H) * W + col, kMaxPixels);
      const int64_t el = min(soff + px * C + ch, a.src_elems - 1);
      acc += (int64_t)tw[w0 + k] * (int64_t)a.src[el];
    }
    inter[r * (kMaxSpan * C) + e] = round_u8(acc);
  }
  __syncthreads();
  // pass 2, columns, out of LDS
  const int out_bytes = twid * C;
  for (int idx = (int)threadIdx.x; idx < th * out_bytes; idx += kThreads) {
    const int r = idx / out_bytes, e = idx - r * out_bytes;
    const int xl = e / C, ch = e - xl * C;
    int phase;
    int64_t base;
    tap_origin(tx0 + xl, a.s, a.up, &phase, &base);
    const int n = tcount[phase], w0 = tstart[phase];
    // 0 <= at, at + n - 1 < span for a checked table; cut to the row all the same
    const int at = (int)(base + tfirst[phase] - c_lo);
    const uint8_t* row = inter + r * (kMaxSpan * C) + ch;
    int64_t acc = 0;
    for (int k = 0; k < n; ++k) acc += (int64_t)tw[w0 + k] * (int64_t)row[clampi(at + k, 0, span - 1) * C];
    const int64_t px = (int64_t)(ty0 + r) * Wo + tx0 + xl;       // < Ho Wo <= a.Ho a.Wo < 2^31
    const int64_t el = doff + px * C + ch;
    if (el < a.dst_elems) a.dst[el] = round_u8(acc);
  }
}

int out_down(int n, int s) { return (n + s - 1) / s; }

// The checks both entry points share, after their own "bad args"; fills t.
grr_status tap_args(const char* what, int s, int up, int n_phase, const int32_t* first, const int32_t* count,
                    const int32_t* taps, Taps* t) {
  GRR_REQUIRE(s >= kMinScale && s <= kMaxScale && (up == 0 || up == 1), GRR_ERR_UNSUPPORTED,
              "%s: needs a scale of %d..%d and up of 0 or 1 (got %d, %d)", what, kMinScale, kMaxScale, s, up);
  GRR_REQUIRE(first && count && taps, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(n_phase == (up ? s : 1), GRR_ERR_INVALID_ARG, "%s: a tap table has %d phase(s) at scale %d (got %d)", what,
              up ? s : 1, s, n_phase);
  *t = Taps{};
  t->n_phase = n_phase;
  // the offsets the definition can give: down |u - j| < 2 s about u = (s - 1) / 2, up |u - j| < 2 about |u| < 1/2
  const int off_lo = up ? -2 : -2 * s, off_hi = up ? 2 : 3 * s;
  int at = 0;
  for (int p = 0; p < n_phase; ++p) {
    GRR_REQUIRE(count[p] >= 1 && count[p] <= 4 * s, GRR_ERR_INVALID_ARG,
                "%s: phase %d has %d taps; a phase has 1..4 s = %d", what, p, count[p], 4 * s);
    GRR_REQUIRE(first[p] >= off_lo && (int64_t)first[p] + count[p] - 1 <= off_hi && at + count[p] <= kMaxTaps,
                GRR_ERR_INVALID_ARG, "%s: phase %d has taps at %d..%lld, outside the kernel's support %d..%d", what, p,
                first[p], (long long)first[p] + count[p] - 1, off_lo, off_hi);
    int64_t sum = 0;
    for (int k = 0; k < count[p]; ++k) {
      sum += taps[at + k];
      t->w[at + k] = taps[at + k];
    }
    GRR_REQUIRE(sum == (1ll << kShift), GRR_ERR_INVALID_ARG, "%s: the taps of phase %d sum to %lld, not 2^%d", what, p,
                (long long)sum, kShift);
    t->first[p] = first[p];
    t->count[p] = count[p];
    t->start[p] = at;
    const int last = first[p] + count[p] - 1;
    if (p == 0 || first[p] < t->lo) t->lo = first[p];
    if (p == 0 || last > t->hi) t->hi = last;
    at += count[p];
  }
  return GRR_OK;
}

void launch(int C, dim3 grid, hipStream_t s, const ResizeArgs& a, const Taps& t) {
  switch (C) {
    case 1: hipLaunchKernelGGL((resize_kernel<1>), grid, dim3(kThreads), 0, s, a, t); break;
    case 2: hipLaunchKernelGGL((resize_kernel<2>), grid, dim3(kThreads), 0, s, a, t); break;
    case 3: hipLaunchKernelGGL((resize_kernel<3>), grid, dim3(kThreads), 0, s, a, t); break;
    default: hipLaunchKernelGGL((resize_kernel<4>), grid, dim3(kThreads), 0, s, a, t); break;
  }
}

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_u8_resize_supported(int C, int H, int W, int s, int up) {
  if (C < 1 || C > 4 || s < kMinScale || s > kMaxScale || H < 1 || W < 1) return 0;
  const int64_t in = (int64_t)H * W;                 // < 2^62
  if (in > kMaxPixels / C) return 0;                 // H W C < 2^31, so in s s below is < 2^37
  const int64_t out = up ? in * s * s : (int64_t)out_down(H, s) * out_down(W, s);
  return out <= kMaxPixels / C ? 1 : 0;              // and the output's element count as well
}

grr_status grr_u8_resize(const uint8_t* src, int H, int W, int C, uint8_t* dst, int Ho, int Wo, int s, int up,
                         int n_phase, const int32_t* first, const int32_t* count, const int32_t* taps, void* stream) {
  clear_error();
  const char* what = "grr_u8_resize";
  GRR_REQUIRE(src && dst && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  Taps t;
  grr_status st = tap_args(what, s, up, n_phase, first, count, taps, &t);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(grr_u8_resize_supported(C, H, W, s, up), GRR_ERR_UNSUPPORTED,
              "%s: needs C <= 4 and fewer than 2^31 input and output elements (got %d x %d x %d, scale %d, up %d)", what,
              H, W, C, s, up);
  if (up) {
    GRR_REQUIRE(Ho > (int64_t)s * (H - 1) && Ho <= (int64_t)s * H && Wo > (int64_t)s * (W - 1) && Wo <= (int64_t)s * W,
                GRR_ERR_SHAPE, "%s: the output of %d x %d at scale %d has sides in (s (n - 1), s n] (got %d x %d)", what,
                H, W, s, Ho, Wo);
  } else {
    GRR_REQUIRE(Ho == out_down(H, s) && Wo == out_down(W, s), GRR_ERR_SHAPE,
                "%s: the output of %d x %d at scale %d is %d x %d (got %d x %d)", what, H, W, s, out_down(H, s),
                out_down(W, s), Ho, Wo);
  }
  ResizeArgs a{};
  a.src = src;
  a.dst = dst;
  a.src_elems = (int64_t)H * W * C;
  a.dst_elems = (int64_t)Ho * Wo * C;
  a.H = H;
  a.W = W;
  a.Ho = Ho;
  a.Wo = Wo;
  a.s = s;
  a.up = up;
  a.tiles_x = (Wo + kTile - 1) / kTile;
  launch(C, dim3((uint32_t)(a.tiles_x * ((Ho + kTile - 1) / kTile))), (hipStream_t)stream, a, t);    // < 2^21 tiles
  return launch_status(what);
}

grr_status grr_u8_resize_images(const uint8_t* src_arena, int64_t src_elems, const int64_t* src_table,
                                uint8_t* dst_arena, int64_t dst_elems, const int64_t* dst_table, int C, int n_img,
                                int max_ho, int max_wo, int s, int up, int n_phase, const int32_t* first,
                                const int32_t* count, const int32_t* taps, void* stream) {
  clear_error();
  const char* what = "grr_u8_resize_images";
  GRR_REQUIRE(src_arena && dst_arena && src_table && dst_table && src_elems > 0 && dst_elems > 0 && C > 0 && n_img > 0 &&
                  max_ho > 0 && max_wo > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  Taps t;
  grr_status st = tap_args(what, s, up, n_phase, first, count, taps, &t);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, src_elems) && grr_image_arena_supported(C, n_img, dst_elems),
              GRR_ERR_UNSUPPORTED, "%s: needs C <= 4, n_img <= arena elements < 2^62 (got C %d, %d images, %lld and %lld)",
              what, C, n_img, (long long)src_elems, (long long)dst_elems);
  GRR_REQUIRE(n_img <= kMaxImages, GRR_ERR_UNSUPPORTED, "%s: at most %d images per call (got %d)", what, kMaxImages,
              n_img);
  GRR_REQUIRE(grr_image_io_supported(C, max_ho, max_wo), GRR_ERR_UNSUPPORTED,
              "%s: the largest output must have fewer than 2^31 elements (got %d x %d x %d)", what, max_ho, max_wo, C);
  GRR_REQUIRE((uintptr_t)src_table % 8 == 0 && (uintptr_t)dst_table % 8 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image tables must be 8-byte aligned", what);
  ResizeArgs a{};
  a.src = src_arena;
  a.dst = dst_arena;
  a.src_elems = src_elems;
  a.dst_elems = dst_elems;
  a.src_table = src_table;
  a.dst_table = dst_table;
  a.Ho = max_ho;
  a.Wo = max_wo;
  a.s = s;
  a.up = up;
  a.tiles_x = (max_wo + kTile - 1) / kTile;
  launch(C, dim3((uint32_t)(a.tiles_x * ((max_ho + kTile - 1) / kTile)), (uint32_t)n_img), (hipStream_t)stream, a, t);
  return launch_status(what);
}

}  // extern "C"
