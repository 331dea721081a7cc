// Joint denoising and demosaicking batches (include/grr.h has the definition): a patch is cut from an RGB arena,
// sampled through the Bayer colour filter array, given signal-dependent sensor noise on the mosaic, quantised to
// `bits` bits and only then filled -- so the fill spreads and correlates the noise as a camera pipeline does -- and
// turned by T_mode, in one launch, gfx950.
//
//   grr_patch_raw_batch          (target, input) planar [n, 3, ph, pw] from a device table of (img, row, col, mode)
//   grr_u8_raw_noise_demosaic    one H x W x 3 uint8 picture -> float32 H x W x 3 (HWC), the same kernel body with
//                                row = col = 0, ph = H, pw = W, mode 0, no device tables and no target
//
// A 256-thread workgroup owns a kRows x kCols tile of one sample's patch in SOURCE orientation and keeps the tile's
// part of the quantised raw plane q, with its 2-sample halo, as int32 words in LDS (20 rows of 68 words, the row
// stride 68 words = 17 x 16 bytes, so a lane's 8-sample window of a row is two 16-byte reads):
//
//   raw      a task is one Philox block of a window row: window elements run along the row, e = wy (pw + 4) + wx, so
//            the 4 normals of block e / 4 belong to 4 adjacent LDS words.  Tasks are laid on the blocks, not on the
//            tile: a row whose first element is not the first of a block starts and ends with a task that uses part of
//            its block.  Each word reads one byte -- the site's channel of the reflected picture pixel -- and is
//            x + sqrt(a x + b) z, clipped, times 2^bits - 1, rounded to even, in float64.  A workgroup whose sample has
//            a == 0 and b == 0 runs no generator.  Halo words are recomputed by the neighbouring tiles: the generator
//            is a function of the element, so they agree.
//   fill     a lane owns 4 adjacent pixels of one row: 10 16-byte LDS reads, the demosaic kernel's sums and selects
//            with int32 q in place of bytes, one float64 division per value; the three filled channels and the three
//            target channels go to a staging tile in LDS
//   output   the staging tile is read in OUTPUT orientation, so that the odd quarter turns too write whole output
//            rows: a lane owns 4 adjacent output floats of a row for the 6 planes, one 16-byte store each where
//            pw % 4 == 0 and the outputs are 16-byte aligned, else plain stores.  The one-image form writes HWC rows.
//
// LDS: 5.4 KB of raw plane and 25 KB of staging.  No atomics; every output float is written once.
//
// The tables are device data: every value read from them is clamped -- img into [0, n_img), the image's offset into
// the arena and its sides into [1, 2^31), row and col into the image, the pattern into 0..3, the mode & 7 and an odd
// turn of a non-square patch read as mode & 5 -- and every element index read is kept inside [0, elems), so a bad
// table gives wrong pixels, never an access outside the buffers.  Outputs are addressed from (s, p, q) inside
// [n, 3, ph, pw] alone.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 16, kCols = 64;     // a workgroup's tile of the patch; kernels.RAW_NOISE_TILE
constexpr int kHalo = 2;
constexpr int kLdsRows = kRows + 2 * kHalo;
constexpr int kStride = kCols + 2 * kHalo;              // words between two LDS rows of the raw plane
constexpr int kRowTasks = kStride / 4 + 1;              // Philox blocks that touch an LDS row, whatever its phase
constexpr int kStage = kCols + 1;                       // floats between two rows of a staging plane
constexpr int64_t kMaxPixels = (1ll << 31) - 1;
constexpr int kQMax = 1 << 24;
static_assert(kRows * (kCols / 4) == kThreads, "a lane owns 4 pixels of the tile");
static_assert(kStride % 4 == 0, "an LDS row starts on 16 bytes");

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct RawArgs {
  const uint8_t* src;           // the arena, or the one picture
  int64_t elems;
  const int64_t* img_table;     // [n_img, 3] (element offset, H, W) on the device; null: the one image below
  const int32_t* patterns;      // [n_img] on the device
  const int32_t* table;         // [n, 4] (img, row, col, mode) on the device
  const int64_t* ids;           // [n] on the device
  const float* noise;           // [n, 2] (a, b) on the device, or null: no noise
  float* target;                // [n, 3, ph, pw]; unused by the one-image form
  float* input;                 // [n, 3, ph, pw]; one image: H x W x 3
  uint64_t seed;
  int n_img, n, ph, pw, tiles_y, tiles_x;
  int full;                     // 2^bits - 1
  int clip, vec;
  int H, W, pattern;            // one image
  float a, b;
  int64_t sample_id;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// any index reflected about the edge samples of a side n, which are not repeated: i mod 2(n - 1), folded
__device__ __forceinline__ int64_t reflect_any(int64_t i, int64_t n) {
  if (n == 1) return 0;
  const int64_t p = 2 * (n - 1);
  int64_t t = i % p;
  t = t < 0 ? t + p : t;
  return t < n ? t : p - t;
}

__device__ __forceinline__ bool flip_i(int m) { return (0xD2u >> m) & 1u; }     // grr_tile_gather_d8's table
__device__ __forceinline__ bool flip_j(int m) { return (0xB4u >> m) & 1u; }

// kFill: 0 zero, 1 bilinear, 2 malvar.  kOne: the one-image form
template <int kFill, bool kOne>
__global__ __launch_bounds__(kThreads) void raw_noise_kernel(RawArgs a) {
  __shared__ __attribute__((aligned(16))) int plane[kLdsRows * kStride];
  __shared__ float stage[6 * kRows * kStage];           // planes 0..2 the input, 3..5 the target
  const uint32_t bid = blockIdx.x;
  const int tx = (int)(bid % (uint32_t)a.tiles_x);
  const uint32_t rest = bid / (uint32_t)a.tiles_x;
  const int ty = (int)(rest % (uint32_t)a.tiles_y), s = (int)(rest / (uint32_t)a.tiles_y);
  const int y0 = ty * kRows, x0 = tx * kCols;
  const int y1 = min(y0 + kRows, a.ph), x1 = min(x0 + kCols, a.pw);
  const int th = y1 - y0, tw = x1 - x0;
  const int t = (int)threadIdx.x;

  int64_t off = 0, H = a.H, W = a.W, row0 = 0, col0 = 0;
  int pat = a.pattern, mode = 0;
  double na = (double)a.a, nb = (double)a.b;
  uint64_t id = (uint64_t)a.sample_id;
  if (!kOne) {
    const int32_t* e = a.table + (int64_t)s * 4;
    const int img = clampi(e[0], 0, a.n_img - 1);
    const int64_t* it = a.img_table + (int64_t)img * 3;
    off = clamp64(it[0], 0, a.elems - 1);
    H = clamp64(it[1], 1, kMaxPixels);
    W = clamp64(it[2], 1, kMaxPixels);
    row0 = clamp64(e[1], 0, H - 1);
    col0 = clamp64(e[2], 0, W - 1);
    mode = e[3] & 7;
    if ((mode & 2) && a.ph != a.pw) mode &= 5;          // an odd turn of a non-square patch has no place
    pat = a.patterns[img];
    na = a.noise ? (double)a.noise[2 * (int64_t)s] : 0.0;
    nb = a.noise ? (double)a.noise[2 * (int64_t)s + 1] : 0.0;
    id = (uint64_t)a.ids[s];
  }
  pat = clampi(pat, 0, 3);
  const int ry = pat >> 1, rx = pat & 1;                // the parities of the R site
  const bool noisy = !(na == 0.0 && nb == 0.0);         // uniform over the workgroup
  const NoiseKey key{(uint32_t)id, (uint32_t)(id >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
  const double full = (double)a.full;
  const uint8_t* img = a.src;

  // raw: LDS word (ly, lx) is q of window position (y0 + ly, x0 + lx), the picture pixel
  // (reflect(row0 + y0 + ly - 2), reflect(col0 + x0 + lx - 2)); words past the tile's own halo are not needed
  const int ww = a.pw + 2 * kHalo;
  for (int task = t; task < kLdsRows * kRowTasks; task += kThreads) {
    const int ly = task / kRowTasks, tk = task % kRowTasks;
    if (ly >= th + 2 * kHalo) continue;
    const uint32_t row_e = (uint32_t)(y0 + ly) * (uint32_t)ww + (uint32_t)x0;     // < (ph + 4)(pw + 4) < 2^31
    const int lx0 = 4 * tk - (int)(row_e & 3u);         // the LDS column of the block's lane 0
    if (lx0 >= tw + 2 * kHalo) continue;
    const int64_t yr = reflect_any(row0 + y0 + ly - kHalo, H);
    const int py = ((int)yr ^ ry) & 1;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (noisy) normals4((uint32_t)((int64_t)row_e + lx0) >> 2, key, z);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int lx = lx0 + l;
      if (lx < 0 || lx >= tw + 2 * kHalo) continue;
      const int64_t xr = reflect_any(col0 + x0 + lx - kHalo, W);
      const int ch = py + (((int)xr ^ rx) & 1);         // R 0 at (0, 0), B 2 at (1, 1), else G 1
      const int64_t el = min(off + min(yr * W + xr, kMaxPixels) * 3 + ch, a.elems - 1);
      const double x = (double)img[el] / 255.0;
      const double var = na * x + nb;
      double v = (noisy && var != 0.0) ? x + sqrt(var) * z[l] : x;
      if (a.clip) v = fmin(fmax(v, 0.0), 1.0);
      const double r = __builtin_rint(v * full);        // ties to even
      plane[ly * kStride + lx] = r != r ? 0 : (int)fmin(fmax(r, -(double)kQMax), (double)kQMax);
    }
  }
  __syncthreads();

  // fill: a lane's 4 pixels (r, 4 k .. 4 k + 3) of the tile
  {
    const int r = t / (kCols / 4), k = t % (kCols / 4);
    if (r < th && 4 * k < tw) {
      i32x4 lo[5], hi[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const i32x4* p = reinterpret_cast<const i32x4*>(plane + (r + j) * kStride + 4 * k);
        lo[j] = p[0];
        hi[j] = p[1];
      }
      auto at = [&](int j, int c) { return c < 4 ? lo[j][c & 3] : hi[j][c & 3]; };
      const int64_t yr = reflect_any(row0 + y0 + r, H);
      const int py = ((int)yr ^ ry) & 1;
      const double denom = 16.0 * full;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = i + 2;
        const int64_t xr = reflect_any(col0 + x0 + 4 * k + i, W);
        const int px = ((int)xr ^ rx) & 1;
        const int ctr = at(2, c);
        int rgb[3] = {0, 0, 0};
        if constexpr (kFill != 0) {
          const int h1 = at(2, c - 1) + at(2, c + 1), v1 = at(1, c) + at(3, c);
          const int diag = at(1, c - 1) + at(1, c + 1) + at(3, c - 1) + at(3, c + 1);
          int green, other, inrow, incol;             // G at R / B; R at B and B at R; at G: the row's and the column's colour
          if constexpr (kFill == 1) {
            green = 4 * (h1 + v1);
            other = 4 * diag;
            inrow = 8 * h1;
            incol = 8 * v1;
          } else {
            const int h2 = at(2, c - 2) + at(2, c + 2), v2 = at(0, c) + at(4, c);
            green = 8 * ctr + 4 * (h1 + v1) - 2 * (h2 + v2);
            other = 12 * ctr + 4 * diag - 3 * (h2 + v2);
            inrow = 10 * ctr + 8 * h1 - 2 * diag - 2 * h2 + v2;
            incol = 10 * ctr + 8 * v1 - 2 * diag - 2 * v2 + h2;
          }
          // at a G site the row's colour is R in an R row (py = 0) and B in a B row
          const bool site_g = py != px;
          rgb[0] = site_g ? (py ? incol : inrow) : other;
          rgb[1] = green;
          rgb[2] = site_g ? (py ? inrow : incol) : other;
        }
        const int site = py + px;                     // R 0, G 1, B 2: a measured sample passes through
        const int64_t el = off + min(yr * W + xr, kMaxPixels) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int sum = ch == site ? 16 * ctr : rgb[ch];
          const int at_stage = (ch * kRows + r) * kStage + 4 * k + i;
          stage[at_stage] = (float)((double)sum / denom);
          if (!kOne) stage[3 * kRows * kStage + at_stage] = __fdiv_rn((float)img[min(el + ch, a.elems - 1)], 255.0f);
        }
      }
    }
  }
  __syncthreads();

  if (kOne) {     // HWC rows: 3 tw adjacent floats per tile row
    const int run = 3 * tw;
    for (int idx = t; idx < th * run; idx += kThreads) {
      const int r = idx / run, m = idx % run;
      a.input[((int64_t)(y0 + r) * a.pw + x0) * 3 + m] = stage[((m % 3) * kRows + r) * kStage + m / 3];
    }
    return;
  }
  // output: pixel (i, j) of the patch, i' = flip_i ? ph - 1 - i : i and j' likewise, lands at (i', j') for even k
  // and at (j', i') for odd k (ph == pw there).  The tile's image is rows [P0, P0 + R) x columns [Q0, Q0 + Cn)
  const bool fi = flip_i(mode), fj = flip_j(mode), odd = (mode & 2) != 0;
  const int ip0 = fi ? a.ph - y1 : y0, jp0 = fj ? a.pw - x1 : x0;
  const int P0 = odd ? jp0 : ip0, Q0 = odd ? ip0 : jp0;
  const int R = odd ? tw : th, Cn = odd ? th : tw;
  const int quads = (Cn + 3) / 4;
  const int64_t area = (int64_t)a.ph * a.pw;
  for (int idx = t; idx < R * quads; idx += kThreads) {
    const int p = P0 + idx / quads, qd = idx % quads, q = Q0 + 4 * qd;
    float v[6][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qq = min(q + k, Q0 + Cn - 1);           // past the tile: unused
      const int ip = odd ? qq : p, jp = odd ? p : qq;
      const int il = (fi ? a.ph - 1 - ip : ip) - y0, jl = (fj ? a.pw - 1 - jp : jp) - x0;
#pragma unroll
      for (int c = 0; c < 6; ++c) v[c][k] = stage[(c * kRows + il) * kStage + jl];
    }
    const int64_t at = (int64_t)s * 3 * area + (int64_t)p * a.pw + q;      // the output's rows are pw wide
    if (a.vec) {      // pw % 4 == 0: Q0, Cn and area are multiples of 4
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 in = {v[c][0], v[c][1], v[c][2], v[c][3]}, tg = {v[3 + c][0], v[3 + c][1], v[3 + c][2], v[3 + c][3]};
        *reinterpret_cast<f32x4*>(a.input + at + c * area) = in;
        *reinterpret_cast<f32x4*>(a.target + at + c * area) = tg;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * qd + k < Cn) {
            a.input[at + c * area + k] = v[c][k];
            a.target[at + c * area + k] = v[3 + c][k];
          }
    }
  }
}

template <bool kOne>
void launch(int fill, dim3 grid, hipStream_t s, const RawArgs& a) {
  if (fill == 0) {
    hipLaunchKernelGGL((raw_noise_kernel<0, kOne>), grid, dim3(kThreads), 0, s, a);
  } else if (fill == 1) {
    hipLaunchKernelGGL((raw_noise_kernel<1, kOne>), grid, dim3(kThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((raw_noise_kernel<2, kOne>), grid, dim3(kThreads), 0, s, a);
  }
}

int tiles(int n, int side) { return (n + side - 1) / side; }

// the checks of fill, bits and clip both entry points share
grr_status raw_params(const char* what, int fill, int bits, int clip) {
  GRR_REQUIRE(fill >= 0 && fill <= 2, GRR_ERR_INVALID_ARG, "%s: the fill is 0 (zero), 1 (bilinear) or 2 (malvar) (got %d)",
              what, fill);
  GRR_REQUIRE(bits >= 8 && bits <= 16, GRR_ERR_INVALID_ARG, "%s: bits is 8..16 (got %d)", what, bits);
  GRR_REQUIRE(clip == 0 || clip == 1, GRR_ERR_INVALID_ARG, "%s: clip is 0 or 1 (got %d)", what, clip);
  return GRR_OK;
}

bool window_ok(int ph, int pw) { return ((int64_t)ph + 4) * ((int64_t)pw + 4) < (1ll << 31); }

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_patch_raw_batch_supported(int n_img, int64_t arena_elems, int n, int ph, int pw) {
  if (!grr_image_arena_supported(3, n_img, arena_elems) || arena_elems < 3 || n < 1 || ph < 1 || pw < 1) return 0;
  const int64_t rows = (int64_t)n * ph;                                       // < 2^62
  return rows < (1ll << 31) && rows * pw <= ((1ll << 31) - 1) / 3 && window_ok(ph, pw) ? 1 : 0;
}

grr_status grr_patch_raw_batch(const uint8_t* arena, int64_t arena_elems, const int64_t* img_table, int n_img,
                               const int32_t* patterns, const int32_t* table, const int64_t* sample_ids,
                               const float* noise, int n, uint64_t seed, int ph, int pw, int fill, int bits, int clip,
                               float* target, float* input, void* stream) {
  clear_error();
  const char* what = "grr_patch_raw_batch";
  GRR_REQUIRE(arena && img_table && patterns && table && sample_ids && target && input && arena_elems > 0 && n_img > 0 &&
                  n > 0 && ph > 0 && pw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  grr_status st = raw_params(what, fill, bits, clip);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(grr_image_arena_supported(3, n_img, arena_elems) && arena_elems >= 3, GRR_ERR_UNSUPPORTED,
              "%s: needs 3 <= 3 n_img <= arena elements < 2^62 (got %d images, %lld elements)", what, n_img,
              (long long)arena_elems);
  GRR_REQUIRE(grr_patch_raw_batch_supported(n_img, arena_elems, n, ph, pw), GRR_ERR_UNSUPPORTED,
              "%s: patch batch 3 n ph pw and the window (ph + 4)(pw + 4) must be below 2^31 (got %d x %d x %d)", what, n,
              ph, pw);
  GRR_REQUIRE((uintptr_t)target % 4 == 0 && (uintptr_t)input % 4 == 0 && (uintptr_t)table % 4 == 0 &&
                  (uintptr_t)patterns % 4 == 0 && (uintptr_t)noise % 4 == 0,
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
  GRR_REQUIRE((uintptr_t)img_table % 8 == 0 && (uintptr_t)sample_ids % 8 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image table and the sample ids must be 8-byte aligned", what);
  RawArgs a{};
  a.src = arena;
  a.elems = arena_elems;
  a.img_table = img_table;
  a.patterns = patterns;
  a.table = table;
  a.ids = sample_ids;
  a.noise = noise;
  a.target = target;
  a.input = input;
  a.seed = seed;
  a.n_img = n_img;
  a.n = n;
  a.ph = ph;
  a.pw = pw;
  a.tiles_y = tiles(ph, kRows);
  a.tiles_x = tiles(pw, kCols);
  a.full = (1 << bits) - 1;
  a.clip = clip;
  a.vec = pw % 4 == 0 && (uintptr_t)target % 16 == 0 && (uintptr_t)input % 16 == 0;
  launch<false>(fill, dim3((uint32_t)((int64_t)n * a.tiles_y * a.tiles_x)), (hipStream_t)stream, a);   // <= n ph pw < 2^31
  return launch_status(what);
}

int grr_u8_raw_noise_demosaic_supported(int H, int W) {
  if (H < 1 || W < 1) return 0;
  return (int64_t)H * W <= ((1ll << 31) - 1) / 3 && window_ok(H, W) ? 1 : 0;
}

grr_status grr_u8_raw_noise_demosaic(const uint8_t* src, int H, int W, float* dst, int pattern, int fill, float a, float b,
                                     int bits, int clip, uint64_t seed, int64_t sample_id, void* stream) {
  clear_error();
  const char* what = "grr_u8_raw_noise_demosaic";
  GRR_REQUIRE(src && dst && H > 0 && W > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  GRR_REQUIRE(pattern >= 0 && pattern <= 3, GRR_ERR_INVALID_ARG,
              "%s: the pattern is 0 (rggb), 1 (grbg), 2 (gbrg) or 3 (bggr) (got %d)", what, pattern);
  grr_status st = raw_params(what, fill, bits, clip);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(a >= 0.0f && a <= 1.0f && b >= 0.0f && b <= 1.0f, GRR_ERR_INVALID_ARG,
              "%s: the noise pair (a, b) lies in [0, 1] (got %g, %g)", what, (double)a, (double)b);
  GRR_REQUIRE(grr_u8_raw_noise_demosaic_supported(H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs 3 H W < 2^31 and (H + 4)(W + 4) < 2^31 (got %d x %d)", what, H, W);
  GRR_REQUIRE((uintptr_t)dst % 4 == 0, GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
  RawArgs r{};
  r.src = src;
  r.elems = (int64_t)H * W * 3;
  r.input = dst;
  r.seed = seed;
  r.n_img = 1;
  r.n = 1;
  r.ph = H;
  r.pw = W;
  r.tiles_y = tiles(H, kRows);
  r.tiles_x = tiles(W, kCols);
  r.full = (1 << bits) - 1;
  r.clip = clip;
  r.H = H;
  r.W = W;
  r.pattern = pattern;
  r.a = a;
  r.b = b;
  r.sample_id = sample_id;
  launch<true>(fill, dim3((uint32_t)(r.tiles_y * r.tiles_x)), (hipStream_t)stream, r);      // < 2^20 tiles
  return launch_status(what);
}

}  // extern "C"
