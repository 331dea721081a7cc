// Inpainting batches (include/grr.h has the definition): a patch is cut from a uint8 arena, a Bernoulli mask that is a
// function of (seed, sample id, window element) decides which pixels are known, the missing ones are filled -- by zero,
// or by a normalised convolution of the known ones under a uint8 weight table -- and the patch is turned by T_mode, in
// one launch, gfx950.  All arithmetic is integer and exact.
//
//   grr_patch_mask_batch   (target, input, mask) planar [n, C, ph, pw] / [n, 1, ph, pw] from a device table of
//                          (img, row, col, mode) and a device list of known shares
//   grr_u8_mask_fill       one H x W x C uint8 picture -> uint8 H x W x C and a uint8 H x W mask of what is known now,
//                          the same kernel body with row = col = 0, ph = H, pw = W, mode 0 and no device tables; the
//                          mask is drawn as the patch form draws it, or given
//
// A 256-thread workgroup owns a kRows x kCols tile of one sample's patch in SOURCE orientation and keeps, with a halo of
// the table's own radius (ry, rx) <= 7, C byte planes of v k (the pixel's bytes, zeroed where it is missing) and one
// byte plane of k (the known bit) in LDS:
//
//   mask     a task is one Philox block of a window row: window elements run along the row, e = wy (pw + 14) + wx, so
//            the 4 words of block e / 4 belong to 4 adjacent LDS bytes.  Tasks are laid on the blocks, not on the tile:
//            a row whose first element is not the first of a block starts and ends with a task that uses part of its
//            block.  Each element reads the C bytes of the mirrored picture pixel.  A workgroup whose share is 0 or
//            2^24, or whose mask is given, runs no generator.  Halo elements are recomputed by the neighbouring tiles:
//            the generator is a function of the element, so they agree.  Elements of the tile itself also put their
//            target bytes, the known bytes (0 where missing) and the mask code into the staging tile
//   fill     a lane owns 4 adjacent pixels of one row and, if one of them is missing, takes den and num_c of all 4 as
//            byte dot products (v_dot4_u32_u8) of the k plane and the v k planes against the weights, four taps of a
//            row to a dword: the window of tap group g of pixel p is bytes 4 (k + g) + p .. + 3 of the LDS row, dword
//            k + g for p = 0 and v_alignbyte_b32 of dwords k + g, k + g + 1 otherwise.  (2 num + den) / (2 den) is an
//            unsigned 32-bit division.  The zero fill has no LDS planes and no such step
//   output   the staging tile is read in OUTPUT orientation, so that the odd quarter turns too write whole output
//            rows: a lane owns 4 adjacent output floats of a row for the 2 C + 1 planes, one 16-byte store each where
//            pw % 4 == 0 and the outputs are 16-byte aligned, else plain stores.  The one-picture form writes HWC bytes
//
// LDS rows of the byte planes are kStride = 192 bytes = 48 dwords apart, so that the two rows of a 32-lane group (16
// lanes each) of a ds_read_b32 fall on disjoint banks (banks are dword mod 32 there); 5.6 KB a plane.  The staging
// tile is bytes, rows 68 apart: 17 dwords, odd, so that an odd turn's walk down a column spreads over the banks.
// No atomics; every output element is written once.
//
// The tables are device data: every value read from them is clamped -- img into [0, n_img), the image's offset into
// the arena and its sides into [1, 2^31), row and col into the image, the mode & 7 and an odd turn of a non-square
// patch read as mode & 5, the share into [0, 2^24] -- and every element index read is kept inside [0, elems), so a bad
// table gives wrong pixels, never an access outside the buffers.  Outputs are addressed from (s, p, q) inside
// [n, C, ph, pw] alone.
#include "grr_device.h"

namespace grr {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 16, kCols = 64;     // a workgroup's tile of the patch; kernels.MASK_TILE
constexpr int kHalo = GRR_MASK_HALO;
constexpr int kMaxSide = GRR_MASK_MAX_SIDE;
constexpr int kUnit = GRR_MASK_ONE;
constexpr int kGroups = (kMaxSide + 3) / 4;               // tap groups of a table row
constexpr int kLdsRows = kRows + 2 * kHalo;
constexpr int kLdsCols = kCols + 2 * kHalo;
constexpr int kRowTasks = (kLdsCols + 3 + 3) / 4;         // Philox blocks that touch an LDS row, whatever its phase
constexpr int kStride = 192;                              // bytes between two LDS rows of a byte plane
constexpr int kPlane = kLdsRows * kStride / 4;            // dwords of one plane
constexpr int kStage = kCols + 4;                         // bytes between two rows of a staging plane
constexpr int kStagePlane = kRows * kStage;
constexpr int64_t kMaxPixels = (1ll << 31) - 1;
static_assert(kRows * (kCols / 4) == kThreads, "a lane owns 4 pixels of the tile");
static_assert(2 * kHalo + 1 == kMaxSide, "the halo is the largest table's radius");
static_assert((kCols / 4 + kGroups) * 4 <= kStride && kStride % 4 == 0, "LDS row: the last group's second dword");
static_assert(kLdsCols <= kStride && kStage % 4 == 0, "LDS rows");

struct MaskArgs {
  const uint8_t* src;           // the arena, or the one picture
  int64_t elems;
  const int64_t* img_table;     // [n_img, 3] (element offset, H, W) on the device; one picture: unused
  const int32_t* table;         // [n, 4] (img, row, col, mode) on the device
  const int64_t* ids;           // [n] on the device
  const int32_t* keep;          // [n] on the device
  const uint8_t* weights;       // [kh, kw] on the device
  const uint8_t* mask_in;       // one picture: H x W, or null (the mask is drawn)
  float* target;                // [n, C, ph, pw]
  float* input;                 // [n, C, ph, pw]
  float* mask;                  // [n, 1, ph, pw] or null
  uint8_t* dst;                 // one picture: H x W x C
  uint8_t* mask_out;            // one picture: H x W
  uint64_t seed;
  int n_img, n, ph, pw, tiles_y, tiles_x;
  int kh, kw, hole, vec;
  int H, W, keep_one;           // one picture
  int64_t sample_id;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index r (any sign) of the mirror ...cba|abc...|cba... of n >= 1 samples: t = r mod 2n; t < n ? t : 2n - 1 - t
__device__ __forceinline__ int64_t sym_any(int64_t r, int64_t n) {
  if (r >= 0 && r < n) return r;
  int64_t t = r % (2 * n);
  if (t < 0) t += 2 * n;
  return t < n ? t : 2 * n - 1 - t;
}

__device__ __forceinline__ bool flip_i(int m) { return (0xD2u >> m) & 1u; }     // grr_tile_gather_d8's table
__device__ __forceinline__ bool flip_j(int m) { return (0xB4u >> m) & 1u; }

// kFill: 0 zero, 1 conv.  kOne: the one-picture form
template <int C, int kFill, bool kOne>
__global__ __launch_bounds__(kThreads) void mask_fill_kernel(MaskArgs a) {
  constexpr int kPlanes = kFill ? C + 1 : 0;              // v k per channel, then k
  __shared__ __attribute__((aligned(16))) uint32_t planes[kPlanes ? kPlanes * kPlane : 1];
  __shared__ __attribute__((aligned(16))) uint8_t stage[(2 * C + 1) * kStagePlane];     // input, target, mask code
  __shared__ uint32_t wts[kMaxSide * kGroups];            // four taps of a table row to a dword
  const uint32_t bid = blockIdx.x;
  const int tx = (int)(bid % (uint32_t)a.tiles_x);
  const uint32_t rest = bid / (uint32_t)a.tiles_x;
  const int ty = (int)(rest % (uint32_t)a.tiles_y), s = (int)(rest / (uint32_t)a.tiles_y);
  const int y0 = ty * kRows, x0 = tx * kCols;
  const int y1 = min(y0 + kRows, a.ph), x1 = min(x0 + kCols, a.pw);
  const int th = y1 - y0, tw = x1 - x0;
  const int t = (int)threadIdx.x;

  int64_t off = 0, H = a.H, W = a.W, row0 = 0, col0 = 0;
  int mode = 0, keep = a.keep_one;
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
    if ((mode & 2) && a.ph != a.pw) mode &= 5;            // an odd turn of a non-square patch has no place
    keep = a.keep[s];
    id = (uint64_t)a.ids[s];
  }
  keep = clampi(keep, 0, kUnit);
  const bool given = kOne && a.mask_in != nullptr;
  const bool draws = !given && keep > 0 && keep < kUnit;  // uniform over the workgroup
  const bool all_known = !given && keep >= kUnit;
  const int kh = kFill ? a.kh : 1, kw = kFill ? a.kw : 1;
  const int ry = kh >> 1, rx = kw >> 1, groups = (kw + 3) >> 2;
  const uint8_t* img = a.src;
  uint8_t* bytes = reinterpret_cast<uint8_t*>(planes);

  if (kFill) {
    for (int idx = t; idx < kh * kGroups; idx += kThreads) {
      const int i = idx / kGroups, g = idx % kGroups;
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * g + b < kw) w |= (uint32_t)a.weights[i * kw + 4 * g + b] << (8 * b);
      wts[idx] = w;
    }
  }

  // mask: LDS byte (ly, lc) is window position (y0 + ly + 7 - ry, x0 + lc + 7 - rx), the picture pixel
  // (sym(row0 + y0 + ly - ry), sym(col0 + x0 + lc - rx)); the element index is the window's, whatever the radius
  const int ww = a.pw + 2 * kHalo;
  const int need_rows = th + 2 * ry, need_cols = tw + 2 * rx;
  for (int task = t; task < kLdsRows * kRowTasks; task += kThreads) {
    const int ly = task / kRowTasks, tk = task % kRowTasks;
    if (ly >= need_rows) continue;
    const uint32_t row_e = (uint32_t)(y0 + ly + kHalo - ry) * (uint32_t)ww + (uint32_t)(x0 + kHalo - rx);   // < 2^31
    const int lc0 = 4 * tk - (int)(row_e & 3u);           // the LDS column of the block's word 0
    if (lc0 >= need_cols) continue;
    const int64_t yr = sym_any(row0 + y0 + ly - ry, H);
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if (draws)
      philox4x32_10((uint32_t)((int64_t)row_e + lc0) >> 2, 1u, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)a.seed,
                    (uint32_t)(a.seed >> 32), x);
    const int r = ly - ry;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int lc = lc0 + l;
      if (lc < 0 || lc >= need_cols) continue;
      const int64_t xr = sym_any(col0 + x0 + lc - rx, W);
      const int64_t px = min(yr * W + xr, kMaxPixels);
      int code = 1;                                       // what mask_out carries for a known pixel
      if (given) code = a.mask_in[px];
      const bool known = given ? code != 0 : (all_known || (draws && (int)(x[l] >> 8) < keep));
      const int64_t el = off + px * C;
      const int j = lc - rx;
      const bool core = r >= 0 && r < th && j >= 0 && j < tw;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint8_t v = img[min(el + c, a.elems - 1)];
        const uint8_t vk = known ? v : (uint8_t)0;
        if (kFill) bytes[c * (kPlane * 4) + ly * kStride + lc] = vk;
        if (core) {
          stage[c * kStagePlane + r * kStage + j] = vk;
          stage[(C + c) * kStagePlane + r * kStage + j] = v;
        }
      }
      if (kFill) bytes[C * (kPlane * 4) + ly * kStride + lc] = known ? 1 : 0;
      if (core) stage[2 * C * kStagePlane + r * kStage + j] = (uint8_t)(known ? code : 0);
    }
  }
  __syncthreads();

  // fill: a lane's 4 pixels (r, 4 k .. 4 k + 3) of the tile; sample (r, j) is LDS byte (r + ry, j + rx), so tap (i, jj)
  // of pixel j is LDS byte (r + i, j + jj)
  if (kFill && !all_known) {
    const int r = t / (kCols / 4), k = t % (kCols / 4);
    uint8_t* code = stage + 2 * C * kStagePlane + r * kStage + 4 * k;
    const uint32_t m4 = *reinterpret_cast<const uint32_t*>(code);
    const bool missing = ((m4 & 0xFFu) == 0) || ((m4 & 0xFF00u) == 0) || ((m4 & 0xFF0000u) == 0) || ((m4 >> 24) == 0);
    if (r < th && 4 * k < tw && missing) {
      uint32_t acc[C + 1][4];
#pragma unroll
      for (int pl = 0; pl <= C; ++pl)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[pl][p] = 0;
      for (int i = 0; i < kh; ++i) {
        uint32_t d0[C + 1];
#pragma unroll
        for (int pl = 0; pl <= C; ++pl) d0[pl] = planes[pl * kPlane + (r + i) * (kStride / 4) + k];
        for (int g = 0; g < groups; ++g) {
          const uint32_t w = wts[i * kGroups + g];
#pragma unroll
          for (int pl = 0; pl <= C; ++pl) {
            const uint32_t d1 = planes[pl * kPlane + (r + i) * (kStride / 4) + k + g + 1];
            acc[pl][0] = __builtin_amdgcn_udot4(d0[pl], w, acc[pl][0], false);
            acc[pl][1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0[pl], 1), w, acc[pl][1], false);
            acc[pl][2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0[pl], 2), w, acc[pl][2], false);
            acc[pl][3] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(d1, d0[pl], 3), w, acc[pl][3], false);
            d0[pl] = d1;
          }
        }
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if ((m4 >> (8 * p)) & 0xFFu) continue;            // known: passes through
        const uint32_t den = acc[C][p];                   // <= 225 * 255
#pragma unroll
        for (int c = 0; c < C; ++c)                       // num <= 255 den: 2 num + den < 2^25
          stage[c * kStagePlane + r * kStage + 4 * k + p] = den ? (uint8_t)((2u * acc[c][p] + den) / (2u * den)) : (uint8_t)a.hole;
        if (kOne && den) code[p] = 2;
      }
    }
  }
  __syncthreads();

  if (kOne) {     // HWC rows: C tw adjacent bytes per tile row, and tw bytes of the mask
    const int run = C * tw;
    for (int idx = t; idx < th * run; idx += kThreads) {
      const int r = idx / run, m = idx % run;
      a.dst[((int64_t)(y0 + r) * a.pw + x0) * C + m] = stage[(m % C) * kStagePlane + r * kStage + m / C];
    }
    for (int idx = t; idx < th * tw; idx += kThreads) {
      const int r = idx / tw, j = idx % tw;
      a.mask_out[(int64_t)(y0 + r) * a.pw + x0 + j] = stage[2 * C * kStagePlane + r * kStage + j];
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
    float v[2 * C + 1][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int qq = min(q + k, Q0 + Cn - 1);             // past the tile: unused
      const int ip = odd ? qq : p, jp = odd ? p : qq;
      const int il = (fi ? a.ph - 1 - ip : ip) - y0, jl = (fj ? a.pw - 1 - jp : jp) - x0;
#pragma unroll
      for (int c = 0; c < 2 * C; ++c) v[c][k] = __fdiv_rn((float)stage[c * kStagePlane + il * kStage + jl], 255.0f);
      v[2 * C][k] = stage[2 * C * kStagePlane + il * kStage + jl] ? 1.0f : 0.0f;
    }
    const int64_t px = (int64_t)p * a.pw + q;             // the output's rows are pw wide
    const int64_t at = (int64_t)s * C * area + px;
    if (a.vec) {      // pw % 4 == 0: Q0, Cn and area are multiples of 4
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const f32x4 in = {v[c][0], v[c][1], v[c][2], v[c][3]}, tg = {v[C + c][0], v[C + c][1], v[C + c][2], v[C + c][3]};
        *reinterpret_cast<f32x4*>(a.input + at + c * area) = in;
        *reinterpret_cast<f32x4*>(a.target + at + c * area) = tg;
      }
      if (a.mask) {
        const f32x4 mk = {v[2 * C][0], v[2 * C][1], v[2 * C][2], v[2 * C][3]};
        *reinterpret_cast<f32x4*>(a.mask + (int64_t)s * area + px) = mk;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * qd + k < Cn) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            a.input[at + c * area + k] = v[c][k];
            a.target[at + c * area + k] = v[C + c][k];
          }
          if (a.mask) a.mask[(int64_t)s * area + px + k] = v[2 * C][k];
        }
    }
  }
}

template <int C, bool kOne>
void launch_c(int fill, dim3 grid, hipStream_t s, const MaskArgs& a) {
  if (fill == 0) {
    hipLaunchKernelGGL((mask_fill_kernel<C, 0, kOne>), grid, dim3(kThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL((mask_fill_kernel<C, 1, kOne>), grid, dim3(kThreads), 0, s, a);
  }
}

template <bool kOne>
void launch(int C, int fill, dim3 grid, hipStream_t s, const MaskArgs& a) {
  switch (C) {
    case 1: launch_c<1, kOne>(fill, grid, s, a); break;
    case 2: launch_c<2, kOne>(fill, grid, s, a); break;
    case 3: launch_c<3, kOne>(fill, grid, s, a); break;
    default: launch_c<4, kOne>(fill, grid, s, a); break;
  }
}

int tiles(int n, int side) { return (n + side - 1) / side; }

// the checks of C, the table's sides, the fill and the hole both entry points share
grr_status mask_params(const char* what, int C, int kh, int kw, int fill, int hole) {
  GRR_REQUIRE(C >= 1 && C <= 4, GRR_ERR_INVALID_ARG, "%s: C is 1..4 (got %d)", what, C);
  GRR_REQUIRE(kh >= 1 && kh <= kMaxSide && kw >= 1 && kw <= kMaxSide && (kh & 1) && (kw & 1), GRR_ERR_INVALID_ARG,
              "%s: the weight table's sides are odd and lie in 1..%d (got %d x %d)", what, kMaxSide, kh, kw);
  GRR_REQUIRE(fill >= 0 && fill <= 1, GRR_ERR_INVALID_ARG, "%s: the fill is 0 (zero) or 1 (conv) (got %d)", what, fill);
  GRR_REQUIRE(hole >= 0 && hole <= 255, GRR_ERR_INVALID_ARG, "%s: the hole is a byte 0..255 (got %d)", what, hole);
  return GRR_OK;
}

bool window_ok(int ph, int pw) { return ((int64_t)ph + 2 * kHalo) * ((int64_t)pw + 2 * kHalo) < (1ll << 31); }

}  // namespace
}  // namespace grr

using namespace grr;

extern "C" {

int grr_patch_mask_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw) {
  return grr_patch_batch_supported(C, n_img, arena_elems, n, ph, pw) && window_ok(ph, pw) ? 1 : 0;
}

grr_status grr_patch_mask_batch(const uint8_t* arena, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                                const int32_t* table, const int64_t* sample_ids, const int32_t* keep, int n, uint64_t seed,
                                int ph, int pw, const uint8_t* weights, int kh, int kw, int fill, int hole, float* target,
                                float* input, float* mask, void* stream) {
  clear_error();
  const char* what = "grr_patch_mask_batch";
  GRR_REQUIRE(arena && img_table && table && sample_ids && keep && weights && target && input && arena_elems > 0 &&
                  n_img > 0 && n > 0 && ph > 0 && pw > 0,
              GRR_ERR_INVALID_ARG, "%s: bad args", what);
  grr_status st = mask_params(what, C, kh, kw, fill, hole);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(grr_image_arena_supported(C, n_img, arena_elems), GRR_ERR_UNSUPPORTED,
              "%s: needs n_img <= arena elements < 2^62 (got %d images, %lld elements)", what, n_img,
              (long long)arena_elems);
  GRR_REQUIRE(grr_patch_mask_batch_supported(C, n_img, arena_elems, n, ph, pw), GRR_ERR_UNSUPPORTED,
              "%s: patch batch n C ph pw and the window (ph + 14)(pw + 14) must be below 2^31 (got %d x %d x %d x %d)", what,
              n, C, ph, pw);
  GRR_REQUIRE((uintptr_t)target % 4 == 0 && (uintptr_t)input % 4 == 0 && (uintptr_t)mask % 4 == 0 &&
                  (uintptr_t)table % 4 == 0 && (uintptr_t)keep % 4 == 0,
              GRR_ERR_INVALID_ARG, "%s: float32 and int32 operands must be 4-byte aligned", what);
  GRR_REQUIRE((uintptr_t)img_table % 8 == 0 && (uintptr_t)sample_ids % 8 == 0, GRR_ERR_INVALID_ARG,
              "%s: the image table and the sample ids must be 8-byte aligned", what);
  MaskArgs a{};
  a.src = arena;
  a.elems = arena_elems;
  a.img_table = img_table;
  a.table = table;
  a.ids = sample_ids;
  a.keep = keep;
  a.weights = weights;
  a.target = target;
  a.input = input;
  a.mask = mask;
  a.seed = seed;
  a.n_img = n_img;
  a.n = n;
  a.ph = ph;
  a.pw = pw;
  a.tiles_y = tiles(ph, kRows);
  a.tiles_x = tiles(pw, kCols);
  a.kh = kh;
  a.kw = kw;
  a.hole = hole;
  a.vec = pw % 4 == 0 && (uintptr_t)target % 16 == 0 && (uintptr_t)input % 16 == 0 && (uintptr_t)mask % 16 == 0;
  launch<false>(C, fill, dim3((uint32_t)((int64_t)n * a.tiles_y * a.tiles_x)), (hipStream_t)stream, a);   // <= n ph pw < 2^31
  return launch_status(what);
}

int grr_u8_mask_fill_supported(int C, int H, int W) {
  return grr_image_io_supported(C, H, W) && window_ok(H, W) ? 1 : 0;
}

grr_status grr_u8_mask_fill(const uint8_t* src, const uint8_t* mask_in, int H, int W, int C, int keep, uint64_t seed,
                            int64_t sample_id, const uint8_t* weights, int kh, int kw, int fill, int hole, uint8_t* dst,
                            uint8_t* mask_out, void* stream) {
  clear_error();
  const char* what = "grr_u8_mask_fill";
  GRR_REQUIRE(src && weights && dst && mask_out && H > 0 && W > 0, GRR_ERR_INVALID_ARG, "%s: bad args", what);
  grr_status st = mask_params(what, C, kh, kw, fill, hole);
  if (st != GRR_OK) return st;
  GRR_REQUIRE(keep >= 0 && keep <= kUnit, GRR_ERR_INVALID_ARG, "%s: keep lies in [0, 2^24] (got %d)", what, keep);
  GRR_REQUIRE(grr_u8_mask_fill_supported(C, H, W), GRR_ERR_UNSUPPORTED,
              "%s: needs C H W < 2^31 and (H + 14)(W + 14) < 2^31 (got %d x %d x %d)", what, H, W, C);
  MaskArgs a{};
  a.src = src;
  a.elems = (int64_t)H * W * C;
  a.weights = weights;
  a.mask_in = mask_in;
  a.dst = dst;
  a.mask_out = mask_out;
  a.seed = seed;
  a.n_img = 1;
  a.n = 1;
  a.ph = H;
  a.pw = W;
  a.tiles_y = tiles(H, kRows);
  a.tiles_x = tiles(W, kCols);
  a.kh = kh;
  a.kw = kw;
  a.hole = hole;
  a.H = H;
  a.W = W;
  a.keep_one = keep;
  a.sample_id = sample_id;
  launch<true>(C, fill, dim3((uint32_t)(a.tiles_y * a.tiles_x)), (hipStream_t)stream, a);      // < 2^21 tiles
  return launch_status(what);
}

}  // extern "C"
