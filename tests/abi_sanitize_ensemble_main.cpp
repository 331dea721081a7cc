// Host-side check of the argument validation of the four self-ensemble entry points of include/grr.h
// (grr_tile_gather_d8, grr_tiles_gather_d8, grr_tile_scatter_mean, grr_tiles_scatter_mean) under
// AddressSanitizer + UBSan (built by tests/test_abi_sanitize_ensemble.py with -fsanitize on the host side only;
// no GPU needed).  Each call has NULL operands, bad sizes or a bad mode list and must be refused with a
// grr_status error other than GRR_ERR_HIP (nothing reaches a launch) and a message that starts with the entry
// point's name, without touching memory: the mode lists are the only operands the host reads, and they are
// real arrays of exactly the length passed.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "grr.h"

static int g_fail = 0;

#define EXPECT_ERR(name, call)                                                                                   \
  do {                                                                                                           \
    grr_status st_ = (call);                                                                                     \
    const char* msg_ = grr_last_error();                                                                         \
    if (st_ == GRR_OK || st_ == GRR_ERR_HIP || !msg_ ||                                                          \
        std::strncmp(msg_, name ": ", std::strlen(name ": ")) != 0) {                                            \
      std::fprintf(stderr, "FAIL %s: status %d msg '%s'\n", #call, (int)st_, msg_ ? msg_ : "(null)");            \
      ++g_fail;                                                                                                  \
    }                                                                                                            \
  } while (0)

int main() {
  void* s = nullptr;
  float* nf = nullptr;
  const int32_t* ni = nullptr;
  const int64_t* nl = nullptr;
  // never dereferenced: validation refuses every call below before a launch
  float* f = reinterpret_cast<float*>(0x1000);
  const int32_t* t = reinterpret_cast<const int32_t*>(0x2000);
  const int64_t* it = reinterpret_cast<const int64_t*>(0x3000);
  void* img = reinterpret_cast<void*>(0x4000);
  const int32_t even[4] = {0, 1, 4, 5}, odd[4] = {2, 3, 6, 7}, all[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  const int32_t one[1] = {0}, high[1] = {8}, low[1] = {-1}, down[2] = {4, 1}, twice[2] = {1, 1}, mixed[2] = {0, 2};
  const int32_t nine[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};

  // grr_tile_gather_d8(img, img_f32, H, W, C, table, n, modes, n_modes, bh, bw, out, stream)
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(nullptr, 0, 16, 16, 3, ni, 1, ni, 1, 16, 16, nf, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(nullptr, 0, 16, 16, 3, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, ni, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, ni, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, odd, 4, 16, 16, nf, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 2, 16, 16, 3, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 0, 16, 3, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, -4, 3, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 0, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 5, t, 1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 0, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, -1, even, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, even, 4, 0, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, even, 4, 16, -16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, even, 0, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, even, -3, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, nine, 9, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, high, 1, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, low, 1, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, down, 2, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, twice, 2, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, mixed, 2, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 3, t, 1, all, 8, 16, 16, f, s));
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 4, t, 512, even, 4, 512, 512, f, s));   // 2^31
  EXPECT_ERR("grr_tile_gather_d8", grr_tile_gather_d8(img, 0, 16, 16, 1, t, 1 << 30, odd, 2, 16, 16, f, s));  // n M

  // grr_tiles_gather_d8(arena, arena_elems, img_f32, C, img_table, n_img, table, n, modes, n_modes, bh, bw, out, stream)
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(nullptr, 768, 0, 3, nl, 1, ni, 1, ni, 1, 16, 16, nf, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(nullptr, 768, 0, 3, it, 1, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, nl, 1, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, ni, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, ni, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, odd, 4, 16, 16, nf, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 0, 0, 3, it, 1, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, -1, 3, it, 1, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 5, it, 1, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 0, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 769, t, 1, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 0, odd, 4, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, odd, 0, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, high, 1, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, down, 2, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, mixed, 2, 16, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 3, it, 1, t, 1, odd, 4, 0, 16, f, s));
  EXPECT_ERR("grr_tiles_gather_d8", grr_tiles_gather_d8(img, 768, 0, 4, it, 1, t, 512, odd, 4, 512, 512, f, s));

  // grr_tile_scatter_mean(y0, y1, table, n, modes, n_modes, n_even, n_odd, th, tw, img, img_f32, H, W, C, stream)
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(nf, nf, ni, 1, ni, 1, 1, 0, 16, 16, nullptr, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(nf, f, t, 1, all, 8, 4, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, nf, t, 1, all, 8, 4, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, ni, 1, all, 8, 4, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, ni, 8, 4, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, nullptr, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 0, all, 8, 4, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 0, 0, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, nine, 9, 5, 4, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, high, 1, 1, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, low, 1, 1, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, down, 2, 2, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, twice, 2, 2, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, mixed, 2, 1, 2, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, mixed, 2, 2, 0, 16, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 0, 16, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, -1, img, 0, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 2, 16, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 0, 0, 16, 3, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 0, 16, 16, 5, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, f, t, 512, all, 8, 4, 4, 512, 512, img, 0, 16, 16, 4, s));
  EXPECT_ERR("grr_tile_scatter_mean", grr_tile_scatter_mean(f, nf, t, 1, one, 1, 1, 0, 16, 16, nullptr, 0, 16, 16, 3, s));

  // grr_tiles_scatter_mean(y0, y1, table, n, modes, n_modes, n_even, n_odd, th, tw, arena, arena_elems, img_f32, C,
  //                        img_table, n_img, stream)
  EXPECT_ERR("grr_tiles_scatter_mean",
             grr_tiles_scatter_mean(nf, nf, ni, 1, ni, 1, 1, 0, 16, 16, nullptr, 768, 0, 3, nl, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(nf, f, t, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, nf, t, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, ni, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, ni, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean",
             grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, nullptr, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 3, nl, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 0, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 0, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 16, img, 768, 0, 5, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 3, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 5, 3, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 0, 0, 0, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, high, 1, 1, 0, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, down, 2, 2, 0, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 0, all, 8, 4, 4, 16, 16, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean", grr_tiles_scatter_mean(f, f, t, 1, all, 8, 4, 4, 16, 0, img, 768, 0, 3, it, 1, s));
  EXPECT_ERR("grr_tiles_scatter_mean",
             grr_tiles_scatter_mean(f, f, t, 512, all, 8, 4, 4, 512, 512, img, 768, 0, 4, it, 1, s));

  std::printf("abi sanitize ensemble check: %d failure(s)\n", g_fail);
  return g_fail ? 1 : 0;
}
