// The Gaussian window of the SSIM kernels (metric_ops.hip: the index of uint8 images; ssim_loss_ops.hip: the
// training loss on float planes) and the tile they share: one set of taps and constants, so the metric and the loss
// are the same index.
#pragma once

namespace grr {

constexpr int kSsimThreads = 256;
constexpr int kSsimCols = 256;      // output columns of a tile (one per lane); kernels.SSIM_TILE[1], LUMA_SSIM_TILE[1]
constexpr int kSsimRows = 32;       // output rows of a tile; kernels.SSIM_TILE[0]
constexpr int kSsimTaps = 11;
constexpr double kSsimC1 = 6.5025, kSsimC2 = 58.5225;   // data range 255: (0.01 x 255)^2, (0.03 x 255)^2
constexpr double kSsimUnitC1 = 1e-4, kSsimUnitC2 = 9e-4;   // data range 1: 0.01^2, 0.03^2

// g[k] = exp(-(k - 5)^2 / (2 x 1.5^2)) / sum in float64, as literals so that every host builds the same taps
struct SsimTaps {
  double g[kSsimTaps];
};
constexpr SsimTaps kTaps = {{0x1.0d956b52a1d70p-10, 0x1.f1fe01ae5a5b8p-8, 0x1.26eb175d83f67p-5, 0x1.bff0fe8e98418p-4,
                             0x1.b43c3f52b19f2p-3, 0x1.106560aa892c0p-2, 0x1.b43c3f52b19f2p-3, 0x1.bff0fe8e98418p-4,
                             0x1.26eb175d83f67p-5, 0x1.f1fe01ae5a5b8p-8, 0x1.0d956b52a1d70p-10}};

}  // namespace grr
