// LocalNonLinearBlock forward on the split-operand MFMA kernels (lnb_ops.hip), C <= 128: what the C ABI
// entry points in feature_ops.hip call.
#pragma once

#include "grr_common.h"

namespace grr {

int64_t lnb_mfma_workspace_floats(int B, int C, int hid, int H, int W);
int64_t fused_pack_floats(int C, int hid);   // the fused block's chunk images + W2 row scales
// C <= 96 runs the whole block as one fused pass (lnb_fused16_kernel); keep_g: it also stores the gated
// activation g [B, hid, H, W] at the workspace's start (where the two-kernel path leaves it anyway)
bool lnb_fused(int C, int hid);
grr_status lnb_forward_mfma(const float* x, const float* ln_w, const float* w1, const float* wdw, const float* w2,
                            const float* skip, float* out, float* ws, int B, int C, int hid, int H, int W,
                            hipStream_t s, bool keep_g = false, int io = 0);
// the same block when x holds R stacked copies of the Ch-channel image xh (GEMM1 runs on xh)
grr_status lnb_forward_mfma_rep(const float* xh, int Ch, int R, const float* x, const float* ln_w, const float* w1,
                                const float* wdw, const float* w2, const float* skip, float* out, float* ws, int B,
                                int hid, int H, int W, hipStream_t s);

}  // namespace grr
