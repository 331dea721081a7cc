/*
 * grr.h — C ABI of the MI355X (gfx950) graph-regularizer restoration engine.
 *
 * One shared library (libgrr.so) built with hipcc for gfx950.  Every entry point
 * takes raw DEVICE pointers (fp32, contiguous NCHW unless stated), explicit sizes
 * and the caller's hipStream_t (passed as void*).  The caller allocates every
 * tensor it computes on; the only library state is the training reverse's per-stream reduction
 * scratch (grr_set_scratch_allocator).  It never synchronises, and is safe to call from several host
 * threads (re-entrant).  Each call returns a
 * grr_status; on failure grr_last_error() (thread-local) holds a message.
 *
 * Reference interfaces replaced (REF = exploration/GGTV_GGLR_v1.0/
 * deep_multiscale_GGLR_GGTV_v1x0.py; REF13 = exploration/model_multiscale_mixture_GLR/
 * lib/model_GLR_GTV_deep_v13_no_latent.py) are cited per function.
 *
 * Shapes: B batch, G graphs, F node features per graph, C = G*F channels,
 * H x W the resolution of the level a call runs at.  Edge order is the
 * reference's: 0 up (-1,0), 1 left (0,-1), 2 right (0,+1), 3 down (+1,0).
 */
#ifndef GRR_H
#define GRR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum grr_status {
  GRR_OK = 0,
  GRR_ERR_INVALID_ARG = 1, /* null pointer / non-positive size            */
  GRR_ERR_SHAPE = 2,       /* shape the reference itself cannot run (odd H at a pooled level, ...) */
  GRR_ERR_UNSUPPORTED = 3, /* outside this build's limits (e.g. F > GRR_MAX_NODE_FTS) */
  GRR_ERR_HIP = 4          /* HIP launch error                           */
} grr_status;

#define GRR_MAX_NODE_FTS 24

/* Library / error plumbing. */
int grr_version(void);
const char* grr_last_error(void);

/* Kernel-variant knob for tests and benchmarks (no reference counterpart): 0 = automatic
 * (row-wave graph operators for W <= 256 with the channel waves of a graph in lockstep,
 * column strips above), 1 = column-strip graph operators at every width, 2 = automatic
 * without the lockstep.  Process-wide; results agree to fp32 rounding either way. */
grr_status grr_set_kernel_variant(int variant);
/* Measurement knob (process-wide, like grr_set_kernel_variant): which phases a C <= 128 LocalNonLinearBlock
 * forward (grr_lnb_forward / grr_lnb_forward_rep) launches -- 1 weight packing, 2 head (LN + W1 +
 * depthwise + gate -> the workspace's g), 4 mix (W2 g + skip -> out).  7 (default) = all; a caller
 * times head and mix apart by running mask 3 then mask 4 on the same workspace. */
grr_status grr_lnb_set_phases(int mask);

/* Reduction scratch of the training reverse (no reference counterpart: the reference reverses through
 * autograd).  The reverse entry points (grr_bwd_*, grr_lnb_*_bwd, grr_dwconv3_bwd, grr_win_bwd_*, the
 * sub-API *_bwd) reduce per-graph scalars, taps and LN / depthwise weights in a fixed order through a
 * small device scratch of partial sums.  The library keeps one grow-only scratch buffer per (device,
 * stream) -- a second one only while calls nest on a stream -- and reuses it for later calls on that
 * stream (stream order makes the reuse safe).  The buffers come from the allocator registered here
 * (alloc(bytes, device, stream, ctx) returns a device pointer or NULL; free(ptr, device, stream, ctx)),
 * or from hipMalloc when none is registered (both NULL).  The Python package registers PyTorch's
 * caching allocator, so the scratch is PyTorch memory.  A call made while its stream is being captured
 * into a HIP graph takes its own scratch as a hipMallocAsync / hipFreeAsync pair on that stream (memory
 * nodes the graph owns): a replayed graph shares no scratch with eager calls on the stream or with
 * another graph, and grr_release_scratch never frees memory a graph uses.
 * grr_release_scratch frees every stream buffer (the caller synchronises the streams first);
 * grr_scratch_bytes reports the bytes held. */
typedef void* (*grr_scratch_alloc_fn)(uint64_t bytes, int device, void* stream, void* ctx);
typedef void (*grr_scratch_free_fn)(void* ptr, int device, void* stream, void* ctx);
grr_status grr_set_scratch_allocator(grr_scratch_alloc_fn alloc, grr_scratch_free_fn free_fn, void* ctx);
grr_status grr_release_scratch(void);
int64_t grr_scratch_bytes(void);

/* Measurement helper (not a reference interface): float4 streaming copy of n floats
 * (n % 4 == 0, 16-byte aligned), the HBM ceiling bench.py reports beside the step kernel. */
grr_status grr_stream_copy(const float* src, float* dst, int64_t n, void* stream);

/* a1 — integer neighbour table (bit-exact target).  out[e*H*W + p] = flat index
 * of clamp(p + delta_e): the pixel the reference's replicate-padded gather reads
 * for edge e (REF:128-144, GLRFast.get_neighbors_pixels).  out: int32 [4,H,W]. */
grr_status grr_neighbor_table(int32_t* out, int H, int W, void* stream);

/* a3+a4 — edge weights of one graph module (REF:146-175, GLRFast/GTVFast
 * .extract_edge_weights).  feat points at channel 0 of the module's [G*F] channel
 * slab inside a feature tensor whose batch stride is feat_bstride elements
 * (so the GTV/GLR halves of the 2C feature conv output need no copy, REF:714).
 * multiM [G,F].  Writes w [B,G,4,H,W] and, if deg != NULL, deg [B,G,H,W]. */
grr_status grr_edge_weights(const float* feat, int64_t feat_bstride, const float* multiM,
                            float* w, float* deg, int B, int G, int F, int H, int W, void* stream);

/* Symmetric pair weights of the linear graph-TV operator C^T C: for the edge
 * between p and its right / lower neighbour, c[.,0,p] = w_right(p)^2 + w_left(p+right)^2,
 * c[.,1,p] = w_down(p)^2 + w_up(p+down)^2 (0 where that neighbour is outside).
 * Algebraically identical to REF:452-516 (op_C then op_C_transpose with the
 * frame-dropped scatter).  w [B,G,4,H,W] -> c [B,G,2,H,W]. */
grr_status grr_gtv_pair_weights(const float* w, float* c, int B, int G, int H, int W, void* stream);

/* Both graph modules of one MixtureGTVGLR level in one call (REF:712-729): the GTV slab
 * (channels [gtv_off, gtv_off + G*F) of feat) -> raw weights wG [B,G,4,H,W] and pair
 * weights cG [B,G,2,H,W] (= grr_gtv_pair_weights(wG)); the GLR slab -> wL.  Same values as
 * grr_edge_weights (+ grr_gtv_pair_weights); a single row-wave launch where W <= 256. */
grr_status grr_edge_weights_block(const float* feat, int64_t feat_bstride, int gtv_off, const float* multiM_gtv,
                                  int glr_off, const float* multiM_glr, float* wG, float* cG, float* wL,
                                  int B, int G, int F, int H, int W, void* stream);

/* D — 2x2 mean pool, stride 2 (REF:613, :662-665).  x [B,C,H,W] -> xd [B,C,H/2,W/2]. */
grr_status grr_pool2(const float* x, float* xd, int B, int C, int H, int W, void* stream);

/* Per-module stencil parameters: the four [C] vectors stats_kernel_p01, _p02a,
 * _p02b, _p03 of one GLRFast/GTVFast module (REF:66-118, :177-215). */
typedef struct grr_stencil {
  const float* p01;
  const float* p02a;
  const float* p02b;
  const float* p03;
} grr_stencil;

/* Half-resolution system term (REF:661-675, inside apply_lightweight_transformer):
 *   t = exp(log_mu[g]) * S_L^T (I - W_L) S_L xd  +  exp(log_ro[g]) * G(xd)
 * G = graph-TV C^T C with pair weights cG.  Either term may be disabled by a NULL
 * weight pointer.  xd [B,C,h,w], wL [B,G,4,h,w], cG [B,G,2,h,w] -> t [B,C,h,w]. */
grr_status grr_system_half(const float* xd, const float* wL, const float* cG,
                           grr_stencil sL, grr_stencil sG,
                           const float* log_mu, const float* log_ro,
                           float* t, int B, int G, int F, int h, int w, void* stream);

/* Half-resolution GTV right-hand-side term: t = C^T phi(C xd), unscaled.
 * prox == 0: phi = identity, wG are pair weights [B,G,2,h,w] (rhs A, REF:739-747).
 * prox != 0: phi(t) = eps - (t - eps), eps = soft_threshold(t, exp(log_gamma[g])),
 *            wG are raw edge weights [B,G,4,h,w] (rhs B, REF:758-779; REF:684-704). */
grr_status grr_gtv_rhs_half(const float* xd, const float* wG, grr_stencil sG, int prox,
                            const float* log_gamma, float* t,
                            int B, int G, int F, int h, int w, void* stream);

/* Full-resolution GTV right-hand side (REF:744-749 rhs A, REF:776-781 rhs B):
 *   b = (y + exp(log_ro0[g]) * C^T phi(C x))  +  exp(log_ro1[g]) * U(t_half)
 * U = 2x2 nearest * 0.25 (conv_transpose2d of scaling_kernel01).  t_half may be NULL
 * (single-scale).  If xd_out != NULL also writes D(b).  prox/wG as grr_gtv_rhs_half. */
grr_status grr_gtv_rhs_full(const float* x, const float* y, const float* wG, grr_stencil sG,
                            int prox, const float* log_gamma, const float* log_ro0,
                            const float* t_half, const float* log_ro1,
                            float* b_out, float* xd_out,
                            int B, int G, int F, int H, int W, void* stream);

/* grr_gtv_rhs_full where x and/or y are given un-replicated, [B, F, H, W], standing for their
 * copies over the G graphs (MultiScaleGraphFilter's input, REF13:918-921; x_rep / y_rep != 0):
 * channel g*F + f reads plane f.  b_out / xd_out stay [B, G*F, ...]. */
grr_status grr_gtv_rhs_full_rep(const float* x, int x_rep, const float* y, int y_rep, const float* wG,
                                grr_stencil sG, int prox, const float* log_gamma, const float* log_ro0,
                                const float* t_half, const float* log_ro1, float* b_out, float* xd_out,
                                int B, int G, int F, int H, int W, void* stream);

/* One unrolled CG / heavy-ball stage (REF:751-753, :784-790, extension :797-807):
 *   A x   = ((x + exp(log_mu0) L0 x) + exp(log_ro0) G0 x) + U(t_half)
 *   r     = b - A x
 *   u     = r + beta[g] * u_prev      (u = r when u_prev == NULL or beta == NULL)
 *   x_out = x + alpha[g] * u
 * optional: u_out (u), xd_out (D x_out), and the LocalLowpassFilteringBlock skip
 * x_out <- skip[0] * y_skip + skip[1] * x_out when skip != NULL (REF:985-988).
 * alpha/beta point at row k of alphaCGD/betaCGD ([G]).  t_half from grr_system_half. */
grr_status grr_system_step(const float* x, const float* b, const float* u_prev, const float* t_half,
                           const float* wL, const float* cG, grr_stencil sL, grr_stencil sG,
                           const float* log_mu0, const float* log_ro0,
                           const float* alpha, const float* beta,
                           const float* skip, const float* y_skip,
                           float* x_out, float* u_out, float* xd_out,
                           int B, int G, int F, int H, int W, void* stream);

/* Two consecutive stages k, k+1 of the loop above (REF:784-790 twice) in one pass
 * (temporal blocking; t_k, x_{k+1}, u_{k+1} and t_{k+1} never leave the chip):
 *   half level A:  t_k = exp(log_mu1) L1 xd + exp(log_ro1) G1 xd, xd = D x (the previous pass's
 *                  xd_out; what grr_system_half computes)
 *   stage A (k):   x_{k+1}, u_{k+1} from x, u_prev (beta_a), t_k
 *   half level B:  t_{k+1} = exp(log_mu1) L1 (D x_{k+1}) + exp(log_ro1) G1 (D x_{k+1})
 *   stage B (k+1): x_out = x_{k+2}, u_out = u_{k+2} (beta_b with u_{k+1}), xd_out = D x_{k+2},
 *                  skip applied to x_out as in grr_system_step.
 * Same values as grr_system_half -> grr_system_step(k) -> grr_system_half -> grr_system_step(k+1) up to fp32
 * rounding order.  GLR + GTV pair at both levels; W = 256, or W % 8 == 0 (column strips of 256 lanes
 * owning 224 columns with a 16-column halo), even H; F > 3 runs as groups of <= 3
 * channels (each group reads its graph's weight rows once); outputs must
 * not alias inputs (u_out != u_prev).  Replaces two iterations of the loop body REF:784-790. */
grr_status grr_system_step2(const float* x, const float* b, const float* u_prev, const float* xd,
                            const float* wL0, const float* cG0, grr_stencil sL0, grr_stencil sG0,
                            const float* log_mu0, const float* log_ro0, const float* wL1, const float* cG1,
                            grr_stencil sL1, grr_stencil sG1, const float* log_mu1, const float* log_ro1,
                            const float* alpha_a, const float* beta_a, const float* alpha_b, const float* beta_b,
                            const float* skip, const float* y_skip, float* x_out, float* u_out, float* xd_out,
                            int B, int G, int F, int H, int W, void* stream);
/* Stage 0, right-hand side B and stage 1 in one pass (the first pair of the loop: REF:751-753, :757-781,
 * :784-790 at k = 1; x_1 never leaves the chip):
 *   half level 0:  t_0 = exp(log_mu1) L1 xd_a + exp(log_ro1) G1 xd_a, xd_a = D b_A (grr_gtv_rhs_full's
 *                  xd_out of right-hand side A; what grr_system_half computes)
 *   stage 0:       x_1 = b_A + alpha0 (b_A - A b_A)                       (grr_system_step, x = b = b_A)
 *   rhs B:         b_out = y + exp(log_ro0) C0^T phi(C0 S x_1) + exp(log_ro1) U(C1^T phi(C1 S D x_1)), the
 *                  soft threshold at exp(log_gamma0) / exp(log_gamma1), raw weights wG0 [B,G,4,H,W] /
 *                  wG1 [B,G,4,H/2,W/2]                     (grr_gtv_rhs_half + grr_gtv_rhs_full, prox)
 *   stage 1:       x_out = x_2, u_out = u_2 = b_B - A x_1, xd_out = D x_2  (grr_system_step, no heavy-ball)
 * y: [B,C,H,W], or the [B,F,H,W] image it replicates over the graphs (y_rep != 0).  Same values as
 * grr_system_half -> grr_system_step -> grr_gtv_rhs_half -> grr_gtv_rhs_full -> grr_system_half ->
 * grr_system_step up to fp32 rounding order.  W = 256, even H; F > 3 as groups of <= 3 channels; 16-byte
 * aligned operands; outputs must not alias inputs. */
grr_status grr_system_first_pair(const float* b_a, const float* xd_a, const float* y, int y_rep, const float* wL0,
                                 const float* cG0, const float* wG0, grr_stencil sL0, grr_stencil sG0,
                                 const float* log_mu0, const float* log_ro0, const float* log_gamma0,
                                 const float* wL1, const float* cG1, const float* wG1, grr_stencil sL1,
                                 grr_stencil sG1, const float* log_mu1, const float* log_ro1,
                                 const float* log_gamma1, const float* alpha0, const float* alpha1, float* b_out,
                                 float* x_out, float* u_out, float* xd_out, int B, int G, int F, int H, int W,
                                 void* stream);
/* grr_system_step2 for training: also writes the middle iterate x_{k+1} (x_mid) and its direction
 * u_{k+1} (u_mid) -- the reverse sweep's saved iterates -- besides x_{k+2}, u_{k+2} (u_out required) and
 * D x_{k+2}; no skip.  xd_mid (may be NULL): D x_{k+1}, the pooled middle iterate the kernel's half level
 * already forms, for the reverse sweep's half-level terms (no pool2 of x_{k+1} there).  Same shape
 * limits. */
grr_status grr_system_step2_train(const float* x, const float* b, const float* u_prev, const float* xd,
                                  const float* wL0, const float* cG0, grr_stencil sL0, grr_stencil sG0,
                                  const float* log_mu0, const float* log_ro0, const float* wL1, const float* cG1,
                                  grr_stencil sL1, grr_stencil sG1, const float* log_mu1, const float* log_ro1,
                                  const float* alpha_a, const float* beta_a, const float* alpha_b,
                                  const float* beta_b, float* x_out, float* u_out, float* xd_out, float* x_mid,
                                  float* u_mid, float* xd_mid, int B, int G, int F, int H, int W, void* stream);

/* One unrolled stage of the GLR-only v10 block (exploration/model_multiscale_mixture_GLR/lib/
 * model_GLR_GTV_deep_v10.py:241-335, MixtureGLR): single scale, A x = x + mu[g] L x with mu
 * stored LINEARLY (not as a log, :283-286, :296-305):
 *   r = b - A x;  u = r + beta[g] u_prev (u = r when u_prev == NULL);  x_out = x + alpha[g] u.
 * u_out may be NULL.  With x = b = y and u_prev = NULL this is stage 0 (:316-318). */
grr_status grr_glr_stage(const float* x, const float* b, const float* u_prev, const float* wL, grr_stencil sL,
                         const float* mu, const float* alpha, const float* beta, float* x_out, float* u_out,
                         int B, int G, int F, int H, int W, void* stream);

/* ---- GLRFast / GTVFast sub-API (module methods outside the fused solver) -------------
 * Standalone versions of the reference module methods, for callers of the module API (the
 * solver itself fuses the same arithmetic into the operator kernels above).  Layouts as above;
 * edge signals are [B,G,F,4,H,W] (REF:452-467). */

/* get_neighbors_pixels (REF:128-144): out[b,c,e,p] = x[b,c,clamp(p + delta_e)], out [B,C,4,H,W]. */
grr_status grr_neighbor_gather(const float* x, float* out, int B, int C, int H, int W, void* stream);
/* normalize_and_transform_features (REF:146-157): out[b, g*F + f] = f / max(|f|_2 over F, 1e-12) * multiM[g,f]. */
grr_status grr_normalize_features(const float* f, const float* multiM, float* out, int B, int G, int F, int H, int W,
                                  void* stream);
/* stats_conv (transpose == 0, replicate frame, REF:177-195) / stats_conv_transpose (transpose != 0,
 * conv_transpose2d padding 1 = zero frame, REF:197-215) with the module's stencil. */
grr_status grr_stats_conv(const float* x, grr_stencil s, int transpose, float* out, int B, int G, int F, int H, int W,
                          void* stream);
/* GLRFast.op_L_norm (REF:218-228): out = x - sum_e w_e x(clamp(p + delta_e)); x [B,G,F,H,W], w [B,G,4,H,W]. */
grr_status grr_glr_op_l_norm(const float* x, const float* w, float* out, int B, int G, int F, int H, int W,
                             void* stream);
/* GTVFast.op_C (REF:452-467): edges[b,g,f,e,p] = w_e(p) (S x)(p) - w_e(p) (S x)(clamp(p + delta_e)). */
grr_status grr_gtv_op_c(const float* x, const float* w, grr_stencil s, float* edges, int B, int G, int F, int H, int W,
                        void* stream);
/* GTVFast.op_C_transpose (REF:469-516): z_e = edges_e w_e; o(q) = sum_e z_e(q) - sum_e z_e(q - delta_e) for
 * q - delta_e inside the image (scatters into the pad frame are dropped); out = S^T o.  work [B,G,F,H,W]
 * is caller scratch (o). */
grr_status grr_gtv_op_c_transpose(const float* edges, const float* w, grr_stencil s, float* work, float* out, int B,
                                  int G, int F, int H, int W, void* stream);

/* Reverses of the sub-API methods above (the reference differentiates them with autograd over its
 * ATen ops, REF:128-228, :452-516).  Gradient outputs are overwritten except gM / gtaps, which
 * accumulate (caller zeroes); gtaps is [G*F, 5] in tap order (centre, up, left, right, down) of the
 * stencil p01 k01 + p02a k02a + p02b k02b + p03 k03.  B*C (B*G for per-graph kernels) < 65536. */
/* get_neighbors_pixels reverse: gx [B,C,H,W] from g [B,C,4,H,W] (adjoint of the clamped gather). */
grr_status grr_neighbor_gather_bwd(const float* g, float* gx, int B, int C, int H, int W, void* stream);
/* normalize_and_transform_features reverse: gf [B,G,F,H,W], gM [G,F] += ; F <= 16. */
grr_status grr_normalize_features_bwd(const float* f, const float* multiM, const float* gout, float* gf, float* gM,
                                      int B, int G, int F, int H, int W, void* stream);
/* stats_conv / stats_conv_transpose reverse: gx = S* g (S^T* g), gtaps += d<g, S x>/d taps (gtaps may be NULL). */
grr_status grr_stats_conv_bwd(const float* x, grr_stencil s, int transpose, const float* g, float* gx, float* gtaps,
                              int B, int G, int F, int H, int W, void* stream);
/* GLRFast.op_L_norm reverse: gx [B,G,F,H,W], gw [B,G,4,H,W]. */
grr_status grr_glr_op_l_norm_bwd(const float* x, const float* w, const float* g, float* gx, float* gw, int B, int G,
                                 int F, int H, int W, void* stream);
/* GTVFast.op_C reverse from gE [B,G,F,4,H,W]: gx, gw, gtaps; work [B,G,F,H,W] caller scratch. */
grr_status grr_gtv_op_c_bwd(const float* x, const float* w, grr_stencil s, const float* gE, float* work, float* gx,
                            float* gw, float* gtaps, int B, int G, int F, int H, int W, void* stream);
/* GTVFast.op_C_transpose reverse: gE [B,G,F,4,H,W], gw, gtaps; z = the forward's work buffer (the
 * pre-S^T value o), work2 [B,G,F,H,W] caller scratch. */
grr_status grr_gtv_op_c_transpose_bwd(const float* edges, const float* w, grr_stencil s, const float* z,
                                      const float* g, float* work2, float* gE, float* gw, float* gtaps, int B, int G,
                                      int F, int H, int W, void* stream);

/* ---- feature CNN (MFMA fp32) ------------------------------------------------ */

/* 1x1 convolution, no bias (nn.Conv2d(k=1, groups=1, bias=False); REF:556-566, REF13:623-632):
 * out[b,m,p] = sum_k wt[m,k] * x[b,k,p].  x [B,K,P], wt [M,K], out [B,M,P] (P = H*W). */
grr_status grr_conv1x1(const float* x, const float* wt, float* out, int B, int K, int M, int64_t P,
                       void* stream);

/* The same 1x1 convolution on bf16 MFMA with an exact 3-term split of both fp32 operands
 * (six products, fp32-accurate; see DESIGN.md "x3 GEMM").  K <= 4096 (K > 128: the K-streaming
 * kernel).  workspace: device
 * memory of grr_conv1x1_workspace_bytes(K, M) bytes, 256-B aligned (the split weights). */
int64_t grr_conv1x1_workspace_bytes(int K, int M);
grr_status grr_conv1x1_ws(const float* x, const float* wt, float* out, void* workspace, int B, int K, int M,
                          int64_t P, void* stream);

/* 2x2 stride-2 convolution, no bias (REF:593-602): x [B,K,H,W], wt [M,K,2,2] -> out [B,M,H/2,W/2]. */
grr_status grr_conv2x2s2(const float* x, const float* wt, float* out, int B, int K, int M, int H, int W,
                         void* stream);

/* ---- v1.0 encoder / decoder convolutions (codec_ops.hip) ---------------------- */

/* ReginalPixelEmbeding (REF:991-1009): 3x3 convolution, replicate padding, no bias.  x [B,Cin,H,W],
 * wt [M,Cin,3,3] -> out [B,M,H,W]; 1 <= Cin <= 4, 1 <= M <= 128 (grr_conv3x3_embed_supported), any H, W >= 1.
 * Every output is one fmaf chain over (c, ky, kx) in ascending order: bitwise independent of tiling,
 * batch and position. */
int grr_conv3x3_embed_supported(int Cin, int M);
grr_status grr_conv3x3_embed(const float* x, const float* wt, float* out, int B, int Cin, int M, int H, int W,
                             void* stream);
/* Its weight gradient gw[m,c,ky,kx] = sum_b sum_p g[b,m,p] x[b,c,clamp(p + (ky-1, kx-1))]: g [B,M,H,W] (16-B
 * aligned), x [B,Cin,H,W] -> gw [M,Cin,3,3].  The clamped taps are gathered into [B, 9 Cin, P] in the
 * workspace and reduced on grr_wgrad (fixed order, no atomics).  workspace:
 * grr_conv3x3_embed_bwd_w_workspace_bytes(B, Cin, M, H, W) bytes, 256-B aligned. */
int64_t grr_conv3x3_embed_bwd_w_workspace_bytes(int B, int Cin, int M, int H, int W);
grr_status grr_conv3x3_embed_bwd_w(const float* g, const float* x, float* gw, void* workspace, int B, int Cin, int M,
                                   int H, int W, void* stream);
/* Its data gradient (the adjoint of the clamped gather, as a gather): g [B,M,H,W], wt [M,Cin,3,3] ->
 * gx [B,Cin,H,W]. */
grr_status grr_conv3x3_embed_bwd_x(const float* g, const float* wt, float* gx, int B, int Cin, int M, int H, int W,
                                   void* stream);

/* Upsampling (REF:1019-1025): nn.ConvTranspose2d(K, M, 2, stride=2, bias=False).  x [B,K,H,W], wt [K,M,2,2] ->
 * out [B,M,2H,2W] (8-B aligned): the 1x1 GEMM with the 4M rows (m, di, dj) on the split-bf16 kernels of
 * grr_conv1x1_ws (K <= 4096), then a 2x2 interleave.  workspace: grr_convt2x2s2_workspace_bytes(B, K, M, H, W)
 * bytes, 256-B aligned (the packed weights and the [B, 4M, H, W] GEMM output). */
int64_t grr_convt2x2s2_workspace_bytes(int B, int K, int M, int H, int W);
grr_status grr_convt2x2s2(const float* x, const float* wt, float* out, void* workspace, int B, int K, int M, int H,
                          int W, void* stream);

/* The decoder's combine (REF:1150-1160): nn.Conv2d(Ka + Kb, M, 1, bias=False) on cat([xa, xb], 1) without
 * materialising the concatenation.  xa [B,Ka,P], xb [B,Kb,P], wt [M,Ka+Kb] -> out [B,M,P].  The GEMM's
 * B-operand loader takes each 16-row k-step from xa or xb, so Ka % 16 == 0 is required
 * (grr_conv1x1_cat2_supported; also Ka + Kb <= 4096 and the 32-bit lane offsets (Ka + Kb + 16) P < 2^30,
 * (M + 128) P < 2^30); the summation order is grr_conv1x1_ws's on the concatenated tensor and the result is
 * bitwise equal to it.  workspace: grr_conv1x1_cat2_workspace_bytes(Ka, Kb, M) bytes, 256-B aligned. */
int grr_conv1x1_cat2_supported(int Ka, int Kb, int M, int64_t P);
int64_t grr_conv1x1_cat2_workspace_bytes(int Ka, int Kb, int M);
grr_status grr_conv1x1_cat2(const float* xa, const float* xb, const float* wt, float* out, void* workspace, int B,
                            int Ka, int Kb, int M, int64_t P, void* stream);

/* FeedForward block of the window models' feature CNN (FFBlock, REF7:13-67, nn.Conv2d bias=False):
 * out = skip[0] x + skip[1] W_out (gelu(d1) * d2), [d1; d2] = dwconv3x3_zero(W_in (ln_w * x / sigma)),
 * sigma = sqrt(var_c x (unbiased) + 1e-5).  x, out [B,C,H,W]; ln_w [C]; w_in [2 hid, C]; w_dw [2 hid, 9];
 * w_out [C, hid]; skip [2] (device).  Split-bf16 MFMA GEMMs (fp32-accurate), exact erf gelu.
 * workspace: grr_ffn_workspace_bytes(B, C, hid, H, W) bytes, 256-B aligned. */
int64_t grr_ffn_workspace_bytes(int B, int C, int hid, int H, int W);
grr_status grr_ffn_forward(const float* x, const float* ln_w, const float* w_in, const float* w_dw, const float* w_out,
                           const float* skip, float* out, void* workspace, int B, int C, int hid, int H, int W,
                           void* stream);

/* Weight gradient of a 1x1 / 2x2-s2 convolution or an LNB GEMM (the reverse of REF:556-612,
 * REF13:564-575 under autograd): out[m,k] = sum_b sum_p a[b,m,p] * bop[b,k,p], a [B,M,P], bop [B,K,P],
 * out [M,K]; fp32 MFMA, partial tiles per pixel chunk added in a fixed order (deterministic, no
 * atomics).  Replaces the library GEMM torch.matmul(g, x^T).sum(0) of the reference's autograd.
 * workspace: grr_wgrad_workspace_bytes(B, M, K, P) bytes of device memory; a, bop 16-B aligned. */
int64_t grr_wgrad_workspace_bytes(int B, int M, int K, int64_t P);
/* grr_wgrad's wave tiles: 1 (default) the plan picks 128 x 96, 192 x 64 or 64 x 96 per output shape
 * (least padded MFMA work), 0 the 128 x 96 tile only.  Results are identical up to the fp32 summation
 * order of the pixel chunks.  A/B and test knob. */
grr_status grr_wgrad_set_tiles(int enable);
grr_status grr_wgrad(const float* a, const float* bop, float* out, void* workspace, int B, int M, int K, int64_t P,
                     void* stream);

/* LocalNonLinearBlock forward, nsubnets = 1 (REF:911-964; REF13:564-575):
 *   n   = gamma_c * x / sqrt(var_c(x) + 1e-5)          (CustomLayerNorm, unbiased var over C)
 *   h   = dwconv3x3_replicate(W1 n)                     (C -> 2*hid -> 2*hid)
 *   g   = sigmoid(h_mask) * h_mask * h_value            (hid)
 *   out = skip[0] * x + skip[1] * (W2 g)               (hid -> C)
 * ln_w [C] (norm.weighted_transform), w1 [2hid,C], wdw [2hid,9], w2 [C,hid], skip [2].
 * workspace: grr_lnb_workspace_bytes(B,C,hid,H,W) bytes of device memory. out may not alias x. */
int64_t grr_lnb_workspace_bytes(int B, int C, int hid, int H, int W);
grr_status grr_lnb_forward(const float* x, const float* ln_w, const float* w1, const float* wdw,
                           const float* w2, const float* skip, float* out, void* workspace,
                           int B, int C, int hid, int H, int W, void* stream);

/* The feature CNN's last 1x1 conv and the edge weights of both graph modules of a level in one pass
 * (REF:146-175, :556-612 -- REF13:887-926's patchs_features_extraction[-1] followed by extract_edge_weights
 * for the GTV and the GLR module): feat = wf x (wf [2 G F, C]: rows 0 .. G F - 1 the GTV features, then
 * the GLR features), then grr_edge_weights_block's outputs (wG, cG, wL) from feat -- without feat in memory.
 * x is [B, C, H, W], or the channel-blocked layout of grr_lnb_forward_c8 when x_blocked.  F = 3, G <= 32,
 * C = G F (grr_feature_edges_supported).  The conv runs as fp16 two-term splits of both operands (three
 * products), fp32-class like the fused LocalNonLinearBlock's GEMMs, so the weights agree with the two-pass
 * path to fp32-class rounding, not bitwise.  workspace: grr_feature_edges_workspace_bytes(G), 256-B aligned. */
int grr_feature_edges_supported(int C, int G, int F, int H, int W);
int64_t grr_feature_edges_workspace_bytes(int G);
grr_status grr_feature_edges(const float* x, int x_blocked, const float* wf, const float* multiM_gtv,
                             const float* multiM_glr, float* wG, float* cG, float* wL, void* workspace, int B,
                             int C, int G, int F, int H, int W, void* stream);

/* grr_lnb_forward with either side in the channel-blocked layout [B, ceil(C / 8), H, W, 8] (channel
 * 8 k + j of pixel p at ((b ceil(C / 8) + k) H W + p) 8 + j; pad channels 0): layout bit 0 -- x (read for
 * LN / W1 and the skip term) blocked, bit 1 -- out blocked.  Needs grr_lnb_fused(C, hid); x and out 16-B
 * aligned; workspace as grr_lnb_forward's.  Results equal grr_lnb_forward's bitwise (same arithmetic; the
 * layout only changes the kernel's memory instructions: 16- and 32-byte accesses per lane instead of
 * dwords).  A chain of blocks passes the blocked tensor from one to the next (no reference counterpart:
 * an internal layout of the feature CNN between its LocalNonLinearBlocks, REF13:541-575). */
grr_status grr_lnb_forward_c8(const float* x, const float* ln_w, const float* w1, const float* wdw,
                              const float* w2, const float* skip, float* out, void* workspace, int B, int C,
                              int hid, int H, int W, int layout, void* stream);
/* [B, C, H, W] -> blocked (to_blocked = 1, pads written 0) or back (0). */
grr_status grr_c8_convert(const float* src, float* dst, int B, int C, int H, int W, int to_blocked, void* stream);

/* grr_lnb_forward that also leaves the gated activation g = sigmoid(m) m v [B, hid, H, W] (fp32) at the
 * start of the workspace, for the training reverse's W2 weight gradient (the eager LocalNonLinearBlock
 * forward keeps it instead of recomputing the depthwise + gate).  C <= 128. */
grr_status grr_lnb_forward_keep(const float* x, const float* ln_w, const float* w1, const float* wdw,
                                const float* w2, const float* skip, float* out, void* workspace, int B, int C,
                                int hid, int H, int W, void* stream);
/* 1 when grr_lnb_forward runs the block as one fused pass for these sizes (C <= 96: LN, W1, depthwise,
 * gate and W2 in one kernel, the gated activation kept on chip).  Phase mask 2 of grr_lnb_set_phases then
 * launches the whole block and mask 4 nothing. */
int grr_lnb_fused(int C, int hid);
/* Workspace bytes grr_lnb_forward needs when grr_lnb_fused(C, hid) holds (the fused pass's chunk images
 * only: no gated tensor, no batch or image size), else 0.  grr_lnb_forward_keep still needs
 * grr_lnb_workspace_bytes (g at the workspace's start). */
int64_t grr_lnb_fused_workspace_bytes(int C, int hid);
/* Measurement knob (process-wide): 0 runs C <= 96 blocks on the two-kernel head + mix path instead of
 * the fused pass (same results to fp32 rounding); 1 (default) fused. */
grr_status grr_lnb_set_fused(int enable);
/* grr_lnb_forward for an input x [B, R*Cs, H, W] that is R stacked copies of src [B, Cs, H, W]
 * (the first feature block of MultiScaleGraphFilter, whose input replicates RGB over the graphs,
 * REF13:918-921): LN statistics and W1 are evaluated on src with W1 diag(ln_w) folded over the
 * copies (GEMM1 depth Cs instead of R*Cs); the skip reads x, or src at channel c mod Cs when
 * x == NULL (then no replicated copy needs to exist).  R*Cs <= 128.  workspace:
 * grr_lnb_workspace_bytes(B, R*Cs, hid, H, W). */
grr_status grr_lnb_forward_rep(const float* src, int Cs, int R, const float* x, const float* ln_w, const float* w1,
                               const float* wdw, const float* w2, const float* skip, float* out, void* workspace,
                               int B, int hid, int H, int W, void* stream);
/* 1 when grr_lnb_forward_rep runs the block as one fused pass for these sizes (R > 1, Cs <= 3: the
 * depthwise folded into an im2col GEMM1, gate and W2 in registers, no gated tensor in memory), else 0.
 * Phase mask 2 of grr_lnb_set_phases then launches the whole block and mask 4 nothing. */
int grr_lnb_rep_fused(int Cs, int R, int C, int hid);

/* Channel replication of MultiScaleGraphFilter.forward (REF13:918-921):
 * img [B,Cin,H,W] -> out [B,G*Cin,H,W], out[b, g*Cin + c] = img[b, c]. */
grr_status grr_repeat_graphs(const float* img, float* out, int B, int Cin, int G, int64_t P, void* stream);

/* ---- reverse pass (training, config C4) -------------------------------------
 * Adjoint building blocks of the solver; the host composes them into the reverse of
 * every operator application of MixtureGTVGLR.forward (REF:707-811), the autograd
 * graph the reference gets from PyTorch.  Layouts as above; taps [C,5] are the 3x3
 * cross stencil of one module in the order centre, up, left, right, down (built from
 * stats_kernel_p01/p02a/p02b/p03, REF:178-183).  scale: per-graph [G] multiplier or
 * NULL (=1); "accumulate"/"+=" outputs are read-modify-write, all others overwritten.
 * Reductions (gtaps, gdot, ggamma, gmultiM) are float atomics: run-to-run order may vary. */

/* mode 0: S x (replicate, REF:177-195); 1: S^T x (conv_transpose zero frame, REF:197-215);
 * 2: adjoint of mode 1; 3: adjoint of mode 0.  out = [out +] scale[g] * mode(x). */
grr_status grr_bwd_stencil(const float* x, const float* taps, int mode, const float* scale, int accumulate,
                           float* out, int B, int G, int F, int H, int W, void* stream);
/* x-gradient pass of two operator terms of one level in one sweep: out += scale1[g] P1*(v1) + scale2[g] P2*(v2),
 * P* = the adjoint of the replicate stencil (grr_bwd_stencil mode 3) with each term's taps [C,5].
 * W % 4 == 0, 16-byte aligned planes. */
grr_status grr_bwd_padj2(const float* v1, const float* taps1, const float* scale1, const float* v2, const float* taps2,
                         const float* scale2, float* out, int B, int G, int F, int H, int W, void* stream);
/* gtaps[c,t] += scale[g] * sum u(q) d(mode(z))(q)/dk_t, mode 0 (S) or 1 (S^T). */
grr_status grr_bwd_tapgrad(const float* u, const float* z, int mode, const float* scale, float* gtaps,
                           int B, int G, int F, int H, int W, void* stream);
/* GLR (I - W) reverse (REF:218-237): s = S x, a = adjoint-S^T(g).
 * z_out = (I-W) s, ap_out = (I-W)^T a, gw += scale * d<a,(I-W)s>/dw, gdot[g] += coef * <a, z>. */
grr_status grr_bwd_glr(const float* s, const float* a, const float* w, const float* scale, float coef,
                       float* z_out, float* ap_out, float* gw, float* gdot,
                       int B, int G, int F, int H, int W, void* stream);
/* Pair-Laplacian (linear C^T C, REF:452-523) reverse with pair weights c [B,G,2,H,W]:
 * z_out = K s, ap_out = K a, gc += scale * d<a,Ks>/dc, gdot[g] += coef * <a, z>. */
grr_status grr_bwd_pair(const float* s, const float* a, const float* c, const float* scale, float coef,
                        float* z_out, float* ap_out, float* gc, float* gdot,
                        int B, int G, int F, int H, int W, void* stream);
/* Prox rhs reverse, o = C^T-part(phi(C s)) with phi(t) = 2 soft(t, exp(log_gamma)) - t
 * (REF:684-704, :757-781): o_out, gs_out = d<a,o>/ds, gw += scale * d<a,o>/dw (raw weights),
 * ggamma[g] += scale * d<a,o>/dgamma, gdot[g] += coef * <a, o>. */
grr_status grr_bwd_prox(const float* s, const float* a, const float* w, const float* log_gamma,
                        const float* scale, float coef, float* o_out, float* gs_out, float* gw,
                        float* ggamma, float* gdot, int B, int G, int F, int H, int W, void* stream);
/* Widest image at which grr_bwd_term_acc_supported offers the LDS-ring row kernel with the x-gradient pass
 * inside (default 128; wider levels fold that pass into grr_bwd_cg_glue).  A/B and test knob. */
grr_status grr_bwd_set_term_acc_max_w(int w);
/* Kernel knob for tests and benchmarks (no reference counterpart): 2 (default) runs grr_bwd_term_fused
 * (and _acc) as the LDS-ring row kernel where the shape allows (W % 4 == 0, F <= 7 at 4-column lanes /
 * 12 below, 16-byte aligned planes), else as the register-prefetch row kernel; 1 always the register
 * kernel; 0 the per-pixel kernels.  grr_bwd_edge_weights: row kernel for 1 and 2.
 * Process-wide; results agree to fp32 rounding. */
grr_status grr_bwd_set_term_rows(int enable);
/* Kernel knob for tests and benchmarks (no reference counterpart): 1 (default; env GRR_TERM_TAIL) runs the
 * last column strip of a wide ring-kernel term reverse (W > 64 V, the last strip owning <= 56 columns) as
 * a second, one-column-lane launch; 0 keeps every strip at V columns per lane.  Process-wide; results
 * agree to fp32 rounding (the per-strip wave sums differ). */
grr_status grr_bwd_set_term_tail(int enable);

/* The three reverses above in one pass each, from x and g directly (s = S x and a = adjoint-S^T g
 * recomputed on the fly) with both tap gradients fused: mode 0 GLR (w raw), 1 pair Laplacian
 * (w = pair weights), 2 prox (w raw, log_gamma).  Writes v_out = (I-W)^T a, K a or d<a,o>/ds
 * (x-gradient = adjoint-S of v); gw, ggamma, gdot, gtaps (+=) as the multi-pass path, whose
 * results it reproduces.  GRR_ERR_UNSUPPORTED for F outside {1,2,3,4}. */
grr_status grr_bwd_term_fused(int mode, const float* x, const float* g, const float* taps, const float* w,
                              const float* log_gamma, const float* scale, float coef, float* v_out, float* gw,
                              float* ggamma, float* gdot, float* gtaps, int B, int G, int F, int H, int W,
                              void* stream);
/* grr_bwd_term_fused and the x-gradient pass that consumes its v (grr_bwd_stencil mode 3 with the
 * same taps and scale, accumulating) in one row-streaming pass: gx += scale[g] * adjoint-S(v), v never
 * written; gw, ggamma, gdot, gtaps as grr_bwd_term_fused.  Two calls on one gx (GLR, then pair) equal
 * grr_bwd_padj2 of the two v's.  GRR_ERR_UNSUPPORTED where grr_bwd_term_acc_supported says 0 (the
 * caller keeps the two-pass path) or a plane is not 4V-byte aligned.  The reference computes these
 * gradients by autograd through REF:218-237, :452-523, :684-704. */
int grr_bwd_term_acc_supported(int mode, int F, int H, int W);
grr_status grr_bwd_term_fused_acc(int mode, const float* x, const float* g, const float* taps, const float* w,
                                  const float* log_gamma, const float* scale, float coef, float* gx, float* gw,
                                  float* ggamma, float* gdot, float* gtaps, int B, int G, int F, int H, int W,
                                  void* stream);
/* Reverse of grr_gtv_pair_weights: gw [B,G,4,H,W] += d<gc, c(w)>/dw. */
grr_status grr_bwd_pair_weights(const float* w, const float* gc, float* gw, int B, int G, int H, int W,
                                void* stream);
/* Reverse of grr_edge_weights (REF:146-175): gfeat (slab, overwritten) and gmultiM [G,F] (+=). */
grr_status grr_bwd_edge_weights(const float* feat, int64_t feat_bstride, const float* multiM, const float* w,
                                const float* gw, float* gfeat, int64_t gfeat_bstride, float* gmultiM,
                                int B, int G, int F, int H, int W, void* stream);
/* gdot[g] += coef * sum_{b,f,p} u v  (per-graph inner product; alpha/beta/gamma gradients). */
grr_status grr_bwd_graph_dot(const float* u, const float* v, float coef, float* gdot,
                             int B, int G, int F, int H, int W, void* stream);
/* out = [out +] sa[g] x + sb[g] y  (sa/sb NULL = 1, y NULL = no second term). */
/* One reverse step of the CG / heavy-ball recurrence glue (autograd of REF:784-807 without the
 * operator term): galpha[g] += <gx, u>; gu = alpha[g] gx + beta_next[g] gu_next (gu_next may be
 * NULL); gbeta[g] += <gu, u_prev> (u_prev may be NULL); gbb += gu (gbb may be NULL);
 * gx_out = gx - gu (may alias gx).  Signals [B, G*F, H, W]; alpha, beta_next, galpha, gbeta [G].
 * Two passes of the previous reverse stage may be folded in, gx taken as
 * ((gx + scale1[g] S1*(v1)) + scale2[g] S2*(v2)) + U gx_half:
 * v1, v2 (both or neither; taps [G*F,5], scales [G]): grr_bwd_padj2's operands (W % 4 == 0, 16-byte
 * aligned); gx_half: a half-level x-gradient [B, G*F, H/2, W/2] (grr_bwd_unpool2_acc; H, W even). */
grr_status grr_bwd_cg_glue(const float* gx, const float* gx_half, const float* v1, const float* taps1,
                           const float* scale1, const float* v2, const float* taps2, const float* scale2,
                           const float* u, const float* gu_next, const float* u_prev, const float* alpha,
                           const float* beta_next, float* gu, float* gbb, float* gx_out, float* galpha, float* gbeta,
                           int B, int G, int F, int H, int W, void* stream);
/* grr_bwd_cg_glue that also writes gu_half = D gu [B, G*F, H/2, W/2] (grr_pool2's arithmetic): the
 * half-level operand of the operator reverse that reads gu next, formed in the pass that writes gu
 * (no separate pool of it).  W % 4 == 0, even H, 16-byte aligned planes. */
grr_status grr_bwd_cg_glue_pool(const float* gx, const float* gx_half, const float* v1, const float* taps1,
                                const float* scale1, const float* v2, const float* taps2, const float* scale2,
                                const float* u, const float* gu_next, const float* u_prev, const float* alpha,
                                const float* beta_next, float* gu, float* gbb, float* gx_out, float* gu_half,
                                float* galpha, float* gbeta, int B, int G, int F, int H, int W, void* stream);
grr_status grr_bwd_lincomb(const float* x, const float* sa, const float* y, const float* sb, float* out,
                           int accumulate, int B, int G, int F, int H, int W, void* stream);
/* out [B,C,H,W] += U(xd): 0.25 * xd(q/2) (conv_transpose2d of scaling_kernel01, REF:676-679). */
grr_status grr_bwd_unpool2_acc(const float* xd, float* out, int B, int C, int H, int W, void* stream);
/* gx[b,k,2i+di,2j+dj] = t[b,(2di+dj)K+k,i,j] (t [B,4K,H/2,W/2]): interleaves the four tap planes of
 * the 2x2 stride-2 conv's data gradient (REF:593-602, computed as one 1x1 GEMM with 4K rows).
 * H even, W % 4 == 0. */
grr_status grr_interleave2x2(const float* t, float* gx, int B, int K, int H, int W, void* stream);
/* Data gradient of grr_conv2x2s2: g [B,M,H/2,W/2], wt [M,K,2,2] -> gx [B,K,H,W]. */
grr_status grr_conv2x2s2_bwd_data(const float* g, const float* wt, float* gx, int B, int K, int M, int H, int W,
                                  void* stream);

/* ---- LocalNonLinearBlock reverse (training; REF:911-964) ---------------------------------
 * n = ln_w * x * isd with isd[b,p] = 1/sqrt(var_c x + 1e-5) (unbiased, uncentred x, REF:919-925). */
grr_status grr_lnb_norm(const float* x, const float* ln_w, float* n, float* isd, int B, int C, int64_t P,
                        void* stream);
/* gx [B,C,P] += d<gn, n>/dx;  gln_w [C] += sum gn x isd. */
grr_status grr_lnb_norm_bwd(const float* x, const float* ln_w, const float* isd, const float* gn, float* gx,
                            float* gln_w, int B, int C, int64_t P, void* stream);
/* grr_lnb_norm_bwd with the block's skip term in the same pass (the LocalNonLinearBlock reverse,
 * out = skip[0] x + skip[1] (...), REF13:541-575 under autograd): gx = skip[0] gout + the norm's data
 * gradient (gx written, not accumulated; gx != gout), gskip0[0] += <gout, x>, gln_w += as above. */
grr_status grr_lnb_norm_bwd_skip(const float* x, const float* ln_w, const float* isd, const float* gn,
                                 const float* gout, const float* skip, float* gx, float* gln_w, float* gskip0, int B,
                                 int C, int64_t P, void* stream);
/* depthwise 3x3 with replicate padding (channels_local_linear_op, REF:934-940): wdw [C,9]. */
grr_status grr_dwconv3(const float* h, const float* wdw, float* out, int B, int C, int H, int W, void* stream);
/* its reverse: gh = exact adjoint of the clamped gather applied to g; gwdw [C,9] += weight gradient. */
grr_status grr_dwconv3_bwd(const float* g, const float* h, const float* wdw, float* gh, float* gwdw, int B, int C,
                           int H, int W, void* stream);
/* gate = sigmoid(m) m v of hp = [m; v] [B,2hid,P] (if gate); ghp from ggate (if ggate) (REF:941-947). */
grr_status grr_lnb_gate(const float* hp, const float* ggate, float* gate, float* ghp, int B, int hid, int64_t P,
                        void* stream);
/* the gate's reverse with the skip scale folded in (autograd of REF:941-947, :962-964):
 * ghp = scale[0] * (d gate / d hp) . gq and gdot[0] += <gq, gate>, gq = W2^T gout — so the skip
 * weight's gradient <gout, W2 gate> needs no recomputed W2 gate. */
grr_status grr_lnb_gate_bwd_scaled(const float* hp, const float* gq, const float* scale, float* ghp, float* gdot, int B,
                                   int hid, int64_t P, void* stream);
/* depthwise 3x3 + gate in one row pass: gate [B,hid,H,W] = sigmoid(m) m v of (m, v) = dw3(hh) (the
 * depthwise output itself is not stored).  W <= 256 with W % V == 0, else GRR_ERR_UNSUPPORTED. */
grr_status grr_lnb_dw3_gate(const float* hh, const float* wdw, float* gate, int B, int hid, int H, int W,
                            void* stream);
/* Kernel knob (no reference counterpart): 1 (default) runs grr_lnb_gate_dw3_bwd's recomputing variant (hp NULL)
 * with its operand rows through a per-wave LDS-DMA ring where W % 4 == 0 and the planes are 16-byte aligned
 * (one strip of 8-column lanes for 256 < W <= 512, W % 8 == 0, 32-byte aligned planes), 0 the
 * register-prefetch row kernel.  Process-wide; results agree to fp32 rounding.  A/B and tests. */
grr_status grr_lnb_set_bwd_ring(int enable);
/* Host replay of the gate + depthwise reverse ring kernel's DMA geometry at image width W (W % 4 == 0): GRR_OK
 * when every ring-row DMA of every column strip writes inside its ring row and reads inside its image row
 * (the invariant whose violation faulted round 5's two-DMAs-per-row attempt), else GRR_ERR_SHAPE with the
 * first violation in grr_last_error.  Covers the strip instance of the width (V = 1, 2, 4) and, for
 * 256 < W <= 512 with W % 8 == 0, the one-strip V = 8 instance (two DMAs per 2-KB ring row) that
 * grr_lnb_gate_dw3_bwd runs there.  No device work. */
grr_status grr_dw3_ring_check(int W);
/* grr_lnb_gate_bwd_scaled and grr_dwconv3_bwd in one row pass (ghp stays on chip): hp [B,2hid,H,W]
 * (depthwise output; NULL = recomputed from hh in-kernel), gq [B,hid,H,W], hh [B,2hid,H,W]
 * (depthwise input), wdw [2hid,9] ->
 * gh [B,2hid,H,W]; gwdw [2hid,9] += ; gdot[0] += <gq, gate>.  W <= 256 with W % V == 0
 * (V = 1 / 2 / 4 for W <= 64 / 128 / 256), else GRR_ERR_UNSUPPORTED. */
grr_status grr_lnb_gate_dw3_bwd(const float* hp, const float* gq, const float* scale, const float* hh,
                                const float* wdw, float* gh, float* gwdw, float* gdot, int B, int hid, int H, int W,
                                void* stream);

/* The same two row passes for the window models' FeedForward (REF7:29-48): zero-padded depthwise
 * (nn.Conv2d padding=1) and gate = gelu(d1) d2 (exact erf gelu); the reverse recomputes the depthwise
 * output from hh (no hp operand) and adds <gq, gate> to gdot[0]. */
grr_status grr_ffn_dw3_gate(const float* hh, const float* wdw, float* gate, int B, int hid, int H, int W,
                            void* stream);
grr_status grr_ffn_gate_dw3_bwd(const float* gq, const float* scale, const float* hh, const float* wdw, float* gh,
                                float* gwdw, float* gdot, int B, int hid, int H, int W, void* stream);

/* ---- window graphs (older image-domain models) ------------------------------
 * REF7 = exploration/model_multiscale_mixture_GLR/lib/model_GLR_GTV_deep_v7.py,
 * REF1 = .../lib/model_GLR_GTV_deep_v1.py.  Graphs connect each pixel to the K
 * neighbours of a connection window; delta is a HOST array int32 [K,2] of (dy, dx)
 * offsets in the reference's edge order (itertools.product over the window, REF7:285-296),
 * |dy|, |dx| <= 2, K <= 24.  Signals x [B,G,Fs,H,W] (Fs = signal channels, 3 for RGB);
 * edge weights [B,G,K,H,W]; taps device [5] = (centre, up, left, right, down) of the
 * module's stats stencil (identity (1,0,0,0,0) for REF1, which has none). */

/* Edge weights of a window graph (GLRFast/GTVFast.extract_edge_weights, REF7:418-446):
 * feat channels [g*F, (g+1)*F) of each batch item (batch stride feat_bstride floats),
 * normalised over F, scaled by multiM [G,F], K dot products with the (replicate-clamped)
 * neighbours, softmax over the K edges -> w [B,G,K,H,W]; deg [B,G,H,W] (may be NULL). */
grr_status grr_win_edge_weights(const float* feat, int64_t feat_bstride, const float* multiM, const int32_t* delta,
                                int K, float* w, float* deg, int B, int G, int F, int H, int W, void* stream);

/* One fused pass of MixtureGTV's solver (REF7:892-1004; REF1:558-676), edge tensors never
 * materialised.  mu, ro [G] linear, log_gamma [G] (gamma = exp), alpha/beta [G] = one row.
 *  mode 0, CG step: A x = x + mu S_L^T(S_L x - W_L S_L x) + ro S_G^T C^T C S_G x (REF7:892-911),
 *          u = (y - A x) + beta u_prev (u = y - A x when u_prev == NULL), out = x + alpha u,
 *          u_out = u (may be NULL); y is the right-hand side [B,G,Fs,H,W].
 *  mode 1, rhs:      out = ro S_G^T C^T (C S_G x) + y        (first ADMM rhs, bias 0, REF7:945-949)
 *  mode 2, prox rhs: out = ro S_G^T C^T (2 soft(C S_G x, gamma) - C S_G x) + y
 *                    (one ADMM bias update from 0, REF7:958-967);
 *          modes 1/2: y [B,Fs,H,W] shared by the graphs, x per graph or (x_rep) [B,Fs,H,W].
 *  mode 3, module apply (GLRFast/GTVFast.forward, REF7:503-511, :776-782):
 *          out = mu S_L^T(S_L x - W_L S_L x) [wL != NULL] + ro S_G^T C^T C S_G x [wG != NULL];
 *          mu / ro may be NULL (= 1); y unused.
 * S reads x with a reflect frame (REF7:449-467); L/C neighbours clamp to the frame; S^T and
 * the C^T scatter drop what lands outside (REF7:469-488, :748-774).
 *  modes 4, 5, 7: modes 0, 1, 3 with wG holding the pair weights of grr_win_pair_weights (the
 *          same linear GTV term, K weight loads per position instead of 2 K). */
grr_status grr_win_solver(int mode, const float* x, int x_rep, const float* y, const float* u_prev, const float* wL,
                          const float* wG, const float* tapsL, const float* tapsG, const float* mu, const float* ro,
                          const float* log_gamma, const float* alpha, const float* beta, const int32_t* delta, int K,
                          float* out, float* u_out, int B, int G, int Fs, int H, int W, void* stream);

/* Pair weights of a window graph's linear GTV term: c [B,G,K,H,W] with
 * c_e(q) = w_e(q)^2 + [q + d_e inside] w_e'(q + d_e)^2, e' the edge of offset -d_e, so that
 * C^T C s (q) = sum_e c_e(q) (s(q) - s(clamp(q + d_e))) (the frame-dropped scatter of
 * GTVFast.op_C_transpose, REF7:748-774, paired edge by edge).  GRR_ERR_UNSUPPORTED when an offset
 * has no reverse in delta. */
grr_status grr_win_pair_weights(const float* w, const int32_t* delta, int K, float* c, int B, int G, int H, int W,
                                void* stream);

/* Graph mixture (REF7:1006-1009): out[b,c] = sum_g x[b,g,c] score[b,g] + dc[b,c] (dc may be NULL).
 * x [B,G,Fs,H,W], score [B,G,H,W], dc/out [B,Fs,H,W]. */
grr_status grr_win_mix(const float* x, const float* score, const float* dc, float* out, int B, int G, int Fs, int H,
                       int W, void* stream);

/* ---- window-graph reverse (training): replaces torch autograd through MixtureGTV's solver,
 * edge weights and mixture (REF7:418-446, :449-488, :892-1011 under loss.backward() of the
 * multiblocks training script).  Planes [B,G,Fs,H,W]; per-graph scale vectors [G] may be
 * NULL (= 1); every reduction output (gw, gdot, ggamma, gtaps, gmultiM) ACCUMULATES.
 * H, W >= 2 (the reflect frame). */

/* Stencil of the reverse: mode 0 S x (reflect frame), 1 S^T* g (zero-frame correlation),
 * 2 S* g (adjoint of the reflect-frame stencil).  out = [out +] scale[g] y. */
grr_status grr_win_bwd_stencil(const float* x, const float* taps, int mode, const float* scale, int accumulate,
                               float* out, int B, int G, int Fs, int H, int W, void* stream);
/* gtaps[t] += sum scale[g] u(p) z(src_t(p)); mode 0 src = reflect(p + d_t) (S), 1 src = p - d_t (S^T). */
grr_status grr_win_bwd_tapgrad(const float* u, const float* z, int mode, const float* scale, float* gtaps, int B,
                               int G, int Fs, int H, int W, void* stream);
/* GLR term reverse, pass 1 (s = S x, b = S^T* g): l_out = (I - W) s, gsd = scale b,
 * E [B,G,Fs,K,H,W] = scale b w_e (gathered by grr_win_bwd_gather; may be NULL with
 * grr_win_bwd_gather_fused), gw += -scale b s(n_e),
 * gdot[g] += coef <b, l>. */
grr_status grr_win_bwd_glr(const float* s, const float* b, const float* w, const int32_t* delta, int K,
                           const float* scale, float coef, float* l_out, float* E, float* gsd, float* gw, float* gdot,
                           int B, int G, int Fs, int H, int W, void* stream);
/* GTV term reverse, pass 1 (C^T C, or with prox C^T phi(C .)): gsd, E as above, PW [B,G,Fs,K,H,W] (E, PW
 * may be NULL with grr_win_bwd_gather_fused)
 * = w_e phi(z_e) (the gather rebuilds o = C^T phi from it), gw, gdot[g] += coef <b, o>,
 * ggamma[g] += dL/dgamma (prox). */
grr_status grr_win_bwd_gtv(const float* s, const float* b, const float* w, const int32_t* delta, int K, int prox,
                           const float* log_gamma, const float* scale, float coef, float* PW, float* E, float* gsd,
                           float* gw, float* gdot, float* ggamma, int B, int G, int Fs, int H, int W, void* stream);
/* Pass 2: gs -= sum_e sum_{p: clamp(p + delta_e) = q} E_e(p) (in place); with PW also o_out. */
grr_status grr_win_bwd_gather(const float* E, const float* PW, const int32_t* delta, int K, float* gs, float* o_out,
                              int B, int G, int Fs, int H, int W, void* stream);
/* Pass 2 without the E / PW planes (pass 1 then runs with E = PW = NULL): each E_e(p) / PW_e(p) is
 * recomputed at the pixel that gathers it from s, b, w (gtv = 0: the GLR term's E; gtv = 1: the GTV
 * term's E and, with o_out, o = C^T phi(C s); prox, log_gamma, scale as in pass 1).  Same result as
 * grr_win_bwd_glr / _gtv writing the planes + grr_win_bwd_gather, without 2 Fs K floats per pixel
 * written and read back. */
grr_status grr_win_bwd_gather_fused(const float* s, const float* b, const float* w, const int32_t* delta, int K,
                                    int gtv, int prox, const float* log_gamma, const float* scale, float* gs,
                                    float* o_out, int B, int G, int Fs, int H, int W, void* stream);
/* Edge-weight reverse of grr_win_edge_weights: gw is overwritten (softmax reverse in place);
 * the [G*F] slab of gfeat and gmultiM [G,F] accumulate (the GTV and GLR graphs share features). */
grr_status grr_win_bwd_edge_weights(const float* feat, int64_t feat_bstride, const float* multiM, const float* w,
                                    float* gw, const int32_t* delta, int K, float* gfeat, int64_t gfeat_bstride,
                                    float* gmultiM, int B, int G, int F, int H, int W, void* stream);
/* Mixture reverse: gx[b,g,c] = gout[b,c] score[b,g], gscore[b,g] = sum_c gout[b,c] x[b,g,c]. */
grr_status grr_win_bwd_mix(const float* gout, const float* x, const float* score, float* gx, float* gscore, int B,
                           int G, int Fs, int H, int W, void* stream);

/* ---- whole-image restoration I/O (no reference counterpart: the reference's test loop pads, crops, clamps
 * and quantises one float image on the host, scripts_v2 ...sigma25.py:249-279).  The image is H x W x C,
 * interleaved (HWC) and contiguous, uint8 (img_f32 = 0, any byte address) or float32 (img_f32 = 1, 4-byte
 * aligned); windows are the model's planar float32 batch [n, C, th, tw].  table: int32 [n, 6] on the
 * device, rows (wr, wc, r0, r1, c0, c1) = a window's origin and its core box in the coordinates of the
 * image padded at the bottom and right (tiling.Window).  Every index taken from the table is clamped into
 * the image and the window, so a bad table gives wrong pixels, never an access outside the buffers. */

/* 1 where the image entry points take an H x W x C image (or a batch of n windows as C, n th, tw): 1 <= C <= 4,
 * H, W >= 1 and H W C < 2^31. */
int grr_image_io_supported(int C, int H, int W);
/* out[i, c, y, x] = padded(wr_i + y, wc_i + x, c): a padded row r >= H reads row 2(H-1) - r, a padded column
 * likewise (nn.functional.pad(..., "reflect") at the bottom / right; the pad must be smaller than the side).
 * uint8 converts as float(v) / 255.0f, correctly rounded; float32 is copied bit for bit. */
grr_status grr_tile_gather(const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n, int th,
                           int tw, float* out, void* stream);
/* img[r, c, :] = y[i, :, r - wr_i, c - wc_i] for (r, c) in window i's core box cut to [0, H) x [0, W): with cores
 * that partition the padded image each pixel is written exactly once.  uint8: clamp to [0, 1], multiply by
 * 255 in float32, round half to even, clip to [0, 255], cast (skimage's img_as_ubyte of the clamped value,
 * REF test loop :278-279); NaN writes 0.  float32: unclamped copy. */
grr_status grr_tile_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* img, int img_f32, int H,
                            int W, int C, void* stream);
/* *out = sum_i (a[i] - b[i])^2 over n < 2^31 bytes, exact (integer) and the same on every run; out: one
 * 8-byte aligned uint64 on the device, overwritten. */
grr_status grr_u8_sse(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out, void* stream);

/* ---- the same for a list of images that share window batches (restore_images).  The images of one call lie in
 * one arena: a contiguous device buffer of arena_elems elements of their own dtype (uint8, any byte address, or
 * float32, 4-byte aligned), HWC each, packed back to back with no padding, so a uint8 image may start at any
 * byte.  img_table: int64 [n_img, 3] on the device, 8-byte aligned, rows (element offset, H, W); all images of a
 * call share C.  table: int32 [n, 7] on the device, rows (img, wr, wc, r0, r1, c0, c1): the image's index, then
 * the window row of the single-image calls in that image's padded coordinates.  Both tables are device data the
 * host cannot see: the image index is clamped into [0, n_img), H and W into [1, 2^31), and every element index
 * derived from them is kept inside [0, arena_elems) -- reads are clamped, writes outside are dropped -- so bad
 * tables give wrong pixels, never an access outside the arena and the window batch. */

/* 1 where the arena entry points take the call: 1 <= C <= 4, 1 <= n_img <= arena_elems (an image has at least
 * one element) and arena_elems < 2^62 (64-bit offsets: the arena may exceed 2^31 elements).  Per image,
 * H W C < 2^31 (grr_image_io_supported) is the caller's to keep: it is device data here.  The window batch is
 * bounded as in the single-image calls (n th tw C < 2^31). */
int grr_image_arena_supported(int C, int n_img, int64_t arena_elems);
/* grr_tile_gather for window i of image table[i][0]: that image's own H and W in the reflect rule, the same
 * element conversion. */
grr_status grr_tiles_gather(const void* arena, int64_t arena_elems, int img_f32, int C, const int64_t* img_table,
                            int n_img, const int32_t* table, int n, int th, int tw, float* out, void* stream);
/* grr_tile_scatter of each window's core box, cut to its own image's H x W, into that image's span of the
 * arena; the same quantisation. */
grr_status grr_tiles_scatter(const float* y, const int32_t* table, int n, int th, int tw, void* arena, int64_t arena_elems,
                             int img_f32, int C, const int64_t* img_table, int n_img, void* stream);
/* out[i] = sum (a[j] - b[j])^2 over j in [offsets[i], offsets[i + 1]), i < n_seg, in one launch: exact 64-bit
 * integers, the same on every run.  offsets: int64 [n_seg + 1] on the device, 8-byte aligned, clamped into
 * [0, total] and made monotone by the kernel; segments may start at any byte.  out: n_seg 8-byte aligned
 * uint64 on the device, overwritten.  n_seg <= 65535 (one grid row per segment), else GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_sse_segments(const uint8_t* a, const uint8_t* b, int64_t total, const int64_t* offsets, int n_seg,
                               uint64_t* out, void* stream);

/* ---- 8-way geometric self-ensemble of the two families above (restore_image(ensemble=...)).  Mode m = 2k + f
 * of 0..7 is T_m(a) = np.rot90(a, k) (k quarter turns counter-clockwise), then np.flipud if f = 1 -- the
 * numbering of the reference's data_augmentation (lib/dataloader*.py).  Pixel (i, j) of a th x tw window lands
 * where k applications of (i, j, th, tw) <- (tw - 1 - j, i, tw, th), then i <- th - 1 - i if f, put it: T_m is
 * th x tw for even k (modes 0, 1, 4, 5) and tw x th for odd k (2, 3, 6, 7).  The transforms act on the model's
 * window, after the reflect rule: the window tables, the padding, the cores and the crop are those of the plain
 * entry points.  modes: n_modes ints on the HOST, strictly ascending, each in 0..7; they are copied into the
 * kernel arguments.  A bad list is GRR_ERR_INVALID_ARG before any launch; image, arena and batch checks as in
 * the plain entry points, with n times the modes of an orientation as the batch's rows. */

/* out[w n_modes + j] = T_modes[j](window w as grr_tile_gather reads it), out: [n n_modes, C, bh, bw].  The modes
 * of one call share an orientation: all of even k, window w is bh x bw in the picture, or all of odd k, it is
 * bw x bh.  Element conversion as grr_tile_gather. */
grr_status grr_tile_gather_d8(const void* img, int img_f32, int H, int W, int C, const int32_t* table, int n,
                              const int32_t* modes, int n_modes, int bh, int bw, float* out, void* stream);
/* The mean of the n_modes members z_j = T_modes[j]^-1(model's result) of each th x tw window, then the steps of
 * grr_tile_scatter (core box, crop, quantisation).  y0: [n n_even, C, th, tw], the even-k members in list order,
 * window-major as grr_tile_gather_d8 lays them out; y1: [n n_odd, C, tw, th], the odd-k members; either is
 * ignored (may be NULL) when its count is 0; n_even + n_odd = n_modes and both must be the list's counts.  The
 * mean is a float32 pairwise tree over the listed order -- [z0 + z1, z2 + z3, ..., the odd one carried], until
 * one is left -- divided by float(n_modes), correctly rounded.  Each core pixel is written once; no atomics. */
grr_status grr_tile_scatter_mean(const float* y0, const float* y1, const int32_t* table, int n, const int32_t* modes,
                                 int n_modes, int n_even, int n_odd, int th, int tw, void* img, int img_f32, int H, int W,
                                 int C, void* stream);
/* grr_tile_gather_d8 for window i of image table[i][0] of the arena (table rows [n, 7]). */
grr_status grr_tiles_gather_d8(const void* arena, int64_t arena_elems, int img_f32, int C, const int64_t* img_table,
                               int n_img, const int32_t* table, int n, const int32_t* modes, int n_modes, int bh, int bw,
                               float* out, void* stream);
/* grr_tile_scatter_mean into each window's own image of the arena. */
grr_status grr_tiles_scatter_mean(const float* y0, const float* y1, const int32_t* table, int n, const int32_t* modes,
                                  int n_modes, int n_even, int n_odd, int th, int tw, void* arena, int64_t arena_elems,
                                  int img_f32, int C, const int64_t* img_table, int n_img, void* stream);

/* ---- SSIM of two uint8 H x W x C images (csrc/metric_ops.hip), beside grr_u8_sse's PSNR.  Wang et al.'s index as
 * skimage.metrics.structural_similarity(a, b, gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
 * data_range=255, channel_axis=2) defines it: an 11 x 11 separable Gaussian window with float64 taps
 * g[k] = exp(-(k - 5)^2 / 4.5) / sum; per channel the filtered moments mx, my, E[x^2], E[y^2], E[xy] at the
 * (H - 10) x (W - 10) pixels whose window lies inside the image (no border rule exists); vx = E[x^2] - mx^2,
 * vy = E[y^2] - my^2, vxy = E[xy] - mx my; C1 = 6.5025, C2 = 58.5225;
 * s = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)); SSIM = the mean of s over the
 * N = (H - 10)(W - 10) C values.  Each s is float64 from the bytes in one fixed order (horizontal taps ascending,
 * then vertical taps ascending), quantised to q = rint(2^32 s), |q| <= 2^32, and the q are added as signed 64-bit
 * integers: the entry points return sum q, which is exact, the same on every run and independent of the grid and
 * of what else an arena holds; SSIM = sum q / (2^32 N), within 2^-32 of the float64 mean.  Equal images give
 * exactly N 2^32. */

/* 1 where grr_u8_ssim takes the image: 1 <= C <= 4, H, W >= 11 and H W C < 2^31. */
int grr_u8_ssim_supported(int C, int H, int W);
/* *out = sum q over the image pair a, b (HWC, contiguous, any byte address); out: one 8-byte aligned int64 on the
 * device, overwritten.  GRR_ERR_UNSUPPORTED where grr_u8_ssim_supported is 0. */
grr_status grr_u8_ssim(const uint8_t* a, const uint8_t* b, int H, int W, int C, int64_t* out, void* stream);
/* out[i] = sum q of image i of the arenas a and b, which share arena_elems and the image table (int64 [n_img, 3]
 * on the device, 8-byte aligned, rows (element offset, H, W), as grr_tiles_gather takes it), in one launch.
 * max_h, max_w: the largest H and the largest W of the table, which the host cannot read here; they size the grid.
 * The table is clamped -- offset into [0, arena_elems), H into [1, max_h], W into [1, max_w], every byte index
 * into [0, arena_elems) -- so a bad table gives wrong sums, never an access outside the arenas.  An image with a
 * side below 11 has no valid pixel: its sum is 0.  out: n_img 8-byte aligned int64 on the device, overwritten.
 * n_img <= 65535 (one grid row per image), else GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_ssim_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, int C, const int64_t* img_table,
                              int n_img, int max_h, int max_w, int64_t* out, void* stream);

/* ---- PSNR and SSIM on the luma of two uint8 H x W x 3 images, channels R, G, B interleaved (csrc/metric_ops.hip):
 * the Y of ITU-R BT.601 "studio range" YCbCr, as MATLAB's rgb2ycbcr, skimage.color.rgb2ycbcr and BasicSR's
 * to_y_channel define it, not rounded to uint8: Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255 = Ny / 255000 with
 * the integer Ny = 4080000 + 65481 R + 128553 G + 24966 B <= 59 925 000, so Y lies in [16, 235].
 *
 * SSE: per pixel D = Ny(a) - Ny(b) = 65481 dR + 128553 dG + 24966 dB, an exact integer with |D| <= 55 845 000 < 2^26;
 * S = sum D^2 over the N = H W pixels; PSNR_Y = 10 log10(255^2 255000^2 N / S).  D^2 < 2^52 and N < 2^30, so S can
 * reach 2^82: the entry points return two words per image, out[0] = sum (D^2 mod 2^32) < 2^62 and
 * out[1] = sum (D^2 >> 32) < 2^50, and S = out[0] + (out[1] << 32).  Integer adds throughout: exact, the same on
 * every run and independent of the grid.
 *
 * SSIM: the index of the section above on the single plane Y, each Y the float64 double(Ny) / 255000.0 (the integer
 * is exact, the division rounds once): the same taps, order, C1, C2, valid (H - 10)(W - 10) positions and
 * quantisation; the entry points return sum q over those N positions, SSIM_Y = sum q / (2^32 N).  Equal images give
 * exactly N 2^32.  No luma of a grey or RGBA image is defined: the entry points take 3 channels only. */

/* 1 where the luma entry points take an H x W x 3 image: H, W >= 1 (need_window != 0, the SSIM: >= 11) and
 * H W 3 < 2^31. */
int grr_u8_luma_supported(int H, int W, int need_window);
/* out[0], out[1] = the two words of S over the image pair a, b (HWC, C = 3, contiguous, any byte address); out: two
 * 8-byte aligned uint64 on the device, overwritten.  GRR_ERR_UNSUPPORTED where grr_u8_luma_supported(H, W, 0)
 * is 0. */
grr_status grr_u8_luma_sse(const uint8_t* a, const uint8_t* b, int H, int W, uint64_t* out, void* stream);
/* out[i][0], out[i][1] = the two words of S of image i of the arenas a and b, which share arena_elems and the image
 * table (int64 [n_img, 3] on the device, 8-byte aligned, rows (element offset, H, W)), all images of 3 channels, in
 * one launch.  The table is clamped -- offset into [0, arena_elems), H and W into [1, 2^31), the pixel count to
 * what the arena holds from the offset on -- so a bad table gives wrong sums, never an access outside the arenas.
 * out: n_img x 2 8-byte aligned uint64 on the device, overwritten.  n_img <= 65535 (one grid row per image), else
 * GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_luma_sse_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, const int64_t* img_table,
                                  int n_img, uint64_t* out, void* stream);
/* *out = sum q of the luma planes of the image pair a, b; out: one 8-byte aligned int64 on the device, overwritten.
 * GRR_ERR_UNSUPPORTED where grr_u8_luma_supported(H, W, 1) is 0. */
grr_status grr_u8_luma_ssim(const uint8_t* a, const uint8_t* b, int H, int W, int64_t* out, void* stream);
/* out[i] = sum q of the luma planes of image i of the arenas a and b: grr_u8_ssim_images' arguments, clamping and
 * limits with C = 3 understood. */
grr_status grr_u8_luma_ssim_images(const uint8_t* a, const uint8_t* b, int64_t arena_elems, const int64_t* img_table,
                                   int n_img, int max_h, int max_w, int64_t* out, void* stream);

/* ---- the SSIM training loss on float32 planar batches (csrc/ssim_loss_ops.hip): the index of the uint8 section
 * above -- the same taps, order of operations, valid positions and quantisation -- on planes of data range 1, so
 * C1 = 1e-4 and C2 = 9e-4.  x is the prediction, y the target, both contiguous float32 [B, C, H, W]; neither is
 * clamped, |s| <= 1 for any real input.  s is defined at N = B C (H - 10)(W - 10) positions and
 * loss = 1 - (sum s) / N.  With A1 = 2 mx my + C1, A2 = 2 vxy + C2, B1 = mx^2 + my^2 + C1, B2 = vx + vy + C2:
 *   c0 = ds/dmx = 2 my (A2 - A1) / (B1 B2) - 2 mx s / B1 + 2 mx s / B2,  c1 = ds/dE[x^2] = -s / B2,
 *   c2 = ds/dE[xy] = 2 A1 / (B1 B2),
 *   dloss/dx = -(1 / N) (F*(c0) + 2 x F*(c1) + y F*(c2)),
 * F* the window's adjoint: the full 2-D correlation of a (H - 10) x (W - 10) plane back to H x W, zero outside.  The
 * three terms cancel at the 1 / C2 scale where x is close to y, so c0, c1, c2 are float64 planes and the gradient is
 * float64 up to its one rounding to float32.  The target takes no gradient.  Base pointers at any 4-byte aligned
 * address, 8-byte for the int64 and float64 buffers. */

/* 1 where the loss takes the batch: B, C >= 1, H, W >= 11, B C <= 65535 (one grid row per plane) and
 * B C H W < 2^31. */
int grr_ssim_loss_supported(int B, int C, int H, int W);
/* qsum[b] = the sum of q = rint(2^32 s) over the C (H - 10)(W - 10) positions of batch item b, exact, the same on
 * every run and independent of the grid; loss = 1 - (sum over b of qsum[b]) / (2^32 N), within 2^-32 of the float64
 * value; equal x and y give exactly C (H - 10)(W - 10) 2^32 per item.  qsum: B int64 on the device, overwritten.
 * coef: float64 [3, B, C, H - 10, W - 10] on the device, overwritten with c0, c1, c2, or NULL where no gradient is
 * wanted (nothing is written then).  GRR_ERR_UNSUPPORTED where grr_ssim_loss_supported is 0. */
grr_status grr_ssim_loss_forward(const float* x, const float* y, int B, int C, int H, int W, int64_t* qsum, double* coef,
                                 void* stream);
/* gx = gout[0] dloss/dx from the forward's coef: float32 [B, C, H, W], every element overwritten, each formed in
 * float64 in one fixed order (a gather: no atomics, the same bits on every run) and rounded once.  gout: one float32
 * on the device, the incoming gradient of the loss, read by the kernel (no host synchronisation).
 * GRR_ERR_UNSUPPORTED where grr_ssim_loss_supported is 0. */
grr_status grr_ssim_loss_backward(const float* x, const float* y, const double* coef, const float* gout, float* gx,
                                  int B, int C, int H, int W, void* stream);

/* ---- training batches cut from an arena of uint8 images (training.DevicePatchLoader; the reference's
 * lib/dataloader_v2.py:ImageSuperResolution does this per sample on the host).  arena, arena_elems, C, img_table,
 * n_img: as grr_tiles_gather takes them, uint8 only.  table: int32 [n, 4] on the device, rows (img, row, col,
 * mode); sample_ids: int64 [n] on the device, 8-byte aligned; sigma: float32 [n] on the device, the noise standard
 * deviation in [0, 1] units (level / 255 as float32); clean, noisy: float32 [n, C, ph, pw], planar.
 *
 * clean: before the transform, pixel (i, j) of sample s is image pixel (sym(row + i, H), sym(col + j, W)) with
 * sym(r, n): t = r mod 2n; t < n ? t : 2n - 1 - t -- the edge-repeating mirror ...cba|abc...|cba... of
 * np.pad(mode="symmetric") and OpenCV's BORDER_REFLECT, periodic where the fill exceeds the side (not the "reflect"
 * of grr_tile_gather).  The pixel then moves by T_mode, numbered and indexed as for grr_tile_gather_d8 above; the
 * value is float(v) / 255.0f, correctly rounded.  The odd quarter turns (modes 2, 3, 6, 7) need ph == pw: the
 * tables are device data, so the caller checks this before upload, and the kernel reads an illegal mode as
 * mode & 5.  Modes are taken & 7.
 *
 * noisy = clean + noise in float32, noise = (float)((double)sigma[s] * z), where z is a function of (seed,
 * sample_ids[s], element) alone: with e = (y pw + x) C + c the element's position in the output patch in HWC
 * order, block b = e / 4 is Philox4x32-10 of counter (b, 0, low32(id), high32(id)) and key (low32(seed),
 * high32(seed)); its words x0..x3 give u_k = (x_k + 0.5) 2^-32 in float64; lanes e % 4 = 0, 1 are r cos(t) and
 * r sin(t) with r = sqrt(-2 log(u0)), t = 6.283185307179586 u1, all float64, and lanes 2, 3 the same from
 * (u2, u3).  sigma = 0 gives noisy == clean bit for bit.  A sample does not depend on the batch it is in.
 *
 * Every index from a table is clamped -- img into [0, n_img), row and col into the image, every element index
 * into [0, arena_elems) -- so a bad table gives wrong pixels, never an access outside the buffers.  No atomics. */

/* 1 where grr_patch_batch takes the call: grr_image_arena_supported(C, n_img, arena_elems), n, ph, pw >= 1 and
 * n C ph pw < 2^31. */
int grr_patch_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw);
grr_status grr_patch_batch(const uint8_t* arena, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                           const int32_t* table, const int64_t* sample_ids, const float* sigma, int n, uint64_t seed,
                           int ph, int pw, float* clean, float* noisy, void* stream);

/* ---- the same batch for degraded / clean picture pairs (training.PairedImageRestoration: real camera noise,
 * JPEG artefacts, blur, rain, published as file pairs).  input_arena and target_arena are two uint8 arenas of
 * arena_elems elements each that share the one image table: image i of input_arena is the degraded version of
 * image i of target_arena, with the same H, W and C.  table, sample_ids, n, seed, ph, pw: as grr_patch_batch takes
 * them.  target, input: float32 [n, C, ph, pw], planar.
 *
 * target[s] is grr_patch_batch's clean patch of target_arena.  input[s] is the same patch -- same origin, same
 * mirror fill, same T_mode -- of input_arena, float(v) / 255.0f as well.  sigma: float32 [n] on the device, or NULL.
 * With sigma, input additionally gets grr_patch_batch's noise, input = degraded + (float)((double)sigma[s] * z), z
 * the same function of (seed, sample_ids[s], element); with sigma == NULL or sigma[s] == 0 input is the degraded
 * pixels bit for bit, and no random number is computed.  input_arena == target_arena is legal: the call is then
 * grr_patch_batch with the outputs named differently (target = clean, input = noisy, bit for bit).
 *
 * One kernel body with grr_patch_batch; its clamping holds for both arenas (one element index, clamped once,
 * addresses both).  A sample does not depend on the batch it is in.  No atomics. */

/* 1 where grr_patch_pair_batch takes the call: the bounds of grr_patch_batch_supported (each output has
 * n C ph pw < 2^31 elements). */
int grr_patch_pair_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw);
grr_status grr_patch_pair_batch(const uint8_t* input_arena, const uint8_t* target_arena, int64_t arena_elems, int C,
                                const int64_t* img_table, int n_img, const int32_t* table, const int64_t* sample_ids,
                                const float* sigma /* NULL: no noise */, int n, uint64_t seed, int ph, int pw,
                                float* target, float* input, void* stream);

/* ---- bicubic resize of uint8 pictures by an integer scale s, 2 <= s <= 8 (csrc/resize_ops.hip): the degradation
 * of the bicubic super-resolution protocol -- mod-crop, antialiased bicubic down, bicubic back up -- made on the
 * device.  The convention is that of MATLAB's imresize (bicubic with a = -0.5, half-pixel centres, antialiasing
 * when shrinking, symmetric edge, a rounding to uint8 after each 1-D pass) with one change that makes the result
 * exact and independent of any order of summation: the weights are fixed-point integers.  No floating point
 * appears in the definition.
 *
 * cubic(x) = 1.5 |x|^3 - 2.5 |x|^2 + 1 for |x| <= 1, -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2 for 1 < |x| < 2, else 0.
 * 1-D down pass, length n -> ceil(n / s): output i has centre u = (i + 1/2) s - 1/2, its taps are all integers j
 *   with |u - j| < 2 s, raw weight cubic((u - j) / s); relative to i s the taps are the same for every i (one
 *   phase).
 * 1-D up pass, length n -> any L with s (n - 1) < L <= s n: output y has phase p = y mod s and base b = y div s;
 *   u = (p + 1/2) / s - 1/2, taps are the integers j with |u - j| < 2 at input index b + j, raw weight
 *   cubic(u - j) (s phases).
 * One tap set is quantised from exact rationals: divide the raw weights by their exact sum, q = round-half-even(
 *   w 2^30), add 2^30 - sum q to the largest q (the lowest index among equals), drop zero taps.  sum q = 2^30, so
 *   a constant picture maps to itself.
 * Applying it: input indices go through sym(r, n) of grr_patch_batch (t = r mod 2n; t < n ? t : 2n - 1 - t,
 *   periodic where the support exceeds the side), acc = sum q v in 64-bit integers,
 *   out = clamp((acc + 2^29) >> 30, 0, 255) with an arithmetic shift.
 * 2-D: rows (axis 0) first, then columns, each pass uint8 -> uint8, per channel.
 *
 * The caller computes the quantised tap sets and passes them as host arrays: n_phase (1 for down, s for up), and
 * per phase p first[p], the offset of its first tap (from i s for down, from b for up), count[p], and count[p]
 * weights in taps, the phases back to back; a phase's taps are consecutive offsets, so a dropped zero tap between
 * two others is passed as a zero.  The library copies them into the kernel arguments.  GRR_ERR_INVALID_ARG, before
 * any launch, for a phase that does not sum to 2^30, has more than 4 s taps, or has a tap outside the offsets the
 * definition can give (down -2 s .. 3 s, up -2 .. 2).
 *
 * src, dst: HWC interleaved uint8 at any byte address; element offsets are 64-bit.  Each output byte is written
 * once; no atomics; the uint8 picture between the two passes lives in LDS only. */

/* 1 where grr_u8_resize takes the image: 1 <= C <= 4, 2 <= s <= 8, H, W >= 1, and both H W C and the output's
 * element count (down: ceil(H / s) ceil(W / s) C; up: s H s W C) below 2^31. */
int grr_u8_resize_supported(int C, int H, int W, int s, int up);
/* One image.  down (up == 0): Ho == ceil(H / s) and Wo == ceil(W / s); up: s (H - 1) < Ho <= s H and likewise Wo;
 * else GRR_ERR_SHAPE. */
grr_status grr_u8_resize(const uint8_t* src, int H, int W, int C, uint8_t* dst, int Ho, int Wo, int s, int up,
                         int n_phase, const int32_t* first, const int32_t* count, const int32_t* taps, void* stream);
/* Every image of src_arena into its place in dst_arena, one launch: image i is read at row i of src_table and
 * written at row i of dst_table (int64 [n_img, 3] each on the device, 8-byte aligned, rows (element offset, H, W)
 * and (element offset, Ho, Wo); the two arenas have different image sizes, hence two tables).  max_ho, max_wo bound
 * every image's output sides.  The tables are clamped -- offsets into the arenas, sides into [1, 2^31) and
 * [1, max_ho] x [1, max_wo], every element index read into [0, src_elems), a write at or past dst_elems dropped --
 * so a bad table gives wrong pixels, never an access outside the two arenas; that Ho, Wo are the legal output sides
 * of H, W is the caller's to check on its host copy.  n_img <= 65535 (one grid row per image), else
 * GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_resize_images(const uint8_t* src_arena, int64_t src_elems, const int64_t* src_table,
                                uint8_t* dst_arena, int64_t dst_elems, const int64_t* dst_table, int C, int n_img,
                                int max_ho, int max_wo, int s, int up, int n_phase, const int32_t* first,
                                const int32_t* count, const int32_t* taps, void* stream);

/* ---- the JPEG round trip of uint8 pictures (csrc/jpeg_ops.hip): decode(encode(x)) of a baseline JPEG at quality
 * q, the degradation of compression-artifact removal, made on the device without a bitstream.  Huffman coding is
 * lossless, so the round trip is: colour transform, optional chroma down-sampling, 8 x 8 forward DCT, quantise,
 * dequantise, inverse DCT, up-sample, colour transform back; in libjpeg's default integer ("islow") arithmetic
 * every step is fixed-point and the bytes are exact.  tests/test_jpeg_ref.py holds a restatement of what follows
 * to Pillow (libjpeg-turbo) byte for byte.
 *
 * All arithmetic is integer; >> is an arithmetic shift; DESCALE(x, n) = (x + (1 << (n - 1))) >> n.
 *
 * Quality: an integer q of 1..100.  scale = 5000 / q (integer division) if q < 50, else 200 - 2 q; a table entry
 *   is clamp((base scale + 50) / 100, 1, 255), base from the Annex-K luminance or chrominance table in natural
 *   (not zig-zag) order.  Gray uses the luminance table.
 * Modes: C = 1: one plane, luminance table (sub is checked and otherwise ignored).  C = 3, sub = 0: 4:4:4.
 *   C = 3, sub = 2: 4:2:0 (Pillow's numbering).  Other channel counts and subsamplings are refused.
 * Colour in (C = 3), F(x) = floor(x 65536 + 0.5):
 *   Y  = ( F(.299) R + F(.587) G + F(.114) B + 32768) >> 16
 *   Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16
 *   Cr = ( F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16
 * Chroma down (4:2:0): the full-resolution chroma plane is extended by replicating its last column out to a
 *   multiple of 16 columns and its last row to an even row count; a sample is (a + b + c + d + bias) >> 2 over its
 *   2 x 2 cell, bias 1 in even output columns and 2 in odd ones.  The plane has ceil(H / 2) rows and a multiple of 8
 *   columns; its rows are then padded as any plane's are.  So the padding columns hold the mean of the last
 *   full-resolution column, not the last chroma sample, and the padding rows hold the last chroma row.
 * Plane codec: the plane is extended to multiples of 8 by replicating its last column and row; samples are taken
 *   minus 128; blocks are 8 x 8 on the plane's own grid from (0, 0).
 *   Forward DCT, rows then columns, is jfdctint's (CONST_BITS 13, PASS1_BITS 2), with the constants 2446, 3196,
 *   4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172 for 0.298631336, 0.390180644, 0.541196100,
 *   0.765366865, 0.899976223, 1.175875602, 1.501321110, 1.847759065, 1.961570560, 2.053119869, 2.562915447,
 *   3.072711026.  With t0..t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4, t7..t4 = d0 - d7, d1 - d6, d2 - d5, d3 - d4,
 *   t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2: outputs 0 and 4 are (t10 +- t11) << 2 in the row
 *   pass and DESCALE(t10 +- t11, 2) in the column pass; with z1 = (t12 + t13) 4433, outputs 2 and 6 are
 *   DESCALE(z1 + 6270 t13, n) and DESCALE(z1 - 15137 t12, n), n = 11 in the row pass and 15 in the column pass.
 *   The odd part, shared with the inverse: ODD(a, b, c, d): z1 = a + d, z2 = b + c, z3 = a + c, z4 = b + d,
 *   z5 = 9633 (z3 + z4), z3 = z5 - 16069 z3, z4 = z5 - 3196 z4, z1 = -7373 z1, z2 = -20995 z2, giving
 *   (2446 a + z1 + z3, 16819 b + z2 + z4, 25172 c + z2 + z3, 12299 d + z1 + z4).  Outputs 7, 5, 3, 1 are
 *   DESCALE(., n) of ODD(t4, t5, t6, t7).
 *   Quantise with v = 8 entry: k = sign(c) ((|c| + (v >> 1)) / v); dequantise: k entry.
 *   Inverse DCT, columns then rows, is jidctint's: z1 = 4433 (c2 + c6), t2 = z1 - 15137 c6, t3 = z1 + 6270 c2,
 *   t0 = (c0 + c4) << 13, t1 = (c0 - c4) << 13, t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2,
 *   (o0, o1, o2, o3) = ODD(c7, c5, c3, c1); outputs 0..7 are DESCALE(t10 + o3, t11 + o2, t12 + o1, t13 + o0,
 *   t13 - o0, t12 - o1, t11 - o2, t10 - o3; n), n = 11 in the column pass and 18 in the row pass.
 *   Then + 128 and a plain clamp to 0..255, as libjpeg-turbo's SIMD path does; the C range table's wrap beyond
 *   +-512 is not reproduced.
 * Chroma up (4:2:0), from the decoded chroma cropped to ceil(H / 2) x ceil(W / 2):
 *   chroma width <= 2: each sample is replicated 2 x 2 (libjpeg turns its triangle filter off there);
 *   chroma width > 2: s = 3 near row + far row, the far row of an even output row the row above, of an odd one the
 *   row below, the first and last rows standing in for the missing ones; left output = (3 s[x] + s[x - 1] + 8) >> 4,
 *   right output = (3 s[x] + s[x + 1] + 7) >> 4, except the first column's left output (4 s[0] + 8) >> 4 and the
 *   last column's right output (4 s[last] + 7) >> 4; crop to H x W.
 * Colour out, cb and cr taken minus 128: R = clamp(Y + ((F(1.402) cr + 32768) >> 16)),
 *   B = clamp(Y + ((F(1.772) cb + 32768) >> 16)), G = clamp(Y + ((-F(.34414) cb - F(.71414) cr + 32768) >> 16)).
 *
 * The quantisation tables are made from the quality on the device.  src, dst: HWC interleaved uint8 at any byte
 * address, distinct buffers; element offsets are 64-bit.  Each output byte is written once; no atomics; one launch;
 * the int intermediates live in LDS only. */

/* 1 where grr_u8_jpeg takes the image: C of 1 or 3, sub of 0 or 2, H, W >= 1, H W C < 2^31. */
int grr_u8_jpeg_supported(int C, int H, int W, int sub);
/* One image.  GRR_ERR_INVALID_ARG for a quality outside 1..100, GRR_ERR_UNSUPPORTED where the query says 0. */
grr_status grr_u8_jpeg(const uint8_t* src, int H, int W, int C, uint8_t* dst, int quality, int sub, void* stream);
/* Every image of arena into the same place of dst_arena (both of elems elements), one launch: image i is row i of
 * table (int64 [n_img, 3] on the device, 8-byte aligned, rows (element offset, H, W)) at quality qualities[i] (int32
 * [n_img] on the device).  max_h, max_w bound every image's sides.  Device data is clamped -- offsets into the
 * arena, sides into [1, max_h] x [1, max_w], qualities into 1..100, every element index read into [0, elems), a
 * write at or past elems dropped -- so a bad table gives wrong pixels, never an access outside the two arenas; the
 * caller checks its host copies.  n_img <= 65535 (one grid row per image), else GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_jpeg_images(const uint8_t* arena, int64_t elems, int C, const int64_t* table, int n_img, int max_h,
                              int max_w, uint8_t* dst_arena, const int32_t* qualities, int sub, void* stream);

/* ---- the blocking sums of PSNR-B (Yim and Bovik; csrc/metric_ops.hip).  Of a uint8 H x W x C picture est take
 * all horizontally and vertically adjacent pairs within one channel.  A pair is a boundary pair if it straddles a
 * multiple-of-8 line: x % 8 == 7 for (x, x + 1), likewise for rows.  S_b, N_b, S_n, N_n are the integer sums of
 * squared differences and the pair counts of the boundary and the non-boundary set.  D_b = S_b / N_b,
 * D_n = S_n / N_n, BEF = (3 / log2 min(H, W)) (D_b - D_n) if D_b > D_n, else 0, and
 * PSNR-B = 10 log10(255^2 / (SSE / (H W C) + BEF)) against a reference ref (SSE: grr_u8_sse), infinite when the
 * denominator is 0; it needs min(H, W) >= 16.  The counts are the true numbers of pairs; some public
 * implementations use H (W / 8 - 1) for the horizontal boundary count, which equals it only for multiples of 8.
 * The device returns the four integers (255^2 2 2^31 < 2^48: they fit); the caller forms the quotients in float64.
 * out: uint64 [4] (S_b, N_b, S_n, N_n) on the device, 8-byte aligned; integer adds, so the result does not depend
 * on the grid or the order the atomics land in. */
grr_status grr_u8_blocking(const uint8_t* est, int H, int W, int C, uint64_t* out, void* stream);
/* The same for every image of an arena in one launch: out is uint64 [n_img, 4]; the table is clamped as
 * grr_u8_ssim_images clamps it.  max_h max_w C < 2^31; n_img <= 65535. */
grr_status grr_u8_blocking_images(const uint8_t* est, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                                  int max_h, int max_w, uint64_t* out, void* stream);

/* ---- Bayer mosaicking and the initial fill of demosaicking (csrc/demosaic_ops.hip): an RGB picture is sampled
 * through a Bayer colour filter array and the two missing channels of every pixel are filled by a fixed linear
 * filter, the input a demosaicking model restores.  No floating point appears in the definition.
 *
 * Pattern: the colours of the top-left 2 x 2 cell in reading order, rggb = 0, grbg = 1, gbrg = 2, bggr = 3.  The R
 *   site has (row parity, column parity) = (0,0), (0,1), (1,0), (1,1) for the four codes, i.e. (code >> 1, code & 1);
 *   the B site has both parities opposite; every other site is G.  Channel order of a picture is R, G, B.
 * Mosaic: the plane of an H x W x 3 picture a is m[y,x] = a[y,x,site(y,x)], one byte per pixel.  A 1-channel source
 *   is already m.
 * Border: a neighbour outside the plane is read by reflection about the edge sample, without repeating it: for a
 *   side n >= 2 index i maps to t = i mod 2(n - 1) (non-negative), then t < n ? t : 2(n - 1) - t; for n = 1 every
 *   index maps to 0.  For n >= 2 this keeps the parity of an index, so a reflected neighbour has the colour the
 *   formula expects -- which sym of grr_patch_batch, repeating the edge sample, would not.  For n = 1 parity is not
 *   kept; the value read is still defined.
 * Fill: every output byte is clamp((s + 8) >> 4, 0, 255), s an int32 sum in sixteenths, >> arithmetic.  The site's own
 *   channel is s = 16 m[y,x] in every mode: a measured sample passes through.  With ctr = m[y,x], cross = the sum of
 *   the 4 neighbours at distance 1 along the axes, far = of the 4 at distance 2 along the axes, diag = of the 4
 *   diagonal neighbours, h1, h2 = of the 2 horizontal neighbours at distance 1 and at distance 2, v1, v2 the same
 *   vertically:
 *   zero (0):     every missing channel is 0 (the masked picture).
 *   bilinear (1): G at an R or B site 4 cross; R or B at a G site 8 h1 when that colour lies in this row, else
 *                 8 v1; R at a B site and B at an R site 4 diag.
 *   malvar (2):   the Malvar-He-Cutler gradient-corrected filters.  G at an R or B site 8 ctr + 4 cross - 2 far;
 *                 R or B at a G site, that colour in this row: 10 ctr + 8 h1 - 2 diag - 2 h2 + v2; in this column:
 *                 10 ctr + 8 v1 - 2 diag - 2 v2 + h2; R at a B site and B at an R site 12 ctr + 4 diag - 3 far.
 *   Every coefficient set sums to 16, so a gray constant maps to itself; |s| <= 2 * 20 * 255.
 *
 * src: HWC uint8 of src_c channels, dst: H x W x 3, both at any byte address, distinct buffers; element offsets are
 * 64-bit.  Each output byte is written once; no atomics; one launch; the mosaic plane lives in LDS only. */

/* 1 where grr_u8_demosaic takes the image: src_c of 1 or 3, H, W >= 1, 3 H W < 2^31. */
int grr_u8_demosaic_supported(int src_c, int H, int W);
/* One image.  GRR_ERR_INVALID_ARG for a pattern outside 0..3 or a fill outside 0..2, before any launch;
 * GRR_ERR_UNSUPPORTED where the query says 0. */
grr_status grr_u8_demosaic(const uint8_t* src, int H, int W, int src_c, uint8_t* dst, int pattern, int fill,
                           void* stream);
/* Every image of an RGB arena into the same place of dst_arena (both of elems elements), one launch: image i is row
 * i of table (int64 [n_img, 3] on the device, 8-byte aligned, rows (element offset, H, W)) with pattern patterns[i]
 * (int32 [n_img] on the device).  max_h, max_w bound every image's sides.  Device data is clamped -- offsets into the
 * arena, sides into [1, max_h] x [1, max_w], patterns into 0..3, every element index read into [0, elems), a write
 * at or past elems dropped -- so a bad table gives wrong pixels, never an access outside the two arenas; the caller
 * checks its host copies.  n_img <= 65535 (one grid row per image), else GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_demosaic_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, int max_h,
                                  int max_w, uint8_t* dst_arena, const int32_t* patterns, int fill, void* stream);

/* ---- joint denoising and demosaicking (csrc/rawnoise_ops.hip): sensor noise on the Bayer mosaic, BEFORE the fill.  A
 * sensor measures one noisy sample per pixel; the fill above then spreads and correlates that noise over the three
 * channels.  Because the noise must be fresh per sample and lie under a 5 x 5 filter, the degradation is made at batch
 * time, inside the patch kernel: cut, mosaic, noise, quantise, fill, turn, one launch.  It ends in exact integers:
 * floating point appears only before one rounding.
 *
 * Per sample s: a table row (img, row, col, mode) and a sample id, as grr_patch_batch takes them; a noise pair (a, b),
 *   float32: the noise variance is a x + b for a signal x in [0, 1], a the shot-noise gain and b the read-noise
 *   variance, both in [0, 1]; the Bayer code 0..3 of image img, as grr_u8_demosaic takes it; the H x W x 3 uint8
 *   picture.  Call-wide: fill 0..2, bits 8..16 with full = 2^bits - 1, clip 0 / 1, a uint64 seed.
 * Window: (ph + 4) x (pw + 4).  Window position (wy, wx) has image coordinates Y = row + wy - 2, X = col + wx - 2 and
 *   reads picture pixel (y', x') = (reflect(Y, H), reflect(X, W)), reflect the border rule of the demosaic section
 *   above taken for any index: no repeated edge sample, parity kept for a side >= 2, index 0 for a side of 1.  The
 *   channel it measures is the site of (y', x').  A patch that sticks out of its picture is therefore continued by
 *   this reflection, not by grr_patch_batch's sym, which would break the colour filter array's parity.
 * Raw sample: with v the byte read, x = v / 255 and var = a x + b, t = x + sqrt(var) z_e, where e = wy (pw + 4) + wx
 *   and z_e is grr_patch_batch's normal of (seed, sample id, element e): block e / 4, lane e % 4.  If clip, t is
 *   clamped to [0, 1].  q is the integer nearest to t full, ties to even, then clamped to +-2^24; a NaN gives 0 (the
 *   clamp cannot bind for a, b in [0, 1]: |z| < 6.8).  Where var == 0 no random number is computed.  Everything
 *   before the rounding is float64, in any association or contraction.
 * Fill: the demosaic section's sums with m replaced by q: s an int32 in sixteenths (|s| <= 40 * 2^24), the site's own
 *   channel s = 16 q, the filter set chosen by the site of (y', x').  The value is (float)((double)s / (16.0 full)):
 *   one float64 division, one conversion; no clamp and no rounding to bytes.  The 2-sample halo of the window is
 *   exactly what the 5 x 5 filters need: the fill itself has no border rule.
 * Outputs: patch pixel (i, j) is window position (i + 2, j + 2), moved by T_mode exactly as grr_patch_batch moves it
 *   (odd quarter turns need ph == pw; an illegal mode is read as mode & 5).  input holds the three filled channels,
 *   target is float(v) / 255.0f of the same picture pixel's three channels; both float32 [n, 3, ph, pw], planar.
 *   noise == NULL means a = b = 0 for every sample.  A sample does not depend on the batch it is in.
 *
 * arena, arena_elems, img_table, n_img, table, sample_ids: as grr_patch_batch takes them, C = 3 understood; patterns:
 * int32 [n_img] on the device; noise: float32 [n, 2] on the device, rows (a, b), or NULL.  Every table value is
 * clamped as in grr_patch_batch, the pattern into 0..3: a bad table gives wrong pixels, never an access outside the
 * buffers.  No atomics. */

/* 1 where grr_patch_raw_batch takes the call: grr_image_arena_supported(3, n_img, arena_elems), n, ph, pw >= 1,
 * 3 n ph pw < 2^31 and (ph + 4)(pw + 4) < 2^31. */
int grr_patch_raw_batch_supported(int n_img, int64_t arena_elems, int n, int ph, int pw);
/* GRR_ERR_INVALID_ARG for a fill outside 0..2, bits outside 8..16 or a clip that is not 0 or 1, before any launch;
 * GRR_ERR_UNSUPPORTED where the query says 0. */
grr_status grr_patch_raw_batch(const uint8_t* arena, int64_t arena_elems, const int64_t* img_table, int n_img,
                               const int32_t* patterns, const int32_t* table, const int64_t* sample_ids,
                               const float* noise /* [n, 2] or NULL */, int n, uint64_t seed, int ph, int pw, int fill,
                               int bits, int clip, float* target, float* input, void* stream);
/* 1 where grr_u8_raw_noise_demosaic takes the image: H, W >= 1, 3 H W < 2^31 and (H + 4)(W + 4) < 2^31. */
int grr_u8_raw_noise_demosaic_supported(int H, int W);
/* One picture: the same kernel body with row = col = 0, ph = H, pw = W, mode 0, no device tables and no target.  src:
 * H x W x 3 uint8 at any byte address; dst: float32 H x W x 3, HWC (the patch form's input up to layout).
 * GRR_ERR_INVALID_ARG for a pattern outside 0..3, a fill, bits or clip as above, or a, b outside [0, 1]. */
grr_status grr_u8_raw_noise_demosaic(const uint8_t* src, int H, int W, float* dst /* float32 H x W x 3, HWC */,
                                     int pattern, int fill, float a, float b, int bits, int clip, uint64_t seed,
                                     int64_t sample_id, void* stream);

/* ---- 2-D blur by an integer point-spread function (csrc/blur_ops.hip): the degradation of deblurring.  No floating
 * point appears in the definition.
 *
 * Kernel: an int32 weight table W[kh][kw], row-major; kh and kw odd, in 1..GRR_BLUR_MAX_SIDE; every W >= 0; the sum of
 *   W exactly GRR_BLUR_ONE.
 * Output: for a uint8 H x W x C picture, C in 1..4,
 *     out[y,x,c] = (32768 + sum_{i<kh, j<kw} W[i][j] * src[b(y + kh/2 - i, H), b(x + kw/2 - j, W), c]) >> 16
 *   a true convolution: the kernel is flipped, which matters for a motion kernel.  The sum is at most
 *   255 * 65536 < 2^24: int32 is exact and a valid table needs no clamp.
 * Boundary b(t, n): wrap (0) t mod n (non-negative), the circular convolution of the deblurring tables; replicate (1)
 *   t clamped into [0, n - 1]; reflect (2) about the edge sample without repeating it, as the demosaic border above:
 *   for n >= 2, m = t mod 2(n - 1) (non-negative), then m < n ? m : 2(n - 1) - m; for n = 1 every index maps to 0.
 *   Each holds for any t, so for a side smaller than the kernel's radius too (several folds).
 * Quantiser: a table is made from a non-negative real kernel k of positive sum by one rule, in float64 on the host
 *   (training.quantise_blur_kernel): q = k / sum(k) * 65536, W = floor(q), and the 65536 - sum(W) units left are
 *   handed out one each to the taps of largest fractional part q - W, ties to the lower flat index.  A table that
 *   already sums to 65536 passes through unchanged.
 *
 * src and dst: HWC uint8 at any byte address, distinct buffers; element offsets are 64-bit.  Each output byte is
 * written once; no atomics; one launch. */
#define GRR_BLUR_MAX_SIDE 31
#define GRR_BLUR_ONE 65536

/* 1 where grr_u8_blur takes the image: C in 1..4, H, W >= 1, C H W < 2^31. */
int grr_u8_blur_supported(int C, int H, int W);
/* One image.  weights: int32 [kh * kw] on the device.  GRR_ERR_INVALID_ARG for an even or out-of-range side or a
 * boundary outside 0..2, before any launch; GRR_ERR_UNSUPPORTED where the query says 0. */
grr_status grr_u8_blur(const uint8_t* src, int H, int W, int C, uint8_t* dst, const int32_t* weights, int kh, int kw,
                       int boundary, void* stream);
/* Every image of an arena of C-channel pictures into the same place of dst_arena (both of elems elements), one launch:
 * image i is row i of table (int64 [n_img, 3] on the device, 8-byte aligned, rows (element offset, H, W)), blurred by
 * kernel kernel_of[i] (int32 [n_img] on the device).  weights: int32 [n_kernels, 31 * 31] on the device, each kernel
 * row-major in the top-left kh x kw of its 31 x 31 slot; sizes: int32 [n_kernels, 2] on the device, rows (kh, kw).
 * max_h, max_w bound every image's sides.  Device data is clamped -- offsets into the arena, sides into
 * [1, max_h] x [1, max_w], kernel indices into [0, n_kernels), kernel sides into 1..31 and made odd, weights into
 * [0, 65536], every element index read into [0, elems), a write at or past elems dropped, the result min-ed to 255 --
 * so a bad table gives wrong pixels, never an access outside the two arenas; the caller checks its host copies.
 * n_kernels <= 16 and n_img <= 65535 (one grid row per image), else GRR_ERR_UNSUPPORTED. */
grr_status grr_u8_blur_images(const uint8_t* arena, int64_t elems, const int64_t* table, int n_img, int max_h, int max_w,
                              int C, uint8_t* dst_arena, const int32_t* weights, const int32_t* sizes, int n_kernels,
                              const int32_t* kernel_of, int boundary, void* stream);

/* ---- inpainting (csrc/inpaint_ops.hip): a random share of the pixels is missing and an initial fill stands in for
 * them.  The mask must be fresh per sample and per epoch and lies under a spatial filter, so the degradation is made
 * at batch time, inside the patch kernel: cut, mask, fill, turn, one launch.  No floating point appears in the
 * definition.
 *
 * Per sample s: a table row (img, row, col, mode) and a sample id, as grr_patch_batch takes them; keep[s], an int32
 *   on the device, clamped into [0, GRR_MASK_ONE]: the known share of the pixels in units of 2^-24.
 * Call-wide: C in 1..4; fill 0 (zero) or 1 (conv); hole, a byte 0..255; a uint64 seed; a weight table w[kh][kw] of
 *   uint8 on the device, row-major, kh and kw odd, in 1..GRR_MASK_MAX_SIDE.
 * Window: (ph + 14) x (pw + 14), whatever the table's sides: the mask is a function of (seed, id, ph, pw) alone, never
 *   of the fill.  Window position (wy, wx) has image coordinates Y = row + wy - 7, X = col + wx - 7 and reads picture
 *   pixel (sym(Y, H), sym(X, W)), sym grr_patch_batch's edge-repeating mirror taken for any index (t = r mod 2n,
 *   non-negative; t < n ? t : 2n - 1 - t) -- not the parity-keeping reflection of grr_patch_raw_batch: there is no
 *   colour filter array here.  With every pixel known the outputs equal grr_patch_batch's clean patch bit for bit.
 * Mask: one bit per pixel, shared by the channels.  With e = wy (pw + 14) + wx, block e / 4 is Philox4x32-10 of
 *   counter (e / 4, 1, low32(id), high32(id)) and key (low32(seed), high32(seed)) -- the second counter word is 1
 *   where the noise of grr_patch_batch has 0, so the two streams never share a block -- and the pixel is known if
 *   (x_{e % 4} >> 8) < keep[s].  keep = 2^24 makes every pixel known and keep = 0 none;
 *   in both cases no generator runs.  A mirrored position draws its own bit.
 * Fill: a known pixel passes through, in every channel.  A missing pixel is, for the zero fill, 0 in every channel;
 *   for conv, with ry = kh / 2, rx = kw / 2, k the known bit and v_c the byte of channel c,
 *     den   = sum_{i<kh, j<kw} w[i][j] k(wy + i - ry, wx + j - rx)
 *     num_c = sum_{i<kh, j<kw} w[i][j] k(wy + i - ry, wx + j - rx) v_c(wy + i - ry, wx + j - rx)
 *   and the byte is (2 num_c + den) / (2 den), floor, when den > 0, otherwise hole.  num_c <= 255 den and
 *   den <= 225 * 255, so int32 is exact and the result needs no clamp.  A normalised convolution; the taps stay
 *   within radius 7, so the window's halo is all it reads: the fill itself has no border rule.
 * Outputs: patch pixel (i, j) is window position (i + 7, j + 7), moved by T_mode exactly as grr_patch_batch moves it
 *   (odd quarter turns need ph == pw; an illegal mode is read as mode & 5).  input and target: float32
 *   [n, C, ph, pw], planar, each value float(byte) / 255.0f; mask: float32 [n, 1, ph, pw], 1.0 known and 0.0 missing,
 *   turned the same way; mask == NULL skips it.  A sample does not depend on the batch it is in.
 *
 * arena, arena_elems, C, img_table, n_img, table, sample_ids: as grr_patch_batch takes them.  Every table value is
 * clamped as in grr_patch_batch: a bad table gives wrong pixels, never an access outside the buffers.  No atomics;
 * every output element is written once. */
#define GRR_MASK_HALO 7
#define GRR_MASK_MAX_SIDE 15
#define GRR_MASK_ONE (1 << 24)

/* 1 where grr_patch_mask_batch takes the call: grr_patch_batch_supported(C, n_img, arena_elems, n, ph, pw) and
 * (ph + 14)(pw + 14) < 2^31. */
int grr_patch_mask_batch_supported(int C, int n_img, int64_t arena_elems, int n, int ph, int pw);
/* GRR_ERR_INVALID_ARG for C outside 1..4, an even or out-of-range side, a fill outside 0..1 or a hole outside 0..255,
 * before any launch; GRR_ERR_UNSUPPORTED where the query says 0. */
grr_status grr_patch_mask_batch(const uint8_t* arena, int64_t arena_elems, int C, const int64_t* img_table, int n_img,
                                const int32_t* table, const int64_t* sample_ids, const int32_t* keep /* int32 [n] */,
                                int n, uint64_t seed, int ph, int pw, const uint8_t* weights /* uint8 [kh kw] */, int kh,
                                int kw, int fill, int hole, float* target, float* input, float* mask /* or NULL */,
                                void* stream);
/* 1 where grr_u8_mask_fill takes the picture: C in 1..4, H, W >= 1, C H W < 2^31 and (H + 14)(W + 14) < 2^31. */
int grr_u8_mask_fill_supported(int C, int H, int W);
/* One picture: the same kernel body with row = col = 0, ph = H, pw = W, mode 0 and no device tables.  src, dst: HWC
 * uint8 at any byte address, distinct buffers.  mask_in == NULL: the mask of (seed, sample_id) is drawn with the
 * share keep, the patch form's mask for the same id.  mask_in given (uint8 H x W): nonzero means known; outside the
 * picture mask_in is read by sym, like the pixels; no generator runs.  mask_out (uint8 H x W) carries through
 * mask_in's nonzero values, is 1 for known pixels when the mask is drawn,
 * 2 where this call filled a pixel with den > 0 and 0 where a hole is left: feeding dst and mask_out back in as src and mask_in is a second pass, in which
 * every nonzero is known and the 1s and 2s are kept, and which grows the filled region by one table radius.  The pass
 * loop is the caller's: each pass is one launch with distinct buffers.  GRR_ERR_INVALID_ARG as above and for a keep
 * outside [0, 2^24]. */
grr_status grr_u8_mask_fill(const uint8_t* src, const uint8_t* mask_in /* uint8 H x W, or NULL */, int H, int W, int C,
                            int keep, uint64_t seed, int64_t sample_id, const uint8_t* weights, int kh, int kw, int fill,
                            int hole, uint8_t* dst /* uint8 HWC */, uint8_t* mask_out /* uint8 H x W */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRR_H */
