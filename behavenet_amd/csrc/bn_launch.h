// Internal launcher prototypes (one per kernel family); implemented in the .hip files,
// dispatched from capi.hip.
#pragma once
#include "bn_common.h"

struct GemmArgs {
    const float* A; long sai, sak;
    const float* B; long sbk, sbj;
    float* C; long sci, scj;
    int M, N, K;               // C is M x N, reduction length K
    const float* bias_j;       // nullable, added per column j
    const float* dact_src;     // nullable, same layout as C
    int dact; float slope;
    int accumulate;
    float* part;               // set by bn_launch_gemm: partial tiles of a cross-workgroup split
    int kslice;                // reduction length per workgroup slice
};

// conv_generic.hip
int bn_launch_down_generic(const float* big, const float* w, const float* bias, float* out,
                           const float* dact_src, const BnGeom& g, int act, int dact, float slope,
                           hipStream_t st);
int bn_launch_up_generic(const float* small, const float* w, const float* bias, float* out,
                         const float* dact_src, const BnGeom& g, int act, int dact, float slope,
                         hipStream_t st);
int bn_launch_wgrad_generic(const float* small, const float* big, float* dw, const BnGeom& g,
                            int accumulate, hipStream_t st);
size_t bn_channel_sum_ws_bytes(int N, int C, int npix);
int bn_launch_channel_sum(const float* t, float* db, int N, int C, int npix, int accumulate,
                          void* ws, size_t ws_bytes, hipStream_t st);

// gemm.hip
int bn_launch_gemm(const GemmArgs& a, hipStream_t st, void* ws = nullptr, size_t ws_bytes = 0);
size_t bn_gemm_ws_bytes(int M, int N, int K);
int bn_launch_col_sum(const float* dy, float* db, int M, int N, int accumulate, hipStream_t st);
// nn.Linear in one launch: up to two products (nullable) and the column sums of dy (M x N) into db
// (nullable), side by side in one grid
int bn_launch_linear_jobs(const GemmArgs* g0, const GemmArgs* g1, const float* dy, float* db, int M,
                          int N, int accumulate, void* ws, size_t ws_bytes, hipStream_t st);
size_t bn_linear_jobs_ws_bytes(int M, int N, int K);

// elementwise.hip
int bn_launch_act_fwd(const float* x, float* y, size_t n, int act, float slope, hipStream_t st);
int bn_launch_act_bwd(const float* dy, const float* y, float* dpre, size_t n, int act, float slope,
                      hipStream_t st);
int bn_launch_sqerr_frame_sums(const float* pred, const float* target, const float* mask,
                               float* frame_sums, int N, size_t D, hipStream_t st);
int bn_launch_sqerr_bwd(const float* pred, const float* target, const float* mask, float* dpred,
                        size_t n, float scale, const float* gscale, hipStream_t st);
int bn_launch_scale_frames(float* t, const float* frame_scale, const float* group_scale,
                           const int* group_of_frame, int N, size_t D, hipStream_t st);
int bn_launch_reduce_sum(const float* in, float* out, size_t n, float scale, hipStream_t st);
int bn_launch_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z,
                          size_t n, hipStream_t st);
int bn_launch_kl_rows(const float* mu, const float* logvar, float* kl_rows, int N, int D,
                      hipStream_t st);
int bn_launch_reparam_bwd(const float* dz, const float* z, const float* mu, float* dlogvar,
                          size_t n, hipStream_t st);
int bn_launch_kl_bwd(const float* mu, const float* logvar, float* dmu, float* dlogvar, size_t n,
                     float scale, const float* gscale, hipStream_t st);
int bn_launch_adam(float* p, const float* g, float* m, float* v, float* vmax, size_t n, float lr,
                   float b1, float b2, float eps, float wd, int step, hipStream_t st);
int bn_launch_u8_to_unit_float(const unsigned char* in, float* out, size_t n, hipStream_t st);

// frame_err.hip: per-frame squared error, a frame's summation order a function of D alone
bool bn_frame_sq_err_ok(int N, size_t D);
size_t bn_frame_sq_err_ws_bytes_impl(int N, size_t D);
int bn_launch_frame_sq_err(const float* xhat, const void* target, int target_is_u8, const float* mask, float* out,
                           int N, size_t D, float scale, void* ws, hipStream_t st);
// out[n] = scale * (part[n][0] + .. + part[n][P - 1]), left to right
int bn_launch_frame_err_finish(const float* part, float* out, int N, unsigned P, float scale, hipStream_t st);

// recon_u8.hip: fp32 unit-float frames -> uint8 grey levels (bn_quantise_u8 of bn_common.h), any n
bool bn_unit_float_to_u8_ok(size_t n);
int bn_launch_unit_float_to_u8(const float* in, unsigned char* out, size_t n, hipStream_t st);

// pixel_stats.hip: per-pixel float64 sums over the frames (squared error, mask weight, first and second moment of
// the target) added onto acc (4, D); a pixel's summation order a function of (N, D) alone
bool bn_pixel_stats_ok(int N, size_t D);
size_t bn_pixel_stats_ws_bytes_impl(int N, size_t D);
int bn_launch_pixel_stats(const float* xhat, const void* target, int target_is_u8, const float* mask, int mask_frames,
                          double* acc, int N, size_t D, void* ws, hipStream_t st);

// cond_input.hip: frames (uint8 or fp32) + label coordinates -> the (N, C + L, H, W) fp32 input of a conditional
// encoder, the one-hot maps built in the pass that writes them
bool bn_cond_input_ok(int N, int C, int H, int W, int L);
int bn_launch_cond_input(const void* frames, int frames_is_u8, const float* coords, int ld, int N, int C, int H, int W,
                         int L, float* out, hipStream_t st);

// frame_mosaic.hip: the channels [ch0, ch0 + n_ch) of frames (fp32 unit floats or uint8 grey levels), cropped,
// quantised and tiled side by side into a (T, R Hc, Cc n_ch Wc) uint8 mosaic by a device table of source frames
// (-1: a blank panel)
bool bn_frame_mosaic_ok(int P, int C, int H, int W, int ch0, int n_ch, int y_min, int x_min, int Hc, int Wc, int T,
                        int R, int Cc);
int bn_launch_frame_mosaic(const void* frames, int frames_u8, int P, int C, int H, int W, int ch0, int n_ch, int y_min,
                           int x_min, int Hc, int Wc, const int* src, int T, int R, int Cc, unsigned char* out,
                           hipStream_t st);
// ... and marker boxes into a finished mosaic, in place: the box [y0, y0 + h) x [x0, x0 + w) of every panel whose
// mark is non-zero, clipped to the panel, set to `value`
bool bn_stamp_boxes_ok(int T, int R, int Cc, int Hp, int Wp, int y0, int x0, int h, int w, int value);
int bn_launch_stamp_boxes(unsigned char* movie, int T, int R, int Cc, int Hp, int Wp, const unsigned char* mark, int y0,
                          int x0, int h, int w, int value, hipStream_t st);

// recon_panels.hip: frames, their reconstruction and the residual 0.5 + (orig * mask - recon) as three uint8 panels
// per row, channels side by side, into frames of out_frame_stride >= 3 C H W bytes (one row of a movie)
bool bn_recon_panels_ok(int N, int C, int H, int W, size_t out_frame_stride);
int bn_launch_recon_panels(const void* orig, int orig_u8, const void* recon, int recon_u8, const float* mask,
                           int mask_per_frame, int N, int C, int H, int W, int show_orig, unsigned char* out,
                           size_t out_frame_stride, hipStream_t st);

// column_select.hip: exact per-column order statistics of an fp32 table (n, d) with leading dimension ld, NaNs taking
// no part: the valid counts, and the values at r device ranks a column by a four-digit radix select
bool bn_column_select_ok(int n, int d, int ld, int r);
size_t bn_column_count_ws_bytes_impl(int n, int d);
size_t bn_column_select_ws_bytes_impl(int n, int d, int r);
int bn_launch_column_count(const float* x, int n, int d, int ld, long long* n_valid, void* ws, hipStream_t st);
int bn_launch_column_select(const float* x, int n, int d, int ld, const long long* ranks, int r, float* out, void* ws,
                            hipStream_t st);

// segment_sums.hip: per row segment and column, the count, sum y, sum y^2 and sum (y - p)^2 of the valid entries of
// fp32 tables (n, L) in float64 -- the sums behind the per-trial label R^2 and MSE
bool bn_segment_label_sums_ok(int n, int S, int L);
size_t bn_segment_label_sums_ws_bytes_impl(int n, int S, int L);
int bn_launch_segment_label_sums(const float* pred, int ld_pred, const float* truth, int ld_truth, const float* mask,
                                 int ld_mask, const long long* offsets, int S, int L, int n, double* out, void* ws,
                                 hipStream_t st);
int bn_launch_segment_offsets(const long long* offsets, int count, int n, int* e, hipStream_t st);

// segment_gram.hip: per row segment the augmented second-moment matrix sum a^T a of a = (1, z - c) over the rows of
// an fp32 table (n, D), float64 (S, D + 1, D + 1) -- the sums behind the latent correlation matrices
bool bn_segment_gram_ok(int n, int S, int D);
size_t bn_segment_gram_ws_bytes_impl(int n, int S, int D);
int bn_launch_segment_gram(const float* z, int ld, const float* c, const long long* offsets, int S, int D, int n,
                           double* out, void* ws, hipStream_t st);

// softmax_cv.hip: loss, gradient and held-out score of M multinomial logistic models (S classes, D columns and an
// intercept each) over the rows of an fp32 table, float64 throughout -- the sums behind the session classifier
bool bn_softmax_cv_ok(int n, int D, int S, int M);
size_t bn_softmax_cv_ws_bytes_impl(int n, int D, int S, int M, bool score);
int bn_launch_softmax_cv_lossgrad(const float* z, int ld, const int* y, const int* fold, const double* W,
                                  const int* leave, int n, int D, int S, int M, double* loss, double* grad,
                                  double* count, void* ws, hipStream_t st);
int bn_launch_softmax_cv_score(const float* z, int ld, const int* y, const int* fold, const double* W,
                               const int* leave, int n, int D, int S, int M, double* out, void* ws, hipStream_t st);

// arhmm.hip: the launches of one EM iteration of an autoregressive HMM on an fp32 table (n, D) cut into trials --
// emission log-likelihoods, forward-backward, weighted lagged moments -- and Viterbi, float64 throughout
bool bn_arhmm_ok(int n, int S, int D, int L, int K);
bool bn_hmm_ok(int n, int S, int K);
size_t bn_arhmm_loglik_ws_bytes_impl(int n, int S, int D, int L, int K);
size_t bn_arhmm_moments_ws_bytes_impl(int n, int S, int D, int L, int K);
size_t bn_hmm_forward_backward_ws_bytes_impl(int n, int S, int K);
size_t bn_hmm_viterbi_ws_bytes_impl(int n, int S, int K);
int bn_launch_arhmm_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                           int K, int n, const double* G, const double* cst, double* ll, void* ws, hipStream_t st);
int bn_launch_arhmm_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                            int K, int n, const double* gamma, double* out, double* gamma0, void* ws, hipStream_t st);
int bn_launch_hmm_forward_backward(const double* ll, const long long* offsets, int S, int K, int n,
                                   const double* logP, const double* logpi0, int want, double* gamma, double* xi,
                                   double* loglik, void* ws, hipStream_t st);
int bn_launch_hmm_viterbi(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                          const double* logpi0, int* states, void* ws, hipStream_t st);
// ... and the same for a grid of M models on one table, KT = sum K_m states side by side (XT = sum K_m^2)
bool bn_arhmm_grid_ok(int n, int S, int D, int L, int KT);
bool bn_hmm_grid_ok(int n, int S, int M, int KT, int XT);
size_t bn_arhmm_grid_loglik_ws_bytes_impl(int n, int S, int D, int L, int KT);
size_t bn_arhmm_grid_moments_ws_bytes_impl(int n, int S, int D, int L, int KT);
size_t bn_hmm_grid_forward_backward_ws_bytes_impl(int n, int S, int M, int KT, int XT);
int bn_launch_arhmm_grid_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D,
                                int L, int KT, int n, const double* G, const double* cst, double* ll, void* ws,
                                hipStream_t st);
int bn_launch_arhmm_grid_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D,
                                 int L, int KT, int n, const double* gamma, double* out, double* gamma0, void* ws,
                                 hipStream_t st);
int bn_launch_hmm_grid_forward_backward(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                                        const int* koff, const int* xoff, const int* order, const int* counts,
                                        const double* logP, const double* logpi0, int want, double* gamma, double* xi,
                                        double* loglik, void* ws, hipStream_t st);
// ... and max-sum for every (trial, model) of the grid: states int32 (M, n)
size_t bn_hmm_grid_viterbi_ws_bytes_impl(int n, int S, int M, int KT, int XT);
int bn_launch_hmm_grid_viterbi(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                               const int* koff, const int* xoff, const int* order, const int* counts,
                               const double* logP, const double* logpi0, int* states, void* ws, hipStream_t st);
// ... and the model's generative process from the caller's noise: states from uniforms (or given), latents from normals
size_t bn_arhmm_sample_ws_bytes_impl(int n, int S, int D, int L, int K);
int bn_launch_arhmm_sample(const double* W, const double* C, const double* cdf0, const double* cdf,
                           const long long* offsets, int S, int D, int L, int K, int n, const double* eps,
                           const double* u, const int* states_in, const float* init, int ld_init, double* x,
                           int* states, void* ws, hipStream_t st);
// ... and one-step-ahead predictions: the causal weights p(z_t | x_0 .. x_{t-1}), and sum_k w_t[k] (b_k + A_k history)
size_t bn_hmm_predictive_ws_bytes_impl(int n, int S, int K);
size_t bn_arhmm_predict_ws_bytes_impl(int n, int S, int D, int L, int K);
int bn_launch_hmm_predictive(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                             const double* logpi0, double* w, void* ws, hipStream_t st);
int bn_launch_arhmm_predict(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int n,
                            const double* W, const double* w, double* xhat, void* ws, hipStream_t st);
// ... and exact multi-step forecasts sum_k w_t[k] N_h[k] phi_t, h = 1 .. H, reduced to five sums per horizon, trial and
// dimension in the launch that forms them
size_t bn_arhmm_forecast_sums_ws_bytes_impl(int n, int S, int D, int L, int K, int H);
int bn_launch_arhmm_forecast_sums(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int H,
                                  int n, const double* N, const double* w, double* sums, void* ws, hipStream_t st);

// state_runs.hip: the runs (trial, beg, end, state) of an int32 state table cut into trials, in table order, with
// the frames per state and the in-trial transition counts
bool bn_state_runs_ok(int n, int S, int K);
size_t bn_state_runs_ws_bytes_impl(int n, int S, int K);
int bn_launch_state_runs(const int* states, const long long* offsets, int S, int K, int n, int* runs,
                         long long runs_cap, long long* frames, long long* trans, long long* n_runs, long long* bad,
                         void* ws, hipStream_t st);

// batchnorm.hip
size_t bn_batchnorm_ws_bytes_impl(int N, int C);
int bn_launch_bn_stats(const float* x, float* mean, float* var, int N, int C, int HW, void* ws,
                       hipStream_t st);
int bn_launch_bn_finalize(const float* mean, const float* var, float* invstd, float* running_mean,
                          float* running_var, int C, float eps, float momentum, float unbias,
                          hipStream_t st);
int bn_launch_bn_act_fwd(const float* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float* y, int N, int C, int HW,
                         int act, float slope, hipStream_t st);
int bn_launch_bn_act_bwd(const float* x, const float* y, const float* dy, const float* mean,
                         const float* invstd, const float* gamma, float* dx, float* dgamma,
                         float* dbeta, int accumulate, int batch_stats, int N, int C, int HW,
                         int act, float slope, void* ws, hipStream_t st);

int bn_launch_bn_moment(const float* x, const float* center, float* sums, int N, int C, int HW,
                        void* ws, hipStream_t st);
int bn_launch_bn_bwd_reduce(const float* x, const float* y, const float* dy, const float* mean,
                            const float* invstd, float* sum_dz, float* sum_dzx, int N, int C,
                            int HW, int act, float slope, void* ws, hipStream_t st);
int bn_launch_bn_train_fwd_chunks(const float* x, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, long long* num_batches,
                                  float* y, float* mean, float* invstd, const int* bounds,
                                  const float* factors, int n_chunks, int C, int HW, float eps, int act,
                                  float slope, void* ws, hipStream_t st);
int bn_launch_bn_act_bwd_chunks(const float* x, const float* y, const float* dy, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, float* dx,
                                float* dgamma, float* dbeta, int accumulate, const int* bounds,
                                int n_chunks, int C, int HW, int act, float slope, void* ws,
                                hipStream_t st);
int bn_launch_bn_bwd_apply(const float* x, const float* y, const float* dy, const float* mean,
                           const float* invstd, const float* gamma, const float* sum_dz,
                           const float* sum_dzx, float* dx, int N, int C, int HW, float inv_count,
                           int act, float slope, hipStream_t st);

// decomposed_kl.hip
int bn_launch_dkl_fwd(const float* z, const float* mu, const float* lv, float* out3,
                      float* log_qz, float* lse, float* terms, int N, int D, hipStream_t st);
int bn_launch_dkl_bwd(const float* z, const float* mu, const float* lv, const float* log_qz,
                      const float* lse, const float* g3, float* dz, float* dmu, float* dlv, int N,
                      int D, hipStream_t st);

// conv_pad.hip: zero-padded copies for geometries off the fast paths, stride-5 1x1 maps as a GEMM
int bn_launch_pad2d(const float* src, float* dst, size_t planes, int H, int W, int Hp, int Wp,
                    int oh, int ow, hipStream_t st);
int bn_launch_crop2d(const float* src, float* dst, size_t planes, int H, int W, int Hp, int Wp,
                     int oh, int ow, const float* dact_src, int dact, float slope, hipStream_t st);
// spatial tiles with halos (maps larger than the specialised kernels take): one axis of the tiling.
// Tile k holds source coordinates step * k - v0 + i for i in [0, D); its elements [v0, v0 + V) are
// the ones it OWNS (every source coordinate is owned by exactly one tile: V == step when T > 1).
struct BnTileAxis { int T, step, v0, V, D; };
// src (N, C, H, W) -> dst ((N Th Tw), C, Dh, Dw), zeros outside the map; masked: owned elements only
int bn_launch_tile_gather(const float* src, float* dst, int N, int C, int H, int W, BnTileAxis th,
                          BnTileAxis tw, int masked, hipStream_t st);
// dst (N, C, H, W) <- the owning tile's element, times act'(dact_src) when given
int bn_launch_tile_scatter(const float* src, float* dst, int N, int C, int H, int W, BnTileAxis th,
                           BnTileAxis tw, const float* dact_src, int dact, float slope,
                           hipStream_t st);
// dst[n][c0d + c][i] <- src[n][c0s + c][i], c < Cg, i < HW (a multiple of 4); optional act' mask
int bn_launch_chan_copy(const float* src, float* dst, int N, int Csrc, int c0s, int Cdst, int c0d,
                        int Cg, int HW, const float* dact_src, int dact, float slope, hipStream_t st);
// im2col + GEMM for whatever no specialised kernel (or detour onto one) serves
bool bn_col_ok(const BnGeom& g);
size_t bn_col_ws_bytes(const BnGeom& g);
int bn_launch_col_down(const float* big, const float* w, const float* bias, float* out,
                       const float* dact_src, const BnGeom& g, int act, int dact, float slope, void* ws,
                       size_t ws_bytes, hipStream_t st);
int bn_launch_col_up(const float* small, const float* w, const float* bias, float* out,
                     const float* dact_src, const BnGeom& g, int act, int dact, float slope, void* ws,
                     size_t ws_bytes, hipStream_t st);
int bn_launch_col_wgrad(const float* small, const float* big, float* dw, const BnGeom& g, int accumulate,
                        void* ws, size_t ws_bytes, hipStream_t st, float* db, int bias_side,
                        bool* bias_done);
// kernels smaller than 5x5 embedded in 5x5 taps (weights [pairs][R][S] <-> [pairs][5][5])
#define BN_PAD_TAPS_MAX_JOBS 16
struct BnPadTapsJob { const float* w; float* w5; unsigned pairs; int R, S, dr, ds, blocks; };
struct BnPadTapsJobs { int n; BnPadTapsJob job[BN_PAD_TAPS_MAX_JOBS]; };
int bn_launch_pad_taps_jobs(BnPadTapsJobs* p, hipStream_t st);
int bn_launch_pad_taps(const float* w, float* w5, size_t pairs, int R, int S, hipStream_t st, int dr = 0,
                       int ds = 0);
int bn_launch_flip_taps(const float* w, float* wf, int Cs, int Cb, int RS, hipStream_t st);
int bn_launch_crop_taps(const float* dw5, float* dw, size_t pairs, int R, int S, int accumulate,
                        hipStream_t st, const float* db5 = nullptr, float* db = nullptr, int nb = 0,
                        int dr = 0, int ds = 0);
// kernels larger than 5x5 with stride 2 as stride-1 5x5 layers on the phases of the big map (conv_pad.hip)
int bn_launch_space_to_depth(const float* x, float* X, int N, int C, int Hy, int Wy, hipStream_t st);
int bn_launch_bigk_phase_pack(const float* w, float* w1, int Cs, int Cb, int R, int S, const int* kr, const int* ofr,
                              const int* kc, const int* ofc, int sgn, int phase_out, hipStream_t st);
int bn_launch_bigk_phase_unpack(const float* dw1, float* dw, int Cs, int Cb, int R, int S, const int* kr,
                                const int* ofr, const int* kc, const int* ofc, int accumulate, const float* db5,
                                float* db, int nb, hipStream_t st);
// ... and with stride 1: four shifted copies of the big map against the four blocks of taps
int bn_launch_shift_cat(const float* x, float* y, int N, int C, int H, int W, int Ho, int Wo, int dr0, int dr1,
                        int dc0, int dc1, hipStream_t st);
int bn_launch_bigk_pack(const float* w, float* w5, int Cs, int Cb, int R, int S, int L0r, int L0c, hipStream_t st);
int bn_launch_bigk_unpack(const float* dw5, float* dw, int Cs, int Cb, int R, int S, int L0r, int L0c,
                          int accumulate, const float* db5, float* db, int nb, hipStream_t st);
int bn_launch_depth_to_space(const float* y, float* out, const float* bias, const float* dact_src, int N, int C,
                             int Hy, int Wy, int act, int dact, float slope, hipStream_t st);
bool bn_s5_down_small_ok(const BnGeom& g);
size_t bn_s5_down_small_ws_bytes(const BnGeom& g);
int bn_launch_s5_down_small(const float* big, const float* w, const float* bias, float* out,
                          const float* dact_src, const BnGeom& g, int act, int dact, float slope,
                          void* ws, size_t ws_bytes, hipStream_t st);

// conv_bf16.hip: the inference-only bf16 encoder stack (operands bf16, accumulation fp32).  The twelve integers
// of the C ABI as they are: (C, H, W) -> (K, P, Q), padding (pt, pl) on top / left, bottom / right implied.
struct BnBf16Geom { int N, C, H, W, K, R, S, stride, pt, pl, P, Q; };
bool bn_bf16_first_ok(const BnBf16Geom& g);
bool bn_bf16_conv_ok(const BnBf16Geom& g);
int bn_launch_bf16_pack_w(const float* w, void* wp, const BnBf16Geom& g, hipStream_t st);
int bn_launch_bf16_first(const void* x, int x_is_u8, const float* w, const float* bias, void* y, const BnBf16Geom& g,
                         int act, float slope, hipStream_t st);
int bn_launch_bf16_conv(const void* x, const void* wp, const float* bias, void* y, int out_f32, const BnBf16Geom& g,
                        int act, float slope, hipStream_t st);

// conv_bf16_dec.hip: the inference-only bf16 decoder stack.  BnBf16Geom read as a transposed convolution:
// (C, H, W) -> (K, P, Q), (pt, pl) the crop on top / left of the full-size map.
bool bn_bf16_convT_ok(const BnBf16Geom& g);
bool bn_bf16_lastT_ok(const BnBf16Geom& g);
int bn_launch_bf16_packT_w(const float* w, void* wp, int Ci, int Co, int R, int S, hipStream_t st);
int bn_launch_bf16_to_nhwc(const float* x, void* y, int N, int C, int H, int W, hipStream_t st);
int bn_launch_bf16_convT(const void* x, const void* wp, const float* bias, void* y, int out_f32, const BnBf16Geom& g,
                         int act, float slope, hipStream_t st);
int bn_launch_bf16_lastT(const void* x, const float* w, const float* bias, float* y, const BnBf16Geom& g, int act,
                         float slope, hipStream_t st);
// the layer onto the frame fused with the per-frame squared error (x_hat is not written); serves what bn_bf16_lastT_ok
// serves; `ws`: bn_bf16_lastT_sqerr_ws_bytes(g) bytes
size_t bn_bf16_lastT_sqerr_ws_bytes(const BnBf16Geom& g);
int bn_launch_bf16_lastT_sqerr(const void* x, const float* w, const float* bias, const void* target, int target_is_u8,
                               const float* mask, float* out, const BnBf16Geom& g, int act, float slope, float scale,
                               void* ws, hipStream_t st);
// the layer onto the frame with bn_quantise_u8 in its epilogue: y uint8 (N, K, P, Q), the fp32 x_hat is not
// written; serves what bn_bf16_lastT_ok serves
int bn_launch_bf16_lastT_u8(const void* x, const float* w, const float* bias, unsigned char* y, const BnBf16Geom& g,
                            int act, float slope, hipStream_t st);
