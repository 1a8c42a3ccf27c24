/*
 * behavenet_hip.h -- C ABI of libbehavenet_hip.so: the MI355X (gfx950) kernels underneath the
 * BehaveNet conv-autoencoder hot path.
 *
 * The reference (themattinthehatt/behavenet) is pure Python and has no FFI of its own: its hot
 * path bottoms out in third-party ATen operators called from `torch.nn` modules.  Each entry
 * point below replaces one such operator call site (cited as reference file:line) with a
 * hand-written HIP kernel.  Everything above this boundary is Python glue.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - tensors are fp32, contiguous, NCHW (images) or row-major (matrices); the fast convolution
 *     kernels need 16-byte aligned base pointers (any allocator gives that; a view at an odd
 *     offset is served by the shape-agnostic kernels instead);
 *   - the caller owns every buffer; the library never allocates, frees or synchronises;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - return value: 0 on success, a positive hipError_t if a launch failed, a negative
 *     BN_E_* code for an argument/shape error.  No entry point throws or exits.
 *   - "accumulate != 0" means the gradient outputs are added to (+=) instead of overwritten,
 *     which is how the reference accumulates over its 200-frame chunks (aes.py:751-771).
 *
 * Deliberately NOT in this ABI: collectives.  SURVEY.md section 8(b) sketched
 * bn_comm_init / bn_allreduce_grads / bn_comm_destroy; they do not exist.  The gradient
 * exchange of the data-parallel path (one flat gradient arena, bucketed, overlapped with the
 * backward pass) is issued from Python through torch.distributed (backend "nccl" = RCCL over
 * xGMI; behavenet_amd/fitting/distributed.py), which already owns the communicator, its
 * streams and the rendezvous.  A second RCCL communicator behind this library would duplicate
 * that state for no kernel of this path: the library only ever sees device pointers, and the
 * all-reduce operates in place on the same arena the backward kernels accumulate into.
 */
#ifndef BEHAVENET_HIP_H
#define BEHAVENET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN_E_BADARG   (-1)  /* null pointer / non-positive size */
#define BN_E_SHAPE    (-2)  /* geometry not representable (e.g. kernel larger than supported) */
#define BN_E_WORKSPACE (-3) /* caller-provided workspace too small */

/* activation codes for fused epilogues */
#define BN_ACT_NONE    0
#define BN_ACT_LRELU   1    /* LeakyReLU(slope)  -- aes.py:114,341 */
#define BN_ACT_SIGMOID 2    /* Sigmoid           -- aes.py:330 */

typedef void* bn_stream_t;

/* library / build info */
int         bn_version(void);                 /* ABI version, currently 1 */
const char* bn_build_arch(void);              /* "gfx950" */
const char* bn_error_string(int code);        /* static string for a BN_E_* / hip code */

/* ------------------------------------------------------------------------------------------
 * Scratch memory.  Some kernels split their reduction dimension over workgroups and combine
 * the partial results in a second, fixed-order pass (deterministic; no atomics).  The caller
 * owns the scratch: ask how much a call needs (0 is common) and pass at least that much.
 * `op` is one of BN_OP_*; the twelve ints are the same geometry arguments, in the same order,
 * as the entry point's.
 * ------------------------------------------------------------------------------------------ */
#define BN_OP_CONV_FWD    1
#define BN_OP_CONV_BWD_D  2
#define BN_OP_CONV_BWD_W  3
#define BN_OP_CONVT_FWD   4
#define BN_OP_CONVT_BWD_D 5
#define BN_OP_CONVT_BWD_W 6
/* Test hook: on != 0 routes every convolution through the shape-agnostic kernels (so the
 * specialised ones can be cross-checked on the device).  Returns the previous setting (initially 0). */
int bn_set_force_generic(int on);
/* Test hook: stride-1 layers with kernels larger than 5x5 run on four shifted copies of their big map, frames in
 * blocks whose copies stay below `bytes` (default and maximum 0x70000000: the kernels' 32-bit offsets); a small value
 * makes a few frames exercise the block loop.  0 restores the default.  Returns the previous setting. */
size_t bn_set_bigk1_block_bytes(size_t bytes);
size_t bn_conv_ws_bytes(int op, int N, int C, int H, int W, int K, int R, int S, int stride,
                        int off_t, int off_l, int P, int Q);
/* Kernels smaller than 5x5 (the reference's architecture search draws 3x3; configs/ae_jsons/ae_arch_2.json has 4x4:
 * models/ae_model_architecture_generator.py:90-100 of the reference) run on the 5x5 kernel families with
 * their taps embedded in 5x5 ones.  Every forward / data-gradient entry point makes that copy itself; a caller that
 * runs a whole stack of layers (and both roles of each) can make the copies of all layers in ONE launch instead:
 *   bn_conv_taps_bytes  bytes of the 5x5 copy if `op` (BN_OP_CONV_FWD / _BWD_D, BN_OP_CONVT_FWD / _BWD_D) pads this
 *                       geometry's taps, 0 if it does not (the copy is the same for the two ops of a layer)
 *   bn_conv_taps_pad    w5[j] <- 5x5 copy of w[j], j < n, one launch; geoms = n x 13 ints (op + the twelve geometry
 *                       arguments); BN_E_SHAPE if an op does not pad
 * The four forward / data-gradient entry points then take that copy as `w5`, directly after `w`.  w5 = NULL: the
 * call pads for itself.  A copy is read only where the call is not on the shape-agnostic path (bn_set_force_generic,
 * operands off 16 bytes), `w5` is 16-byte aligned and the op pads this geometry's taps (bn_conv_taps_bytes != 0);
 * anywhere else -- any 5x5 layer, say -- it is ignored, which is not an error.  Nothing is kept between calls.
 * The caller's one obligation: `w5` was made by bn_conv_taps_pad from the CURRENT contents of `w`, for this geometry
 * and this role pair, and is made again after every update of `w` -- in-place updates that no version counter sees
 * (a flat-arena Adam step) included.  The library cannot check this and does not try. */
size_t bn_conv_taps_bytes(int op, int N, int C, int H, int W, int K, int R, int S, int stride,
                          int off_t, int off_l, int P, int Q);
int bn_conv_taps_pad(int n, const float* const* w, float* const* w5, const int* geoms, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Convolution (replaces ZeroPad2d + nn.Conv2d + LeakyReLU, aes.py:81-86,113-114,145-155).
 *   y[n,k,p,q] = act( b[k] + sum_{c,r,s} x[n,c,p*stride+r-pad_t,q*stride+s-pad_l] * w[k,c,r,s] )
 * reads outside [0,H)x[0,W) are zero, so TF-"same" asymmetric padding needs no padded copy.
 * x:(N,C,H,W) w:(K,C,R,S) w5: NULL or the 5x5 copy of w (above)  b:(K) or NULL  y:(N,K,P,Q)
 * ------------------------------------------------------------------------------------------ */
int bn_conv2d_fwd(const float* x, const float* w, const float* w5, const float* b, float* y,
                  int N, int C, int H, int W, int K, int R, int S, int stride,
                  int pad_t, int pad_l, int P, int Q,
                  int act, float slope, void* ws, size_t ws_bytes, bn_stream_t stream);

/* dx[n,c,h,w] = act'(dact_src[n,c,h,w]) * sum_{k,r,s} dy[n,k,p,q] * w[k,c,r,s],
 * p*stride+r-pad_t == h.  `dy` is the gradient w.r.t. the PRE-activation of this layer.
 * `dact_src` (nullable) is the saved post-activation input of this layer (= output of the layer
 * below); when given, the derivative of the lower layer's activation `dact` is applied in the
 * epilogue so dx is the lower layer's pre-activation gradient (autograd of aes.py:203-211). */
int bn_conv2d_bwd_data(const float* dy, const float* w, const float* w5, float* dx, const float* dact_src,
                       int N, int C, int H, int W, int K, int R, int S, int stride,
                       int pad_t, int pad_l, int P, int Q,
                       int dact, float slope, void* ws, size_t ws_bytes, bn_stream_t stream);

/* dw[k,c,r,s] (+)= sum_{n,p,q} dy[n,k,p,q] * x[n,c,p*stride+r-pad_t,q*stride+s-pad_l]
 * db[k]       (+)= sum_{n,p,q} dy[n,k,p,q]                      (db nullable) */
int bn_conv2d_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                         int N, int C, int H, int W, int K, int R, int S, int stride,
                         int pad_t, int pad_l, int P, int Q,
                         int accumulate, void* ws, size_t ws_bytes, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Transposed convolution (replaces nn.ConvTranspose2d + crop F.pad(x,[-l,-r,-t,-b]) +
 * LeakyReLU/Sigmoid, aes.py:315-321,326-341,466-470).  The crop (or torch `padding`) is folded
 * into the output index range; the un-cropped tensor is never materialised:
 *   y[n,co,h,w] = act( b[co] + sum_{ci,r,s} x[n,ci,p,q] * w[ci,co,r,s] ),
 *   p*stride + r == h + crop_t,  q*stride + s == w + crop_l,  0<=h<Ho, 0<=w<Wo.
 * x:(N,Ci,Hi,Wi) w:(Ci,Co,R,S) w5: NULL or the 5x5 copy of w  b:(Co) or NULL  y:(N,Co,Ho,Wo)
 * ------------------------------------------------------------------------------------------ */
int bn_convT2d_fwd(const float* x, const float* w, const float* w5, const float* b, float* y,
                   int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                   int crop_t, int crop_l, int Ho, int Wo,
                   int act, float slope, void* ws, size_t ws_bytes, bn_stream_t stream);

/* dx[n,ci,p,q] = act'(dact_src[n,ci,p,q]) * sum_{co,r,s} dy[n,co,p*stride+r-crop_t,...] * w[ci,co,r,s] */
int bn_convT2d_bwd_data(const float* dy, const float* w, const float* w5, float* dx, const float* dact_src,
                        int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                        int crop_t, int crop_l, int Ho, int Wo,
                        int dact, float slope, void* ws, size_t ws_bytes, bn_stream_t stream);

/* dw[ci,co,r,s] (+)= sum_{n,p,q} x[n,ci,p,q] * dy[n,co,p*stride+r-crop_t,q*stride+s-crop_l]
 * db[co]        (+)= sum_{n,h,w} dy[n,co,h,w] */
int bn_convT2d_bwd_weight(const float* x, const float* dy, float* dw, float* db,
                          int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                          int crop_t, int crop_l, int Ho, int Wo,
                          int accumulate, void* ws, size_t ws_bytes, bn_stream_t stream);

/* dpre[i] = dy[i] * act'(y[i]) where y is the saved POST-activation output
 * (autograd of LeakyReLU / Sigmoid at the top of a conv stack).  In-place (dpre == dy) allowed. */
/* y = act(x)  (the Sigmoid after the optional dense last decoder layer, aes.py:345-359) */
int bn_act_fwd(const float* x, float* y, size_t n, int act, float slope, bn_stream_t stream);
int bn_act_bwd(const float* dy, const float* y, float* dpre, size_t n,
               int act, float slope, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * nn.MaxPool2d(return_indices=True, ceil_mode) / nn.MaxUnpool2d of 'max_pooling' architectures
 * (aes.py:99-110,196-208,281-294,460-464).  planes = N*C; x: planes x (H,W); y: planes x (Ho,Wo);
 * idx: int32 position h*W+w of each maximum inside its (H,W) plane (torch's convention; ties go
 * to the first maximum in row-major window order).  The unpool pair works on flat planes:
 * in_plane = pooled H*W, out_plane = H*W of the tensor that was pooled.
 * ------------------------------------------------------------------------------------------ */
int bn_maxpool2d_fwd(const float* x, float* y, int* idx, int planes, int H, int W, int Ho, int Wo,
                     int k, int stride, int pad_t, int pad_l, bn_stream_t stream);
int bn_maxpool2d_bwd(const float* dy, const int* idx, float* dx, int planes, int H, int W,
                     int Ho, int Wo, int k, int stride, int pad_t, int pad_l, bn_stream_t stream);
/* Conv2d + the 2x2 / stride-2 max pooling + the activation behind it in ONE kernel (the reference's conv -> pool ->
 * LeakyReLU order, aes.py:200-211): y:(N,K,P/2,Q/2), idx:(N,K,P/2,Q/2) int32 = h * Q + w of each window's winner in
 * the (P, Q) plane of the convolution's output (torch's MaxPool2d(return_indices) convention, first maximum in row-major
 * window order) -- that output itself is never written.  Served for the stride-1 5x5 layers of a max-pooling architecture
 * on even maps: from 1 or 2 input channels onto a multiple of 16, and from a multiple of 4 onto a multiple of 32 where the
 * matrix-core kernel's tile is whole even row blocks (bn_conv2d_pool2_act_ok); BN_E_SHAPE otherwise
 * (the caller then runs bn_conv2d_fwd and bn_maxpool2d_act_fwd).  Backward: bn_maxpool2d_act_bwd on (y, idx), then the
 * layer's own weight gradient. */
int bn_conv2d_pool2_act_fwd(const float* x, const float* w, const float* b, float* y, int* idx,
                            int N, int C, int H, int W, int K, int R, int S, int stride,
                            int pad_t, int pad_l, int P, int Q, int act, float slope, bn_stream_t stream);
/* 1 if bn_conv2d_pool2_act_fwd serves this geometry (16-byte aligned operands assumed), else 0 */
int bn_conv2d_pool2_act_ok(int N, int C, int H, int W, int K, int R, int S, int stride,
                           int pad_t, int pad_l, int P, int Q);
/* Weight (+ bias, db nullable) gradient of such a layer straight from the POOLED side: dy, y (the saved output of
 * bn_conv2d_pool2_act_fwd) and idx are (N,K,P/2,Q/2); dw (+)= sum_n,windows dy act'(y) x[winner + tap], db (+)= sum dy act'(y).
 * The dense gradient of the convolution's output is never built.  Served for 1 or 2 input channels and 16 / 32 / 64 output
 * channels (the first layer); the scratch query returns 0 where it is not, the call BN_E_SHAPE. */
size_t bn_conv2d_pool2_bwd_weight_ws_bytes(int N, int C, int H, int W, int K, int R, int S, int stride,
                                           int pad_t, int pad_l, int P, int Q);
int bn_conv2d_pool2_bwd_weight(const float* x, const float* dy, const float* y, const int* idx, float* dw, float* db,
                               int N, int C, int H, int W, int K, int R, int S, int stride,
                               int pad_t, int pad_l, int P, int Q, int act, float slope, int accumulate,
                               void* ws, size_t ws_bytes, bn_stream_t stream);
/* 2x2 / stride-2 / unpadded max pooling of an even map WITH the activation that follows it (aes.py:204-211: conv ->
 * pool -> LeakyReLU), one pass each way: y = act(max), idx as bn_maxpool2d_fwd; dx = spread(dy * act'(y)).
 * BN_E_SHAPE if W / 2 is odd or a pointer is not 16-byte aligned (use bn_maxpool2d_fwd + the activation then). */
int bn_maxpool2d_act_fwd(const float* x, float* y, int* idx, int planes, int H, int W, int act, float slope,
                         bn_stream_t stream);
int bn_maxpool2d_act_bwd(const float* dy, const float* y, const int* idx, float* dx, int planes, int H, int W,
                         int act, float slope, bn_stream_t stream);
int bn_maxunpool2d_fwd(const float* x, const int* idx, float* y, int planes, int in_plane,
                       int out_plane, bn_stream_t stream);
/* The same for the indices of a 2x2 / stride-2 / unpadded pooling of a (2 Hi) x (2 Wi) map (every index lies inside its
 * own window -- the caller vouches for it; what nn.MaxPool2d(2, return_indices=True) hands to the decoder,
 * aes.py:204-207,460-464): one pass without the memset.  BN_E_SHAPE if Wi is odd or a pointer is not 16-byte aligned. */
int bn_maxunpool2d_fwd_k2(const float* x, const int* idx, float* y, int planes, int Hi, int Wi, bn_stream_t stream);
int bn_maxunpool2d_bwd(const float* dy, const int* idx, float* dx, int planes, int in_plane,
                       int out_plane, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d + activation for `ae_batch_norm = 1` architectures (replaces nn.BatchNorm2d +
 * LeakyReLU, aes.py:90-97,113-114,332-341).  x,y,dy,dx: (N,C,HW) fp32; per-channel vectors: (C).
 *   stats:    mean[c], var[c] (biased) over (N, HW) -- two-pass, deterministic
 *   finalize: invstd = 1/sqrt(var+eps); running = (1-momentum)*running + momentum*{mean,
 *             var*unbias}  (running_* nullable; pass momentum = 1/num_batches_tracked for
 *             nn.BatchNorm2d(momentum=None))
 *   act_fwd:  y = act((x-mean)*invstd*gamma + beta)      (eval mode: pass the running stats)
 *   act_bwd:  dy is the gradient w.r.t. y; dx w.r.t. x; dgamma/dbeta (+)= their sums;
 *             batch_stats=1 when mean/invstd are the batch's own (train mode), 0 when they are
 *             the running statistics (constants w.r.t. x)
 * ------------------------------------------------------------------------------------------ */
size_t bn_batchnorm_ws_bytes(int N, int C);
int bn_batchnorm_stats(const float* x, float* mean, float* var, int N, int C, int HW,
                       void* ws, size_t ws_bytes, bn_stream_t stream);
int bn_batchnorm_finalize(const float* mean, const float* var, float* invstd,
                          float* running_mean, float* running_var, int C, float eps,
                          float momentum, float unbias, bn_stream_t stream);
int bn_batchnorm_act_fwd(const float* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float* y, int N, int C, int HW,
                         int act, float slope, bn_stream_t stream);
int bn_batchnorm_act_bwd(const float* x, const float* y, const float* dy, const float* mean,
                         const float* invstd, const float* gamma, float* dx, float* dgamma,
                         float* dbeta, int accumulate, int batch_stats, int N, int C, int HW,
                         int act, float slope, void* ws, size_t ws_bytes, bn_stream_t stream);

/* The same two passes for a batch whose statistics are per CHUNK of frames (rows [bounds[2i],
 * bounds[2i+1]) of x, in order -- the reference runs its 200-frame chunks one after another through
 * nn.BatchNorm2d, aes.py:748-771 with :90-97): one call per layer.  mean / invstd: [n_chunks][C];
 * factors[i]: the running-estimate factor of chunk i's update (momentum, or 1 / num_batches_tracked);
 * bounds, factors: host arrays.  ws: bn_batchnorm_ws_bytes(largest chunk, C).
 * Round 4: both moments in ONE pass over x (shifted sums around the chunk's first value of the channel),
 * one small launch for mean / invstd / the running estimates / the device counter
 * num_batches_tracked (+= n_chunks; NULL: none, nn.BatchNorm2d's int64 buffer); the backward pass with
 * y == NULL (identity / LeakyReLU) rebuilds the sign of the activation's input from x through
 * (gamma, beta) with the forward pass's own fused multiply-adds instead of reading y back. */
int bn_batchnorm_train_fwd_chunks(const float* x, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var,
                                  long long* num_batches_tracked, float* y, float* mean,
                                  float* invstd, const int* bounds, const float* factors,
                                  int n_chunks, int C, int HW, float eps, int act, float slope,
                                  void* ws, size_t ws_bytes, bn_stream_t stream);
int bn_batchnorm_act_bwd_chunks(const float* x, const float* y, const float* dy, const float* mean,
                                const float* invstd, const float* gamma, const float* beta,
                                float* dx, float* dgamma, float* dbeta, int accumulate,
                                const int* bounds, int n_chunks, int C, int HW, int act, float slope,
                                void* ws, size_t ws_bytes, bn_stream_t stream);

/* Split forms of the two reductions above for statistics taken over ALL ranks' frames (frame-sharded
 * data parallelism; the reference's single-device nn.BatchNorm2d sees the whole chunk, aes.py:90-97):
 * the caller all-reduces the per-channel SUMS between the passes.
 *   bn_batchnorm_moment:     sums[c] = sum x            (center == NULL)
 *                            sums[c] = sum (x-center[c])^2   -- NOT divided by the count
 *   bn_batchnorm_bwd_reduce: sum_dz[c] = sum dy act'(y),  sum_dzx[c] = sum dy act'(y) xhat
 *   bn_batchnorm_bwd_apply:  dx = gamma invstd (dz - sum_dz inv_count - xhat sum_dzx inv_count)
 * ws: bn_batchnorm_ws_bytes(N, C). */
int bn_batchnorm_moment(const float* x, const float* center, float* sums, int N, int C, int HW,
                        void* ws, size_t ws_bytes, bn_stream_t stream);
int bn_batchnorm_bwd_reduce(const float* x, const float* y, const float* dy, const float* mean,
                            const float* invstd, float* sum_dz, float* sum_dzx, int N, int C,
                            int HW, int act, float slope, void* ws, size_t ws_bytes,
                            bn_stream_t stream);
int bn_batchnorm_bwd_apply(const float* x, const float* y, const float* dy, const float* mean,
                           const float* invstd, const float* gamma, const float* sum_dz,
                           const float* sum_dzx, float* dx, int N, int C, int HW, float inv_count,
                           int act, float slope, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense latent projections (replaces nn.Linear, aes.py:121,125,266 and the PS-VAE heads
 * vaes.py:1288-1302).  MFMA (v_mfma_f32_32x32x2_f32: exact fp32).
 *   y[m,n] = b[n] + sum_k x[m,k] * w[n,k]        x:(M,K) w:(N,K) b:(N) or NULL  y:(M,N)
 *   ws: scratch of bn_linear_ws_bytes(M, K, N) bytes (may be NULL / 0: then a long reduction
 *       feeding few output tiles is not split over workgroups)
 * ------------------------------------------------------------------------------------------ */
size_t bn_linear_ws_bytes(int M, int K, int N);
int bn_linear_fwd(const float* x, const float* w, const float* b, float* y,
                  int M, int K, int N, void* ws, size_t ws_bytes, bn_stream_t stream);
/* dx[m,k] = act'(dact_src[m,k]) * sum_n dy[m,n] w[n,k]   (dx, dact_src nullable)
 * dw[n,k] (+)= sum_m dy[m,n] x[m,k]   db[n] (+)= sum_m dy[m,n]   (dw, db nullable) */
int bn_linear_bwd(const float* x, const float* w, const float* dy,
                  float* dx, const float* dact_src, int dact, float slope,
                  float* dw, float* db, int accumulate,
                  int M, int K, int N, void* ws, size_t ws_bytes, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pixel losses (replaces losses.mse / losses.gaussian_ll, losses.py:56-59,84-96).
 * frame_sums[n] = sum_d (pred[n,d]-target[n,d])^2 * mask[n,d]   (mask nullable), d < D.
 * The caller turns frame sums into mse (sum/(N*D)) or gaussian ll; see fitting/losses.py.
 * ------------------------------------------------------------------------------------------ */
int bn_sqerr_frame_sums(const float* pred, const float* target, const float* mask,
                        float* frame_sums, int N, size_t D, bn_stream_t stream);
/* dpred[i] = (*gscale) * scale * 2 * (pred[i]-target[i]) * mask[i];  gscale: device scalar or NULL */
int bn_sqerr_bwd(const float* pred, const float* target, const float* mask, float* dpred,
                 size_t n, float scale, const float* gscale, bn_stream_t stream);
/* out[0] = sum_i in[i] * scale  (deterministic single-workgroup tree; n small) */
int bn_reduce_sum(const float* in, float* out, size_t n, float scale, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Variational tail (replaces vaes.reparameterize + losses.kl_div_to_std_normal,
 * vaes.py:33-35, losses.py:146-147).  NOTE std = exp(logvar), as in the reference.
 *   z = mu + eps*exp(logvar);  kl_rows[n] = 0.5*sum_d(exp(lv) - lv + mu^2 - 1)
 * ------------------------------------------------------------------------------------------ */
int bn_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z,
                   size_t n, bn_stream_t stream);
int bn_kl_rows(const float* mu, const float* logvar, float* kl_rows, int N, int D,
               bn_stream_t stream);
/* autograd of the two ops above:
 *   dlogvar[i] = dz[i] * (z[i] - mu[i])                       (dmu = dz needs no kernel)
 *   dmu[i] = s*mu[i], dlogvar[i] = s*0.5*(exp(logvar[i])-1),  s = scale * (*gscale) */
int bn_reparam_bwd(const float* dz, const float* z, const float* mu, float* dlogvar, size_t n,
                   bn_stream_t stream);
int bn_kl_bwd(const float* mu, const float* logvar, float* dmu, float* dlogvar, size_t n,
              float scale, const float* gscale, bn_stream_t stream);

/* Decomposed KL of the beta-TC-VAE / PS-VAE (replaces losses.decomposed_kl, losses.py:284-351,
 * and its autograd graph).  z, mu, logvar: (N, D) fp32, N >= 1, D <= 64 (BN_E_SHAPE above; one
 * kernel generation for D <= 32, a second, column-split one for 32 < D <= 64).
 *   fwd: out3 = (index-code MI, total correlation, dimension-wise KL); log_qz (N) and lse (N, D)
 *        are saved for the backward pass; terms is 3N floats of scratch.
 *   bwd: g3 = the three upstream gradients (device); dz, dmu, dlogvar: (N, D). */
int bn_decomposed_kl_fwd(const float* z, const float* mu, const float* logvar, float* out3,
                         float* log_qz, float* lse, float* terms, int N, int D,
                         bn_stream_t stream);
int bn_decomposed_kl_bwd(const float* z, const float* mu, const float* logvar,
                         const float* log_qz, const float* lse, const float* g3, float* dz,
                         float* dmu, float* dlogvar, int N, int D, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Latent head of the PS-VAE (reference vaes.py:571-601 forward, :669-704 per-chunk loss terms):
 * everything between the encoder's two heads / the decomposed-KL kernels and the decoder, fused.
 *   y (N, L) supervised means, w (N, U) unsupervised means, logvar / eps / z (N, L + U), D = the
 *   diagonal label map (Dw, Db of length L; Db nullable), labels / lmask (N, L; lmask nullable).
 *   fwd:     z = [y | w] + eps exp(logvar); z_u, lv_u: the unsupervised columns of z / logvar as
 *            contiguous (N, U) tensors (inputs of bn_decomposed_kl_fwd); yhat = D y;
 *            row_sq[n] = sum_l (yhat - labels)^2 lmask; row_kl[n] = 0.5 sum_{l<L} (e^lv - lv + y^2 - 1)
 *   combine: per chunk c = rows [bounds[2c], bounds[2c+1]) (device ints), dkl3 = (n_chunks, 3) from
 *            bn_decomposed_kl_fwd: cols5[c] = (ll_labels, KL_s, MI, TC, DWKL),
 *            T[c] = -alpha ll_labels + KL_s + kl MI + beta TC + kl DWKL
 *   bwd:     gT[c] = dL/dT[c], dz = dL/dz from the decoder, gz_u / gmu_u / glv_u = the outputs of
 *            bn_decomposed_kl_bwd (called with g3 = gT[c] (kl, beta, kl)) -> dy, dw, dlogvar and the
 *            gradients of D (written, or added to when accumulate) */
int bn_psvae_head_fwd(const float* y, const float* w, const float* logvar, const float* eps,
                      const float* Dw, const float* Db, const float* labels, const float* lmask,
                      float* z, float* z_u, float* lv_u, float* yhat, float* row_sq,
                      float* row_kl, int N, int L, int U, bn_stream_t stream);
int bn_psvae_head_combine(const float* row_sq, const float* row_kl, const float* dkl3,
                          const int* bounds, int n_chunks, float alpha, float kl, float beta,
                          int L, float* T, float* cols5, bn_stream_t stream);
int bn_psvae_head_bwd(const float* dz, const float* gT, const int* bounds, int n_chunks,
                      const float* y, const float* logvar, const float* eps, const float* yhat,
                      const float* labels, const float* lmask, const float* Dw, const float* gz_u,
                      const float* gmu_u, const float* glv_u, float alpha, float* dy, float* dw,
                      float* dlogvar, float* dDw, float* dDb, int accumulate, int N, int L, int U,
                      bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Last decoder layer fused with the pixel loss (replaces, in ONE pass, the ConvTranspose2d + crop
 * + Sigmoid of aes.py:315-330,466-470 and the squared error of losses.py:56-59 / 84-96 together
 * with their derivatives): for every frame n
 *     xhat   = act(convT(x, w, b))                     written only if xhat != NULL
 *     part[n][j], j < P:  sum_j part[n][j] = sum_{c,h,w} (xhat - target)^2 * mask
 *     dpre   = 2 (xhat - target) mask act'(xhat)       = d(frame sum)/d(pre-activation)
 * so that training never writes or re-reads xhat.  P = bn_convT2d_fwd_sqerr_parts(geometry)
 * (partial sums per frame, summed by the caller in index order: deterministic).  mask nullable.
 * `ws`: bn_convT2d_fwd_sqerr_ws_bytes(geometry, xhat != NULL) bytes (0 for the benchmark layer).
 * bn_scale_frames: t[n, :] *= frame_scale[n] * (group_scale ? group_scale[group_of_frame[n]] : 1)
 * -- the backward pass applies the per-chunk loss normalisation and the upstream gradient of a
 * frame's chunk to dpre with it (aes.py:751-771: one mean per 200-frame chunk).
 * ------------------------------------------------------------------------------------------ */
int bn_convT2d_fwd_sqerr_parts(int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                               int crop_t, int crop_l, int Ho, int Wo);
size_t bn_convT2d_fwd_sqerr_ws_bytes(int N, int Ci, int Hi, int Wi, int Co, int R, int S,
                                     int stride, int crop_t, int crop_l, int Ho, int Wo,
                                     int with_xhat);
int bn_convT2d_fwd_sqerr(const float* x, const float* w, const float* b, const float* target,
                         const float* mask, float* xhat, float* dpre, float* part,
                         int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                         int crop_t, int crop_l, int Ho, int Wo, int act, float slope,
                         void* ws, size_t ws_bytes, bn_stream_t stream);
int bn_scale_frames(float* t, const float* frame_scale, const float* group_scale,
                    const int* group_of_frame, int N, size_t D, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser (replaces torch.optim.Adam(amsgrad=True).step, training.py:284-286,352), over one
 * flat fp32 parameter arena.  `step` is 1-based.  weight_decay adds wd*p to the gradient.
 * ------------------------------------------------------------------------------------------ */
int bn_adam_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, size_t n,
                         float lr, float beta1, float beta2, float eps, float weight_decay,
                         int step, bn_stream_t stream);

/* First encoder layer straight from the stored uint8 frames: y = act(conv(x_u8 / 255) + b).  The
 * reference converts every batch on the host (data_generator.py:251-263: astype(float32) / 255)
 * and feeds the float copy to nn.Conv2d (aes.py:81-86,153); here the conversion (an IEEE division,
 * bit-identical to numpy's) happens while the input patch is staged, so a frame is read as 1 byte
 * per pixel and no float copy of it is ever written.  Same geometry arguments as bn_conv2d_fwd;
 * `ws`: bn_conv2d_fwd_u8_ws_bytes(..., act) bytes for the SAME geometry and activation (0 for the
 * benchmark layer with BN_ACT_NONE / BN_ACT_LRELU; other geometries / activations convert into it
 * and run the float kernels; BN_E_WORKSPACE if it is missing or too small). */
size_t bn_conv2d_fwd_u8_ws_bytes(int N, int C, int H, int W, int K, int R, int S, int stride,
                                 int pad_t, int pad_l, int P, int Q, int act);
int bn_conv2d_fwd_u8(const unsigned char* x, const float* w, const float* b, float* y,
                     int N, int C, int H, int W, int K, int R, int S, int stride,
                     int pad_t, int pad_l, int P, int Q, int act, float slope,
                     void* ws, size_t ws_bytes, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Inference-only conv encoder stack on bf16 operands with fp32 accumulation (opt-in; nothing
 * above dispatches to it).  Between the layers the activations are bf16 in a private layout,
 * (N, H, W, C) channels last; it never leaves a chain of these calls.  Geometry arguments as
 * bn_conv2d_fwd.  Fixed-order reductions: the same operands give the same bits.
 *   bn_conv2d_first_bf16_ok  1 if bn_conv2d_first_bf16 serves the geometry: 1..4 input channels,
 *                       K a multiple of 16, kernel up to 5x5 (host only, needs no GPU)
 *   bn_conv2d_bf16_ok   1 if bn_conv2d_fwd_bf16 serves it: C a multiple of 16 (one matrix-core
 *                       step is 16 channels of one tap), any K, H, W, stride, kernel up to 5x5,
 *                       x and wp below 2 GiB each
 *   bn_conv_pack_w_bf16 fp32 weights (K, C, R, S) -> bf16 [K][(r S + s) C + c] in `wp`,
 *                       bn_conv_pack_w_bf16_bytes(K, C, R, S) bytes (a multiple of 256)
 *   bn_conv2d_first_bf16 layer 1 from fp32 (x_is_u8 == 0) or uint8 (value / 255 fused) NCHW frames:
 *                       fp32 arithmetic, bias (nullable) + activation, one rounding to bf16
 *                       (nearest even), y in the private layout: N P Q K bf16
 *   bn_conv2d_fwd_bf16  x in the private layout, wp packed; bias + activation in fp32; out_f32 == 0:
 *                       y in the private layout (one rounding), out_f32 != 0: y fp32 (N, K, P, Q)
 * BN_E_SHAPE (nothing written) for a geometry that is not served, an activation other than
 * BN_ACT_NONE / BN_ACT_LRELU or operands that are not 16-byte aligned. */
int bn_conv2d_first_bf16_ok(int N, int C, int H, int W, int K, int R, int S, int stride,
                            int pad_t, int pad_l, int P, int Q);
int bn_conv2d_bf16_ok(int N, int C, int H, int W, int K, int R, int S, int stride,
                      int pad_t, int pad_l, int P, int Q);
size_t bn_conv_pack_w_bf16_bytes(int K, int C, int R, int S);
int bn_conv_pack_w_bf16(const float* w, void* wp, int K, int C, int R, int S, bn_stream_t stream);
int bn_conv2d_first_bf16(const void* x, int x_is_u8, const float* w, const float* b, void* y,
                         int N, int C, int H, int W, int K, int R, int S, int stride,
                         int pad_t, int pad_l, int P, int Q, int act, float slope, bn_stream_t stream);
int bn_conv2d_fwd_bf16(const void* x, const void* wp, const float* b, void* y, int out_f32,
                       int N, int C, int H, int W, int K, int R, int S, int stride,
                       int pad_t, int pad_l, int P, int Q, int act, float slope, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Inference-only transposed-conv decoder stack on bf16 operands with fp32 accumulation (opt-in;
 * nothing above dispatches to it).  The same private layout between the layers as the encoder
 * stack: bf16 (N, H, W, C) channels last.  Geometry arguments as bn_convT2d_fwd: (off_t, off_l)
 * is the crop, output pixel o is pixel o + off of the full-size map; output pixels past the full
 * size (output_padding) receive the bias alone.  Gather formulation, fixed-order reductions, no
 * atomics: the same operands give the same bits.
 *   bn_convT2d_bf16_ok  1 if bn_convT2d_fwd_bf16 serves the geometry: Ci a multiple of 16, any Co,
 *                       Hi, Wi, Ho, Wo, kernel up to 5x5, stride up to 5, x and wp below 2 GiB each
 *                       (host only, needs no GPU)
 *   bn_convT2d_last_bf16_ok  1 if bn_convT2d_last_bf16 serves it: Co 1..4, Ci a multiple of 16,
 *                       kernel up to 5x5, stride up to 5, R S Co Ci floats within 48 KiB (host only)
 *   bn_convT_pack_w_bf16  fp32 nn.ConvTranspose2d weights (Ci, Co, R, S) -> bf16
 *                       [co][(r S + s) Ci + ci] in `wp`, bn_convT_pack_w_bf16_bytes(Ci, Co, R, S)
 *                       bytes (a multiple of 256), round to nearest even
 *   bn_to_nhwc_bf16     the stack's input: fp32 (N, C, H, W) -> bf16 (N, H, W, C), one rounding
 *   bn_convT2d_fwd_bf16 body layer: x in the private layout, wp packed; bias (nullable) + activation
 *                       in fp32; out_f32 == 0: y in the private layout (one rounding), out_f32 != 0:
 *                       y fp32 (N, Co, Ho, Wo)
 *   bn_convT2d_last_bf16  the layer onto the frame: x in the private layout, w fp32 (Ci, Co, R, S)
 *                       as stored (not rounded), fp32 arithmetic, bias (nullable) + activation,
 *                       y fp32 (N, Co, Ho, Wo)
 * Activations: BN_ACT_NONE / BN_ACT_LRELU / BN_ACT_SIGMOID.  BN_E_SHAPE (nothing written) for a
 * geometry that is not served, another activation or operands that are not 16-byte aligned. */
int bn_convT2d_bf16_ok(int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                       int off_t, int off_l, int Ho, int Wo);
int bn_convT2d_last_bf16_ok(int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                            int off_t, int off_l, int Ho, int Wo);
size_t bn_convT_pack_w_bf16_bytes(int Ci, int Co, int R, int S);
int bn_convT_pack_w_bf16(const float* w, void* wp, int Ci, int Co, int R, int S, bn_stream_t stream);
int bn_to_nhwc_bf16(const float* x, void* y, int N, int C, int H, int W, bn_stream_t stream);
int bn_convT2d_fwd_bf16(const void* x, const void* wp, const float* b, void* y, int out_f32,
                        int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                        int off_t, int off_l, int Ho, int Wo, int act, float slope, bn_stream_t stream);
int bn_convT2d_last_bf16(const void* x, const float* w, const float* b, float* y,
                         int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                         int off_t, int off_l, int Ho, int Wo, int act, float slope, bn_stream_t stream);

/* The layer onto the frame fused with the per-frame squared error: every x_hat value is computed by the
 * device code of bn_convT2d_last_bf16 and scored in the epilogue instead of being stored,
 *   out[n] = scale * sum_{co, h, w} (x_hat[n] - target[n])^2 * mask[n]        fp32 (N,)
 * target: fp32 (N, Co, Ho, Wo), or with target_is_u8 stored uint8 frames (value / 255); mask: fp32 of
 * the target's shape, nullable.  A frame's summation order depends on the geometry of one frame
 * alone: out[n] does not change with N or with the frame's position, and there are no atomics.
 * `ws`: bn_convT2d_last_bf16_sqerr_ws_bytes(geometry) bytes (per-frame partial sums; 0 for small
 * frames).  Serves exactly what bn_convT2d_last_bf16_ok reports; BN_E_SHAPE (nothing written)
 * otherwise, for another activation or an x that is not 16-byte aligned. */
size_t bn_convT2d_last_bf16_sqerr_ws_bytes(int N, int Ci, int Hi, int Wi, int Co, int R, int S,
                                           int stride, int off_t, int off_l, int Ho, int Wo);
int bn_convT2d_last_bf16_sqerr(const void* x, const float* w, const float* b, const void* target,
                               int target_is_u8, const float* mask, float* out,
                               int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                               int off_t, int off_l, int Ho, int Wo, int act, float slope, float scale,
                               void* ws, size_t ws_bytes, bn_stream_t stream);

/* The layer onto the frame writing stored grey levels: every x_hat value is computed by the device
 * code of bn_convT2d_last_bf16 and leaves through the rounding rule of bn_unit_float_to_u8 in the
 * epilogue, y uint8 (N, Co, Ho, Wo); the fp32 x_hat is never written.  The bytes are those of
 * bn_unit_float_to_u8 applied to bn_convT2d_last_bf16's output.  y needs no alignment.  Serves exactly
 * what bn_convT2d_last_bf16_ok reports; BN_E_SHAPE (nothing written) otherwise, for another
 * activation or an x that is not 16-byte aligned. */
int bn_convT2d_last_bf16_u8(const void* x, const float* w, const float* b, unsigned char* y,
                            int N, int Ci, int Hi, int Wi, int Co, int R, int S, int stride,
                            int off_t, int off_l, int Ho, int Wo, int act, float slope, bn_stream_t stream);

/* Per-frame squared error of a reconstruction that is already in memory:
 *   out[n] = scale * sum_{i < D} (xhat[n, i] - target[n, i])^2 * mask[n, i]        fp32 (N,)
 * xhat fp32 (N, D); target fp32 (N, D), or with target_is_u8 uint8 (value / 255, the division of
 * bn_u8_to_unit_float); mask fp32 (N, D), nullable.  Any N and D.  16-byte loads where every frame
 * of every operand starts on a 16-byte boundary, element-by-element loads otherwise -- the summation
 * order is a function of D alone either way, so out[n] has the same bits whatever N, the frame's
 * position and the alignment; no atomics.  `ws`: bn_frame_sq_err_ws_bytes(N, D) bytes (0 up to 4096
 * elements a frame).  BN_E_SHAPE (nothing written) for fp32 operands off a 4-byte boundary or more
 * than 2^31 partial sums. */
size_t bn_frame_sq_err_ws_bytes(int N, size_t D);
int bn_frame_sq_err(const float* xhat, const void* target, int target_is_u8, const float* mask,
                    float* out, int N, size_t D, float scale, void* ws, size_t ws_bytes,
                    bn_stream_t stream);

/* Per-pixel sums over the frames of a reconstruction that is already in memory, ADDED ONTO acc, float64
 * (4, D), plane by plane (t = target, m = mask or 1):
 *   0  sse[i] += sum_n ((xhat[n,i] - t[n,i]) * (xhat[n,i] - t[n,i])) * m[n,i]   the fp32 term of
 *                bn_frame_sq_err, widened to double; the plane is not touched when xhat is NULL
 *   1  w[i]   += sum_n (double)m[n,i]
 *   2  s1[i]  += sum_n (double)m[n,i] * (double)t[n,i]
 *   3  s2[i]  += sum_n (double)m[n,i] * ((double)t[n,i] * (double)t[n,i])
 * xhat fp32 (N, D), nullable; target fp32 (N, D), or with target_is_u8 uint8 (value / 255, the
 * division of bn_u8_to_unit_float); mask fp32, nullable: (N, D) with mask_frames == N, or one (D,)
 * mask for all frames with mask_frames == 1 (mask_frames is not read without a mask).
 * Order: every sum is float64, without atomics.  A workgroup walks a block of consecutive frames in
 * ascending order; the blocks' partial sums are added from left to right, and that sum onto acc.  The
 * cut into frame blocks is a function of (N, D) alone, so equal calls give equal bits; 16-byte loads
 * where every operand sits on a 16-byte boundary (4 bytes for a uint8 target) and D is a multiple of
 * 4, element-by-element loads otherwise, with the same bits either way.
 * `ws`: bn_pixel_stats_ws_bytes(N, D) bytes (0 while one frame block serves the call).
 * Refusals, all BN_E_SHAPE with nothing written: N <= 0, D == 0, a mask with mask_frames not in
 * {1, N}, a workspace smaller than the query says, an acc or ws off a 16-byte boundary, fp32 operands
 * off a 4-byte boundary.  (A NULL target or acc is BN_E_BADARG.) */
size_t bn_pixel_stats_ws_bytes(int N, size_t D);
int bn_pixel_stats_accum(const float* xhat, const void* target, int target_is_u8, const float* mask,
                         int mask_frames, double* acc, int N, size_t D, void* ws, size_t ws_bytes,
                         bn_stream_t stream);

/* uint8 frames -> float32/255 (replaces the host-side astype(float32)/255 of
 * data_generator.py:251-263 for device-resident uint8 trials) */
int bn_u8_to_unit_float(const unsigned char* in, float* out, size_t n, bn_stream_t stream);

/* The input of a conditional encoder in one pass (replaces the host-side MakeOneHot2D of
 * data/transforms.py:186-245 and the torch.cat of aes.py:818-826): out fp32 (n, c + n_maps, h, w),
 *   out[i, k]         = frames[i, k]            k < c: fp32 frames (n, c, h, w) copied; with frames_is_u8
 *                                               uint8 frames, value / 255 (the division of bn_u8_to_unit_float)
 *   out[i, c + l]     = zeros but for one 1.0f at (y, x)                              l < n_maps
 * where x = pixel(coords[i * ld + l], w) and y = pixel(coords[i * ld + n_maps + l], h), and pixel(v, size)
 * is the transform's rule: NaN counts as 0, clip to [0, size - 1], round half to even.  coords fp32 (n, ld),
 * ld >= 2 * n_maps; columns from 2 * n_maps on are not read.  The coordinates are read on the device: no
 * host read, no synchronisation, capturable in a graph.  Every output byte is written once, by plain
 * stores; no atomics.  16-byte stores with 16-byte (uint8 frames: 4-byte) loads where h * w is a multiple
 * of 4 and `out` sits on a 16-byte and `frames` on a 16-byte (uint8: 4-byte) boundary, element by element
 * otherwise, with the same values.
 * n_maps == 0 is the plain conversion (coords is not read and may be NULL); n == 0 returns 0 and launches
 * nothing.  BN_E_SHAPE (nothing written): n < 0, c, h or w <= 0, n_maps < 0, ld < 2 * n_maps, an output of
 * more than 2^40 elements, fp32 operands off a 4-byte boundary.  BN_E_BADARG: a NULL pointer (n > 0). */
int bn_cond_encoder_input(const void* frames, int frames_is_u8, const float* coords, int ld,
                          int n, int c, int h, int w, int n_maps, float* out, bn_stream_t stream);

/* One channel of decoded frames, cropped, quantised and tiled into a uint8 mosaic in one pass (replaces the
 * host-side get_crop of plotting/__init__.py:41-73 and the panel grids of plot_2d_frame_array and
 * make_latent_traversal_movie, plotting/cond_ae_utils.py): out uint8 (t, r * hc, cc * wc),
 *   out[i, j * hc + y, k * wc + x] = 0                        s < 0, y_min + y >= h or x_min + x >= w
 *                                  = quantise(frames[s, ch, y_min + y, x_min + x])     fp32 frames
 *                                  = frames[s, ch, y_min + y, x_min + x]               frames_u8
 * with s = src[(i * r + j) * cc + k].  frames: (p, c, h, w) fp32 unit floats, or with frames_u8 uint8 grey
 * levels; quantise is the rule of bn_unit_float_to_u8 (NaN -> 0, else clamp(rint(v * 255), 0, 255), round half
 * to even).  (y_min, x_min, hc, wc) is the crop window, the whole frame being (0, 0, h, w); where it passes
 * the bottom or right edge the mosaic is zero, as get_crop fills.  src: DEVICE int32 (t, r, cc), read on the
 * device; -1 is a blank panel, an index may repeat.  The caller keeps src below p: the kernel shows a panel
 * with s >= p as blank and reads nothing for it.  Every output byte is written once, by plain stores; no
 * memset is needed and no atomics are used.  16-byte stores where `out` and cc * wc are multiples of 16,
 * with four 16-byte loads (frames_u8: one) where the 16 bytes lie in one panel, inside the frame and on a
 * 16-byte boundary of the source; byte by byte otherwise, with the same values.
 * t * r * cc == 0 returns 0 and launches nothing.  BN_E_SHAPE (nothing written): a negative count, c, h or
 * w <= 0, ch outside [0, c), y_min or x_min < 0 (a numpy slice would wrap there), hc or wc <= 0, t * r * hc
 * or cc * wc or a window's end at 2^31 or beyond, a grid of 2^32 threads or more, src or fp32 frames off a
 * 4-byte boundary.  BN_E_BADARG: a NULL pointer (frames may be NULL when p == 0). */
int bn_frame_mosaic_u8(const void* frames, int frames_u8, int p, int c, int h, int w, int ch,
                       int y_min, int x_min, int hc, int wc, const int* src, int t, int r, int cc,
                       unsigned char* out, bn_stream_t stream);

/* bn_frame_mosaic_u8 with a range of channels per panel (the panels of make_session_swap_movie and
 * make_reconstruction_movie, plotting/cond_ae_utils.py and ae_utils.py, which show concat(ims[i]): all channels
 * of a frame side by side): out uint8 (t, r * hc, cc * n_ch * wc); panel (i, j, k) is n_ch sub-panels of wc
 * columns, and sub-panel q shows channel ch0 + q of frame s = src[(i * r + j) * cc + k],
 *   out[i, j * hc + y, (k * n_ch + q) * wc + x] = 0          s < 0, s >= p, y_min + y >= h or x_min + x >= w
 *                                  = quantise(frames[s, ch0 + q, y_min + y, x_min + x])     fp32 frames
 *                                  = frames[s, ch0 + q, y_min + y, x_min + x]               frames_u8
 * src keeps naming frames: one index is read per panel, whatever n_ch is.  Everything else is the contract
 * of bn_frame_mosaic_u8 -- the crop window and its zero fill, blank panels, quantise, every output byte written
 * once by plain stores, no memset, no atomics -- and bn_frame_mosaic_u8 is this call with n_ch == 1, byte for
 * byte.  16-byte stores where `out` and cc * n_ch * wc are multiples of 16, with four 16-byte loads
 * (frames_u8: one) where the 16 bytes lie in one sub-panel, inside the frame and on a 16-byte boundary of the
 * source; byte by byte otherwise, with the same values.
 * t * r * cc == 0 returns 0 and launches nothing.  BN_E_SHAPE (nothing written): n_ch < 1, ch0 < 0,
 * ch0 + n_ch > c, cc * n_ch * wc at 2^31 or beyond, and every refusal of bn_frame_mosaic_u8.  BN_E_BADARG: a
 * NULL pointer (frames may be NULL when p == 0). */
int bn_frame_mosaic_ch_u8(const void* frames, int frames_u8, int p, int c, int h, int w, int ch0, int n_ch,
                          int y_min, int x_min, int hc, int wc, const int* src, int t, int r, int cc,
                          unsigned char* out, bn_stream_t stream);

/* Marker boxes into a finished mosaic, in place (the red Rectangle((5, 5), 10, 10) that make_syllable_movies,
 * plotting/arhmm_utils.py:476-482, draws on the first frames of a syllable instance, in grey): movie uint8
 * (t, r * hp, cc * wp), panels of hp rows and wp columns; mark uint8 (t, r, cc).  For every panel (i, j, k) with
 * mark[(i * r + j) * cc + k] != 0
 *   movie[i, j * hp + y, k * wp + x] = value      y0 <= y < y0 + h, x0 <= x < x0 + w, 0 <= y < hp, 0 <= x < wp
 * -- the box is clipped to its panel -- and no other byte is written or read.  Plain byte stores, no atomics; one
 * wave a panel, which leaves at once where the mark is 0.  t * r * cc == 0, h or w == 0 and a box wholly outside the
 * panel return 0 and launch nothing.  BN_E_SHAPE (nothing written): a negative count, hp or wp <= 0, h or w < 0,
 * value outside [0, 255], t * r * cc, r * hp, cc * wp or hp * wp at 2^31 or beyond.  BN_E_BADARG: a NULL pointer. */
int bn_stamp_boxes_u8(unsigned char* movie, int t, int r, int cc, int hp, int wp, const unsigned char* mark,
                      int y0, int x0, int h, int w, int value, bn_stream_t stream);

/* The strips of a reconstruction movie in one pass (replaces the three fp32 arrays ims_orig, ims_recon and
 * 0.5 + (ims_orig - ims_recon) of make_ae_reconstruction_movie_wrapper, plotting/ae_utils.py:147-186, their
 * concat per frame and matplotlib's vmin=0, vmax=1 clip): for frame i and row y three panels of c * w bytes,
 * the channels side by side,
 *   o  = orig[i, k, y, x]                        fp32 unit float, or with orig_u8 stored uint8 as value / 255.f
 *   om = mask ? o * mask[i or 0, k, y, x] : o    (the original alone is masked, as the reference masks)
 *   r  = recon[i, k, y, x]                       fp32 unit float, or with recon_u8 uint8 grey levels as value / 255.f
 *   panel 0: show_orig ? quantise(om) : 0        (no mask and orig_u8: the stored byte, which is the same value)
 *   panel 1: recon_u8 ? the byte : quantise(r)
 *   panel 2: quantise(0.5f + (om - r))
 *   out[i * out_frame_stride + y * (3 * c * w) + p * (c * w) + k * w + x]
 * quantise is the rule of bn_unit_float_to_u8 (NaN -> 0, else clamp(rint(v * 255), 0, 255), round half to even).
 * Every step is one fp32 operation, none contracted into an fma: numpy's float32 arithmetic bit for bit.
 * orig, recon: (n, c, h, w); mask: NULL, fp32 (n, c, h, w) with mask_per_frame, else fp32 (c, h, w) for all
 * frames.  out_frame_stride >= 3 * c * h * w bytes: a larger stride writes one row of a movie of several rows
 * (row j of r at out + j * h * 3 * c * w with stride r * h * 3 * c * w; show_orig = 0 leaves panel 0 black).
 * A call writes each byte of its n strips once, by plain stores, and nothing else.  16-byte stores where out,
 * out_frame_stride and 3 * c * w are multiples of 16, with 16-byte loads where the 16 bytes lie inside one
 * channel of one panel and the operands sit on a 16-byte boundary; byte by byte otherwise, with the same values.
 * n == 0 returns 0 and launches nothing.  BN_E_SHAPE (nothing written): n < 0, c, h or w <= 0,
 * out_frame_stride < 3 * c * h * w, n * h or 3 * c * w or c * h * w at 2^31 or beyond, a grid of 2^32 threads
 * or more, an fp32 operand off a 4-byte boundary.  BN_E_BADARG: orig, recon or out NULL. */
int bn_recon_panels_u8(const void* orig, int orig_u8, const void* recon, int recon_u8, const float* mask,
                       int mask_per_frame, int n, int c, int h, int w, int show_orig, unsigned char* out,
                       size_t out_frame_stride, bn_stream_t stream);

/* Exact per-column order statistics of a table, selected on the device (replaces the np.nanpercentile calls of
 * compute_range, plotting/cond_ae_utils.py:148-178, on the stacked latents or labels): x is fp32 (n, d), row-major
 * with leading dimension ld >= d (columns from d on are not counted), and is never written.  Values are ordered by
 * the key that flips all bits of a negative value and the sign bit of any other: infinities and denormals are
 * ordinary values, -0.0 sorts directly below +0.0 (a selected zero may carry either sign; the two are equal under
 * ==), and a NaN of any sign or payload takes no part.
 *
 * bn_column_count: n_valid[j], int64 (d,) = the number of non-NaN values of column j -- what a caller needs
 * before it can name ranks among the valid values.
 * bn_column_select: ranks is a DEVICE table int64 (r, d), zero-based among a column's valid values in ascending
 * order; out fp32 (r, d), out[k, j] = the value of column j with exactly ranks[k, j] valid values before it in
 * sorted order, NaN for a rank below 0 or at least n_valid[j] (an all-NaN column is reported so; no error).  A
 * rank may repeat among a column's slots.  Four passes over the table, one per 8-bit digit of the key, each
 * followed by a small launch that sums the workgroups' histograms and narrows every slot's prefix; counts are
 * integers and no global atomics are used, so the result is the same bits on every call.
 * ws: bn_column_select_ws_bytes(n, d, r) bytes on a 16-byte boundary (it serves bn_column_count for the same n and
 * d too, for any r).  Nothing is read from it that the call has not written.
 * BN_E_SHAPE (nothing written): n < 1, d < 1 or d > 1024, ld < d, r < 1 or r > 8 (the query returns 0 for
 * these), a workspace smaller than the query's, x or out off a 4-byte, ranks or n_valid off an 8-byte, ws off a
 * 16-byte boundary.  BN_E_BADARG: a NULL pointer. */
size_t bn_column_select_ws_bytes(int n, int d, int r);
int bn_column_count(const float* x, int n, int d, int ld, long long* n_valid, void* ws, size_t ws_bytes,
                    bn_stream_t stream);
int bn_column_select(const float* x, int n, int d, int ld, const long long* ranks, int r, float* out,
                     void* ws, size_t ws_bytes, bn_stream_t stream);

/* Masked column sums per row segment, reduced on the device: the sums behind the per-trial, per-label R^2 and MSE of
 * get_label_r2 (plotting/cond_ae_utils.py:1234-1279, an sklearn call per trial and label on the host).  pred, truth
 * and mask are fp32 tables of n rows, row-major with leading dimensions ld_* >= L; only the first L columns are read
 * (pred is in practice the (n, D) table of transformed latents, ld_pred = D > L) and none is ever written.  mask may
 * be NULL: every entry is valid.  Otherwise entry (i, j) is valid where mask[i, j] == 1.0f exactly; any other value,
 * NaN included, is not.
 *
 * offsets: DEVICE int64 (S + 1).  Made safe first: e[i] = the largest of offsets[0 .. i], each clamped into [0, n].
 * Segment s is the rows [e[s], e[s+1]): a segment may be empty, an offset that steps back gives an empty segment, the
 * segments never overlap, and rows outside [e[0], e[S]) are never read.
 *
 * out: DEVICE float64 (S, L, 4); for segment s and column j, over the valid entries of the segment's rows,
 *   { count, sum y, sum y^2, sum (y - p)^2 }     with y = (double)truth[i, j], p = (double)pred[i, j]
 * Every term is formed in float64 from the fp32 operands and summed in float64.  An invalid entry is selected out,
 * not multiplied by zero: a NaN or Inf under a mask that is not one reaches no sum; a NaN under a one mask propagates.
 * Every element of out is written (zeros for an empty segment).  Long segments are cut into row blocks whose partial
 * sums are combined in block order, short ones are finished where they are read; no global atomics, and the order of
 * every sum is fixed by (n, S, L) and the offsets: the same bits on every call.
 * ws: bn_segment_label_sums_ws_bytes(n, S, L) bytes on a 16-byte boundary; nothing is read from it that the call has
 * not written.
 * BN_E_SHAPE (nothing written): L < 1 or L > 64, S < 0, n < 0 (the query returns 0 for these), a leading dimension
 * below L, a workspace smaller than the query's, a table off a 4-byte, offsets or out off an 8-byte, ws off a 16-byte
 * boundary.  BN_E_BADARG: pred, truth, offsets, out or ws NULL. */
size_t bn_segment_label_sums_ws_bytes(int n, int S, int L);
int bn_segment_label_sums(const float* pred, int ld_pred, const float* truth, int ld_truth, const float* mask,
                          int ld_mask, const long long* offsets, int S, int L, int n, double* out, void* ws,
                          size_t ws_bytes, bn_stream_t stream);

/* Augmented second-moment matrices per row segment, reduced on the device: the sums behind the correlation of the
 * unsupervised latents "per batch or across all time points" that the PS-VAE and MSPS-VAE hyperparameter searches
 * plot (plotting/cond_ae_utils.py:1679-1700, 2802-2835: np.vstack + np.corrcoef per batch on the host).
 * z: fp32 table of n rows and D columns, 1 <= D <= 64, row-major with leading dimension ld >= D, on any 4-byte
 * boundary (a column slice of a wider table is served as it is; the columns from D on are never read).  c: D fp32
 * values, the shift, or NULL for zeros.  Neither is ever written.
 *
 * offsets: DEVICE int64 (S + 1), made safe as bn_segment_label_sums makes them: e[i] = the largest of
 * offsets[0 .. i], each clamped into [0, n]; segment s is the rows [e[s], e[s+1]) and rows outside [e[0], e[S]) are
 * never read.
 *
 * out: DEVICE float64 (S, D + 1, D + 1); for segment s, with a = (1, (double)z_0 - (double)c_0, ...,
 * (double)z_{D-1} - (double)c_{D-1}) per row,
 *   out[s] = sum over the segment's rows of a^T a
 * i.e. out[s][0][0] the row count (an exact integer), out[s][0][1 + j] = out[s][1 + j][0] = sum a_j and
 * out[s][1 + i][1 + j] = sum a_i a_j.  Both triangles are written, with the same bits in [i][j] and [j][i].  Every term
 * is formed in float64 from the fp32 operands and summed in float64 (covariance is shift-invariant: a shift near the
 * data keeps the raw moments from losing digits where |mean| >> std).  A NaN or Inf in column j of a segment reaches
 * row and column 1 + j of that segment's matrix and nothing else.  Every element of out is written exactly once
 * (zeros for an empty segment).  Long segments are cut into row blocks whose partial matrices are combined in block
 * order, short ones are finished where they are read; no global atomics, and the order of every sum is fixed by
 * (n, S, D) and the offsets: the same bits on every call.
 * ws: bn_segment_gram_ws_bytes(n, S, D) bytes (32 MiB of partials at most) on a 16-byte boundary; nothing is read from
 * it that the call has not written.  S == 0 returns 0 and writes nothing.
 * BN_E_SHAPE (nothing written, to out or to ws): D < 1 or D > 64, S < 0, n < 0 (the query returns 0 for these),
 * ld < D, a workspace smaller than the query's, z or c off a 4-byte, offsets or out off an 8-byte, ws off a 16-byte
 * boundary.  BN_E_BADARG: z, offsets, out or ws NULL. */
size_t bn_segment_gram_ws_bytes(int n, int S, int D);
int bn_segment_gram(const float* z, int ld, const float* c, const long long* offsets, int S, int D, int n,
                    double* out, void* ws, size_t ws_bytes, bn_stream_t stream);

/* M multinomial logistic models at once over the rows of a table of latents: the sums behind the session classifier
 * that the MSPS-VAE hyperparameter search scores its models by (plotting/cond_ae_utils.py:1282-1369: sklearn's
 * LogisticRegressionCV on the host copy of every training frame).  The 5 x 8 (fold, C) models of a cross-validated
 * fit differ only in their weights and in the fold they leave out, so ONE pass over the table serves all of them.
 * z: fp32 table of n rows and D columns, 1 <= D <= 64, row-major with leading dimension ld >= D, on any 4-byte
 * boundary.  y: int32 (n), the class of a row; a row whose y is outside [0, S) belongs to no model.  fold: int32 (n),
 * the fold of a row, or NULL (a row belongs to no fold).  W: float64 (M, S, D + 1), one weight row a class and
 * model, column D the intercept.  leave: int32 (M), the fold model m leaves out, -1 for none.  2 <= S <= 8,
 * 1 <= M <= 64, n >= 0.  None of these is ever written.
 *
 * bn_softmax_cv_lossgrad: with l = W[m] (z, 1), formed in float64 from the fp32 row, over the rows with y in [0, S)
 * and fold != leave[m],
 *   loss[m]  = sum (logsumexp_k l_k - l_y)                              float64 (M)
 *   grad[m]  = sum (softmax(l) - onehot(y)) (x) (z, 1)                  float64 (M, S, D + 1)
 *   count[m] = the number of those rows (an exact integer)              float64 (M)
 * logsumexp is taken with the row maximum subtracted (logits of +-800 give finite sums) and every sum is float64.
 * Regularisation and the 1 / n scaling are the caller's.  A row with a NaN or Inf among its D values gives NaN as
 * loss[m] and all of grad[m] for the models that include it and nothing to the others.
 *
 * bn_softmax_cv_score: out float64 (M, 2); over the rows with y in [0, S) and, where leave[m] >= 0,
 * fold == leave[m]: out[m][0] = the rows whose float64 argmax_k l_k is y (a tie goes to the lowest class; a row with
 * a NaN or Inf among its values reads as class 0, as np.argmax of NaNs does), out[m][1] = the rows.  Exact integers.
 *
 * Every output element is written exactly once (zeros for n == 0).  The rows are cut into row blocks and the models
 * into groups of at most 128 / S; every (block, model) leaves one partial in the workspace and the partials are added
 * in block order: no global atomics, and the order of every sum is fixed by (n, D, S, M): the same bits on every
 * call.  The inner products run on v_mfma_f64_16x16x4_f64.
 * ws: bn_softmax_cv_{lossgrad,score}_ws_bytes(n, D, S, M) bytes (32 MiB at most) on a 16-byte boundary; nothing is
 * read from it that the call has not written.
 * BN_E_SHAPE (nothing written, to the outputs or to ws): D, S, M or n outside the limits above (the queries return 0
 * for these), ld < D, a workspace smaller than the query's, z, y, fold or leave off a 4-byte, W or an output off an
 * 8-byte, ws off a 16-byte boundary.  BN_E_BADARG: z, y, W, leave, an output or ws NULL. */
size_t bn_softmax_cv_lossgrad_ws_bytes(int n, int D, int S, int M);
int bn_softmax_cv_lossgrad(const float* z, int ld, const int* y, const int* fold, const double* W, const int* leave,
                           int n, int D, int S, int M, double* loss, double* grad, double* count, void* ws,
                           size_t ws_bytes, bn_stream_t stream);
size_t bn_softmax_cv_score_ws_bytes(int n, int D, int S, int M);
int bn_softmax_cv_score(const float* z, int ld, const int* y, const int* fold, const double* W, const int* leave,
                        int n, int D, int S, int M, double* out, void* ws, size_t ws_bytes, bn_stream_t stream);

/* EM for autoregressive hidden Markov models on a table of latents: the launches behind the second stage of the
 * BehaveNet pipeline (fitting/arhmm_grid_search.py:132-209 drives the `ssm` library on the host copy of every frame).
 * Gaussian AR observations with full covariance, L lags (L = 0: a plain Gaussian HMM), K states.
 *
 * Common operands.  z: fp32 table of n rows and D columns, row-major with leading dimension ld >= D, on any 4-byte
 * boundary; never written.  c: D float64 values, the shift, or NULL for zeros.  offsets: DEVICE int64 (S + 1), made
 * safe as bn_segment_gram makes them; segment s = trial s = the rows [e[s], e[s+1]).  Rows outside [e[0], e[S])
 * belong to no trial: no call reads them and no call writes their rows of ll, gamma or states.  Within a trial, row t
 * (counted from the trial's first row) is an INITIAL row if t < L and an AR row otherwise, and for an AR row
 *   a_t = (1, x_t - c, x_{t-1} - c, ..., x_{t-L} - c)          float64, P = 1 + (L + 1) D entries
 * Limits: 1 <= K <= 32, 0 <= L <= 8, D >= 1, (L + 1) D <= 64, n >= 0, S >= 0.  Everything but z is float64
 * (states: int32).  No call uses global atomics, every output element named below is written exactly once, and the
 * order of every sum is fixed by the shapes and the offsets: the same bits on every call.
 *
 * bn_arhmm_loglik -> ll (n, K).  G: (K, D, P) and cst: (K), the state's parameters folded by the caller:
 * G_k = R_k [-(b_k + c-terms) | I | -A_k] with R_k^T R_k = Sigma_k^-1, cst_k = -D/2 log 2 pi + log det R_k.  For an AR
 * row ll[t][k] = cst_k - 1/2 |G_k a_t|^2 (the (n x P) (P x K D) product on v_mfma_f64_16x16x4_f64, the squared norm
 * over D taken in the epilogue); for an initial row ll[t][k] = -D/2 log 2 pi - 1/2 |x_t|^2 for every k (x_t not
 * shifted).  A NaN or Inf in row t reaches the K values of row t and of the AR rows among the L rows after it in its
 * trial (an initial row does not look back), and nothing else.  ws: bn_arhmm_loglik_ws_bytes bytes (the offsets and one byte a row).
 *
 * bn_hmm_forward_backward.  ll: (n, K) as above (any log-likelihoods), logP: (K, K) log transition matrix (row: from),
 * logpi0: (K).  -> loglik (S): the log-likelihood of every trial, 0 for an empty trial; and, with want = 1,
 * gamma (n, K): the posterior state marginals, and xi (S, K, K): per trial the sum over t of the pairwise posteriors
 * p(z_t = i, z_{t+1} = j | trial), zeros for a trial of fewer than two rows.  With want = 0 (likelihood only) gamma
 * and xi may be NULL and are never written.  One wave a trial, scaled recursion: the row maximum of ll is taken out
 * before exp, alpha is normalised at every step and the log normalisers and maxima are summed, so a trial of
 * thousands of rows with ll near -1e4 neither underflows nor loses the likelihood.  gamma holds alpha between the two
 * sweeps.  A trial is one serial chain: the call's time is (longest trial) x (step latency).
 * ws: bn_hmm_forward_backward_ws_bytes bytes (the offsets and two doubles a row).
 *
 * bn_arhmm_moments -> out (K, P, P): out[k] = sum over the AR rows of every trial of gamma[t][k] a_t^T a_t, both
 * triangles with the same bits, out[k][0][0] the state's expected count over the AR rows; and gamma0 (K): the sum of
 * gamma[t][k] over the initial rows (so sum_k (out[k][0][0] + gamma0[k]) is the number of rows in trials when gamma's
 * rows sum to 1).  gamma: (n, K), never written.  The rows are cut into row blocks (a function of (n, D, L, K)
 * alone), every (block, state) leaves one partial matrix in the workspace and the partials are added in block order.
 * ws: bn_arhmm_moments_ws_bytes bytes (60 MiB of partials at most, the offsets and one byte a row).
 *
 * bn_hmm_viterbi -> states int32 (n): the most likely state path of every trial, max-sum in float64.  A tie goes to
 * the lowest state, in every maximum over predecessors and at the trial's last row.  ws: bn_hmm_viterbi_ws_bytes
 * bytes (the offsets and uint8 back-pointers (n, K)).
 *
 * Every ws on a 16-byte boundary; nothing is read from it that the call has not written.  S == 0 returns 0 and writes
 * nothing.  BN_E_SHAPE (nothing written, to the outputs or to ws): K, L, D, n or S outside the limits (the queries
 * return 0 for these), ld < D, want not 0 or 1, a workspace smaller than the query's, z off a 4-byte, states off a
 * 4-byte, any float64 operand or offsets off an 8-byte, ws off a 16-byte boundary.  BN_E_BADARG: an operand NULL (c
 * may be; gamma and xi may be with want = 0). */
size_t bn_arhmm_loglik_ws_bytes(int n, int S, int D, int L, int K);
int bn_arhmm_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L, int K,
                    int n, const double* G, const double* cst, double* ll, void* ws, size_t ws_bytes,
                    bn_stream_t stream);
size_t bn_hmm_forward_backward_ws_bytes(int n, int S, int K);
int bn_hmm_forward_backward(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                            const double* logpi0, int want, double* gamma, double* xi, double* loglik, void* ws,
                            size_t ws_bytes, bn_stream_t stream);
size_t bn_arhmm_moments_ws_bytes(int n, int S, int D, int L, int K);
int bn_arhmm_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L, int K,
                     int n, const double* gamma, double* out, double* gamma0, void* ws, size_t ws_bytes,
                     bn_stream_t stream);
size_t bn_hmm_viterbi_ws_bytes(int n, int S, int K);
int bn_hmm_viterbi(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                   const double* logpi0, int* states, void* ws, size_t ws_bytes, bn_stream_t stream);

/* The same three launches for a GRID of M models on one table: models with the same D and L, their states side by
 * side as KT = sum K_m columns.  Model m owns the columns koff[m] .. koff[m + 1] of G (KT, D, P), cst (KT), ll (n, KT),
 * gamma (n, KT), out (KT, P, P) and gamma0 (KT), the entries xoff[m] .. xoff[m + 1] (xoff: prefix sums of K_m^2) of
 * logP -- its (K_m, K_m) matrix, row-major -- and of every row of xi (S, XT), and row m of loglik (M, S).
 * Limits: 1 <= K_m <= 32, KT <= 512, M <= 512, D, L, n and S as above.
 *
 * bn_arhmm_grid_loglik and bn_arhmm_grid_moments are bn_arhmm_loglik and bn_arhmm_moments for KT states: the same
 * kernels, the same arithmetic per state (full 16-state tiles, whole state groups, the table read once for all
 * models), the same partition rule (row blocks of at least 512 rows, the KT partials of all blocks within 60 MiB: the
 * blocks grow with KT).
 *
 * bn_hmm_grid_forward_backward: bn_hmm_forward_backward for every (trial, model).  koff, xoff: DEVICE int32 (M + 1);
 * order: DEVICE int32 (M), every model once -- the n4 models with K_m <= 4 first, then the n8 with 4 < K_m <= 8, the
 * n16 with 8 < K_m <= 16 and the n32 others (n4 + n8 + n16 + n32 = M).  One launch a class KP = 4, 8, 16, 32; a wave
 * takes one trial and 64 / KP models that follow each other in `order`, a slot of KP lanes a model.  Nothing crosses
 * a slot: a model's outputs have the same bits wherever it sits in `order` and whoever shares its wave, and a NaN or
 * Inf in a model's ll, logP or logpi0 stays in that model's outputs.  An entry of order outside [0, M), a K_m outside
 * its class and columns outside [0, KT) / [0, XT) make an empty slot (nothing read or written for it).  want = 0:
 * loglik only, gamma and xi may be NULL.  ws: bn_hmm_grid_forward_backward_ws_bytes bytes (the offsets and two doubles a
 * (model, row)).  BN_E_SHAPE / BN_E_BADARG as above; koff, xoff and order on 4-byte boundaries. */
size_t bn_arhmm_grid_loglik_ws_bytes(int n, int S, int D, int L, int KT);
int bn_arhmm_grid_loglik(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L, int KT,
                         int n, const double* G, const double* cst, double* ll, void* ws, size_t ws_bytes,
                         bn_stream_t stream);
size_t bn_arhmm_grid_moments_ws_bytes(int n, int S, int D, int L, int KT);
int bn_arhmm_grid_moments(const float* z, int ld, const double* c, const long long* offsets, int S, int D, int L,
                          int KT, int n, const double* gamma, double* out, double* gamma0, void* ws, size_t ws_bytes,
                          bn_stream_t stream);
size_t bn_hmm_grid_forward_backward_ws_bytes(int n, int S, int M, int KT, int XT);
int bn_hmm_grid_forward_backward(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                                 const int* koff, const int* xoff, const int* order, int n4, int n8, int n16, int n32,
                                 const double* logP, const double* logpi0, int want, double* gamma, double* xi,
                                 double* loglik, void* ws, size_t ws_bytes, bn_stream_t stream);

/* bn_hmm_grid_viterbi: bn_hmm_viterbi for every (trial, model) of a grid -> states int32 (M, n), row m the path of
 * model m.  ll, koff, xoff, order, n4 .. n32, logP and logpi0 exactly as bn_hmm_grid_forward_backward takes them, the
 * same packing (one launch a class, a slot of KP lanes a model) and the same empty-slot rules.  The arithmetic of a
 * slot is bn_hmm_viterbi's term for term, ties to the lowest state: a model's path has the integers bn_hmm_viterbi
 * gives on that model's own columns, wherever it sits in `order` and whoever shares its wave; a NaN in a model's ll
 * stays in that model's path, which still lies in [0, K_m).  Rows outside the trials are not written.
 * ws: bn_hmm_grid_viterbi_ws_bytes bytes (the offsets and uint8 back-pointers (n, KT)).  BN_E_SHAPE / BN_E_BADARG as
 * above; states on a 4-byte boundary. */
size_t bn_hmm_grid_viterbi_ws_bytes(int n, int S, int M, int KT, int XT);
int bn_hmm_grid_viterbi(const double* ll, const long long* offsets, int S, int M, int KT, int XT, int n,
                        const int* koff, const int* xoff, const int* order, int n4, int n8, int n16, int n32,
                        const double* logP, const double* logpi0, int* states, void* ws, size_t ws_bytes,
                        bn_stream_t stream);

/* The generative process of the same model, from noise the CALLER brings: no random number is drawn on the device, so
 * the call is a deterministic function of its operands (the same bits on every call).  Trials as above: offsets
 * int64 (S + 1) made safe, rows outside [e[0], e[S]) neither read nor written.  float64 but for init and the states.
 *
 * W: (K, D, 1 + L D), [b_k | A_k] in the model's own coordinates (no shift); C: (K, D, D), a factor of Sigma_k
 * (its lower Cholesky factor; all D columns are multiplied); cdf0: (K) and cdf: (K, K), the cumulative sums in state
 * order of exp(logpi0) and of every row of exp(logP), formed by the caller; eps: (n, D) standard-normal draws.
 * Exactly one of u: (n) uniform draws in [0, 1), and states_in: int32 (n).  init: NULL or fp32 (n, D) with row stride
 * ld_init >= D.  -> x (n, D) and states int32 (n).
 *
 * States from u: row 0 of a trial takes cdf0, row t > 0 row z_{t-1} of cdf, and z_t is the number of j in [0, K - 1)
 * with u_t >= cdf[j] -- the last column is never compared, so a row that sums below 1 cannot fall off the end, and
 * only comparisons happen on the device: the path is the caller's own, bit for bit.  With states_in, states is its
 * copy.  Rows: for t >= L  x_t = b_z + C_z eps_t + sum_l A_z[l] x_{t-1-l}  with the float64 x the call itself produced
 * (the drive b_z + C_z eps_t first, one FMA a column in ascending order; then per output row the L D products in NP
 * interleaved partial sums, NP = 8, 4, 2 for D up to 8, 16, 32, added as a fixed tree); for t < L  x_t = init[t]
 * widened, or eps_t without init (the model's N(0, I) initial rows).  L = 0 has no initial rows.
 * A NaN in init or eps stays inside its trial.  A state outside [0, K) in states_in makes its row and the rest of its
 * trial NaN in x (states still is the copy); nothing is read outside W and C for it.  One wave a trial for the states
 * and for the recursion, which is one serial chain: the call's time is (longest trial) x (step latency).
 * ws: bn_arhmm_sample_ws_bytes bytes (the offsets, one int a trial and one a row, C transposed), on a 16-byte
 * boundary.  S == 0 returns 0 and writes nothing.  BN_E_SHAPE (nothing written): K, L, D, n or S outside the limits
 * (the query returns 0 for these), init with ld_init < D, a workspace smaller than the query's, a float64 operand or
 * offsets off an 8-byte, init, states_in or states off a 4-byte, ws off a 16-byte boundary.  BN_E_BADARG: an operand
 * NULL (init may be), or both or neither of u and states_in. */
size_t bn_arhmm_sample_ws_bytes(int n, int S, int D, int L, int K);
int bn_arhmm_sample(const double* W, const double* C, const double* cdf0, const double* cdf, const long long* offsets,
                    int S, int D, int L, int K, int n, const double* eps, const double* u, const int* states_in,
                    const float* init, int ld_init, double* x, int* states, void* ws, size_t ws_bytes,
                    bn_stream_t stream);

/* One-step-ahead predictions of the same model, in the latents' own units.  Trials, limits, alignment and error rules
 * as above; rows outside [e[0], e[S]) are neither read nor written.  No atomics, every sum in a fixed order: the same
 * bits on every call.
 *
 * bn_hmm_predictive -> w (n, K): the causal state weights w_t = p(z_t | x_0 .. x_{t-1}) of every trial.  ll, logP and
 * logpi0 as bn_hmm_forward_backward takes them.  w_0 = exp(logpi0) and w_t[j] = sum_i ahat_{t-1}[i] P[i][j] divided by
 * sum_i ahat_{t-1}[i], with ahat the filtered marginals of bn_hmm_forward_backward's scaled forward sweep: one wave a
 * trial, that sweep with one store a step added (the call's time is (longest trial) x (step latency)).  Row t of ll
 * does not reach w_t.  A row of ll that is not finite makes the weights of the LATER rows of its trial non-finite (all
 * K of each) and touches nothing else.  ws: bn_hmm_predictive_ws_bytes bytes (the offsets).
 *
 * bn_arhmm_predict -> xhat (n, D): for an AR row  xhat_t = sum_k w_t[k] (b_k + sum_l A_k[l] x_{t-1-l}),  for an
 * initial row (nothing to predict from) the row's own values widened.  W: (K, D, 1 + L D), [b_k | A_k] in the model's
 * own coordinates as bn_arhmm_sample takes it; w: (n, K), any weights (bn_hmm_predictive's, or gamma of
 * bn_hmm_forward_backward for the smoothed mean); read for AR rows only.  The (n x K Q) (K Q x D) product, Q = 1 + L D,
 * on v_mfma_f64_16x16x4_f64 with the A entry w_t[k] phi_t[q], phi_t = (1, x_{t-1}, .., x_{t-L}); sums over (k, q) in
 * ascending order.  No shift: a product of fp32 values in float64, not a difference of moments.  A NaN or Inf in row t
 * of z reaches xhat of the AR rows among the L rows after it in its trial (and row t itself if it is an initial row);
 * one in row t of w reaches row t of xhat.  ws: bn_arhmm_predict_ws_bytes bytes (the offsets, one byte a row and W
 * as a padded operand, under 1 MiB).  BN_E_SHAPE also for ld < D. */
size_t bn_hmm_predictive_ws_bytes(int n, int S, int K);
int bn_hmm_predictive(const double* ll, const long long* offsets, int S, int K, int n, const double* logP,
                      const double* logpi0, double* w, void* ws, size_t ws_bytes, bn_stream_t stream);
size_t bn_arhmm_predict_ws_bytes(int n, int S, int D, int L, int K);
int bn_arhmm_predict(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int n,
                     const double* W, const double* w, double* xhat, void* ws, size_t ws_bytes, bn_stream_t stream);

/* Exact multi-step forecasts of the same model and their sums.  Origin row t of a trial forecasts the rows
 * t .. t + H - 1 of its trial from the history before t:  xhat_{t,h} = E[x_{t+h-1} | x_0 .. x_{t-1}]
 * = sum_k w_t[k] N_h[k] phi_t,  phi_t = (1, x_{t-1}, .., x_{t-L}), with N: (H, K, D, 1 + L D) the forecast maps
 * (N_1[k] = [b_k | A_k]; models/arhmm.py forecast_maps) and w: (n, K) the causal weights of bn_hmm_predictive.  The
 * pair
 * (t, h) counts iff t - beg >= max(L, 1) and t + h - 1 < end.
 * -> sums (H, S, D, 5): per horizon, trial and dimension over the pairs that count, with y = x_{t+h-1}: the count,
 * sum y, sum y^2, sum (y - xhat_{t,h})^2 and sum (y - x_{t-1})^2 (the h-step persistence baseline).  The forecasts
 * themselves are not written.  H <= 32; the other limits, alignment and error rules as above.  The
 * (n x K Q) (K Q x H D) product on v_mfma_f64_16x16x4_f64; the targets are widened and the five terms formed in
 * float64.
 * Row blocks of at most 256 origin rows never cross a trial; a block's rows are added in a fixed order and a trial's
 * blocks in block order, no atomics: the same bits on every call and for every ld.  Rows outside [e[0], e[S]) are
 * never read, and w is read for origin rows only.  A NaN or Inf in a row of z or of w makes sums of its own trial
 * non-finite and touches no other trial.  A trial without a pair gets zeros.  ws: bn_arhmm_forecast_sums_ws_bytes
 * bytes (the offsets, the block plan, N as a padded operand and one (H, D, 5) partial a row block: (n / 256 + S) of
 * them at most); 0 for sizes that are not served.  BN_E_SHAPE also for ld < D. */
size_t bn_arhmm_forecast_sums_ws_bytes(int n, int S, int D, int L, int K, int H);
int bn_arhmm_forecast_sums(const float* z, int ld, const long long* offsets, int S, int D, int L, int K, int H, int n,
                           const double* N, const double* w, double* sums, void* ws, size_t ws_bytes,
                           bn_stream_t stream);

/* The runs of a table of discrete states (get_discrete_chunks / get_state_durations of plotting/arhmm_utils.py:24-99,
 * which pad and difference every trial on the host): states int32 (n), the output of bn_hmm_viterbi; offsets int64
 * (S + 1) made safe as above (clamped into [0, n], ascending), empty trials allowed; rows outside [e[0], e[S]) are
 * never loaded.  1 <= K <= 32.  A run is a maximal stretch of equal states inside ONE trial: row i of trial s starts
 * one iff i == e[s] or states[i] != states[i - 1], so two neighbouring trials that end and begin in the same state
 * are two runs.
 *   runs    int32 (runs_cap, 4): row p = (trial, beg, end, state) of the p-th run in the order of the table rows
 *           the runs begin at, beg and end relative to e[trial], end exclusive; rows p >= runs_cap are not written
 *           (n rows always suffice) and rows p >= n_runs are left as they are
 *   frames  int64 (K): the rows in trials per state
 *   trans   int64 (K, K): trans[j][k] = the rows i with states[i - 1] == j, states[i] == k and both in one trial
 *           (self-pairs included)
 *   n_runs  int64: the number of runs, whatever runs_cap is
 *   bad     int64: the rows in trials whose state is outside [0, K); they count in neither frames nor trans, and the
 *           caller is expected to refuse the result when bad != 0
 * Positions come from a prefix sum over the start flags (tiles of 1024 rows, their counts scanned by one workgroup),
 * never from the order atomics land in; frames, trans and bad are integer sums from LDS histograms.  So every
 * output is exact and the same for every launch geometry.  n up to 2^31 - 1.
 * ws: bn_state_runs_ws_bytes bytes (the offsets and two ints per tile of rows) on a 16-byte boundary.  S == 0 returns
 * 0 and writes nothing; n == 0 with S > 0 writes zeros to frames, trans, n_runs and bad.  BN_E_SHAPE (nothing
 * written): K, n or S outside the limits (the query returns 0 for these), runs_cap < 0, a workspace smaller than the
 * query's, states off a 4-byte, an int64 operand off an 8-byte, runs or ws off a 16-byte boundary.  BN_E_BADARG: an
 * operand NULL (states may be when n == 0, runs when runs_cap == 0). */
size_t bn_state_runs_ws_bytes(int n, int S, int K);
int bn_state_runs(const int* states, const long long* offsets, int S, int K, int n, int* runs, long long runs_cap,
                  long long* frames, long long* trans, long long* n_runs, long long* bad, void* ws, size_t ws_bytes,
                  bn_stream_t stream);

/* unit-float frames -> stored uint8 grey levels, the inverse of bn_u8_to_unit_float on k / 255:
 *   out[i] = NaN -> 0, else clamp(rint(in[i] * 255), 0, 255)
 * The product is one fp32 multiplication and rint rounds half to even, i.e. numpy's
 * rint(float32(x) * float32(255)) bit for bit; values below 0 and above 1 saturate.  Any n.  16-byte
 * loads and stores where `in` and `out` both sit on a 16-byte boundary, element by element otherwise,
 * with the same arithmetic.  BN_E_SHAPE (nothing written) for an `in` off a 4-byte boundary. */
int bn_unit_float_to_u8(const float* in, unsigned char* out, size_t n, bn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * In-library kernel timing used by bench.py's roofline line: when enabled, every call of the
 * selected kernel family is bracketed by hipEvents on its own stream, and the dispatch of its
 * main kernel carries a second pair.
 * ------------------------------------------------------------------------------------------ */
#define BN_PROF_NONE        0
#define BN_PROF_CONV_FWD    1
#define BN_PROF_CONV_BWD_D  2
#define BN_PROF_CONV_BWD_W  3
#define BN_PROF_CONVT_FWD   4
#define BN_PROF_CONVT_BWD_D 5
#define BN_PROF_CONVT_BWD_W 6
#define BN_PROF_ADAM        7
#define BN_PROF_LINEAR_FWD  8   /* nn.Linear forward; C = in features, K = out features */
#define BN_PROF_LINEAR_BWD  9   /* nn.Linear backward: all launches of one bn_linear_bwd call */
/* select family + optional geometry filter (C<=0 / K<=0 = any).  Resets the accumulators. */
int bn_prof_select(int family, int C, int K);
/* the same, but only the nth (0-based) matching call after the selection is timed: tells layers
 * apart that share a family and a channel pair (ae_arch_2.json: four 64 -> 64 layers) */
int bn_prof_select_nth(int family, int C, int K, int nth);
/* host-synchronising: total milliseconds and call count since bn_prof_select, everything a
 * call launched (its combine / finish kernels, the two event records and the gaps included) */
int bn_prof_read(double* total_ms, long* launches);
/* the same calls, the MAIN kernel of each alone: interval of the events attached to its dispatch
 * (launches = 0 when the path that served the call does not attach them) */
int bn_prof_read_main(double* total_ms, long* launches);
/* on == 0: no bracketing event records (only the dispatch pair; nothing extra goes on the stream
 * inside a timed region).  Returns the previous setting; default on. */
int bn_prof_set_bracket(int on);
/* name of the device kernel that served the most recent launch of the selected family */
const char* bn_prof_kernel_name(void);
/* constant part of a dispatch-attached event interval (empty kernel, minimum over iters), us */
double bn_prof_dispatch_overhead_us(int iters, bn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BEHAVENET_HIP_H */
