/* libsvae_hip.so — C ABI of the MI355X Sequential-VAE training-step engine.
 *
 * Drop-in boundary.  The reference has no FFI: its path sits
 * behind the Python methods
 *     SequentialVAE.train(input_batch, batch_target) -> float   sequential_vae.py:1341-1375
 *     SequentialVAE.test(input_batch) -> ndarray[B,H,W,C]        sequential_vae.py:1381-1391
 * which run  sess.run([train_op, loss, final_loss])  (sequential_vae.py:1365) over the
 * graph built by construct_network (sequential_vae.py:877-984).  The Python mirror of that
 * interface (sequential-variational-autoencoder_amd/sequential_vae.py) binds the entry points
 * below through ctypes; the binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success or a negative svae_status; the
 * message is available from svae_last_error(ctx) (ctx may be NULL for create/layout
 * errors).  No function calls exit().  All device work is enqueued on the caller's
 * stream (hipStream_t passed as void*); no call allocates or synchronises on the hot
 * path.  Tensors are NHWC fp32, row-major.
 */
#ifndef SVAE_HIP_H
#define SVAE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum svae_status {
  SVAE_OK = 0,
  SVAE_EBADCONFIG = -1, /* config rejected (sequential_vae.py:861-862, :1617-1627 analogue) */
  SVAE_EBADARG = -2,    /* null pointer / unbound buffers / bad index */
  SVAE_EHIP = -3,       /* HIP runtime error */
  SVAE_ENOMEM = -4      /* device allocation failed */
};

/* Geometry + hyper-parameters of one SequentialVAE (sequential_vae.py:201-258, netname
 * overrides :281-862).  Only the executed-path knobs of the BASELINE configs. */
typedef struct svae_config {
  int32_t batch;            /* per-GPU batch B (BN statistics are per shard) */
  int32_t height, width, channels;   /* dataset.data_dims */
  int32_t levels;           /* vlae_levels L */
  int32_t mc_steps;         /* T */
  int32_t filter_sizes[10]; /* L+2 entries */
  int32_t latent_dims[8];   /* L entries */
  int32_t intermediate_reconstruction;
  float first_step_loss_coeff;
  float latent_prior_stddev;
  float latent_mean_clip;   /* +inf = no clip */
  float range_lo, range_hi; /* dataset.range */
  float min_highway, max_highway;
  int32_t dtype;            /* 0 = fp32 (parity, fp32 MFMA); 1 = bf16 MFMA, fp32 accumulate (throughput);
                             * 2 = bf16x6: fp32-accurate on bf16 MFMA (operands split into bf16 planes,
                             * 6 plane products in the forward / input-gradient GEMMs, 3 in the
                             * weight-gradient GEMMs; fp32 storage) */
  /* homogeneous chain (sequential_vae.py:107-113, scopes :1573-1577, :1683-1687, :1757-1761):
   * share_phi: one "phi/inference_network" for every step; share_theta: one
   * "theta/generative_encoder_network" and one "theta/generative_network" for steps >= 1
   * ("theta/generative_step_0" stays its own).  The parameter table then lists each shared
   * tensor once and its gradient is the sum over the steps that use it. */
  int32_t share_theta, share_phi;
  /* Latent InfoMax (predict_latent_code :129-131, create_recognition_network :1013-1020):
   * q(z_t | x_{t-1}) for t >= 1 (gradient flows into x_{t-1}); the KL term only at step 0
   * unless predict_latent_code_with_regularization (:1170-1172).  Under share_phi step 0 keeps
   * its own "phi/inference_step_0" (:1573). */
  int32_t predict_latent_code, predict_latent_code_with_regularization;
  /* regularized_steps (:220, :1154): bit t set = step t carries NO KL term (0 = every step) */
  uint32_t unregularized_steps_mask[2];
  /* ---- chain variants ---- */
  int32_t use_uniform_prior;          /* KL_b = mean_d(-log sigma) (:1159-1160) */
  /* add_noise_to_chain (:1088-1090): the sample fed to step t+1 is mle_t + reg * sd_t * N(0,1);
   * sd_t = noise_stddevs[t] (:1665-1666), or predicted (below).  The loss keeps the MLE. */
  int32_t add_noise_to_chain;
  float noise_stddevs[64];            /* mc_steps entries (:239) */
  /* predict_generator_noise (:1667, stddevs_prediction :1866-1875): sd_t = max * sigmoid(1x1 conv of
   * stddev_layers x conv2d_bn_lrelu(4x4, s1) of the output conv-T's sigmoid); the reconstruction
   * term becomes the Gaussian NLL mean(log sd + 0.5 log 2pi + 0.5 ((mle - target)/sd)^2) (:1149-1150).
   * Requires add_noise_to_chain.  Filter sizes <= 8 (reference default 5 x 5). */
  int32_t predict_generator_noise;
  float predict_generator_stddev_max;
  int32_t stddev_layers;
  int32_t stddev_filter_sizes[8];
  /* add_improvement_maximization_loss (:1182-1201): imp = reg * latent_pred_loss_coeff *
   * -mean_b sum_{t>=1} ||mle_t - mle_{t-1}||^2, minimised over the recognition variables only by its
   * own clip + Adam update (:1299-1316): svae_backward_imp / svae_adam_imp. */
  int32_t add_improvement_maximization_loss;
  float latent_pred_loss_coeff;
  /* External generator (c_pixelvae, :529-543; generator_pixelcnn :1943-1971): steps t >= this run
   * the caller's generator (the PixelCNN++ head of svae_pcnn.h); the engine runs only their
   * recognition (z_t, KL_t) and creates no encoder / generator variables for them.  The caller hands
   * d loss / d x_hat_{e-1} and d loss / d z_t back with svae_set_external_grads.  0 = off. */
  int32_t external_generator_from;
  /* Flat generator (the "infusion" netnames c_infusion_test :769, c_homog_infusion_test :775 / :793,
   * m_infusion_test :781; generator_flat :1880-1936): step 0 stays the ladder generator; every step
   * t >= 1 maps the previous sample to x_hat_t through flat_conv_layers - 1 conv2d_bn_lrelu (4x4,
   * stride 1, flat_conv_filter_sizes[1..] channels) and one sigmoid conv2d (xavier, live bias) at full
   * resolution, in scope theta/generative_flat_step_<t> (share_theta: theta/generative_network_flat).
   * No encoder, split-latent, highway or shortcut: z_t (t >= 1) reaches the loss through its KL term
   * only.  Requires add_noise_to_chain; not with predict_generator_noise, predict_latent_code,
   * add_improvement_maximization_loss or external_generator_from.  flat_conv_layers in [1, 8]; the
   * sizes in [1, 32], [0] = channels; entry flat_conv_layers is never read (:245-247). */
  int32_t flat_generator;
  int32_t flat_conv_layers;
  int32_t flat_conv_filter_sizes[9];
} svae_config;

typedef struct svae_param_desc {
  char name[96];            /* TF variable name, e.g. "phi/inference_step_0/Conv/weights" */
  int32_t ndim;
  int32_t shape[4];         /* TF shape: conv [kh,kw,Cin,Cout], conv-T [kh,kw,Cout,Cin], FC [in,out] */
  int64_t offset;           /* element offset in the flat parameter / gradient buffers */
  int32_t init;             /* 0 zeros, 1 normal(0,0.02), 2 glorot-uniform */
  int32_t flags;            /* bit0: dead (never on the executed path), bit1: gradient identically 0 */
} svae_param_desc;

typedef struct svae_ctx svae_ctx;

/* Buffers readable through svae_copy_out. */
enum svae_buffer {
  SVAE_BUF_XHAT = 0,     /* training_mles[t]  [B,H,W,C] (sequential_vae.py:962) */
  SVAE_BUF_MU = 1,       /* latent mean (pre-clip) [B,Dz] */
  SVAE_BUF_SIGMA = 2,    /* latent stddev [B,Dz] */
  SVAE_BUF_Z = 3,        /* latent sample [B,Dz] */
  SVAE_BUF_STEP_STATS = 4, /* [T][2] = (mean_b recon_t, mean_b KL_t)   (:1163-1164) */
  SVAE_BUF_REC_IMG = 5,  /* [B] per-image recon of step t */
  SVAE_BUF_KL_IMG = 6,   /* [B] per-image KL of step t */
  SVAE_BUF_DZ = 7,       /* [B,Dz] d loss / d z_t (after svae_backward) */
  SVAE_BUF_SAMPLE = 8,   /* training_samples[t] [B,H,W,C] (= the MLE without chain noise, :963) */
  SVAE_BUF_STDDEV = 9,   /* predicted stddevs [B,H,W,1] of step t (predict_generator_noise) */
  SVAE_BUF_IMP_IMG = 10  /* [B] ||mle_t - mle_{t-1}||^2 per image (improvement loss, t >= 1) */
};

/* Hash (16 hex digits) of the sources this library was compiled from (build.py src_hash); the
 * Python mirror refuses a library whose hash differs from its tree's.  No reference counterpart. */
const char* svae_build_hash(void);

/* Parameter table (pure host; callable without a GPU).  Live (trainable, non-zero-grad)
 * tensors occupy [0, n_live); dead / pre-BN-bias tensors the tail [n_live, n_total). */
int svae_param_count(const svae_config* cfg, int64_t* n_total, int64_t* n_live, int32_t* n_tensors);
int svae_param_layout(const svae_config* cfg, svae_param_desc* out, int32_t cap);

/* Context: owns the activation arena (sized for cfg->batch) and Adam state. */
int svae_create(const svae_config* cfg, int device, svae_ctx** out);
int svae_destroy(svae_ctx* ctx);
const char* svae_last_error(const svae_ctx* ctx);
/* Borrow caller-owned flat fp32 buffers (n_total elements each). */
int svae_bind(svae_ctx* ctx, float* params, float* grads);
int64_t svae_workspace_bytes(const svae_ctx* ctx);

/* Forward of the whole chain: x, target [B,H,W,C]; eps [T,B,Dz] or NULL (device Philox).
 * reg_coeff as fed at sequential_vae.py:1357. */
int svae_forward(svae_ctx* ctx, const float* x, const float* target, const float* eps, float reg_coeff,
                 void* stream);
/* d self.loss / d every variable (sequential_vae.py:1273) into the bound gradient buffer. */
/* Generative mode (sequential_vae.py:947-952 / :1025 / generate_mc_samples :1393-1428): run the
 * unrolled generator chain on latents z [T,B,Dz] fp32 (device; NULL = N(0,1) drawn on device),
 * without the recognition networks: x_0 = generator_first_step(z_0), x_t = generator(x_{t-1}, z_t),
 * BatchNorm on the generated batch's statistics (training mode, as the reference's shared
 * variables).  Outputs via svae_copy_out(SVAE_BUF_XHAT, t).  Invalidates the training forward
 * state (svae_backward needs a new svae_forward). */
int svae_generate(svae_ctx* ctx, const float* z, void* stream);
int svae_backward(svae_ctx* ctx, void* stream);
/* external_generator_from = e: gradients from the caller's generator steps for the NEXT backward
 * (device pointers, one-shot): dxhat [B,H,W,C] = d loss / d x_hat_{e-1} (the chain sample the
 * external step reads, e.g. the PixelVAE highway's previous sample, pixelvae.py:136), dz [T,B,Dz]
 * whose rows t >= e are d loss / d z_t (the head's conditioning and highway ratio, :123-136); the
 * KL terms' gradients are the engine's own.  NULL = zero. */
int svae_set_external_grads(svae_ctx* ctx, const float* dxhat, const float* dz);
/* Chain noise N(0,1) [T,B,H,W,C] for the NEXT svae_forward or svae_generate only (device pointer,
 * kept by reference until that call's backward; NULL or not set = drawn on device, as
 * tf.random_normal :1090-1091).  One-shot: every forward / generate call clears it, so a generative
 * chain never reuses the noise injected for an earlier training forward. */
int svae_set_chain_noise(svae_ctx* ctx, const float* noise);
/* The counter of the context's own Philox draws (eps, prior latents and chain noise drawn on the device when the
 * caller passes none; every such draw advances it).  *get (may be NULL) receives the current value, then *set (may
 * be NULL) replaces it: a checkpoint that carries it lets a resumed run draw what the uninterrupted run would. */
int svae_rng_offset(svae_ctx* ctx, const uint64_t* set, uint64_t* get);
/* Improvement-maximisation loss (add_improvement_maximization_loss): bind a caller-owned gradient
 * buffer (n_total elements, public layout), then after svae_forward, svae_backward_imp writes
 * d imp / d every variable into it (the optimiser uses only the recognition part, :1302).
 * svae_adam_imp applies clip + Adam to the recognition variables [0, phi_end) with that gradient and
 * the same Adam moments (one AdamOptimizer, :1267); *phi_end from svae_imp_range. */
int svae_bind_imp(svae_ctx* ctx, float* grads_imp);
int svae_backward_imp(svae_ctx* ctx, void* stream);
int svae_adam_imp(svae_ctx* ctx, float lr, int64_t step, float clip, void* stream);
int svae_imp_range(svae_ctx* ctx, int64_t* phi_end);
/* Data-parallel hook (no reference counterpart; the reference has no collective).  During
 * svae_backward, hook(user, t) is called on the host after the backward of chain step t is
 * enqueued (t = T-1 .. 0): at that point svae_hook_stream(ctx) is ordered after every kernel of
 * that step, so a collective enqueued on it reduces the step's complete generator/encoder
 * gradients while the earlier steps' backward still runs.  hook(user, -1) follows the whole
 * backward (recognition gradients complete, on the caller's stream).  NULL hook: off. */
typedef void (*svae_step_hook)(void* user, int t);
int svae_set_backward_hook(svae_ctx* ctx, svae_step_hook hook, void* user);
void* svae_hook_stream(svae_ctx* ctx);
/* clip(+-clip) + TF Adam on the live region (sequential_vae.py:1274-1276); step >= 1.  In bf16
 * mode (no weight sharing) the update also refreshes the engine's bf16 weight copies, and the next
 * svae_forward reuses them when the updates since the last forward covered the whole live region.
 * Parameters the caller writes itself must be announced with svae_bind before the next forward. */
int svae_adam(svae_ctx* ctx, float lr, int64_t step, float clip, void* stream);
/* The same update on the live sub-range [lo, hi) (lo a multiple of 4; tensor-aligned ranges). */
int svae_adam_range(svae_ctx* ctx, int64_t lo, int64_t hi, float lr, int64_t step, float clip, void* stream);
/* svae_backward then svae_adam as one call (sess.run(train_op), sequential_vae.py:1365), bit for bit
 * the same parameters: each chain step's generator/encoder bucket is updated on the engine's side
 * stream as soon as its gradient is final, right after hook(user, t) -- a hook that exchanges
 * gradients must have made svae_hook_stream(ctx) wait for the exchange of that bucket before it
 * returns -- and the recognition bucket after hook(user, -1).  Shared weights: the two calls in
 * sequence. */
int svae_backward_adam(svae_ctx* ctx, float lr, int64_t step, float clip, void* stream);
/* Polyak (exponential moving) average of the parameters, TF's ExponentialMovingAverage.apply.  ema is a
 * caller-owned device buffer of n_total floats in the public layout, borrowed until changed; omd = 1 - decay_t in
 * [0, 1].  Sticky: ema == NULL or omd == 0 turns it off, and with it off no launch is made.  While on, every Adam
 * update of a live range [lo, hi) (svae_adam, svae_adam_range, the buckets of svae_backward_adam, svae_adam_imp) is
 * followed on the same stream by svae_op_ema(ema + lo, params + lo, hi - lo, omd): under svae_backward_adam a
 * bucket's average moves on the side stream as soon as that bucket's Adam is done.  One training step therefore
 * averages every live parameter exactly once, after its last update.  With a gradient buffer bound by
 * svae_bind_imp the recognition range [0, phi_end) gets two updates per step, so svae_adam, svae_adam_range and
 * svae_backward_adam leave that range of the average alone and svae_adam_imp averages it after its own update (a
 * caller that never calls svae_adam_imp never averages it).  Parameters, Adam moments and the bf16 / fp16 weight
 * copies are bit for bit what they are with averaging off.  The dead tail [n_live, n_total) of ema is never
 * written: the caller initialises it (a copy of the parameters).  SVAE_EBADARG: null ctx, omd outside [0, 1] or
 * NaN. */
int svae_set_ema(svae_ctx* ctx, float* ema, float omd);
/* Adam moments of the live region [0, n_live) (tf.train.Saver's "<var>/Adam", "<var>/Adam_1" slots,
 * abstract_network.py:124-152): dir 0 copies them out to m, v; dir 1 in.  Device pointers. */
int svae_adam_state(svae_ctx* ctx, int dir, float* m, float* v, int64_t n, void* stream);
/* Copy an internal buffer (device -> caller device pointer). */
int svae_copy_out(svae_ctx* ctx, int which, int step, float* dst, int64_t n, void* stream);

/* Launch probe (instrumentation, no reference counterpart): between begin and end, every
 * launch of the bf16 GEMM instance `kernel_id` (see svae_kernel_name) issued by forward /
 * backward is bracketed by an event pair on the launch stream.  end() synchronises those
 * events and returns the launch count, the number timed (<= max_launches), their summed
 * algorithmic FLOPs and summed duration in ms.  Used by bench.py for roofline.achieved. */
int svae_probe_begin(svae_ctx* ctx, int kernel_id, int max_launches);
int svae_probe_end(svae_ctx* ctx, int64_t* launches, int64_t* timed, double* flops, double* total_ms);
const char* svae_kernel_name(int kernel_id);

/* ---- per-op entry points (kernel-level parity tests) ---- */
/* TF-SAME conv2d (transpose=0, W [4,4,Cin,Cout]) or conv2d_transpose (transpose=1,
 * W [4,4,Cout,Cin]) forward on x [N,H,H,Cin]; stride 1|2. */
int svae_op_conv(const float* x, int n, int h, int cin, const float* w, int cout, int stride, int transpose,
                 float* y, void* stream);
/* input gradient and weight gradient of the same op */
/* bf16 gather-GEMM (throughput mode kernels): y = conv2d (transpose=0) or conv2d_transpose
 * (transpose=1) of fp32 NHWC x with bf16 weights already in the engine's NK shadow layout
 * w_nk[tap][cout][cin] (tap = ky*4+kx); x is rounded to bf16 while staged, fp32 accumulate.
 * path: 0 per-tap gather kernel, 1 halo-tile kernel (SVAE_EBADARG if the shape does not
 * qualify), 2 automatic.  scratch (optional) enables split-K.  path | 16: the split-bf16 mode
 * (dtype bf16x6): w_nk holds three planes of 16*cin*cout elements each (x = p0 + p1 + p2); path | 48:
 * two more planes follow, the scaled fp16 pair fp16(w * 2^10), fp16(w * 2^10 - h0) that the
 * wave-split gathers use in that mode. */
int svae_op_gather_bf16(const float* x, int n, int h, int cin, const void* w_nk, int cout, int stride, int transpose,
                        int path, float* y, void* scratch, int64_t scratch_bytes, void* stream);
/* bf16 weight gradient of a conv (transpose=0) / conv-T (transpose=1) layer: dw in TF layout
 * ([4,4,cin,cout] / [4,4,cout,cin]) from fp32 NHWC x and dy, operands rounded to bf16, fp32
 * accumulation.  path: 0 tap-merged weight-GEMM kernel, 2 halo weight-GEMM where it qualifies;
 * + 16: x is a bf16 tensor, + 32: dy is a bf16 tensor (the engine's bf16 activation / BN-backward
 * storage, opload.h).  + 32 is ignored for a layer whose input gradient takes the fp32 small-N gather, as the
 * engine keeps that layer's dy in fp32: cin % 4 != 0, unless it is a conv with cout % 32 == 0.
 * + 64: the split mode (dtype bf16x6): fp32 x and dy, each staged as two bf16 planes, three plane products
 * per pair (opload.h split8 / mfma_split<2>); SVAE_EBADARG together with + 16 or + 32.
 * scratch: split slab (required). */
int svae_op_wgrad_bf16(const float* x, int n, int h, int cin, const float* dy, int cout, int stride, int transpose,
                       int path, float* dw, void* scratch, int64_t scratch_bytes, void* stream);
/* kernel the last svae_op_wgrad_bf16 call of this process launched, as the engine's dispatch recorded it
 * (pure host; SVAE_WGRAD_NONE before the first call or after one that failed before its launch) */
enum {
  SVAE_WGRAD_NONE = 0,
  SVAE_WGRAD_TAP_MERGED = 1, /* wgrad_bf16_kernel, taps merged into M */
  SVAE_WGRAD_HALO = 2,       /* wgrad_halo_kernel, run-time geometry (bf16 mode only) */
  SVAE_WGRAD_HALO2 = 3,      /* wgrad_halo2_kernel, compile-time geometry */
  SVAE_WGRAD_SMALLC = 4,     /* wgrad_smallc_kernel, <= 4 image channels */
  SVAE_WGRAD_FP32 = 5        /* the fp32 weight-GEMM (never from svae_op_wgrad_bf16) */
};
int svae_op_wgrad_last_kernel(void);
int svae_op_conv_dgrad(const float* dy, int n, int h, int cin, const float* w, int cout, int stride, int transpose,
                       float* dx, void* stream);
int svae_op_conv_wgrad(const float* x, int n, int h, int cin, const float* dy, int cout, int stride, int transpose,
                       float* dw, void* scratch, int64_t scratch_bytes, void* stream);
/* Flat-generator layer (4x4 stride-1 TF-SAME conv, W [4,4,cin,cout], cin, cout <= 32; exact fp32 on
 * v_mfma_f32_16x16x4_f32).  in_mean / in_invstd / in_beta != NULL: the conv reads lrelu(bn(x)) of
 * the producer's pre-BN tensor x (zeros pad the activated tensor); NULL: x as it is.  stats_out
 * (optional): 2*cout floats, (sum, sum of squares) of y per channel, interleaved.  SVAE_EBADCONFIG
 * when the block's window does not fit the LDS.  With stats_out the call keeps a process-wide device
 * scratch for the block partials, grown (device synchronise + reallocation) when a larger shape comes
 * and never freed: a test entry point, not for stream capture or concurrent callers (the engine's own
 * partials live in its arena). */
int svae_op_flat_conv(const float* x, int n, int h, int cin, const float* w, int cout, const float* in_mean,
                      const float* in_invstd, const float* in_beta, float* y, float* stats_out, void* stream);
/* its input gradient dx [n,h,h,cin] from dy [n,h,h,cout], and its weight gradient dw [4,4,cin,cout]
 * (scratch: the per-block slabs, >= ceil(h / max(1, 256 / h)) * n * 16*cin*cout floats) */
int svae_op_flat_dgrad(const float* dy, int n, int h, int cin, const float* w, int cout, float* dx, void* stream);
int svae_op_flat_wgrad(const float* x, int n, int h, int cin, const float* dy, int cout, float* dw, void* scratch,
                       int64_t scratch_bytes, void* stream);
/* training BN (+act 0 none,1 relu,2 lrelu) over rows of x [rows,C].
 * scratch: >= 1032*c bytes (sharded fixed-point column accumulators + constants); bwd: >= 1024*c bytes */
int svae_op_bn_act(const float* x, int64_t rows, int c, const float* beta, int act, float* y, float* mean,
                   float* invstd, void* scratch, int64_t scratch_bytes, void* stream);
int svae_op_bn_act_bwd(const float* dy, const float* y, const float* x, int64_t rows, int c, const float* mean,
                       const float* invstd, int act, float* dx, float* dbeta, void* scratch, int64_t scratch_bytes,
                       void* stream);
/* y[B,N] = x[B,K] @ w[K,N]  (fully_connected, no bias) */
int svae_op_fc(const float* x, int b, int k, const float* w, int nout, float* y, void* stream);
/* FC GEMM of the bf16 and split modes: y[b][nout] = x[b][k] . w_nk[nout][k]^T through the engine's bf16
 * dispatch on a dense launch.  The FC forward (weights [out][in]) and the FC input gradient (weights
 * [in][out] read as n = in, k = out) are this launch at different shapes.  x fp32, rounded to bf16 while
 * staged; w_nk bf16.  path: 2 the engine's choice (dense_kw where it qualifies, else the tiled per-tap
 * kernel), 0 the tiled per-tap kernel.
 *   + 16: the split mode on three bf16 planes: w_nk holds three planes nout*k elements apart, fp32 x split
 *         in registers, six plane products
 *   + 32 (with + 16): two scaled fp16 planes fp16(w * 2^10), fp16(w * 2^10 - h0) follow the three; x takes
 *         a per-wave running exponent, three fp16 products
 *   + 64: x is a bf16 tensor (bf16 mode only: SVAE_EBADARG with + 16)
 * scratch (optional, NULL: no grid split): the split-K slabs.  *variant (may be NULL) reports the kernel.
 * No allocation, no synchronisation.  SVAE_EBADARG: k % 4 or nout % 4, + 32 without + 16, or a split
 * launch (+ 16) that has no split kernel (path 0, k % 16, nout % 32). */
enum { SVAE_DENSE_TILED = 0, SVAE_DENSE_KW = 1, SVAE_DENSE_KW_SPLITK = 2 };
int svae_op_dense_bf16(const void* x, int b, int k, const void* w_nk, int nout, int path, float* y, void* scratch,
                       int64_t scratch_bytes, int32_t* variant, void* stream);
/* FC weight gradient dw[k][nout] = x[b][k]^T . dy[b][nout] through the engine's weight-GEMM dispatch, set up
 * as the FC backward does (one tap, one split over the batch rows).  mode 0: fp32; 1: bf16 (operands rounded
 * while staged; + 16: x is a bf16 tensor, + 32: dy is a bf16 tensor); 2: the split mode (fp32 operands as
 * three bf16 planes, six plane products).  nout % 4 == 0.  No allocation, no synchronisation. */
int svae_op_fc_wgrad(const void* x, int b, int k, const void* dy, int nout, int mode, float* dw, void* stream);
/* ---- recognition heads, latent and split-latent kernels (csrc/misc.hip), each through the engine's own
 * launcher.  Device pointers unless said otherwise, the caller's stream, no allocation.  SVAE_EBADARG: a
 * null pointer, a non-positive size, d > 32 (heads), Dz > 256 (latent), k > 32 (split-latent), or what
 * the entry says below.  "groups" is the engine's T-batched recognition: group g of a tensor lies one
 * group stride after group g - 1. ---- */
/* number of K splits the heads forward writes: ceil(k / 2048) (pure host) */
int svae_op_heads_splits(int k);
/* kernel taken by a heads launch (reported through *variant, which may be NULL) */
enum { SVAE_HEADS_FWD_NARROW = 0, SVAE_HEADS_FWD_TILE = 1, SVAE_HEADS_FWD_SKINNY = 2 };
enum { SVAE_HEADS_BWD_ROWGROUP = 0, SVAE_HEADS_BWD_PLAIN = 1, SVAE_HEADS_BWD_TILE = 2 };
/* Partial products of both heads of one level: x [groups][b][k], wm and ws [k][d] per group, w_gs elements
 * apart; part [groups][nsplit][b][pcols].  Split s < svae_op_heads_splits(k) of row n receives
 * sum_{kk in split s} x[n][kk] * wm[kk][o] at column coff + o and the ws sum at column pcols / 2 + coff + o;
 * nothing else of part is written (rows past the level's own splits stay as they are: the latent forward
 * sums all nsplit rows, so the caller keeps them zero).  SVAE_EBADARG also for nsplit <
 * svae_op_heads_splits(k), an odd pcols, or coff + d > pcols / 2. */
int svae_op_heads_fwd(const float* x, int b, int k, const float* wm, const float* ws, int64_t w_gs, int d, float* part,
                      int nsplit, int pcols, int coff, int groups, int32_t* variant, void* stream);
/* Latent of a step from the head partials: part [groups][nsplit][b][2*Dz] with Dz = sum of dims[levels]
 * (dims: HOST pointer, 1 <= levels <= 8), eps, mu, sig, z [groups][b][Dz], kl_img [groups][b].  Biases bm, bs
 * [groups][Dz + levels * bias_gap]: every level's biases are a tensor of their own in the engine, so level l's
 * start bias_gap (>= 0) floats after the end of level l - 1's, and the first level's at the group's start.
 * mu = sum_s part + bm (raw), sig = sigmoid(sum_s part + bs), z = clamp(mu, +-clip) + sig * eps, kl_img =
 * mean_d(-0.5 - log sig + (sig^2 + clamp(mu)^2) / (2 prior^2)), or mean_d(-log sig) when uniform != 0. */
int svae_op_latent_fwd(const float* part, int nsplit, int b, int levels, const int32_t* dims, const float* bm,
                       const float* bs, int bias_gap, float clip, float prior, int uniform, const float* eps,
                       float* mu, float* sig, float* z, float* kl_img, int groups, void* stream);
/* Its backward: dhead [groups][b][2*Dz] = gradient of sum(dz * z) + kl_coef[g] * sum_n kl_img[n] with
 * respect to the raw mean (columns 0 .. Dz - 1; zero where |mu| > clip) and to the pre-sigmoid value
 * (columns Dz ..).  kl_coef: device, one float per group. */
int svae_op_latent_bwd(const float* mu, const float* sig, const float* eps, const float* dz, int b, int dz_dim,
                       const float* kl_coef, float prior, int uniform, float clip, float* dhead, int groups,
                       void* stream);
/* Heads backward of one level from columns coff .. coff + d - 1 (mean) and dcols / 2 + coff .. (stddev) of
 * dhead [groups][b][dcols]: dx [groups][b][k] = (accumulate ? dx : 0) + dhead_l @ [wm | ws]^T, dwm, dws
 * [k][d] = x^T dhead_l, dbm, dbs [d] = sum_n dhead_l.  wm, ws, dwm, dws, dbm and dbs all step w_gs elements
 * per group. */
int svae_op_heads_bwd(const float* x, float* dx, int b, int k, const float* wm, const float* ws, int64_t w_gs, int d,
                      const float* dhead, int dcols, int coff, float* dwm, float* dws, float* dbm, float* dbs,
                      int accumulate, int groups, int32_t* variant, void* stream);
/* split_latent level: out = lrelu_0.1(BN_batch(z[:, zoff : zoff + k] @ w) + beta) (biased variance, eps
 * 1e-3) for z [b][ldz], w [k][j], beta, mean, invstd [j]; element (n, jj) is written at
 * out + n * o_n + (jj / f) * ldo + jj % f.  nt == 1: one launch.  1 < nt <= 16: the chain's one launch over nt
 * steps; step i reads z + i * z_ts, w + i * w_ts, beta + i * bn_ts and writes mean / invstd + i * bn_ts and
 * out + i * out_ts. */
int svae_op_splitfc(const float* z, int ldz, int zoff, int b, int k, const float* w, const float* beta, int j, int f,
                    int ldo, int64_t o_n, float* mean, float* invstd, float* out, int nt, int64_t z_ts, int64_t w_ts,
                    int64_t bn_ts, int64_t out_ts, void* stream);
/* Its backward from dout (addressed like out) and the forward's mean / invstd: dw [k][j], dbeta [j], and
 * dz[n][zoff + kk] += the input gradient (dz [b][ldz]; the block partials go through scratch, at least
 * ceil(j / 64) * b * k floats). */
int svae_op_splitfc_bwd(const float* z, int ldz, int zoff, int b, int k, const float* w, const float* beta, int j,
                        int f, int ldo, int64_t o_n, const float* mean, const float* invstd, const float* dout,
                        float* dw, float* dbeta, float* dz, void* scratch, int64_t scratch_bytes, void* stream);
/* ---- the output tail of a chain step (csrc/misc.hip) and the chain-variant kernels (csrc/chain.hip), each group
 * of launches the engine always issues together through the engine's own launchers.  Device pointers, the caller's
 * stream and scratch, no allocation, no synchronisation.  SVAE_EBADARG (message prefixed by the op's name): a null
 * pointer that the entry does not allow, a non-positive size, or what the entry says below. ---- */
/* kernel family of a small-N gather launch, reported as variant[0]; variant[1] = lanes per pixel (LP; 0 for the
 * plain kernel) */
enum { SVAE_GCONV_PLAIN = 0, SVAE_GCONV_LP = 1, SVAE_GCONV_S2T = 2 };
/* pure host: the family and LP of a 4x4 small-N gather with k gathered channels at pitch lda, nout <= 4 outputs and
 * ho x wo output pixels per image; transpose != 0: the conv-T gather (the output layer and, with the roles of the
 * tensors exchanged, the input gradient svae_op_conv_dgrad runs for a conv layer with cin % 4 != 0: k = lda = cout,
 * nout = cin, ho = wo = h) */
int svae_op_gconv_variant(int k, int lda, int nout, int transpose, int stride, int ho, int wo, int32_t* variant);
/* family and LP of the last small-N gather launch of this process, as the launcher itself recorded it (-1, -1
 * before the first; pure host; a test entry point, one caller at a time, like svae_op_wgrad_last_kernel) */
int svae_op_gconv_last_kernel(int32_t* variant);
/* The small-N gather as it is: c [n,ho,wo,n0+n1] (+)= bias + the 4x4 conv (transpose = 0) or conv-T of
 * a [n,hi,wi,k] with w0 [16][n0][k] for columns 0 .. n0-1 and, when n1 > 0, w1 [16][n1][k] for the columns behind
 * them (the launcher's dual-pointer form); bias0 [n0] and bias1 [n1] may be NULL; accumulate != 0 adds into c.
 * k <= 256, n0 + n1 <= 4, stride 1|2; variant (two ints, may be NULL) reports the launch. */
int svae_op_gconv_smalln(const float* a, int n, int hi, int wi, int k, const float* w0, int n0, const float* w1, int n1,
                         const float* bias0, const float* bias1, int transpose, int stride, int accumulate, float* c,
                         int32_t* variant, void* stream);
/* The packed [C | ratio] output conv-T of a step: pack_out of w_out [4,4,c,f1], w_ratio [4,4,1,f1], b_out [c],
 * b_ratio [1] (w_ratio and b_ratio both NULL: step 0, the ratio row and its bias packed as zeros) into wpack
 * (16*(c+1)*f1 + 4 floats: [tap][c+1][f1] weights, then the 4 bias floats) and, in modes 1 and 2, its bf16 copy
 * wpack_h (mode 1: 16*(c+1)*f1 bf16; mode 2: three such planes, plane q = bf16(w - the earlier planes)); then the
 * stride-2 conv-T of x [n,hs,hs,f1] into a_out [n,2hs,2hs,c+1] through the engine's branch for the mode.
 *   mode 0: the fp32 small-N gather; variant = (SVAE_GCONV_*, LP).  wpack_h may be NULL.
 *   mode 1: the bf16 dispatch with the bias epilogue (x rounded to bf16 while staged); variant[0] =
 *           SVAE_OUTCONVT_SMALLN_BF16 or the bf16 GEMM instance id (svae_kernel_name), variant[1] = 0.
 *   mode 2: the split mode on the three planes where a split kernel takes the shape (variant as in mode 1), else
 *           the fp32 gather-GEMM on wpack (SVAE_OUTCONVT_FP32_GEMM), as the engine falls back.
 * f1 <= 256, and f1 % 4 == 0 in modes 1 and 2; x, wpack, wpack_h, a_out 16-byte aligned when f1 % 4 == 0.
 * scratch (optional, 16-byte aligned): split-K slabs of the bf16 dispatch. */
enum { SVAE_OUTCONVT_SMALLN_BF16 = 100, SVAE_OUTCONVT_FP32_GEMM = 101 };
int svae_op_output_convt(const float* x, int n, int hs, int f1, const float* w_out, const float* w_ratio,
                         const float* b_out, const float* b_ratio, int c, int mode, float* wpack, void* wpack_h,
                         float* a_out, void* scratch, int64_t scratch_bytes, int32_t* variant, void* stream);
/* output_fwd + loss_reduce on a [b,h,w,c+1]: out = (hi - lo) sigmoid(a[..c]) + lo; with xprev (may be NULL: step 0),
 * r = minh + (maxh - minh) sigmoid(a[c]) and xhat = r out + (1 - r) xprev, else xhat = out.  rec_part
 * [b][ceil(h w / 256)] (scratch and output: the per-block sums of (xhat - target)^2), rec_img [b] = the image's
 * mean squared error, stats [2] = (mean_b rec_img, mean_b kl_img).  c in [1, 4]; c = 3 reads a in 16-byte rows. */
int svae_op_output_fwd(const float* a, int b, int h, int w, int c, const float* xprev, const float* target, float lo,
                       float hi, float minh, float maxh, const float* kl_img, float* xhat, float* rec_part,
                       float* rec_img, float* stats, void* stream);
/* output_bwd + colsum_small: g = (dxhat_in ? dxhat_in : 0) + 2 rec_coef (xhat - target); da [b,h,w,c+1] = the
 * gradient of the pre-activations (ratio column 0 without xprev), dxprev = (1 - r) g (written only with xprev, then
 * required), db_out [c] and db_ratio [1] (may be NULL: dropped) = the column sums of da.  scratch >= 1024 floats.
 * c = 4 (outside any model): no bias sums, db_out and db_ratio NULL. */
int svae_op_output_bwd(const float* a, int b, int h, int w, int c, const float* xprev, const float* xhat,
                       const float* target, float lo, float hi, float minh, float maxh, float rec_coef,
                       const float* dxhat_in, float* da, float* dxprev, float* db_out, float* db_ratio, void* scratch,
                       int64_t scratch_bytes, void* stream);
/* One layer of the stddev network on in [n,h,w] pixels of pitch ldi (in_sig != 0: the layer reads sigmoid(in), as
 * layer 0 reads the output conv-T pre-activation at ldi = c + 1): pre = conv2d_same(in, wt [4,4,ci,co]) (stride 1,
 * pad 1 before / 2 after), mean / invstd [co] over the n h w rows (biased variance, eps 1e-3), act = lrelu_0.1((pre
 * - mean) invstd + beta).  ci, co <= 8; h % 4 == 0 (the limit of the layer's weight gradient, shared by both entry
 * points); scratch >= ceil(n h w / 256) * 2 co doubles, 16-byte aligned. */
int svae_op_sd_layer(const float* in, int ldi, int in_sig, int n, int h, int w, int ci, const float* wt, int co,
                     const float* beta, float* pre, float* mean, float* invstd, float* act, void* scratch,
                     int64_t scratch_bytes, void* stream);
/* Its backward from dact [n,h,w,co] and the forward's pre, mean, invstd, beta: dpre [n,h,w,co], dbeta [co],
 * dw [4,4,ci,co], and the input gradient: mode 0: din[q * ldd + i] = v; mode 1 (layer 0): din[q * ldd + i] +=
 * v s (1 - s) with s = sigmoid(in[q * ldi + i]).  scratch (16-byte aligned) >= ceil(n h w / 256) * 2 co doubles
 * rounded up to 16 bytes + 16 floats + n (h / 4) 16 ci co floats. */
int svae_op_sd_layer_bwd(const float* dact, const float* pre, const float* mean, const float* invstd,
                         const float* beta, const float* in, int ldi, int in_sig, int n, int h, int w, int ci,
                         const float* wt, int co, int mode, float* dpre, float* dbeta, float* dw, float* din, int ldd,
                         void* scratch, int64_t scratch_bytes, void* stream);
/* The stddev head: sd [b,h,w] = smax sigmoid(act . w5 + b5) on act [b,h,w,ci]; sample = mle + reg sd noise
 * ([b,h,w,c] each); rec_part [b][ceil(h w / 256)] = per-block sums of log sd + 0.5 log 2 pi + 0.5 ((mle - target) /
 * sd)^2 over pixels and channels (the layout loss_reduce reads). */
int svae_op_sd_head_fwd(const float* act, int ci, const float* w5, const float* b5, float smax, const float* mle,
                        const float* target, const float* noise, float reg, int b, int h, int w, int c, float* sd,
                        float* sample, float* rec_part, void* stream);
/* Its backward for the loss sum(dsample * sample) + nll_coef * sum(NLL terms) (dsample may be NULL: zero): dmle
 * [b,h,w,c], dact [b,h,w,ci], dw5 [ci], db5 [1].  scratch >= ceil(b h w / 256) * (ci + 1) floats. */
int svae_op_sd_head_bwd(const float* act, int ci, const float* w5, const float* b5, float smax, const float* mle,
                        const float* target, const float* noise, float reg, float nll_coef, const float* dsample, int b,
                        int h, int w, int c, float* dmle, float* dact, float* dw5, float* db5, void* scratch,
                        int64_t scratch_bytes, void* stream);
/* sample = mle + scale * noise over n elements */
int svae_op_chain_noise(const float* mle, const float* noise, float scale, int64_t n, float* sample, void* stream);
/* out = (dxin ? dxin : 0) + 2 coef ((xp ? x - xp : 0) - (xn ? xn - x : 0)); dxin, xp, xn may be NULL; out may be dxin */
int svae_op_imp_seed(const float* dxin, const float* xp, const float* x, const float* xn, float coef, int64_t n,
                     float* out, void* stream);
/* out[i] = sum over image i's per_img elements of (a - b)^2 */
int svae_op_sqdiff_img(const float* a, const float* b, int nimg, int64_t per_img, float* out, void* stream);
/* The training batch in one launch on `stream` (no allocation, no synchronisation): rows of a
 * device-resident dataset data [N, per_image] (uint8 when data_u8 = 1, else fp32) are gathered,
 * dequantised into the clean `target` and corrupted into the denoising `input`, both [n, per_image]
 * fp32; either may be NULL, not both.  Row b is data[idx[b]], or data[start + b] when idx == NULL
 * (indices are the caller's contract: no device-side check).
 *   target = lo + u8 * ((hi - lo) / 255)            (fp32 rows: the row as it is)
 *   input  = clip(target * keep + salt + gaussian_scale * N(0,1), lo, hi)
 * keep is 0 with probability pepper_prob and salt is 1 with probability salt_prob (pepper multiplies by
 * 0, salt ADDS 1: the reference's apply_noise as written).  Draws are Philox4x32-10 with key
 * (lo32(seed), hi32(seed)): flat output element e uses counter offset + e / 4 in words (c0, c1), c3 = 0,
 * and c2 = 0 for the four normals (Box-Muller on words (0,1) and (2,3) -> lanes 0..3), c2 = 1 for the
 * pepper words (keep_j = w_j >= thr(pepper_prob)), c2 = 2 for the salt words (salt_j = w_j <
 * thr(salt_prob)), thr(p) = min(floor(p * 2^32), 2^32 - 1).  The result depends on no launch geometry;
 * a caller advances offset by ceil(n * per_image / 4) per call.  In place (input == data) is allowed
 * for fp32 data with idx == NULL and start == 0.  SVAE_EBADARG: null data, both outputs null, n or
 * per_image <= 0, a probability outside [0, 1], a negative scale, lo > hi. */
int svae_op_make_batch(const void* data, int data_u8, const int32_t* idx, int64_t start, int n, int64_t per_image,
                       float lo, float hi, float pepper_prob, float salt_prob, float gaussian_scale, uint64_t seed,
                       uint64_t offset, float* target, float* input, void* stream);

/* Structured corruptions of a clean batch in one launch on `stream` (no allocation, no synchronisation; no
 * reference counterpart: the inputs of inpainting, deblurring and super-resolution runs).  target [n,h,w,c] is the
 * clean fp32 batch (what svae_op_make_batch writes with input == NULL); input receives the degraded batch and mask
 * [n,h,w] (may be NULL) 1 where a pixel was cut out, 0 elsewhere.  Per image b, in this order:
 *   1 blur      with probability p_blur: separable Gaussian, sigma = sigma_lo + u * (sigma_hi - sigma_lo) (the
 *               difference, the product and the sum each rounded to fp32), r = min(ceil(3 sigma), 12) taps to each
 *               side (fp32 product, fp32 ceil; r = 0: identity), weights g_k = expf(-k^2 / (2 sigma^2)) divided by
 *               g_0 + 2 sum_{k=1..r} g_k (the sum in ascending k).  Horizontal pass, then vertical pass, each
 *               sum_{k=-r..r} w_|k| x[clamp(i + k)] per channel, started from 0 and accumulated in fp32 in
 *               ascending k, every product and sum rounded on its own; out-of-image taps read the clamped index.
 *   2 down      with probability p_down (factor > 1): pixel (i, j) becomes the mean of the in-image pixels of its
 *               block (i / factor, j / factor), per channel: sequential fp32 adds from 0 in row-major order, then one
 *               correctly rounded fp32 division by the count (edge blocks are partial).
 *   3 cut-out   with probability p_cut: every pixel inside any of the `boxes` boxes becomes `fill` in all channels.
 *   4 noise     svae_op_make_batch's contract on the result, word for word: flat element e of the [n*h*w*c] batch,
 *               group e / 4, counter offset + e / 4, c3 = 0, streams c2 = 0, 1, 2, the same roundings; clip to [lo, hi].
 * Per-image draws are Philox4x32-10 under the key (lo32(seed), hi32(seed)) with the 64-bit value offset + b in the
 * counter words (c0, c1), c2 = 3 (a stream make_batch does not use) and c3 = the block index.  Block 0 gives words
 * a0..a3: blur iff a0 < thr(p_blur), u = (a1 >> 8) * 2^-24, down iff a2 < thr(p_down), cut-out iff a3 < thr(p_cut),
 * thr as in svae_op_make_batch.  Block 1 + k gives box k from words b0..b3, all integer (mulhi = the high 32 bits of
 * the 32 x 32 product): bh = min(h, min_side + mulhi(b0, max_side - min_side + 1)), bw likewise from b1 and w,
 * y0 = mulhi(b2, h - bh + 1), x0 = mulhi(b3, w - bw + 1); the box covers rows y0 .. y0 + bh - 1, columns x0 ..
 * x0 + bw - 1.  A caller advances offset by ceil(n*h*w*c / 4) per call as for svae_op_make_batch; h*w*c >= 4 makes
 * that at least n, so consecutive calls share no image counter.  The result depends on the arguments alone: on no
 * launch geometry, not on the kernel chosen (LDS bands, or global memory when a band of 8 rows plus halos exceeds
 * 64 KB) and not on the alignment path; two calls give the same bytes.
 * SVAE_EBADARG (checked on the host before any launch): null target, input or spec; input == target (the blur reads
 * neighbours); n, h, w or c <= 0; h*w*c < 4; a probability outside [0, 1]; sigma_lo < 0, sigma_lo > sigma_hi or
 * sigma_hi > 4; factor not in {1, 2, 4, 8}; boxes outside 0 .. 4; min_side < 1 or min_side > max_side; a negative
 * gaussian_scale; lo > hi.  SVAE_EBADCONFIG: h*w*c > 2^31 - 1. */
typedef struct svae_degrade_spec {
  float p_blur, sigma_lo, sigma_hi;      /* Gaussian blur, sigma uniform in [lo, hi], hi <= 4 */
  float p_down; int32_t factor;          /* box down-sample by factor in {1,2,4,8}, replicated back */
  float p_cut;  int32_t boxes, min_side, max_side; float fill;   /* boxes in 0..4 */
  float pepper_prob, salt_prob, gaussian_scale;                  /* make_batch's pixel noise */
} svae_degrade_spec;
int svae_op_degrade_batch(const float* target, int n, int h, int w, int c, float lo, float hi,
                          const svae_degrade_spec* spec, uint64_t seed, uint64_t offset, float* input, float* mask,
                          void* stream);

/* Random crops of large images as the clean batch, in one launch on `stream` (no allocation, no synchronisation, no
 * atomics; no reference counterpart: the front of the restoration workflow, whose network of tile size h x w is
 * trained on windows of images of any size H x W).  images [nimg,H,W,c] (uint8 when data_u8 = 1, else fp32, any base
 * alignment) -> target [n,h,w,c] fp32 and target_u8 of the same shape in uint8; either may be NULL, not both, and
 * target_u8 is legal only for uint8 images (it materialises fixed evaluation sets).  meta [n,5] int32 (may be NULL)
 * receives (m, s, g, y0, x0) of every row.
 * Row b with crops == NULL: draws are Philox4x32-10 under the key (lo32(seed), hi32(seed)) with the 64-bit value
 * offset + b in the counter words (c0, c1), c2 = 4 (a stream neither svae_op_make_batch, 0 .. 2, nor
 * svae_op_degrade_batch, 3, uses) and c3 = the block index; mulhi = the high 32 bits of the 32 x 32 product.
 * Block 0 gives words a0..a3: image m = mulhi(a0, nimg), scale s = scales[mulhi(a1, n_scales)], symmetry
 * g = mulhi(a2, symmetries).  Block 1 gives b0, b1: y0 = mulhi(b0, H - s*h + 1), x0 = mulhi(b1, W - s*w + 1).  A
 * caller advances offset by at least n per call (the trainer advances it by ceil(n*h*w*c / 4), the step of the
 * streams it shares the offset with).  With crops given ([n,5] int32 on the device) row b uses crops[b] =
 * (m, s, g, y0, x0) as it is and nothing is drawn; values outside their ranges (m in [0, nimg), s in 1 .. 8 with
 * s*h <= H and s*w <= W, g in [0, 8) and below 4 unless h == w, y0 in [0, H - s*h], x0 in [0, W - s*w]) are the
 * caller's contract, as for svae_op_make_batch's idx: no device-side check.
 * Symmetry g: bit 0 mirrors x, bit 1 mirrors y, bit 2 transposes.  For output pixel (i, j): (i', j') = (j, i) if
 * bit 2 is set, else (i, j); then i' <- h - 1 - i' if bit 1 is set; then j' <- w - 1 - j' if bit 0 is set.
 * symmetries = 2 yields g in {0, 1}, 4 yields {0 .. 3}, 8 yields {0 .. 7}.
 * Output (b, i, j, ch) is the mean of the s x s source block at rows y0 + s*i' + p, columns x0 + s*j' + q of image m:
 *   uint8   the exact integer sum; qbar = (float)sum / (float)(s*s), one correctly rounded fp32 division (s = 1:
 *           none, qbar = the pixel); target = lo + qbar * ((hi - lo) / 255) with the constant, the product and the
 *           sum each rounded to fp32, word for word svae_op_make_batch's dequantisation;
 *           target_u8 = min(255, rintf(qbar)) (ties to even)
 *   fp32    sequential fp32 adds from 0 in row-major order (p outside, q inside), then one correctly rounded fp32
 *           division by s*s; s = 1 is a copy of the pixel
 * Consequences: for s = 1, g = 0 the row equals svae_op_make_batch on the pre-cut tile, bit for bit.  The result
 * depends on the arguments alone: on no launch geometry, not on the kernel variant (a block stages its source patch
 * in LDS, or reads it from global memory where the patch of the largest listed scale exceeds 64 KB) and not on the
 * alignment path; two calls give the same bytes.
 * SVAE_EBADARG (checked on the host before any launch): null images or spec; target and target_u8 both null;
 * target_u8 with fp32 images; nimg, H, W, c, h, w or n <= 0; n_scales outside 1 .. 4; a scale outside 1 .. 8 or
 * listed twice; s*h > H or s*w > W for a listed scale; symmetries not in {1, 2, 4, 8}; 8 with h != w; lo >= hi
 * with uint8 images.  SVAE_EBADCONFIG: H*W*c or h*w*c > 2^31 - 1. */
typedef struct svae_crop_spec {
  int32_t n_scales; int32_t scales[4];   /* integer box factors, each in 1..8, all distinct */
  int32_t symmetries;                    /* 1: none, 2: mirror x, 4: mirror x and/or y, 8: dihedral group (needs h == w) */
} svae_crop_spec;
int svae_op_crop_batch(const void* images, int data_u8, int nimg, int H, int W, int c, int h, int w,
                       const svae_crop_spec* spec, const int32_t* crops, uint64_t seed, uint64_t offset, int n,
                       float lo, float hi, float* target, uint8_t* target_u8, int32_t* meta, void* stream);

/* JPEG compression artefacts on a batch in one launch on `stream` (no allocation, no synchronisation, no atomics; no
 * reference counterpart: the inputs of deblocking and de-ringing runs).  in and out are [n,h,w,c] fp32 with values in
 * [lo, hi], c = 1 (grey) or 3 (RGB); out == in is legal (any other overlap is the caller's contract).  quality [n]
 * int32 (may be NULL) receives the quality used, 0 for an image that was not compressed.  There is no entropy
 * coding: only the decoded pixels exist.
 * Draws per image b: Philox4x32-10 under the key (lo32(seed), hi32(seed)) with the 64-bit value offset + b in the
 * counter words (c0, c1), c2 = 5 (a stream neither svae_op_make_batch, 0 .. 2, svae_op_degrade_batch, 3, nor
 * svae_op_crop_batch, 4, uses) and c3 = 0.  With the words a0..a3: compress iff a0 < thr(p), q = q_lo +
 * mulhi(a1, q_hi - q_lo + 1), thr and mulhi as above.  An image that is not compressed is copied byte for byte (in
 * place: nothing is done).  A compressed image, in this order, every product, sum and division rounded to fp32 on its
 * own, sums left to right as written:
 *   1 levels    L = clamp(rintf((x - lo) * (255 / (hi - lo))), 0, 255), the constant rounded to fp32 (rintf: ties to even)
 *   2 colour    (c = 3) JFIF full-range BT.601 with fp32 constants:
 *                 Y  = 0.299 R + 0.587 G + 0.114 B
 *                 Cb = 128 - 0.168735892 R - 0.331264108 G + 0.5 B
 *                 Cr = 128 + 0.5 R - 0.418687589 G - 0.081312411 B
 *               each then rintf and clamped to [0, 255], as a codec's 8-bit component planes are.  c = 1: Y = L.
 *   3 chroma    subsample = 1 (4:4:4): the chroma planes are h x w.  subsample = 2 (4:2:0; c = 3 only, ignored for
 *               c = 1): they are ceil(h/2) x ceil(w/2), each value the mean of the in-image pixels of its 2 x 2 block:
 *               sequential fp32 adds from 0 in row-major order, then one correctly rounded fp32 division by the count.
 *               The means are not rounded to integers.
 *   4 blocks    each plane is extended to multiples of 8 by replicating its last row and column; 128 is subtracted
 *               from every value.  Per 8 x 8 block f, F = C f C^T with C[u][x] = cos((2x + 1) u pi / 16) / 2 and
 *               C[0][x] = 1 / sqrt(8), a table of the fp32 constants 0.353553391 (u = 0), then for m = (2x + 1) u
 *               folded into the first octant (cos(m pi / 16) / 2, m = 1 .. 7, with its sign): 0.490392640,
 *               0.461939766, 0.415734806, 0.353553391, 0.277785117, 0.191341716, 0.0975451610.  Row pass first:
 *               t[y][u] = sum_x f[y][x] * C[u][x] from 0 in ascending x; then the column pass F[v][u] =
 *               sum_y C[v][y] * t[y][u] from 0 in ascending y.
 *   5 quantiser the JPEG standard's Annex K luminance (Y) and chrominance (Cb, Cr) tables in natural order, IJG
 *               scaling in integers: s = q < 50 ? 5000 / q : 200 - 2 q, T = clamp((base * s + 50) / 100, 1, 255).
 *               k = rintf(F / (float)T), the division correctly rounded; dequantised G = k * T.
 *   6 inverse   column pass s[y][u] = sum_v C[v][y] * G[v][u], then row pass g[y][x] = sum_u s[y][u] * C[u][x], both
 *               from 0 in ascending order; then rintf(g + 128) clamped to [0, 255].
 *   7 chroma up subsample = 2: pixel (i, j) reads chroma (i / 2, j / 2).
 *   8 colour    (c = 3)  R = Y + 1.402 (Cr - 128),  G = Y - 0.344136286 (Cb - 128) - 0.714136286 (Cr - 128),
 *               B = Y + 1.772 (Cb - 128); then rintf, clamped to [0, 255].  c = 1: L' = Y.
 *   9 out       lo + L' * ((hi - lo) / 255) with the constant, the product and the sum each rounded to fp32, word for
 *               word svae_op_make_batch's dequantisation.
 * The result depends on the arguments alone: on no launch geometry and not on the alignment path (16-byte accesses
 * where the base and h*w*c rows allow, element by element otherwise); two calls give the same bytes.  A block of
 * threads owns 16 x 16 pixels, so no image size exceeds what a block can hold.
 * SVAE_EBADARG (checked on the host before any launch): null in, out or spec; n, h or w <= 0; c not in {1, 3}; p
 * outside [0, 1]; q_lo < 1, q_hi > 100 or q_lo > q_hi; subsample not in {1, 2}; lo >= hi.  SVAE_EBADCONFIG:
 * h*w*c > 2^31 - 1. */
typedef struct svae_jpeg_spec {
  float p;                 /* probability per image */
  int32_t q_lo, q_hi;      /* IJG quality, uniform integer in [q_lo, q_hi], 1 <= q_lo <= q_hi <= 100 */
  int32_t subsample;       /* 1: 4:4:4, 2: 4:2:0 (c == 3 only; ignored for c == 1) */
} svae_jpeg_spec;
int svae_op_jpeg_batch(const float* in, int n, int h, int w, int c, float lo, float hi,
                       const svae_jpeg_spec* spec, uint64_t seed, uint64_t offset,
                       float* out, int32_t* quality, void* stream);

/* Overlapping tiles: the work around the forward when a network of tile size th x tw restores whole images (no
 * reference counterpart).  Both ops are one launch on `stream`, no allocation, no synchronisation, no atomics: the
 * result depends on the arguments alone (on no launch geometry, not on the alignment path or the kernel variant),
 * and two calls give the same bytes.
 * Geometry, per axis with image extent L, tile extent t <= L and stride 1 <= s <= t: k = ceil((L - t) / s) + 1
 * tiles, tile i at o_i = min(i s, L - t) (the last tile is pulled back to the edge: nothing is padded).  Tile
 * (m, i, j) of image m, row tile i, column tile j has id (m k_y + i) k_x + j; n_tiles = nimg k_y k_x.  The window
 * weight of tile pixel (p, q) is w1_y(p) w1_x(q) with w1(p) = min(p + 1, t - p), a small exact integer.
 *
 * svae_op_extract_tiles: images [nimg,H,W,c] (uint8 when data_u8 = 1, else fp32, any base alignment) -> tiles
 * [count,th,tw,c] fp32.  Row r receives tile (first + r) mod n_tiles; count > n_tiles is legal and wraps.  A uint8
 * pixel q becomes lo + q * ((hi - lo) / 255) exactly as in svae_op_make_batch (the product and the sum each rounded
 * to fp32); fp32 pixels are copied as they are.
 *
 * svae_op_blend_tiles: tiles holds nstack sets of all n_tiles tiles in id order, set k at tiles + k * stack_stride
 * floats; out [nstack,nimg,H,W,c] fp32 and out_u8 of the same shape in uint8, either may be NULL, not both.
 * Output element (k, m, y, x, ch):
 *   acc = sum_i sum_j (double)(w1_y(y - oy_i) * w1_x(x - ox_j)) * (double)tile value   over the covering tiles,
 *         i ascending outside, j ascending inside, from 0, every product and sum in fp64
 *   Wgt = sum_i sum_j of the same weights (an exact integer)
 *   v   = (float)(acc / Wgt)             one IEEE fp64 division, one rounding to fp32
 * The tiles covering a position of an axis form one contiguous index range (origins are non-decreasing; the
 * clamped last tile is an ordinary member).  Where known [nimg,H,W] (uint8, may be NULL) is non-zero at (m, y, x),
 * v is instead the source pixel at (m, y, x, ch) in every stack: source has the layout of images (uint8 when
 * source_u8 = 1, dequantised as above; else fp32 as it is) and is required when and only when known is given.
 *   out_u8 = (uint8) min(max(rintf((v - lo) * (255 / (hi - lo))), 0), 255)
 * with the constant 255 / (hi - lo) rounded to fp32 and the difference and the product each rounded to fp32.
 * Two consequences:
 *   (a) where every covering tile carries the same value u (and Wgt < 2^29, which SVAE_EBADCONFIG enforces) every
 *       partial sum is exact and v == u bit for bit: blend(extract(img)) == img bitwise for fp32 images;
 *   (b) for uint8 images, extract followed by blend into out_u8 returns the input bytes.
 * SVAE_EBADARG (checked on the host before any device call): null images or tiles, out and out_u8 both null; known
 * without source or source without known; nimg, H, W, c, th, tw, sy, sx, count or nstack <= 0; th > H, tw > W,
 * sy > th or sx > tw; first < 0 or first >= n_tiles; stack_stride < n_tiles*th*tw*c; lo >= hi where a uint8 side
 * (images, source or out_u8) is involved.  SVAE_EBADCONFIG: th*tw*c or H*W*c > 2^31 - 1; (blend) the largest
 * per-axis weight sums have a product of 2^29 or more. */
int svae_op_extract_tiles(const void* images, int data_u8, int nimg, int H, int W, int c, int th, int tw, int sy,
                          int sx, float lo, float hi, int64_t first, int64_t count, float* tiles, void* stream);
int svae_op_blend_tiles(const float* tiles, int nstack, int64_t stack_stride, int nimg, int H, int W, int c, int th,
                        int tw, int sy, int sx, const void* source, int source_u8, const uint8_t* known, float lo,
                        float hi, float* out, uint8_t* out_u8, void* stream);

/* Segmented statistics of one fp32 device array in one pass (no reference counterpart; the numbers behind
 * the training summaries).  Segments (offset, length) in elements of x: disjoint, ascending, gaps allowed,
 * any alignment, length 0 legal.  With y = clamp(x, -c, +c) (c = +inf: none), row s of out [n_seg][8] (fp64):
 *   col 0  number of finite elements
 *   col 1  sum y
 *   col 2  sum |y|
 *   col 3  sum y^2
 *   col 4  max |x| over the finite elements (0 if none)
 *   col 5  number of finite elements with |x| > c
 *   col 6  number of non-finite elements (NaN, +-inf)
 *   col 7  0 (reserved)
 * A non-finite element is counted in col 6 and contributes to nothing else.  Sums are accumulated in fp64 in
 * a fixed order (csrc/stats.hip): the result depends on x, the segments and c only, two calls give the same
 * bytes, and nothing outside a segment is read.
 *
 * The plan is built on the host (no GPU needed) and uploaded once per (array, segmentation).  It cuts segment
 * s at the element indices (offset_s & ~3) + k * SVAE_STATS_CHUNK, so no chunk crosses a segment or exceeds
 * SVAE_STATS_CHUNK elements.  Layout, in int64 words:
 *   table[s], s = 0 .. n_seg      index of segment s's first chunk; table[n_seg] = n_chunks
 *   table[n_seg + 1 + 2 k]        first element of chunk k
 *   table[n_seg + 2 + 2 k]        (segment of chunk k) << 32 | its length
 * so a table holds n_seg + 1 + 2 * n_chunks words.  The plan call returns n_chunks (>= 0); table == NULL only
 * counts.  SVAE_EBADARG: a null array with n_seg > 0, a negative count, offset or length, segments out of order or
 * overlapping, or cap_words (the words table can hold) too small -- the message names both sizes. */
#define SVAE_STATS_CHUNK 16384
int64_t svae_op_stats_plan(const int64_t* offsets, const int64_t* lengths, int32_t n_seg, int64_t* table,
                           int64_t cap_words);
/* The launch: plan is the table in device memory, partials a device scratch of max(1, n_chunks) * 8 doubles, out
 * n_seg * 8 doubles (rows past n_seg are not touched).  At most two kernel launches on `stream`, no allocation,
 * no synchronisation; 16-byte loads when x is 16-byte aligned, the same sums in the same order when it is not.
 * n_seg and n_chunks must be the plan's (the device cannot check them).  SVAE_EBADARG: a null pointer, a
 * negative count, c < 0 or NaN. */
int svae_op_tensor_stats(const float* x, const int64_t* plan, int32_t n_seg, int64_t n_chunks, float c,
                         double* partials, double* out, void* stream);

/* Per-image quality metrics in one launch on `stream` (no allocation, no synchronisation; no reference
 * counterpart: the numbers behind NoisyTrainer.evaluate).  x [n, h, w, c] and y [ny, h, w, c] are fp32 NHWC on
 * the device; image i of x is compared with image i % ny of y, so one call scores a stack of k * ny images
 * against ny targets.  Row i of out [n][4] (fp64; rows past n are not touched):
 *   col 0  sum (x - y)^2 over the h * w * c elements
 *   col 1  sum |x - y|
 *   col 2  mean SSIM over the (h - 10) * (w - 10) valid window positions and the c channels
 *   col 3  number of non-finite elements (NaN, +-inf) among the two images
 * SSIM is Wang et al. 2004: per channel, an SVAE_SSIM_WINDOW^2 Gaussian window w of standard deviation
 * SVAE_SSIM_SIGMA normalised to sum 1 (the outer product of the normalised 1-D window with itself), weighted
 * population statistics mu = sum w x, var = sum w x^2 - mu^2, cov = sum w x y - mu_x mu_y, and
 *   SSIM = (2 mu_x mu_y + C1) (2 cov + C2) / ((mu_x^2 + mu_y^2 + C1) (var_x + var_y + C2)),
 * C1 = (SVAE_SSIM_K1 L)^2, C2 = (SVAE_SSIM_K2 L)^2, L = data_range; only window positions that lie wholly
 * inside the image count.  All arithmetic after the load is fp64, in a fixed order without atomics
 * (csrc/metrics.hip): row i depends on image i and its reference only (not on n, the grid or an address) and
 * two calls give the same bytes.  16-byte loads where both images are 16-byte aligned, the same values in the
 * same order where not.  A non-finite element is counted in col 3; cols 0 .. 2 of that row then follow IEEE
 * arithmetic (NaN or inf), other rows are not affected.  The kernel walks the valid positions in tiles of
 * SVAE_METRICS_TILE x SVAE_METRICS_TILE.  SVAE_EBADARG (checked on the host before any device call): a null
 * pointer, n, ny or c <= 0, n not a multiple of ny, h or w < SVAE_SSIM_WINDOW, data_range <= 0 or NaN. */
#define SVAE_SSIM_WINDOW 11
#define SVAE_SSIM_SIGMA 1.5
#define SVAE_SSIM_K1 0.01
#define SVAE_SSIM_K2 0.03
#define SVAE_METRICS_TILE 16
int svae_op_image_metrics(const float* x, int n, const float* y, int ny, int h, int w, int c, float data_range,
                          double* out, void* stream);

/* Log-density of query points under an equal-weight mixture of diagonal Gaussians, per group of dimensions, without
 * the 1 / nm (no reference counterpart: the numbers behind NoisyTrainer.latent_information).  z [nq] rows ldz
 * floats apart, mu and sigma [nm] rows ldm floats apart (fp32, device, any base alignment, ldz, ldm >= d); seg is a
 * HOST array of n_seg (offset, length) pairs, dimension sets S = [offset, offset + length) of [0, d) that may
 * overlap and come in any order.  Row n of out [nq][n_seg] (fp64, device; nothing else is written):
 *   out[n][s] = log sum_{m < nm} exp( sum_{j in S} ( -((z[n][j] - mu[m][j]) / sigma[m][j])^2 / 2
 *                                                    - log sigma[m][j] - log(2 pi) / 2 ) )
 * All arithmetic after the load is fp64 in an order fixed by the shapes (csrc/latents.hip): the dimensions of S in
 * ascending order, then a streaming logsumexp over the components in ascending m.  out[n][s] depends on z[n], the
 * components and the segment only: not on nq, on the other segments, on the launch or on an address; two calls give
 * the same bytes.  No [nq, nm] intermediate exists: components are staged in tiles of SVAE_LATENTS_TILE.  The
 * segments travel as kernel arguments, sixteen consecutive ones to a block: one launch on `stream` per run of up
 * to 256 segments whose groups of sixteen span alike many dimensions (<= 16, 64, 128 or 256), so one or two
 * launches for a whole / levels / single-dimensions list; no allocation, no synchronisation.  sigma > 0 and finite is the
 * caller's contract: a
 * component or query that breaks it (or a NaN) makes the rows that read it non-finite and nothing else.
 * SVAE_EBADARG (checked on the host before any launch): a null pointer, nq, nm, d or n_seg <= 0, ldz or ldm < d, a
 * segment with length < 1 or outside [0, d).  SVAE_EBADCONFIG: d > SVAE_LATENTS_MAX_DIM, n_seg >
 * SVAE_LATENTS_MAX_SEGMENTS, nq > 2^31 - 1. */
#define SVAE_LATENTS_TILE 16
#define SVAE_LATENTS_MAX_DIM 256
#define SVAE_LATENTS_MAX_SEGMENTS 1024
int svae_op_mixture_logdensity(const float* z, int64_t nq, int64_t ldz, const float* mu, const float* sigma,
                               int64_t nm, int64_t ldm, int d, const int32_t* seg, int n_seg, double* out,
                               void* stream);

/* Row-wise statistics of pairwise squared distances (no reference counterpart: the numbers behind
 * NoisyTrainer.sample_quality).  x is [n] rows of d fp32, ldx floats apart; y, m, ldy are HOST arrays of n_groups
 * device pointers, row counts and leading dimensions, the column groups (separate tensors: nothing is
 * concatenated).  Any base alignment, ldx, ldy[g] >= d.  self_group = g >= 0 says the rows ARE group g's points
 * (x == y[g], n == m[g], row i is column i): the pair (i, i) of that group enters neither output; -1: no exclusion.
 * inv_two_sigma2 is a HOST array of n_bw values 1 / (2 sigma_l^2).  With d2(i, j) = sum_k (x[i][k] - y_g[j][k])^2,
 * the outputs (device; nothing else is written) are
 *   ksum  [n][n_groups][n_bw] (fp64)  = sum_j exp(-d2(i, j) * inv_two_sigma2[l]) over the group's admitted columns,
 *   nn_d2 [n][n_groups]       (fp64)  = min_j d2(i, j) over the same columns, +inf where there is none,
 *   nn_idx[n][n_groups]       (int64) = the smallest j that attains the computed minimum, -1 where there is none.
 * ksum, or nn_d2 and nn_idx together, may be NULL to skip that part; n_bw == 0 requires ksum == NULL.
 * Numerics (csrc/pairwise.hip): d2 = max(0, (a_i + b_j) - 2 g_ij) in fp64, a and b the squared norms summed in fp64
 * in an order fixed by d, g_ij the inner product on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation
 * in ascending k); exp and every sum over j in fp64, ascending j within column tiles of SVAE_PAIRWISE_TILE_COLS,
 * the tiles in ascending order; no atomics.  Row i of every output depends on x[i], the groups and the bandwidths
 * only: not on n, on the other rows, on the launch or on an address; two calls give the same bytes.  A NaN or inf
 * element makes the rows and columns that read it non-finite and nothing else.  The launches go on `stream`; no
 * allocation, no synchronisation: the caller provides svae_op_pairwise_scratch_bytes(n, m, n_groups, n_bw) bytes
 * of 8-byte aligned device scratch (norms and per-column-tile partials).
 * SVAE_EBADARG (checked on the host before any launch): a null required pointer or only one of nn_d2 / nn_idx, n,
 * d, n_groups or an m[g] <= 0, a leading dimension < d, n_bw < 0, n_bw == 0 with ksum or n_bw > 0 without, nothing
 * to compute, a bandwidth value <= 0 or non-finite, self_group >= n_groups or set with n != m[self_group] or
 * x != y[self_group], null scratch.  SVAE_EBADCONFIG: n_groups > SVAE_PAIRWISE_MAX_GROUPS, n_bw >
 * SVAE_PAIRWISE_MAX_BW, d > 2^31 - 1, more than 65535 row tiles or 2^31 - 1 column tiles.
 * svae_op_pairwise_scratch_bytes returns -1 for arguments the op would reject. */
#define SVAE_PAIRWISE_TILE_ROWS 128
#define SVAE_PAIRWISE_TILE_COLS 128
#define SVAE_PAIRWISE_TILE_K 32
#define SVAE_PAIRWISE_MAX_GROUPS 4
#define SVAE_PAIRWISE_MAX_BW 8
int64_t svae_op_pairwise_scratch_bytes(int64_t n, const int64_t* m, int n_groups, int n_bw);
int svae_op_pairwise_stats(const float* x, int64_t n, int64_t ldx, const float* const* y, const int64_t* m,
                           const int64_t* ldy, int n_groups, int64_t d, int self_group,
                           const double* inv_two_sigma2, int n_bw, double* ksum, double* nn_d2, int64_t* nn_idx,
                           void* scratch, void* stream);

/* Row-wise order statistics and ball counts of the same pairwise squared distances (no reference counterpart: the
 * numbers behind quality.manifold, the k-NN precision / recall / density / coverage of NoisyTrainer.sample_quality).
 * x, n, ldx, y, m, ldy, n_groups, d and self_group are svae_op_pairwise_stats' own, and so is d2(i, j), bit for bit
 * (csrc/pairwise_tile.h: the two ops share the norms and the distance tile): max(0, (a_i + b_j) - 2 g_ij) in fp64,
 * the norms summed in fp64 in an order fixed by d, g_ij on v_mfma_f32_32x32x2_f32 in ascending k, a non-finite value
 * NaN.  radius2 is a HOST array of n_groups device pointers, entry g [m[g]][n_radii] fp64: the squared radii of
 * column j of group g; a NULL entry: that group has no radii.  Per row i and group g, over the group's admitted
 * columns (all but (i, i) of the self group), the outputs (device; nothing else is written) are
 *   knn_d2   [n][n_groups][k]       (fp64)  = the k smallest d2(i, j) in ascending order (values, not columns: ties
 *                                             cannot make it ambiguous), +inf where fewer than k columns are admitted,
 *   inside   [n][n_groups][n_radii] (int64) = the number of admitted columns j with d2(i, j) <= radius2[g][j][r]; a
 *                                             NaN radius admits nothing, a +inf radius every finite d2, a group
 *                                             without radii gives 0,
 *   nonfinite[n][n_groups]          (int64) = the number of admitted pairs whose d2 is NaN; may be NULL.
 * A pair whose d2 is NaN enters neither knn_d2 nor inside: it is counted, not propagated.  That differs from
 * svae_op_pairwise_stats, where a NaN spoils the sums and the minimum of the rows that read it: a sum has no
 * answer without the term, an order statistic and a count over the remaining pairs have one, and nonfinite says
 * how many pairs they leave out.  knn_d2 (with k == 0) or inside (with n_radii == 0) may be NULL to skip that part;
 * a part computed alone has the bytes it has beside the other.  knn_d2[.][.][0] has the bytes of
 * svae_op_pairwise_stats' nn_d2 wherever no admitted pair is NaN.
 * Row i of every output depends on x[i], the groups and the radii only: not on n, on the other rows, on the row tile
 * or the grid, or on an address; two calls give the same bytes.  No atomics, no allocation, no synchronisation; the
 * launches go on `stream`; the caller provides svae_op_knn_scratch_bytes(n, m, n_groups, k, n_radii) bytes of
 * 8-byte aligned device scratch (norms and per-column-tile partials).
 * SVAE_EBADARG (checked on the host before any launch): a null required pointer, n, d, n_groups or an m[g] <= 0, a
 * leading dimension < d, k < 0 or n_radii < 0, k == 0 with knn_d2 or k > 0 without, n_radii == 0 with inside or
 * n_radii > 0 without inside or without radius2, nothing to compute, self_group >= n_groups or set with
 * n != m[self_group] or x != y[self_group], null scratch.  SVAE_EBADCONFIG: n_groups > SVAE_PAIRWISE_MAX_GROUPS,
 * k > SVAE_KNN_MAX_K, n_radii > SVAE_KNN_MAX_RADII, d > 2^31 - 1, more than 65535 row tiles or 2^31 - 1 column
 * tiles.  svae_op_knn_scratch_bytes returns -1 for arguments the op would reject. */
#define SVAE_KNN_MAX_K 8
#define SVAE_KNN_MAX_RADII 4
int64_t svae_op_knn_scratch_bytes(int64_t n, const int64_t* m, int n_groups, int k, int n_radii);
int svae_op_pairwise_knn(const float* x, int64_t n, int64_t ldx, const float* const* y, const int64_t* m,
                         const int64_t* ldy, int n_groups, int64_t d, int self_group, int k, double* knn_d2,
                         const double* const* radius2, int n_radii, int64_t* inside, int64_t* nonfinite,
                         void* scratch, void* stream);

/* Binned power spectra of a stack of images and of their differences to reference images, one launch on `stream`
 * (no allocation, no synchronisation; no reference counterpart: the numbers behind NoisyTrainer.spectrum).
 * x [n, h, w, c] and y [ny, h, w, c] or NULL are fp32 NHWC on the device at any alignment; image i of x is paired
 * with image i % ny of y, as in svae_op_image_metrics.  The tables are the caller's, on the device: win_y [h] and
 * win_x [w] (fp64), tw_y [h][2] and tw_x [w][2] with tw[k] = (cos 2 pi k / len, -sin 2 pi k / len) (fp64), and
 * bin [h][wu], wu = w / 2 + 1 (int32): the output bin of spectrum entry (v, u), any value outside [0, n_bins)
 * (-1 by convention) leaves the entry out.  out is [n][c][2][n_bins] fp64: plane 0 the binned power of the windowed
 * image, plane 1 that of the windowed difference x - y (not touched when y == NULL); rows past n are not touched, a
 * bin no entry maps to is written 0.  nonfinite [n][c] (int64, may be NULL) counts the NaN and +-inf among the
 * elements read for that row: channel k of image i and, when y is given, of its partner.
 * Per (image i, channel k, plane), everything after the load in fp64 on the vector ALU, every product, sum and
 * difference rounded once in the order written (no fused multiply-add, no matrix instruction, no atomics):
 *   a[yy][xx] = ((double)value * win_y[yy]) * win_x[xx]; in plane 1 the value is (double)x - (double)y, which is exact
 *   T[yy][u]  = sum_xx a[yy][xx] * tw_x[(u xx) mod w]   for u in [0, w / 2], from 0 in ascending xx (a real times a
 *               complex number: two products)
 *   F[v][u]   = sum_yy T[yy][u] * tw_y[(v yy) mod h]    from 0 in ascending yy, the complex product as
 *               (Tr c - Ti s, Tr s + Ti c) with tw = (c, s), each part added to its sum
 *   P[v][u]   = (Re F * Re F + Im F * Im F) * m(u), m(u) = 1 for u = 0 and for u = w / 2 with w even, 2 otherwise
 *   out[b]    = sum_u ( sum over the v with bin[v][u] == b of P[v][u], from 0 in ascending v ), from 0 in ascending u
 *               (a column without such an entry adds 0)
 * The op calls no trigonometric function; the table index is reduced in integers.  Row (i, k) depends on image i,
 * its partner and the tables only: not on n, on the grid, on an address or on the load path (16-byte loads where
 * the images are 16-byte aligned, element by element where not: the same values either way); two calls give the
 * same bytes.  A non-finite element makes the rows that read it NaN or inf and no others.
 * SVAE_EBADARG (checked on the host before any device call): a null pointer other than y and nonfinite; n, ny, c or
 * n_bins <= 0 (ny also when y == NULL); h or w < 2; n not a multiple of ny when y is given.  SVAE_EBADCONFIG: h or
 * w > SVAE_SPECTRUM_MAX_DIM (the plane and its half spectrum live in LDS), n_bins > SVAE_SPECTRUM_MAX_BINS,
 * h * w * c or n * c > 2^31 - 1. */
#define SVAE_SPECTRUM_MAX_DIM 96
#define SVAE_SPECTRUM_MAX_BINS 64
int svae_op_power_spectrum(const float* x, int n, const float* y, int ny, int h, int w, int c, const double* win_y,
                           const double* win_x, const double* tw_y, const double* tw_x, const int32_t* bin, int n_bins,
                           double* out, int64_t* nonfinite, void* stream);

/* The averaging kernel alone (csrc/ema.hip): ema[i] = ema[i] - omd * (ema[i] - w[i]) for i in [0, n), one launch
 * on `stream`, no allocation, no synchronisation.  The inner difference, the product and the outer difference are
 * each rounded to fp32 once (no fused multiply-add): bitwise a numpy float32 restatement, whatever the grid and
 * whatever the alignment of either pointer (16-byte accesses from the first 16-byte boundary of ema, on w too when
 * it is aligned there; element by element before and after).  A NaN or inf in w or ema propagates as the formula
 * says.  ema and w must not overlap.  omd == 0 makes no launch.  SVAE_EBADARG: a null pointer, n <= 0, omd outside
 * [0, 1] or NaN. */
int svae_op_ema(float* ema, const float* w, int64_t n, float omd, void* stream);

#ifdef __cplusplus
}
#endif
#endif
